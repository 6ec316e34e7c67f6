"""Cost of the defect list on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg, TargetNum
3: bench.py PARAMS and its synthetic Src7), `--batch` staged sources, the model trained on the batch's own hits as in
scripts/model_time.py and the whole template as rectangle.  Needs a gfx950 device and torch.

All in one run, on one context, every form timed to the caller by the host clock (each call returns after its device
work is synchronised and its results are in the caller's arrays), the forms alternating call by call:
  (a) last_inspect()                          the inspection's records alone, no image
  (b) last_blobs()                            the defect list, labelled where the excess images lie
  (c) last_inspect(image=True) + blobs_host   the excess images through the host, labelled there by one core
(b) and (c) are compared once: equal.  The yardstick of (b) is (c) of the same run.  The per-kernel times of (b) come
from fpm_blobs_profile in a pass of their own (HIP events around each launch).
Good parts leave nearly empty excess images, so the labelling kernels are also timed on `--masks` synthetic 762 x 521
masks of tests/blobs_ref.py's random kind at densities 0.05 and 0.4: op_blobs (upload included) against blobs_host, the
results compared once.  Every form is warmed up.  Writes `blobs_src7.json` and `README.txt` into `--out-dir`.

    python scripts/blobs_time.py [--batch 64] [--reps 5] [--masks 192] [--out-dir profiles/blobs]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DISTINCT = 8   # distinct scenes generated on the host; a larger batch repeats them
ABS_THRESHOLD, K = 8, 3.0
BLOBS = dict(level=0, min_area=4, connectivity=8, cap=64)
DENSITIES = (0.05, 0.4)


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and len(a[1]) == len(b[1]) and all(
        x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


def alternate(forms, reps, warm=1):
    """{name: [ms]}: the forms in turn, `reps` timed rounds after `warm` untimed ones"""
    out = {name: [] for name in forms}
    for rep in range(reps + warm):
        for name, run in forms.items():
            t0 = time.perf_counter()
            run()
            if rep >= warm:
                out[name].append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--masks", type=int, default=192)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "blobs"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 runs per form"

    import numpy as np
    import torch   # noqa: F401  one HIP runtime, loaded before libfpm_hip.so

    import bench
    from fastest_image_pattern_matching_amd import TemplateMatcher, synth
    from fastest_image_pattern_matching_amd import _lib as L
    from fastest_image_pattern_matching_amd.matcher import blobs_host

    templ = synth.load_templates()["Dst7"]
    scenes = bench.make_sources(templ, min(DISTINCT, args.batch), 7)
    h, w = scenes[0].shape
    m = TemplateMatcher(0)
    for k, v in bench.PARAMS.items():
        setattr(m._params, k, v)
    assert m.learnPattern(templ)
    m.stage([scenes[i % len(scenes)] for i in range(args.batch)])
    counts, _ = m.match_staged_array()
    assert counts.tolist() == [bench.PARAMS["max_pos"]] * args.batch, counts.tolist()
    n = int(counts.sum())
    pw, ph = m.patch_size()
    assert m.model_train_last(-1) == n

    def form_a():
        return m.last_inspect(-1, ABS_THRESHOLD, K)

    def form_b():
        return m.last_blobs(-1, ABS_THRESHOLD, K, **BLOBS)

    def form_c():
        return blobs_host(m.last_inspect(-1, ABS_THRESHOLD, K, image=True)[1], **BLOBS)

    got_b, got_c = form_b(), form_c()
    assert same(got_b, got_c), "last_blobs differs from last_inspect(image=True) + blobs_host"
    hits = {"fg_pixels": int(got_b[0]["fg_pixels"].sum()), "n_components": int(got_b[0]["n_components"].sum()),
            "n_blobs": int(got_b[0]["n_blobs"].sum())}
    call_ms = alternate({"a_last_inspect": form_a, "b_last_blobs": form_b, "c_inspect_image_blobs_host": form_c}, args.reps)

    # the kernels of (b), in a pass of their own
    names = L.BLOB_KERNEL_SYMBOLS
    kernel_ms = {k: [] for k in names}
    kernel_info = {}
    m.profile(True)
    for rep in range(args.reps + 1):
        m.profile_reset()
        form_b()
        for i, k in enumerate(names):
            ms, launches, nbytes = m.blobs_profile(i)
            kernel_info[k] = {"launches": launches, "bytes": nbytes}
            if rep >= 1:
                kernel_ms[k].append(ms)
        ins = m.model_profile(L.MODEL_INSPECT)
    m.profile(False)

    # synthetic masks: the labelling alone, upload included, against the host entry
    rng = np.random.default_rng(762521)
    v, u = np.mgrid[0:ph, 0:pw]
    tone = (200 + (u + 3 * v) % 50).astype(np.uint8)
    masks = {}
    for d in DENSITIES:
        imgs = np.ascontiguousarray((rng.random((args.masks, ph, pw)) < d) * tone).astype(np.uint8)
        dev, host = m.op_blobs(imgs, **BLOBS), blobs_host(imgs, **BLOBS)
        assert dev[0].tobytes() == host[0].tobytes(), "op_blobs' summaries differ from blobs_host's"
        trunc = int((host[0]["flags"] != 0).sum())
        assert trunc > 0 or same(dev, host), "op_blobs differs from blobs_host"
        t = alternate({"op_blobs": lambda: m.op_blobs(imgs, **BLOBS), "blobs_host": lambda: blobs_host(imgs, **BLOBS)},
                      args.reps)
        masks[str(d)] = {"op_blobs_ms": stat(t["op_blobs"]), "blobs_host_ms": stat(t["blobs_host"]),
                         "host_over_device": statistics.median(t["blobs_host"]) / statistics.median(t["op_blobs"]),
                         "n_components": int(host[0]["n_components"].sum()), "n_blobs": int(host[0]["n_blobs"].sum()),
                         "truncated_images": trunc}

    a, b, c = (statistics.median(call_ms[k]) for k in ("a_last_inspect", "b_last_blobs", "c_inspect_image_blobs_host"))
    out = {"frame": [w, h], "template": [pw, ph], "params": bench.PARAMS, "batch": args.batch, "hits": n,
           "abs_threshold": ABS_THRESHOLD, "k": K, "blobs": BLOBS, "reps": args.reps, "excess": hits,
           "call_ms": {k: stat(x) for k, x in call_ms.items()},
           "b_minus_a_ms": b - a, "c_over_b": c / b,
           "kernel_ms": {k: dict(stat(x), **kernel_info[k]) for k, x in kernel_ms.items()},
           "inspect_launch_ms_last": ins[0], "masks": args.masks, "mask_ms": masks}
    os.makedirs(args.out_dir, exist_ok=True)
    line = json.dumps(out)
    print(line)
    with open(os.path.join(args.out_dir, "blobs_src7.json"), "w") as f:
        f.write(line + "\n")

    def row(label, s, extra=""):
        return f"  {label:<58}{s['median']:10.3f} ms  ({s['min']:.3f} .. {s['max']:.3f}){extra}\n"

    with open(os.path.join(args.out_dir, "README.txt"), "w") as f:
        f.write(f"blobs_src7.json: `python scripts/blobs_time.py --batch {args.batch} --reps {args.reps} --masks {args.masks}` on "
                "one MI355X.\n"
                f"The Src7 configuration ({w} x {h} sources, Dst7 {pw} x {ph}, +-180 deg, TargetNum 3), {args.batch} staged sources, "
                f"the model trained on\nthe batch's {n} hits, the whole template as rectangle; level 0, min_area 4, connectivity 8, "
                f"cap 64.  Host clock to the caller,\nmedians of {args.reps} calls per form, the forms alternating call by call, in "
                "parentheses the range of the calls:\n\n")
        f.write(row("(a) last_inspect(), no image", out["call_ms"]["a_last_inspect"]))
        f.write(row("(b) last_blobs()", out["call_ms"]["b_last_blobs"]))
        f.write(row("(c) last_inspect(image=True) + blobs_host", out["call_ms"]["c_inspect_image_blobs_host"]))
        f.write(f"  (b) - (a), added by the defect list{'':<22}{b - a:10.3f} ms\n")
        f.write(f"  (c) / (b){'':<49}{c / b:10.1f}\n\n")
        f.write(f"(b) and (c) returned the same bytes.  The excess images of these hits hold {hits['fg_pixels']} foreground pixels in "
                f"{hits['n_components']} components,\n{hits['n_blobs']} of them of at least 4 pixels.  The kernels of (b), HIP events "
                "around each launch, summed over the call's rounds:\n\n")
        for k in names:
            f.write(row(f"{k} ({kernel_info[k]['launches']} launches, {kernel_info[k]['bytes'] / 1e6:.0f} MB)", out["kernel_ms"][k]))
        f.write(f"\nThe labelling alone on {args.masks} synthetic {pw} x {ph} masks (upload included) against fpm_blobs_host, same "
                "arguments:\n\n")
        for d in DENSITIES:
            s = masks[str(d)]
            f.write(row(f"density {d}: op_blobs", s["op_blobs_ms"]))
            f.write(row(f"density {d}: blobs_host", s["blobs_host_ms"], f"   host / device {s['host_over_device']:.1f}"))
            f.write(f"    ({s['n_components']} components, {s['n_blobs']} of at least 4 pixels, {s['truncated_images']} images "
                    "truncated at cap 64)\n")


if __name__ == "__main__":
    main()
