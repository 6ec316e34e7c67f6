"""Cost of edge calipers on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg, TargetNum 3:
bench.py PARAMS and its synthetic Src7), `--batch` staged sources, K = 8 calipers of 256 x 32 samples, half 2, spread
over the template at four scan directions.  Needs a gfx950 device and torch.

All in one run, on one context, both forms timed to the caller by the host clock (each call returns after its device
work is synchronised and its results are in the caller's arrays), the forms alternating call by call:
  (a) last_calipers()                         the edges measured where the pixels are, one launch of k_caliper
  (b) the same numbers without the entry      caliper_pose per (hit, caliper) on the host, patches_at at those poses,
                                              a torch sum over the patch rows, caliper_edges_host + caliper_derive
(a) and (b) are compared once: the same bytes.  fpm_patches_at writes host memory and no entry writes patches at
caller-supplied poses to device memory, so (b)'s patches cross the host and its sum runs there.  In a pass of their own
(HIP events around each launch) k_caliper is held against k_patch_warp over the same rectangles: the same pixels by the
same sampler, the patches written there and only the records here.  Every form is warmed up.  Writes
`calipers_src7.json` and `README.txt` into `--out-dir`.

    python scripts/calipers_time.py [--batch 64] [--reps 5] [--out-dir profiles/calipers]
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
LENGTH, WIDTH, HALF, CONTRAST, CAP = 256, 32, 2, 12, 8
PHIS = (0.0, 90.0, 37.5, -137.5)


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


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
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "calipers"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 runs per form"

    import numpy as np
    import torch   # one HIP runtime, loaded before libfpm_hip.so

    import bench
    from fastest_image_pattern_matching_amd import TemplateMatcher, synth
    from fastest_image_pattern_matching_amd import _lib as L
    from fastest_image_pattern_matching_amd import matcher as M

    templ = synth.load_templates()["Dst7"]
    scenes = bench.make_sources(templ, min(DISTINCT, args.batch), 7)
    h, w = scenes[0].shape
    th, tw = templ.shape
    m = TemplateMatcher(0)
    for k, v in bench.PARAMS.items():
        setattr(m._params, k, v)
    assert m.learnPattern(templ)
    m.stage([scenes[i % len(scenes)] for i in range(args.batch)])
    counts, _ = m.match_staged_array()
    assert counts.tolist() == [bench.PARAMS["max_pos"]] * args.batch, counts.tolist()
    n = int(counts.sum())
    cals = [M.caliper(cx=tw * (k + 1) / 9.0, cy=th * (0.3 + 0.4 * (k % 2)), phi=PHIS[k % 4], length=LENGTH, width=WIDTH,
                      half=HALF, contrast=CONTRAST, polarity=0) for k in range(8)]
    K = len(cals)

    def form_a():
        return m.last_calipers(cals, source=-1, cap=CAP)

    idx = np.repeat(np.arange(args.batch, dtype=np.int32), bench.PARAMS["max_pos"])

    def outside(lt_k, ak):
        """FPM_CALIPER_OUTSIDE by the header's rule: a corner sample through the inverted patch matrix"""
        mm = [float(v) for v in M.patch_matrix(w, h, lt_k, ak, (0, 0)).reshape(-1)]
        d = mm[0] * mm[4] - mm[1] * mm[3]
        d = 1.0 / d if d != 0 else 0.0
        a11, a22 = mm[4] * d, mm[0] * d
        mm[0] = a11
        mm[1] *= -d
        mm[3] *= -d
        mm[4] = a22
        b1 = -mm[0] * mm[2] - mm[1] * mm[5]
        b2 = -mm[3] * mm[2] - mm[4] * mm[5]
        mm[2], mm[5] = b1, b2
        for e in range(4):
            x, y = (float(LENGTH - 1) if e & 1 else 0.0), (float(WIDTH - 1) if e & 2 else 0.0)
            sx, sy = mm[0] * x + mm[1] * y + mm[2], mm[3] * x + mm[4] * y + mm[5]
            if not (0.0 <= sx <= float(w - 1) and 0.0 <= sy <= float(h - 1)):
                return True
        return False

    # the hits' raw poses: Qt semantics give them back as ptLT and the angle (tests/test_gpu_align.py's way)
    results = m.match_staged()
    lts = [r.ptLT for rs in results for r in rs]
    angs = [r.dMatchedAngle for rs in results for r in rs]
    assert len(lts) == n and [len(rs) for rs in results] == counts.tolist()

    def form_b():
        lt_k = np.zeros((n, K, 2), np.float32)
        ang_k = np.zeros((n, K), np.float64)
        for i in range(n):
            for k in range(K):
                (lt_k[i, k, 0], lt_k[i, k, 1]), ang_k[i, k] = M.caliper_pose(lts[i], angs[i], cals[k])
        patches = m.patches_at(np.repeat(idx, K), lt_k.reshape(-1, 2), ang_k.reshape(-1), rect=(0, 0, LENGTH, WIDTH))
        prof = torch.from_numpy(patches).to(torch.int32).sum(dim=1).numpy()
        summary = np.zeros((n, K), M.CALIPER_SUMMARY_DTYPE)
        edges = np.zeros((n, K, CAP), M.EDGE_DTYPE)
        for i in range(n):
            for k in range(K):
                p = (float(lt_k[i, k, 0]), float(lt_k[i, k, 1]))
                raw, cnt, flags = M.caliper_edges_host(prof[i * K + k], cals[k], CAP)
                edges[i, k, :len(raw)] = M.caliper_derive(cals[k], p, ang_k[i, k], raw)
                if outside(p, ang_k[i, k]):
                    flags |= L.CALIPER_OUTSIDE
                strongest = int(np.argmax(np.abs(raw["d"]))) if len(raw) else -1
                summary[i, k] = (cnt, len(raw), strongest, flags, p[0], p[1], ang_k[i, k])
        return summary, edges

    summary_a, edges_a = form_a()      # after the second search: the same hits, the same poses
    summary_b, edges_b = form_b()
    assert summary_a.tobytes() == summary_b.tobytes(), "the summaries of (a) and (b) differ"
    assert edges_a.tobytes() == edges_b.tobytes(), "the edges of (a) and (b) differ"
    found = {"n_edges": int(summary_a["n_edges"].sum()), "truncated": int(((summary_a["flags"] & L.CALIPER_TRUNCATED) != 0).sum()),
             "outside": int(((summary_a["flags"] & L.CALIPER_OUTSIDE) != 0).sum())}
    call_ms = alternate({"a_last_calipers": form_a, "b_patches_at_sum_edges_host": form_b}, args.reps)

    # the two launches over the same rectangles, in a pass of their own
    lt_k, ang_k = np.stack([summary_a["lt_x"], summary_a["lt_y"]], -1).reshape(-1, 2), summary_a["angle"].reshape(-1)
    kern = {"k_caliper": [], "k_patch_warp": []}
    info = {}
    m.profile(True)
    for rep in range(args.reps + 1):
        for name in kern:
            m.profile_reset()
            if name == "k_caliper":
                form_a()
                ms, launches, nbytes = m.caliper_profile()
            else:
                m.patches_at(np.repeat(idx, K), lt_k, ang_k, rect=(0, 0, LENGTH, WIDTH))
                ms, launches, nbytes = m.profile_get(L.K_PATCH)
            info[name] = {"launches": launches, "bytes": nbytes}
            if rep >= 1:
                kern[name].append(ms)
    m.profile(False)

    a, b = statistics.median(call_ms["a_last_calipers"]), statistics.median(call_ms["b_patches_at_sum_edges_host"])
    kc, kp = statistics.median(kern["k_caliper"]), statistics.median(kern["k_patch_warp"])
    out = {"frame": [w, h], "template": [tw, th], "params": bench.PARAMS, "batch": args.batch, "hits": n, "calipers": K,
           "caliper": {"length": LENGTH, "width": WIDTH, "half": HALF, "contrast": CONTRAST, "phis": list(PHIS), "cap": CAP},
           "reps": args.reps, "found": found, "call_ms": {k: stat(x) for k, x in call_ms.items()}, "b_over_a": b / a,
           "kernel_ms": {k: dict(stat(x), **info[k]) for k, x in kern.items()}, "k_caliper_over_k_patch_warp": kc / kp}
    os.makedirs(args.out_dir, exist_ok=True)
    line = json.dumps(out)
    print(line)
    with open(os.path.join(args.out_dir, "calipers_src7.json"), "w") as f:
        f.write(line + "\n")

    def row(label, s, extra=""):
        return f"  {label:<58}{s['median']:10.3f} ms  ({s['min']:.3f} .. {s['max']:.3f}){extra}\n"

    with open(os.path.join(args.out_dir, "README.txt"), "w") as f:
        f.write(f"calipers_src7.json: `python scripts/calipers_time.py --batch {args.batch} --reps {args.reps}` on one MI355X.\n"
                f"The Src7 configuration ({w} x {h} sources, Dst7 {tw} x {th}, +-180 deg, TargetNum 3), {args.batch} staged sources, "
                f"{n} hits,\n{K} calipers of {LENGTH} x {WIDTH} samples, half {HALF}, contrast {CONTRAST}, both polarities, cap {CAP}, "
                f"at the scan directions {', '.join(f'{p:g}' for p in PHIS)}:\n{n * K} jobs.  Host clock to the caller, medians of "
                f"{args.reps} calls per form, the forms alternating call by call, in parentheses the\nrange of the calls:\n\n")
        f.write(row("(a) last_calipers()", out["call_ms"]["a_last_calipers"]))
        f.write(row("(b) caliper_pose, patches_at, sum, edges_host + derive", out["call_ms"]["b_patches_at_sum_edges_host"]))
        f.write(f"  (b) / (a){'':<49}{b / a:10.1f}\n\n")
        f.write(f"(a) and (b) returned the same bytes: {found['n_edges']} edges, {found['truncated']} calipers truncated at cap {CAP}, "
                f"{found['outside']} leaving the source.\nThe two launches over the same {n * K} rectangles, HIP events around "
                "each launch, in a pass of their own:\n\n")
        for k in kern:
            f.write(row(f"{k} ({info[k]['launches']} launch, {info[k]['bytes'] / 1e6:.1f} MB)", out["kernel_ms"][k]))
        f.write(f"  k_caliper / k_patch_warp{'':<34}{kc / kp:10.2f}\n")


if __name__ == "__main__":
    main()
