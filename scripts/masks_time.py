"""Cost of a template mask on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg, TargetNum 3:
bench.py PARAMS and its synthetic Src7), `--batch` staged sources, an elliptic mask of about 0.7 of the template's area.
Needs a gfx950 device and torch.

All in one run, on one context: k_patch_compare (last_compare, one launch), k_model_inspect (last_inspect against a model
of the batch's own hits, one launch) and k_patch_align (align_last, iters 3: four launches, reported per launch), launch
against launch with the mask enabled and disabled, the two forms alternating call by call, HIP events around each
launch through the existing profile entries (fpm_profile_get FPM_K_COMPARE, fpm_model_profile 2, fpm_align_profile).
Every form is warmed up.  Writes `masks_src7.json` and `README.txt` into `--out-dir`; what an existing README.txt holds
from its line "(Added by hand below this line" on is kept.

`--unmasked-only --tag NAME` measures the launches without a mask alone and writes `unmasked_NAME.json`; with `--repo
DIR` the package and bench.py of another checkout are used (one without the mask entries, too), so that the same launches
of two commits can be run alternately from one shell loop.

    python scripts/masks_time.py [--batch 64] [--reps 5] [--out-dir profiles/masks]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_patch_compare", "k_model_inspect", "k_patch_align")
DISTINCT = 8      # distinct scenes generated on the host; a larger batch repeats them
AXES = 0.944      # the ellipse's half-axes as a fraction of the half-sides: pi / 4 * 0.944^2 = 0.70 of the area


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "masks"))
    ap.add_argument("--repo", default=REPO)
    ap.add_argument("--unmasked-only", action="store_true")
    ap.add_argument("--tag", default="this")
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 runs per form"
    sys.path.insert(0, os.path.abspath(args.repo))

    import numpy as np
    import torch   # noqa: F401  one HIP runtime, loaded before libfpm_hip.so

    import bench
    from fastest_image_pattern_matching_amd import TemplateMatcher, synth
    from fastest_image_pattern_matching_amd import _lib as L

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
    assert m.model_train_last(-1) == n

    forms = ["unmasked"]
    used = tw * th
    if not args.unmasked_only:
        v, u = np.mgrid[0:th, 0:tw].astype(np.float64)
        mask = ((u - (tw - 1) / 2.0) / (AXES * tw / 2.0)) ** 2 + ((v - (th - 1) / 2.0) / (AXES * th / 2.0)) ** 2 <= 1.0
        m.set_mask(mask)
        used = m.mask_info()[2]
        forms.append("masked")

    def launches():
        """{kernel: (ms per launch, launches, bytes)} of one round of the three calls under the profile"""
        m.profile_reset()
        m.last_compare(-1)
        m.last_inspect(-1)
        m.align_last(-1, iters=3)
        out = {"k_patch_compare": m.profile_get(L.K_COMPARE), "k_model_inspect": m.model_profile(L.MODEL_INSPECT),
               "k_patch_align": m.align_profile()}
        return {k: (ms / max(cnt, 1), cnt, nbytes) for k, (ms, cnt, nbytes) in out.items()}

    runs = {f: {k: [] for k in KERNELS} for f in forms}
    info = {f: {} for f in forms}
    m.profile(True)
    for rep in range(args.reps + 1):          # one untimed round first
        for f in forms:
            if not args.unmasked_only:
                m.mask_enable(f == "masked")
            got = launches()
            for k in KERNELS:
                info[f][k] = {"launches": got[k][1], "bytes": got[k][2]}
                if rep >= 1:
                    runs[f][k].append(got[k][0])
    m.profile(False)

    out = {"frame": [w, h], "template": [tw, th], "params": bench.PARAMS, "batch": args.batch, "hits": n, "reps": args.reps,
           "tag": args.tag, "mask_used": used, "mask_fraction": used / float(tw * th),
           "launch_ms": {f: {k: dict(stat(runs[f][k]), **info[f][k]) for k in KERNELS} for f in forms}}
    os.makedirs(args.out_dir, exist_ok=True)
    if args.unmasked_only:
        line = json.dumps(out)
        print(line)
        with open(os.path.join(args.out_dir, f"unmasked_{args.tag}.json"), "w") as f:
            f.write(line + "\n")
        return
    med = {f: {k: statistics.median(runs[f][k]) for k in KERNELS} for f in forms}
    out["masked_over_unmasked"] = {k: med["masked"][k] / med["unmasked"][k] for k in KERNELS}
    # one search's worth of the three tools: one comparison, one inspection and an alignment of iters 3 (four launches)
    per = {"k_patch_compare": 1, "k_model_inspect": 1, "k_patch_align": 4}
    out["all_three_ms"] = {f: sum(per[k] * med[f][k] for k in KERNELS) for f in forms}
    out["mask_cost_ms"] = out["all_three_ms"]["masked"] - out["all_three_ms"]["unmasked"]
    line = json.dumps(out)
    print(line)
    with open(os.path.join(args.out_dir, "masks_src7.json"), "w") as f:
        f.write(line + "\n")
    # what was written by hand below the marker line of an earlier README.txt stays
    readme, marker, kept = os.path.join(args.out_dir, "README.txt"), "(Added by hand below this line", ""
    if os.path.exists(readme):
        old = open(readme).read()
        if marker in old:
            kept = "\n" + old[old.index(marker):]
    with open(readme, "w") as f:
        f.write(f"masks_src7.json: `python scripts/masks_time.py --batch {args.batch} --reps {args.reps}` on one MI355X.\n"
                f"The Src7 configuration ({w} x {h} sources, Dst7 {tw} x {th}, +-180 deg, TargetNum 3), {args.batch} staged sources, "
                f"{n} hits,\nan elliptic mask of {used} of {tw * th} pixels ({used / float(tw * th):.3f}).  HIP events around each "
                f"launch, medians of {args.reps} launches per form,\nthe forms alternating call by call, in parentheses the range:\n\n")
        for k in KERNELS:
            for form in forms:
                s = out["launch_ms"][form][k]
                f.write(f"  {k + ' ' + form:<34}{s['median']:10.4f} ms  ({s['min']:.4f} .. {s['max']:.4f})  {s['bytes'] / s['launches'] / 1e6:8.1f} MB\n")
            f.write(f"  {'masked / unmasked':<34}{out['masked_over_unmasked'][k]:10.3f}\n")
        f.write(f"\nOne comparison, one inspection and one alignment of iters 3 (four launches) over the {n} hits: "
                f"{out['all_three_ms']['unmasked']:.4f} ms of launches\nwithout the mask, {out['all_three_ms']['masked']:.4f} ms with it: "
                f"{out['mask_cost_ms']:+.4f} ms per search of {args.batch} frames.\n")
        f.write(kept)


if __name__ == "__main__":
    main()
