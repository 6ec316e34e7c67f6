"""Cost of the sub-pattern locators on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg,
TargetNum 3: bench.py PARAMS and its synthetic Src7), `--batch` staged sources, 8 features of 64 x 64 with rx = ry = 8.
Needs a gfx950 device and torch.

All in one run, on one context.  Launch against launch (HIP events around each launch, the forms alternating call by
call, medians of `--reps`):
  k_patch_locate over all (hit, feature) jobs against k_patch_warp over the same 8 windows per hit (8 launches of
      patches_at, one per window rectangle, summed): the sampling floor.
To the caller (host clock; each call returns with its results in the caller's arrays), the forms alternating:
  (a) last_locate()
  (b) last_patches_device of the 8 windows + the same integers in torch (unfold, int64 sums) + the copy to the host:
      what a caller has today
(a) and (b) are compared once: the same sums at every offset.

    python scripts/locate_time.py [--batch 64] [--reps 5] [--out-dir profiles/locate]
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
SIDE, RADIUS = 64, 8


def stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "runs": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "locate"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 runs per form"

    import numpy as np
    import torch   # one HIP runtime, loaded before libfpm_hip.so

    import bench
    from fastest_image_pattern_matching_amd import _lib as L
    from fastest_image_pattern_matching_amd import TemplateMatcher, synth
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
    results = m.match_staged()
    n = sum(len(rs) for rs in results)
    idx = np.repeat(np.arange(args.batch, dtype=np.int32), bench.PARAMS["max_pos"])
    lts = [r.ptLT for rs in results for r in rs]
    angs = [r.dMatchedAngle for rs in results for r in rs]
    # 8 features spread over the template, x of every residue mod 4
    origins = [(40 + 84 * k + k % 4, 30 + 110 * (k % 4)) for k in range(8)]
    feats = np.array([M.feature(x, y, SIDE, SIDE, RADIUS) for x, y in origins], M.FEATURE_DTYPE)
    windows = [(x - RADIUS, y - RADIUS, SIDE + 2 * RADIUS, SIDE + 2 * RADIUS) for x, y in origins]
    assert all(x + SIDE <= tw and y + SIDE <= th for x, y in origins)

    # ---- launch against launch --------------------------------------------------------------------------------------
    def warp8():
        for r in windows:
            m.patches_at(idx, lts, angs, rect=r)

    forms = {"k_patch_locate": (lambda: m.locate_at(idx, lts, angs, feats), m.locate_profile, 1),
             "k_patch_warp_8_windows": (warp8, lambda: m.profile_get(L.K_PATCH), 8)}
    kernel_ms = {name: [] for name in forms}
    info = {}
    m.profile(True)
    for rep in range(args.reps + 1):
        for name, (run, read, launches) in forms.items():
            m.profile_reset()
            run()
            t, ln, nbytes = read()
            assert ln == launches, (name, ln)
            info[name] = {"launches": ln, "bytes": nbytes}
            if rep >= 1:
                kernel_ms[name].append(t)
    m.profile(False)
    kernels = {k: dict(stat(v), **info[k]) for k, v in kernel_ms.items()}

    # ---- to the caller ----------------------------------------------------------------------------------------------
    t0 = templ.astype(np.int32)
    regions = [torch.from_numpy(np.ascontiguousarray(t0[y:y + SIDE, x:x + SIDE])).cuda() for x, y in origins]

    def form_a():
        return m.last_locate(feats, source=-1, maps=True)

    def form_b():
        out = []
        for r, T in zip(windows, regions):
            p = m.last_patches_device(source=-1, rect=r)
            p = p if isinstance(p, torch.Tensor) else p[0]
            u = p.to(torch.int32).unfold(1, SIDE, 1).unfold(2, SIDE, 1)          # (n, 17, 17, 64, 64)
            out.append(torch.stack([u.sum((3, 4), dtype=torch.int64), (u * u).sum((3, 4), dtype=torch.int64),
                                    (u * T).sum((3, 4), dtype=torch.int64)], 1))
        return torch.stack(out, 1).cpu().numpy()                                 # (n, 8, 3, 17, 17)

    res, maps = form_a()
    assert np.array_equal(maps.reshape(n, 8, 3, 2 * RADIUS + 1, 2 * RADIUS + 1), form_b()), "the sums of (a) and (b) differ"
    call_ms = {"a_last_locate": [], "b_patches_device_torch": []}
    for rep in range(args.reps + 1):
        for name, run in (("a_last_locate", lambda: m.last_locate(feats, source=-1)), ("b_patches_device_torch", form_b)):
            t = time.perf_counter()
            run()
            if rep >= 1:
                call_ms[name].append((time.perf_counter() - t) * 1e3)
    out = {"frame": [w, h], "template": [tw, th], "params": bench.PARAMS, "batch": args.batch, "hits": n, "reps": args.reps,
           "features": [list(map(int, (x, y, SIDE, SIDE, RADIUS, RADIUS))) for x, y in origins],
           "kernel_ms": kernels, "call_ms": {k: stat(v) for k, v in call_ms.items()},
           "locate_over_warp": kernels["k_patch_locate"]["median"] / kernels["k_patch_warp_8_windows"]["median"],
           "found": {"score_min": float(res["score"].min()), "score_median": float(np.median(res["score"])),
                     "offset_max": float(np.hypot(res["ox"], res["oy"]).max()),
                     "flags": sorted(set(res["flags"].reshape(-1).tolist()))}}
    os.makedirs(args.out_dir, exist_ok=True)
    line = json.dumps(out)
    print(line)
    with open(os.path.join(args.out_dir, "locate_src7.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
