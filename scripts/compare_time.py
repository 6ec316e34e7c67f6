"""Cost of the patch comparison on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg,
TargetNum 3: bench.py PARAMS and its synthetic Src7), `--batch` staged sources, the whole template as rectangle: every
result of the batch compared with the template in one launch.  Needs a gfx950 device and torch.

All in one run, on one context:
  * device_ms of the staged search (fpm_profile_last: events around the whole device pass, graph replay);
  * HIP events around the launches alone, one reading per call, the forms alternating call by call:
      compare_raw   the one launch of last_compare (profiling index patch_compare)
      patch_warp    k_patch_warp over the same jobs (last_patches; profiling index patch_warp)
      compare_norm  the two launches of last_compare(normalize=True), summed
  * what a caller waits for, host clock around the whole call, in the same alternation:
      compare_raw_call / compare_norm_call   last_compare (job table, launches, the copy of the records; the normalised
                                             call also its copy of the sums to the host and of the tables back)
      two_step_call                          what a caller can do today: last_patches_device, then torch reductions on the
                                             device for the same five sums, sum |I - T|, max and the count over the
                                             threshold (no bounding box), and their copy to the host
    and torch events around the two-step's device work (two_step_stream).
The two-step's numbers are compared with last_compare's once.  Every form is warmed up; the series is repeated
(`--series`) and the spread reported is that of the series' medians.  Prints one JSON line.

    python scripts/compare_time.py [--batch 64] [--reps 10] [--series 3] [--out FILE]
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
THRESHOLD = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from fastest_image_pattern_matching_amd import TemplateMatcher, synth
    from fastest_image_pattern_matching_amd import _lib as L

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
    host = np.zeros((n, ph, pw), np.uint8)
    dev = torch.empty((n, ph, pw), dtype=torch.uint8, device="cuda:0")
    t32 = torch.from_numpy(templ.astype(np.int32)).to("cuda:0")

    def spread(series_medians):
        return {"median": statistics.median(series_medians), "min": min(series_medians), "max": max(series_medians),
                "series": series_medians}

    def two_step():
        """The caller's alternative: the patches into device memory, then exact integer reductions there."""
        m.last_patches_device(-1, out=dev)
        i32 = dev.to(torch.int32)
        d = (i32 - t32).abs()
        cols = [i32.sum((1, 2), dtype=torch.int64), (i32 * i32).sum((1, 2), dtype=torch.int64),
                (i32 * t32).sum((1, 2), dtype=torch.int64), d.sum((1, 2), dtype=torch.int64),
                d.amax((1, 2)).to(torch.int64), (d > THRESHOLD).sum((1, 2), dtype=torch.int64)]
        return torch.stack(cols, 1)

    # the two ways agree, once
    stats = m.last_compare(-1, threshold=THRESHOLD)
    ts = two_step().cpu().numpy()
    for k, f in enumerate(("sum_i", "sum_ii", "sum_it", "sum_abs", "max_abs", "n_over")):
        assert np.array_equal(ts[:, k], stats[f].astype(np.int64)), f
    assert (stats["sum_t"] == int(templ.astype(np.int64).sum())).all()

    # ---- the search's device pass -------------------------------------------------------------------------------
    search_ms = []
    for _ in range(args.series):
        d = []
        for _ in range(args.reps):
            m.match_staged_array()
            d.append(m.profile_last()[0])
        search_ms.append(statistics.median(d))

    # ---- the launches alone (HIP events) and the calls (host clock), alternating --------------------------------
    def run_raw():
        m.last_compare(-1, threshold=THRESHOLD)
        return m.profile_get(L.K_COMPARE)

    def run_norm():
        m.last_compare(-1, threshold=THRESHOLD, normalize=True)
        return m.profile_get(L.K_COMPARE)

    def run_warp():
        m.last_patches(-1, out=host)
        return m.profile_get(L.K_PATCH)

    launch_forms = {"compare_raw": (run_raw, 1), "patch_warp": (run_warp, 1), "compare_norm": (run_norm, 2)}
    m.profile(True)
    launch_ms = {name: [] for name in launch_forms}
    nbytes = {}
    for _ in range(args.series):
        d = {name: [] for name in launch_forms}
        for rep in range(args.reps + 2):
            for name, (run, want) in launch_forms.items():
                m.profile_reset()
                ms, launches, nbytes[name] = run()
                assert launches == want, (name, launches)
                if rep >= 2:   # the first two calls of a series warm up
                    d[name].append(ms)
        for name in launch_forms:
            launch_ms[name].append(statistics.median(d[name]))
    m.profile(False)
    assert nbytes["compare_raw"] == 2 * n * pw * ph and nbytes["compare_norm"] == 4 * n * pw * ph, nbytes

    def call_two_step():
        two_step().cpu()

    call_forms = {"compare_raw_call": lambda: m.last_compare(-1, threshold=THRESHOLD),
                  "compare_norm_call": lambda: m.last_compare(-1, threshold=THRESHOLD, normalize=True),
                  "two_step_call": call_two_step}
    call_ms = {name: [] for name in call_forms}
    stream_ms = []
    for _ in range(args.series):
        d = {name: [] for name in call_forms}
        ds = []
        for rep in range(args.reps + 2):
            for name, run in call_forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                t1 = time.perf_counter()
                if rep >= 2:
                    d[name].append((t1 - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            two_step()
            e1.record()
            e1.synchronize()
            if rep >= 2:
                ds.append(e0.elapsed_time(e1))
        for name in call_forms:
            call_ms[name].append(statistics.median(d[name]))
        stream_ms.append(statistics.median(ds))

    s_med = statistics.median(search_ms)
    raw, warp = statistics.median(launch_ms["compare_raw"]), statistics.median(launch_ms["patch_warp"])
    out = {"frame": [w, h], "template": [pw, ph], "params": bench.PARAMS, "batch": args.batch, "hits": n,
           "threshold": THRESHOLD, "reps": args.reps, "series": args.series, "hbm_peak_gb_per_s": bench.HBM_PEAK_GBS,
           "bytes_definition": "source pixels read + template pixels read (+ difference pixels written), per launch",
           "search_device_ms": spread(search_ms), "launch_ms": {}, "call_ms": {}, "two_step_stream_ms": spread(stream_ms)}
    for name in launch_forms:
        med = statistics.median(launch_ms[name])
        gbs = nbytes[name] / (med * 1e-3) / 1e9
        out["launch_ms"][name] = dict(spread(launch_ms[name]), bytes=nbytes[name], gb_per_s=round(gbs, 1),
                                      hbm_frac=round(gbs / bench.HBM_PEAK_GBS, 4), per_search_ms=med / args.batch,
                                      frac_of_search_device_ms=med / s_med)
    for name in call_forms:
        out["call_ms"][name] = spread(call_ms[name])
    out["compare_raw_over_patch_warp"] = {"median": raw / warp,
                                          "series": [a / b for a, b in zip(launch_ms["compare_raw"], launch_ms["patch_warp"])]}
    out["two_step_stream_over_compare_raw_launch"] = statistics.median(stream_ms) / raw
    out["two_step_call_over_compare_raw_call"] = (statistics.median(call_ms["two_step_call"]) /
                                                  statistics.median(call_ms["compare_raw_call"]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
