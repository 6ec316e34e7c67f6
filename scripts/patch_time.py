"""Cost of the match patches on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg,
TargetNum 3: bench.py PARAMS and its synthetic Src7), `--batch` staged sources, default rectangle (the template's frame):
every result of the batch turned upright and cropped in one launch.  Needs a gfx950 device and torch.

All in one run, on one context:
  * device_ms of the staged search (fpm_profile_last: events around the whole device pass, graph replay);
  * the device time of the patch launch, k_patch_warp (FPM_PATCH_FORM_TILED) and the k_warp form of the same job list
    (FPM_PATCH_FORM_WARP): HIP events around the launch alone (profiling index patch_warp), one reading per call, the
    two forms alternating call by call;
  * bytes written + footprint bytes read (the index's byte count: 2 x patches x pw x ph) over that time, against the
    HBM roofline;
  * what a consumer on the device sees: torch events on its stream around last_patches_device (job table, launch and
    the two stream waits; no host synchronisation inside).
The two forms' bytes are compared once.  Every form is warmed up; the series is repeated (`--series`) and the spread
reported is that of the series' medians.  Prints one JSON line.

    python scripts/patch_time.py [--batch 64] [--reps 10] [--series 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DISTINCT = 8   # distinct scenes generated on the host; a larger batch repeats them


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
    forms = {"k_patch_warp": L.PATCH_FORM_TILED, "k_warp": L.PATCH_FORM_WARP}

    def spread(series_medians):
        return {"median": statistics.median(series_medians), "min": min(series_medians), "max": max(series_medians),
                "series": series_medians}

    # the two forms' bytes, once
    host = np.zeros((n, ph, pw), np.uint8)
    ref = None
    for name, form in forms.items():
        m.setPatchForm(form)
        host[...] = 0
        m.last_patches(-1, out=host)
        if ref is None:
            ref = host.copy()
            assert ref.any()
        assert np.array_equal(host, ref), name
    del ref

    # ---- the search's device pass -------------------------------------------------------------------------------
    search_ms = []
    for _ in range(args.series):
        d = []
        for _ in range(args.reps):
            m.match_staged_array()
            d.append(m.profile_last()[0])
        search_ms.append(statistics.median(d))

    # ---- the patch launch alone, event-timed ----------------------------------------------------------------------
    m.profile(True)
    launch_ms = {name: [] for name in forms}
    nbytes = 0
    for _ in range(args.series):
        d = {name: [] for name in forms}
        for rep in range(args.reps + 2):
            for name, form in forms.items():
                m.setPatchForm(form)
                m.profile_reset()
                m.last_patches(-1, out=host)
                ms, launches, nbytes = m.profile_get(L.K_PATCH)
                assert launches == 1, launches
                if rep >= 2:   # the first two calls of a series warm up
                    d[name].append(ms)
        for name in forms:
            launch_ms[name].append(statistics.median(d[name]))
    m.profile(False)
    assert nbytes == 2 * n * pw * ph, (nbytes, n, pw, ph)

    # ---- as a consumer on the device sees it ------------------------------------------------------------------------
    dev = torch.empty((n, ph, pw), dtype=torch.uint8, device="cuda:0")
    stream_ms = {name: [] for name in forms}
    for _ in range(args.series):
        d = {name: [] for name in forms}
        for rep in range(args.reps + 2):
            for name, form in forms.items():
                m.setPatchForm(form)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m.last_patches_device(-1, out=dev)
                e1.record()
                e1.synchronize()
                if rep >= 2:
                    d[name].append(e0.elapsed_time(e1))
        for name in forms:
            stream_ms[name].append(statistics.median(d[name]))
    m.setPatchForm(L.PATCH_FORM_TILED)
    assert np.array_equal(dev.cpu().numpy(), host)

    s_med = statistics.median(search_ms)
    out = {"frame": [w, h], "template": [pw, ph], "params": bench.PARAMS, "batch": args.batch, "patches": n,
           "reps": args.reps, "series": args.series, "hbm_peak_gb_per_s": bench.HBM_PEAK_GBS,
           "bytes_per_launch": nbytes, "bytes_definition": "patch pixels written + as many source pixels read",
           "search_device_ms": spread(search_ms), "launch_ms": {}, "consumer_stream_ms": {}}
    for name in forms:
        med = statistics.median(launch_ms[name])
        gbs = nbytes / (med * 1e-3) / 1e9
        out["launch_ms"][name] = dict(spread(launch_ms[name]), gb_per_s=round(gbs, 1),
                                      hbm_frac=round(gbs / bench.HBM_PEAK_GBS, 4),
                                      per_search_ms=med / args.batch, frac_of_search_device_ms=med / s_med)
        out["consumer_stream_ms"][name] = spread(stream_ms[name])
    out["k_warp_over_k_patch_warp"] = (statistics.median(launch_ms["k_warp"]) /
                                       statistics.median(launch_ms["k_patch_warp"]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
