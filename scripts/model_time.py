"""Cost of the variation model on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg,
TargetNum 3: bench.py PARAMS and its synthetic Src7), `--batch` staged sources, the whole template as rectangle: every
result of the batch trained into the model in one launch, and inspected against it in one launch.  Needs a gfx950
device and torch.

All in one run, on one context, HIP events around the launches alone, one reading per call, the forms alternating call
by call:
  (1) train_auto / train_chunk1 / train_chunk_all   k_model_accum over the hits (fpm_model_profile), at the engine's
                                                    chunk and at forced chunks 1 and the hit count
  (2) patch_warp                                    k_patch_warp over the same jobs: the sampling alone
  (4) inspect_raw against compare_raw               k_model_inspect and k_patch_compare over the same jobs
and what a caller can do today, torch events around its device work:
  (3) two_step                                      last_patches_device, then torch reductions to the same S and Q
The two-step's planes are compared with model_sums once.  Every form is warmed up; the series is repeated (`--series`)
and the spread reported is that of the series' medians.  Prints one JSON line.

    python scripts/model_time.py [--batch 64] [--reps 10] [--series 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DISTINCT = 8   # distinct scenes generated on the host; a larger batch repeats them
ABS_THRESHOLD, K = 8, 3.0


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
    px = pw * ph
    host = np.zeros((n, ph, pw), np.uint8)
    dev = torch.empty((n, ph, pw), dtype=torch.uint8, device="cuda:0")

    def spread(series_medians):
        return {"median": statistics.median(series_medians), "min": min(series_medians), "max": max(series_medians),
                "series": series_medians}

    def two_step():
        """The caller's alternative: the patches into device memory, then exact integer reductions there."""
        m.last_patches_device(-1, out=dev)
        i32 = dev.to(torch.int32)
        return i32.sum(0, dtype=torch.int64), (i32 * i32).sum(0, dtype=torch.int64)

    # the ways agree, once: every chunk rule and the two-step give the same planes
    planes = {}
    for name, chunk in (("auto", 0), ("chunk1", 1), ("chunk_all", n)):
        m.model_clear()
        m.model_set_chunk(chunk)
        assert m.model_train_last(-1) == n
        planes[name] = m.model_sums()
    m.model_set_chunk(0)
    ts, tq = (t.cpu().numpy() for t in two_step())
    for name, (s, q) in planes.items():
        assert np.array_equal(s, ts) and np.array_equal(q, tq), name

    def run_train(chunk):
        def run():
            m.model_clear()
            m.model_set_chunk(chunk)
            m.model_train_last(-1)
            return m.model_profile(L.MODEL_TRAIN)
        return run

    def run_warp():
        m.last_patches(-1, out=host)
        return m.profile_get(L.K_PATCH)

    def run_inspect():
        m.last_inspect(-1, ABS_THRESHOLD, K)
        return m.model_profile(L.MODEL_INSPECT)

    def run_compare():
        m.last_compare(-1, threshold=16)
        return m.profile_get(L.K_COMPARE)

    # the last form trains at the engine's chunk, so the inspections of the next round see a complete model; the planes
    # for (ABS_THRESHOLD, K) are prepared anew after each training and timed on their own (fpm_model_profile, prepare)
    forms = {"train_chunk1": run_train(1), "train_chunk_all": run_train(n), "train_auto": run_train(0),
             "patch_warp": run_warp, "inspect_raw": run_inspect, "compare_raw": run_compare}
    m.profile(True)
    launch_ms = {name: [] for name in forms}
    prepare_ms = []
    nbytes = {}
    for _ in range(args.series):
        d = {name: [] for name in forms}
        dp = []
        for rep in range(args.reps + 2):
            for name, run in forms.items():
                m.profile_reset()
                ms, launches, nbytes[name] = run()
                assert launches == 1, (name, launches)
                if rep >= 2:   # the first two calls of a series warm up
                    d[name].append(ms)
                    if name == "inspect_raw":
                        pms, pl, nbytes["prepare"] = m.model_profile(L.MODEL_PREPARE)
                        assert pl == 1
                        dp.append(pms)
        for name in forms:
            launch_ms[name].append(statistics.median(d[name]))
        prepare_ms.append(statistics.median(dp))
    m.profile(False)
    m.model_set_chunk(0)
    assert nbytes["train_auto"] == n * px + 8 * px and nbytes["inspect_raw"] == 3 * n * px, nbytes

    stream_ms = []
    for _ in range(args.series):
        ds = []
        for rep in range(args.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            two_step()
            e1.record()
            e1.synchronize()
            if rep >= 2:
                ds.append(e0.elapsed_time(e1))
        stream_ms.append(statistics.median(ds))

    def ratio(a, b):
        return {"median": statistics.median(a) / statistics.median(b), "series": [x / y for x, y in zip(a, b)]}

    out = {"frame": [w, h], "template": [pw, ph], "params": bench.PARAMS, "batch": args.batch, "hits": n,
           "abs_threshold": ABS_THRESHOLD, "k": K, "reps": args.reps, "series": args.series,
           "hbm_peak_gb_per_s": bench.HBM_PEAK_GBS,
           "bytes_definition": {"train": "source pixels read + plane bytes written",
                                "prepare": "plane bytes in and out",
                                "inspect": "source pixels read + lo and hi read (+ excess pixels written)"},
           "launch_ms": {}, "prepare_ms": dict(spread(prepare_ms), bytes=nbytes["prepare"]),
           "two_step_stream_ms": spread(stream_ms)}
    for name in forms:
        med = statistics.median(launch_ms[name])
        gbs = nbytes[name] / (med * 1e-3) / 1e9
        out["launch_ms"][name] = dict(spread(launch_ms[name]), bytes=nbytes[name], gb_per_s=round(gbs, 1),
                                      hbm_frac=round(gbs / bench.HBM_PEAK_GBS, 4))
    for name in ("train_auto", "train_chunk1", "train_chunk_all"):
        out[name + "_over_patch_warp"] = ratio(launch_ms[name], launch_ms["patch_warp"])
    out["two_step_stream_over_train_auto"] = ratio(stream_ms, launch_ms["train_auto"])
    out["inspect_raw_over_compare_raw"] = ratio(launch_ms["inspect_raw"], launch_ms["compare_raw"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
