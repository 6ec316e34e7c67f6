"""Cost of the pose alignment on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg,
TargetNum 3: bench.py PARAMS and its synthetic Src7), `--batch` staged sources, the whole template as rectangle: every
result of the batch aligned against the template.  Needs a gfx950 device and torch.

All in one run, on one context, the forms alternating call by call:
  * HIP events around the launches alone, one reading per call:
      compare_raw   the one launch of last_compare (profiling index patch_compare)
      align         k_patch_align, per launch: the four launches of align_last(iters=3), divided by four
  * what a caller waits for, host clock around the whole call:
      align_call     align_last(iters=3): four job tables, launches and copies of the records, three host solves
      two_step_call  ONE iteration of what a caller can do today: last_patches_device, then torch on the device --
                     r = I - T and the four per-hit reductions g_x, g_y, g_t, ssd against the template's central
                     differences -- and their copy to the host.  The seven sums of the normal matrix depend on the
                     template alone there and are computed once, outside the timing: the baseline is given every
                     advantage.
    and torch events around the two-step's device work (two_step_stream).
The two-step's integers are compared with the kernel's once, at the poses of the search.  Every form is warmed up; the
series is repeated (`--series`) and the spread reported is that of the series' medians.  Prints one JSON line.

    python scripts/align_time.py [--batch 64] [--reps 10] [--series 3] [--iters 3] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
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
    dev = torch.empty((n, ph, pw), dtype=torch.uint8, device="cuda:0")

    # the template's side of the sums, on the device: central differences, the used mask, Jt
    t64 = torch.from_numpy(templ.astype(np.int64)).to("cuda:0")
    tx, ty = torch.zeros_like(t64), torch.zeros_like(t64)
    tx[1:-1, 1:-1] = t64[1:-1, 2:] - t64[1:-1, :-2]
    ty[1:-1, 1:-1] = t64[2:, 1:-1] - t64[:-2, 1:-1]
    used = torch.zeros_like(t64)
    used[1:-1, 1:-1] = 1
    X = (2 * torch.arange(pw, device="cuda:0", dtype=torch.int64) - (pw - 1))[None, :]
    Y = (2 * torch.arange(ph, device="cuda:0", dtype=torch.int64) - (ph - 1))[:, None]
    jt = X * ty - Y * tx
    t32, tx32, ty32, jt32, used32 = (v.to(torch.int32) for v in (t64, tx, ty, jt, used))   # |Jt| < 255 * 1283 fits
    h_const = [int(v) for v in (used.sum(), (tx * tx).sum(), (tx * ty).sum(), (ty * ty).sum(), (tx * jt).sum(),
                                (ty * jt).sum(), (jt * jt).sum())]

    def spread(series_medians):
        return {"median": statistics.median(series_medians), "min": min(series_medians), "max": max(series_medians),
                "series": series_medians}

    def two_step():
        """One iteration's device work of the caller's alternative: the patches, then the four per-hit reductions."""
        m.last_patches_device(-1, out=dev)
        r = (dev.to(torch.int32) - t32) * used32
        cols = [(r * tx32).sum((1, 2), dtype=torch.int64), (r * ty32).sum((1, 2), dtype=torch.int64),
                (r.to(torch.int64) * jt).sum((1, 2)), (r * r).sum((1, 2), dtype=torch.int64)]
        return torch.stack(cols, 1)

    # the two ways agree, once: the kernel's records at the raw poses of the search (a step limit nothing passes makes
    # align_last hand the start poses back)
    start = m.align_last(-1, iters=1, max_step=1e-9)
    assert (start["best_eval"] == 0).all()
    idx = np.repeat(np.arange(args.batch), counts)
    sums = m.align_sums_at(idx, np.stack([start["lt_x"], start["lt_y"]], 1), start["angle"])
    ts = two_step().cpu().numpy()
    for k, f in enumerate(("g_x", "g_y", "g_t", "ssd")):
        assert np.array_equal(ts[:, k], sums[f]), f
    for k, f in enumerate(("n_used", "h_xx", "h_xy", "h_yy", "h_xt", "h_yt", "h_tt")):
        assert (sums[f] == h_const[k]).all(), f

    # ---- the launches alone (HIP events), alternating -----------------------------------------------------------
    def run_raw():
        m.last_compare(-1)
        return m.profile_get(L.K_COMPARE)

    def run_align():
        m.align_last(-1, iters=args.iters)
        ms, launches, nbytes = m.align_profile()
        return ms / launches, launches - args.iters, nbytes // launches

    launch_forms = {"compare_raw": run_raw, "align": run_align}
    m.profile(True)
    launch_ms = {name: [] for name in launch_forms}
    nbytes = {}
    for _ in range(args.series):
        d = {name: [] for name in launch_forms}
        for rep in range(args.reps + 2):
            for name, run in launch_forms.items():
                m.profile_reset()
                ms, launches, nbytes[name] = run()
                assert launches == 1, (name, launches)
                if rep >= 2:   # the first two calls of a series warm up
                    d[name].append(ms)
        for name in launch_forms:
            launch_ms[name].append(statistics.median(d[name]))
    m.profile(False)
    assert nbytes["compare_raw"] == nbytes["align"] == 2 * n * pw * ph, nbytes

    # ---- the calls (host clock), alternating ---------------------------------------------------------------------
    call_forms = {"align_call": lambda: m.align_last(-1, iters=args.iters), "two_step_call": lambda: two_step().cpu()}
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

    res = m.align_last(-1, iters=args.iters)
    raw, aln = statistics.median(launch_ms["compare_raw"]), statistics.median(launch_ms["align"])
    out = {"frame": [w, h], "template": [pw, ph], "params": bench.PARAMS, "batch": args.batch, "hits": n,
           "iters": args.iters, "reps": args.reps, "series": args.series, "hbm_peak_gb_per_s": bench.HBM_PEAK_GBS,
           "bytes_definition": "source pixels read + template pixels read, per launch",
           "launch_ms": {}, "call_ms": {}, "two_step_stream_ms": spread(stream_ms)}
    for name in launch_forms:
        med = statistics.median(launch_ms[name])
        gbs = nbytes[name] / (med * 1e-3) / 1e9
        out["launch_ms"][name] = dict(spread(launch_ms[name]), bytes=nbytes[name], gb_per_s=round(gbs, 1),
                                      hbm_frac=round(gbs / bench.HBM_PEAK_GBS, 4))
    for name in call_forms:
        out["call_ms"][name] = spread(call_ms[name])
    out["align_over_compare_raw"] = {"median": aln / raw,
                                     "series": [a / b for a, b in zip(launch_ms["align"], launch_ms["compare_raw"])]}
    out["two_step_stream_over_align_launch"] = statistics.median(stream_ms) / aln
    out["two_step_call_per_iteration_over_align_call_per_evaluation"] = (
        statistics.median(call_ms["two_step_call"]) / (statistics.median(call_ms["align_call"]) / (args.iters + 1)))
    out["result"] = {"ssd_start_sum": int(res["ssd_start"].sum()), "ssd_sum": int(res["ssd"].sum()),
                     "improved": int((res["best_eval"] > 0).sum()), "clamped": int((res["flags"] & 2 != 0).sum()),
                     "singular": int((res["flags"] & 1 != 0).sum())}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
