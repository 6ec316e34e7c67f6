"""Device time of fast mode (Params.stop_layer) against the normal search on the Src7 configuration (bench.py PARAMS):
a staged batch and a lone search, two contexts over the same sources called in turn, `fpm_profile_last` device_ms.
Also the per-kernel launch counts of one eager pass of each (fast mode launches a subset of the normal pass's kernels)
and the time of k_bitwise_not over the batch.  Prints one JSON line; needs a gfx950 device.

    python scripts/fast_mode_time.py [--batch 64] [--reps 30] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import bench
    from fastest_image_pattern_matching_amd import TemplateMatcher, synth
    from fastest_image_pattern_matching_amd import _lib as L

    templ = synth.load_templates()["Dst7"]
    sources = bench.make_sources(templ, args.batch, 7)

    def matcher(stop):
        m = TemplateMatcher(0)
        for k, v in bench.PARAMS.items():
            setattr(m._params, k, v)
        m.setStopLayer1(bool(stop))
        assert m.learnPattern(templ)
        return m

    ms = {0: matcher(0), 1: matcher(1)}
    out = {"batch": args.batch, "reps": args.reps, "params": bench.PARAMS}

    def series(call):
        """device_ms of `reps` calls per mode, the two modes in turn, after two warm calls each."""
        t = {0: [], 1: []}
        for stop in (0, 1):
            for _ in range(2):
                call(ms[stop])
        for _ in range(args.reps):
            for stop in (0, 1):
                call(ms[stop])
                t[stop].append(ms[stop].profile_last()[0])
        return t

    def summary(t):
        med = {s: statistics.median(v) for s, v in t.items()}
        return {"normal_ms": {"median": med[0], "min": min(t[0]), "max": max(t[0])},
                "fast_ms": {"median": med[1], "min": min(t[1]), "max": max(t[1])},
                "fast_over_normal": med[1] / med[0]}

    for m in ms.values():
        m.stage(sources)
    out["batch_device"] = summary(series(lambda m: m.match_staged_array()))
    counts = {s: [int(c) for c in ms[s].match_staged_array()[0]] for s in (0, 1)}
    out["results_per_source"] = {"normal": sorted(set(counts[0])), "fast": sorted(set(counts[1]))}
    out["search_stats"] = {"normal": ms[0].search_stats(), "fast": ms[1].search_stats()}

    # one eager pass each: launches and time per kernel
    kern = {}
    for stop, name in ((0, "normal"), (1, "fast")):
        m = ms[stop]
        m.profile(True)
        m.match_staged_array()
        m.profile_reset()
        m.match_staged_array()
        kern[name] = {n: {"launches": m.profile_get(k)[1], "ms": round(m.profile_get(k)[0], 4)}
                      for k, n in enumerate(L.KERNEL_NAMES) if m.profile_get(k)[1]}
        m.profile(False)
    out["eager_pass_kernels"] = kern
    out["fast_launches_subset"] = all(kern["fast"][n]["launches"] <= kern["normal"].get(n, {"launches": 0})["launches"]
                                      for n in kern["fast"])

    # k_bitwise_not over the staged batch: the first pass after the switch flips carries the launch
    m = ms[0]
    m.profile(True)
    nots = []
    for rep in range(6):
        m.setBitwiseNot(rep % 2 == 0)
        m.profile_reset()
        m.match_staged_array()
        ms_, n, b = m.profile_get(L.K_NOT)
        assert n == 1
        nots.append(ms_)
    m.setBitwiseNot(False)
    m.profile(False)
    out["bitwise_not_kernel"] = {"ms": nots, "bytes": b, "median_gb_per_s": b / statistics.median(nots) / 1e6}

    out["lone_device"] = summary(series(lambda m: m.match(sources[0])))

    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
