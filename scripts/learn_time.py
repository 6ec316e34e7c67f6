"""Cost of learning a template: fpm_learn from a host array against fpm_learn_device from a tensor of the same pixels,
for the Dst7 template (762 x 521, bench.py's) and a 64 x 64 one (the centre of Dst7).  Needs a gfx950 device and torch.

All in one run, on one context per size, the two entries alternating call by call:
  * what a caller waits for, host clock around the whole call:
      learn_host_call     learnPattern(array): upload, pyramid, every level back to the host, three host passes over
                          all pixels, two blocking uploads of the operands
      learn_device_call   learn_device(tensor): the staging kernel, pyramid, k_tmpl_prep, the sums and the top level
                          back, one synchronisation
  * HIP events around the one launch of k_tmpl_prep (profiling index tmpl_prep), in a second alternation with the
    kernel timing on.
The two templates are compared once (levels, statistics, operands: equal).  Every form is warmed up; the series is
repeated (`--series`) and the spread reported is that of the series' medians.  Prints one JSON line.

    python scripts/learn_time.py [--reps 10] [--series 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from fastest_image_pattern_matching_amd import TemplateMatcher, synth
    from fastest_image_pattern_matching_amd import _lib as L

    dst7 = synth.load_templates()["Dst7"]
    th, tw = dst7.shape
    small = np.ascontiguousarray(dst7[th // 2 - 32:th // 2 + 32, tw // 2 - 32:tw // 2 + 32])
    templates = {"dst7_762x521": dst7, "centre_64x64": small}

    def spread(series_medians):
        return {"median": statistics.median(series_medians), "min": min(series_medians), "max": max(series_medians),
                "series": series_medians}

    def state(m):
        n, border = m.template_info()
        t8, tsum = m.template_operands()
        levels = [m.template_level(l) for l in range(n)]
        return (n, border, [(px.tobytes(), a, b, c, d) for px, a, b, c, d in levels], t8.tobytes(), tsum.tobytes())

    out = {"params": bench.PARAMS, "reps": args.reps, "series": args.series, "hbm_peak_gb_per_s": bench.HBM_PEAK_GBS,
           "bytes_definition": "template pixels read + operand bytes (slack included) and row sums written",
           "templates": {}}
    for name, t in templates.items():
        m = TemplateMatcher(0)
        for k, v in bench.PARAMS.items():
            setattr(m._params, k, v)
        dev = torch.from_numpy(t).to("cuda:0")
        torch.cuda.synchronize()

        # the two ways agree, once
        assert m.learnPattern(t)
        host_state = state(m)
        m.learn_device(dev)
        assert state(m) == host_state, name

        forms = {"learn_host_call": lambda: m.learnPattern(t), "learn_device_call": lambda: m.learn_device(dev)}
        call_ms = {f: [] for f in forms}
        for _ in range(args.series):
            d = {f: [] for f in forms}
            for rep in range(args.reps + 2):
                for f, run in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run()
                    t1 = time.perf_counter()
                    if rep >= 2:   # the first two calls of a series warm up
                        d[f].append((t1 - t0) * 1e3)
            for f in forms:
                call_ms[f].append(statistics.median(d[f]))

        # the launch alone, the host learn still alternating with it
        m.profile(True)
        launch_ms, nbytes = [], 0
        for _ in range(args.series):
            d = []
            for rep in range(args.reps + 2):
                m.learnPattern(t)
                m.profile_reset()
                m.learn_device(dev)
                ms, launches, nbytes = m.profile_get(L.K_LEARN)
                assert launches == 1, launches
                if rep >= 2:
                    d.append(ms)
            launch_ms.append(statistics.median(d))
        m.profile(False)

        host, device = statistics.median(call_ms["learn_host_call"]), statistics.median(call_ms["learn_device_call"])
        med = statistics.median(launch_ms)
        gbs = nbytes / (med * 1e-3) / 1e9
        out["templates"][name] = {
            "size": [int(t.shape[1]), int(t.shape[0])], "levels": m.template_info()[0],
            "call_ms": {f: spread(call_ms[f]) for f in forms},
            "host_over_device": {"median": host / device,
                                 "series": [a / b for a, b in zip(call_ms["learn_host_call"], call_ms["learn_device_call"])]},
            "tmpl_prep_launch_ms": dict(spread(launch_ms), bytes=nbytes, gb_per_s=round(gbs, 2),
                                        hbm_frac=round(gbs / bench.HBM_PEAK_GBS, 5)),
        }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
