"""Cost of edge probes on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg, TargetNum 3:
bench.py PARAMS and its synthetic Src7), `--batch` staged sources, 1024 probes of 24 x 5 samples, half 2, taught along
the template's own contour (contour_probes).  Needs a gfx950 device and torch.

All in one run, on one context, both forms timed to the caller by the host clock (each call returns after its device
work is synchronised and its results are in the caller's arrays), the forms alternating call by call:
  (a) last_probes()                           one launch of k_probe, one job-table entry per hit and one per probe
  (b) the form a caller had before            last_calipers in 16 calls of 64 calipers of the same length, width, half
                                              and directions, then the NEAREST select rule on the host
(b)'s pixels differ from (a)'s in the last bits because the pose convention differs (a caliper rounds a per-caliper
ptLT to f32 and samples at cos(angle + phi); a probe composes the hit's matrix with its frame), so the two are
compared by their counts of found edges, not by bytes.  In a pass of their own (HIP events around each launch) k_probe
is held against the sum of the 16 k_caliper launches, with the job-table bytes of both.  Every form is warmed up.
Writes `probes_src7.json` and `README.txt` into `--out-dir`.

    python scripts/probes_time.py [--batch 64] [--reps 5] [--out-dir profiles/probes]
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
N_PROBES, LENGTH, WIDTH, HALF, CONTRAST = 1024, 24, 5, 2, 12
CALS_PER_CALL, CAP = 64, 16
PATCH_JOB_BYTES, PROBE_FRAME_BYTES, CALIPER_JOB_BYTES = 64, 32, 96   # sizeof PatchJob, ProbeFrame, CaliperJob (fpm_kernels.h)


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


def round_up(a, b):
    return -(-a // b) * b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "probes"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 runs per form"

    import numpy as np
    import torch   # noqa: F401  one HIP runtime, loaded before libfpm_hip.so

    import bench
    from fastest_image_pattern_matching_amd import TemplateMatcher, synth
    from fastest_image_pattern_matching_amd import _lib as L
    from fastest_image_pattern_matching_amd import matcher as M

    templ = synth.load_templates()["Dst7"]
    scenes = bench.make_sources(templ, min(DISTINCT, args.batch), 7)
    h, w = scenes[0].shape
    th, tw = templ.shape
    for step in (4.0, 3.0, 2.0, 1.0):
        contour = M.contour_probes(templ, step, 20.0)
        if len(contour) >= N_PROBES:
            break
    assert len(contour) >= N_PROBES, f"the template's contour gives {len(contour)} probes"
    probes = np.ascontiguousarray(contour[np.linspace(0, len(contour) - 1, N_PROBES).astype(np.int64)])
    params = M.probe_params(LENGTH, WIDTH, HALF, CONTRAST, 0, "nearest")

    m = TemplateMatcher(0)
    for k, v in bench.PARAMS.items():
        setattr(m._params, k, v)
    assert m.learnPattern(templ)
    m.stage([scenes[i % len(scenes)] for i in range(args.batch)])
    counts, _ = m.match_staged_array()
    assert counts.tolist() == [bench.PARAMS["max_pos"]] * args.batch, counts.tolist()
    n = int(counts.sum())

    def form_a():
        return m.last_probes(probes, params, source=-1)

    cals = np.zeros(N_PROBES, M.CALIPER_DTYPE)
    cals["cx"], cals["cy"], cals["phi"] = probes["x"], probes["y"], probes["phi"]
    cals["length"], cals["width"], cals["half"], cals["contrast"] = LENGTH, WIDTH, HALF, CONTRAST

    def form_b():
        """(index [n, N_PROBES], n_edges): the caliper nearest the centre of every (hit, probe), 0 = none"""
        index = np.zeros((n, N_PROBES), np.int32)
        n_edges = np.zeros((n, N_PROBES), np.int32)
        for c0 in range(0, N_PROBES, CALS_PER_CALL):
            summary, edges = m.last_calipers(cals[c0:c0 + CALS_PER_CALL], source=-1, cap=CAP)
            i = edges["index"].astype(np.int64)
            key = np.where(np.arange(CAP)[None, None, :] < summary["n_returned"][:, :, None], np.abs(2 * i - LENGTH) * 128 + i,
                           np.iinfo(np.int64).max)
            best = np.argmin(key, axis=2)
            pick = np.take_along_axis(i, best[:, :, None], axis=2)[:, :, 0]
            index[:, c0:c0 + CALS_PER_CALL] = np.where(summary["n_returned"] > 0, pick, 0)
            n_edges[:, c0:c0 + CALS_PER_CALL] = summary["n_edges"]
        return index, n_edges

    summary_a, results_a = form_a()
    index_b, n_edges_b = form_b()
    found = {"a_found": int(summary_a["n_found"].sum()), "b_found": int((index_b > 0).sum()),
             "a_ambiguous": int(summary_a["n_ambiguous"].sum()), "b_ambiguous": int((n_edges_b > 1).sum()),
             "a_outside": int(summary_a["n_outside"].sum()), "same_index": int((results_a["index"] == index_b).sum()),
             "probes": n * N_PROBES}
    call_ms = alternate({"a_last_probes": form_a, "b_16_last_calipers_select_on_host": form_b}, args.reps)

    # launch against launch, in a pass of its own
    kern = {"k_probe": [], "k_caliper_x16": []}
    info = {}
    m.profile(True)
    for rep in range(args.reps + 1):
        for name in kern:
            m.profile_reset()
            if name == "k_probe":
                form_a()
                ms, launches, nbytes = m.probe_profile()
            else:
                form_b()
                ms, launches, nbytes = m.caliper_profile()
            info[name] = {"launches": launches, "bytes": nbytes}
            if rep >= 1:
                kern[name].append(ms)
    m.profile(False)
    assert info["k_probe"]["launches"] == 1 and info["k_caliper_x16"]["launches"] == N_PROBES // CALS_PER_CALL
    table = {"k_probe": round_up(PATCH_JOB_BYTES * n + PROBE_FRAME_BYTES * N_PROBES, 256),
             "k_caliper_x16": (N_PROBES // CALS_PER_CALL) * round_up(CALIPER_JOB_BYTES * n * CALS_PER_CALL, 256)}

    a, b = statistics.median(call_ms["a_last_probes"]), statistics.median(call_ms["b_16_last_calipers_select_on_host"])
    kp, kc = statistics.median(kern["k_probe"]), statistics.median(kern["k_caliper_x16"])
    out = {"frame": [w, h], "template": [tw, th], "params": bench.PARAMS, "batch": args.batch, "hits": n, "probes": N_PROBES,
           "probe": {"length": LENGTH, "width": WIDTH, "half": HALF, "contrast": CONTRAST, "select": "nearest",
                     "contour_step": step, "contour_points": int(len(contour))},
           "reps": args.reps, "found": found, "call_ms": {k: stat(x) for k, x in call_ms.items()}, "b_over_a": b / a,
           "kernel_ms": {k: dict(stat(x), **info[k]) for k, x in kern.items()}, "k_caliper_x16_over_k_probe": kc / kp,
           "job_table_bytes": table}
    os.makedirs(args.out_dir, exist_ok=True)
    line = json.dumps(out)
    print(line)
    with open(os.path.join(args.out_dir, "probes_src7.json"), "w") as f:
        f.write(line + "\n")

    def row(label, s, extra=""):
        return f"  {label:<58}{s['median']:10.3f} ms  ({s['min']:.3f} .. {s['max']:.3f}){extra}\n"

    with open(os.path.join(args.out_dir, "README.txt"), "w") as f:
        f.write(f"probes_src7.json: `python scripts/probes_time.py --batch {args.batch} --reps {args.reps}` on one MI355X.\n"
                f"The Src7 configuration ({w} x {h} sources, Dst7 {tw} x {th}, +-180 deg, TargetNum 3), {args.batch} staged sources, "
                f"{n} hits,\n{N_PROBES} probes of {LENGTH} x {WIDTH} samples, half {HALF}, contrast {CONTRAST}, both polarities, "
                f"NEAREST, taken evenly from the {len(contour)} points\ncontour_probes(step {step:g}, min_contrast 20) finds on the "
                f"template: {n * N_PROBES} (hit, probe) pairs.  Host clock to the caller, medians of\n{args.reps} calls per form, the "
                "forms alternating call by call, in parentheses the range of the calls:\n\n")
        f.write(row("(a) last_probes()", out["call_ms"]["a_last_probes"]))
        f.write(row("(b) 16 x last_calipers(64 calipers), select on the host", out["call_ms"]["b_16_last_calipers_select_on_host"]))
        f.write(f"  (b) / (a){'':<49}{b / a:10.1f}\n\n")
        f.write("(b)'s pixels differ from (a)'s in the last bits: a caliper rounds its own ptLT to f32 and samples at cos(angle + phi),\n"
                "a probe composes the hit's matrix with its frame.  So the two are compared by counts, not bytes: found edges "
                f"{found['a_found']} (a)\nand {found['b_found']} (b) of {found['probes']}, the same index in {found['same_index']}; "
                f"ambiguous {found['a_ambiguous']} and {found['b_ambiguous']}; {found['a_outside']} probes leave the source.\n"
                "Launch against launch, HIP events around each launch, in a pass of their own:\n\n")
        f.write(row(f"k_probe (1 launch, job table {table['k_probe'] / 1e3:.1f} KB)", out["kernel_ms"]["k_probe"]))
        f.write(row(f"k_caliper (16 launches, job tables {table['k_caliper_x16'] / 1e6:.1f} MB)", out["kernel_ms"]["k_caliper_x16"]))
        f.write(f"  16 x k_caliper / k_probe{'':<34}{kc / kp:10.2f}\n")


if __name__ == "__main__":
    main()
