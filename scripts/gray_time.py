"""Cost of the gray-value tools on the Src7 configuration (4024 x 3036 sources, Dst7 762 x 521 template, +-180 deg,
TargetNum 3: bench.py PARAMS and its synthetic Src7), `--batch` staged sources, the whole template as the region.
Needs a gfx950 device and torch.

All in one run, on one context.  Launch against launch (HIP events around each launch, the forms alternating call by
call, medians of `--reps`):
  k_patch_hist against the sums form of k_patch_compare over the same jobs (align_sums_at(normalize=True) launches that
      form once, counted under FPM_K_COMPARE): the same sampling, so the ratio is the price of the histogram.  For the
      sources as they are and for a batch of constant sources, at the hits' poses, and for the run lengths --runs
      (tiles per workgroup; 0 = the engine's choice).
  k_patch_threshold against k_patch_warp over the same rectangles.
To the caller (host clock; each call returns with its results in the caller's arrays), the forms alternating:
  (a) last_histogram()      (b) last_segment("otsu")      (c) last_segment(128)
  (d) last_patches_device + torch.bincount per hit: the histograms a caller has today
  (e) last_patches + blobs_host of the images thresholded on the host: the blobs a caller has today (of (c))
(a) and (d), and (c) and (e), are compared once: the same numbers.  `--lib PATH` loads another build of the library (a
contention variant of k_patch_hist) and `--tag` names the output, `gray_src7<tag>.json`; README.txt is written only
without a tag.

    python scripts/gray_time.py [--batch 64] [--reps 5] [--out-dir profiles/gray] [--lib PATH --tag _variant]
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
    ap.add_argument("--runs", default="0,1,4,16")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "gray"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 5, "at least 5 runs per form"
    runs = [int(v) for v in args.runs.split(",")]

    import numpy as np
    import torch   # one HIP runtime, loaded before libfpm_hip.so

    import bench
    from fastest_image_pattern_matching_amd import _lib as L
    if args.lib:
        L.LIB_PATH = os.path.abspath(args.lib)
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
    batch = [scenes[i % len(scenes)] for i in range(args.batch)]
    m.stage(batch)
    results = m.match_staged()
    n = sum(len(rs) for rs in results)
    assert [len(rs) for rs in results] == [bench.PARAMS["max_pos"]] * args.batch
    idx = np.repeat(np.arange(args.batch, dtype=np.int32), bench.PARAMS["max_pos"])
    lts = [r.ptLT for rs in results for r in rs]
    angs = [r.dMatchedAngle for rs in results for r in rs]
    cap = 64

    # ---- launch against launch -----------------------------------------------------------------------------------------
    def kernel_pass(forms):
        """{name: [ms]} and {name: (launches, bytes)}: each form runs under the profile, the forms alternating"""
        ms = {name: [] for name in forms}
        info = {}
        m.profile(True)
        for rep in range(args.reps + 1):
            for name, (run, read) in forms.items():
                m.profile_reset()
                run()
                t, launches, nbytes = read()
                assert launches == 1, (name, launches)
                info[name] = {"launches": launches, "bytes": nbytes}
                if rep >= 1:
                    ms[name].append(t)
        m.profile(False)
        return {k: dict(stat(v), **info[k]) for k, v in ms.items()}

    def hist_forms():
        forms = {"k_patch_compare_sums": (lambda: m.align_sums_at(idx, lts, angs, normalize=True),
                                          lambda: m.profile_get(L.K_COMPARE))}
        for r in runs:
            def run(r=r):
                m.gray_set_run(r)
                m.histogram_at(idx, lts, angs)
                m.gray_set_run(0)
            forms[f"k_patch_hist_run{r}"] = (run, lambda: m.gray_profile(L.GRAY_HIST))
        return forms

    kernels = {"source": kernel_pass(hist_forms())}
    kernels["source"].update(kernel_pass({
        "k_patch_threshold": (lambda: m.segment_at(idx, lts, angs, threshold=128, cap=cap), lambda: m.gray_profile(L.GRAY_THRESHOLD)),
        "k_patch_warp": (lambda: m.patches_at(idx, lts, angs), lambda: m.profile_get(L.K_PATCH))}))
    out = {"frame": [w, h], "template": [tw, th], "params": bench.PARAMS, "batch": args.batch, "hits": n, "reps": args.reps,
           "lib": os.path.basename(args.lib) if args.lib else "libfpm_hip.so", "runs": runs}

    if not args.kernels_only:
        # ---- to the caller -------------------------------------------------------------------------------------------
        dev = torch.device("cuda:0")

        def form_a():
            return m.last_histogram(source=-1)

        def form_b():
            return m.last_segment(source=-1, threshold="otsu", cap=cap)

        def form_c():
            return m.last_segment(source=-1, threshold=128, cap=cap)

        def form_d():
            p = m.last_patches_device(source=-1)
            p = p if isinstance(p, torch.Tensor) else p[0]
            flat = p.reshape(n, -1).to(torch.int64)
            hist = torch.stack([torch.bincount(flat[i], minlength=256) for i in range(n)])
            return hist.cpu().numpy().astype(np.uint32)

        def form_e():
            p = m.last_patches(source=-1)[0].astype(np.int32)
            e = np.clip(128 - p, 0, 255).astype(np.uint8)
            return M.blobs_host(e, 0, 4, 8, cap)

        ha, hd = form_a(), form_d()
        assert np.array_equal(ha[:, 0], hd), "the histograms of (a) and (d) differ"
        sc, se = form_c(), form_e()
        assert sc[1].tobytes() == se[0].tobytes(), "the summaries of (c) and (e) differ"
        untrunc = [i for i in range(n) if not sc[1]["flags"][i]]
        assert all(sc[2][i].tobytes() == se[1][i].tobytes() for i in untrunc), "the blobs of (c) and (e) differ"
        out["found"] = {"otsu_thresholds": sorted(set(form_b()[0]["threshold"].tolist())),
                        "blobs_at_128": int(sc[1]["n_blobs"].sum()), "truncated_hits": n - len(untrunc)}
        call_ms = alternate({"a_last_histogram": form_a, "b_last_segment_otsu": form_b, "c_last_segment_128": form_c,
                             "d_patches_device_bincount": form_d, "e_last_patches_blobs_host": form_e}, args.reps)
        out["call_ms"] = {k: stat(v) for k, v in call_ms.items()}
        # where (c)'s time goes: its launches, summed per kernel over the labelling rounds of one call
        m.profile(True)
        m.profile_reset()
        form_c()
        out["segment_128_kernel_ms"] = dict({"k_patch_threshold": m.gray_profile(L.GRAY_THRESHOLD)[0]},
                                            **{name: m.blobs_profile(k)[0] for k, name in enumerate(L.BLOB_KERNEL_SYMBOLS)})
        out["segment_128_labelling_launches"] = m.blobs_profile(0)[1]
        m.profile(False)

    # ---- a batch of constant sources: every lane of every wave meets one bin ----------------------------------------
    m.stage([np.full((h, w), 128, np.uint8)] * args.batch)
    kernels["constant"] = kernel_pass(hist_forms())
    hc = m.histogram_at(idx[:3], lts[:3], angs[:3])
    assert (hc.sum(axis=2) == tw * th).all() and (hc[:, 0, 128] > 0.99 * tw * th).all()
    out["kernel_ms"] = kernels
    for kind in ("source", "constant"):
        base = kernels[kind]["k_patch_compare_sums"]["median"]
        out[f"hist_over_compare_sums_{kind}"] = {f"run{r}": kernels[kind][f"k_patch_hist_run{r}"]["median"] / base for r in runs}
    out["threshold_over_warp"] = kernels["source"]["k_patch_threshold"]["median"] / kernels["source"]["k_patch_warp"]["median"]

    os.makedirs(args.out_dir, exist_ok=True)
    line = json.dumps(out)
    print(line)
    with open(os.path.join(args.out_dir, f"gray_src7{args.tag}.json"), "w") as f:
        f.write(line + "\n")
    if args.tag or args.kernels_only:
        return

    def row(label, s, extra=""):
        return f"  {label:<58}{s['median']:10.3f} ms  ({s['min']:.3f} .. {s['max']:.3f}){extra}\n"

    with open(os.path.join(args.out_dir, "README.txt"), "w") as f:
        f.write(f"gray_src7.json: `python scripts/gray_time.py --batch {args.batch} --reps {args.reps}` on one MI355X.\n"
                f"The Src7 configuration ({w} x {h} sources, Dst7 {tw} x {th}, +-180 deg, TargetNum 3), {args.batch} staged sources, "
                f"{n} hits,\nthe whole {tw} x {th} template as the region.  Launch against launch: HIP events around each launch, "
                f"medians of {args.reps},\nthe forms alternating call by call, in parentheses the range.  run = tiles per workgroup "
                "of k_patch_hist (0 = the\nengine's choice).  The sources as they are:\n\n")
        for k, s in kernels["source"].items():
            f.write(row(f"{k} ({s['bytes'] / 1e6:.1f} MB)", s))
        f.write("\nA batch of constant sources (gray 128) at the same poses:\n\n")
        for k, s in kernels["constant"].items():
            f.write(row(f"{k} ({s['bytes'] / 1e6:.1f} MB)", s))
        f.write("\nk_patch_hist / k_patch_compare (sums form), the price of the histogram:\n")
        for kind in ("source", "constant"):
            f.write(f"  {kind:<10}" + "".join(f"  run {r}: {v:.2f}" for r, v in
                                              zip(runs, out[f'hist_over_compare_sums_{kind}'].values())) + "\n")
        f.write(f"k_patch_threshold / k_patch_warp: {out['threshold_over_warp']:.2f}\n\n"
                f"To the caller, host clock, medians of {args.reps} calls per form, the forms alternating:\n\n")
        labels = {"a_last_histogram": "(a) last_histogram()", "b_last_segment_otsu": "(b) last_segment('otsu')",
                  "c_last_segment_128": "(c) last_segment(128)",
                  "d_patches_device_bincount": "(d) last_patches_device + torch.bincount per hit",
                  "e_last_patches_blobs_host": "(e) last_patches + threshold + blobs_host"}
        for k, s in out["call_ms"].items():
            f.write(row(labels[k], s))
        c = out["call_ms"]
        f.write(f"  (d) / (a){'':<49}{c['d_patches_device_bincount']['median'] / c['a_last_histogram']['median']:10.1f}\n")
        f.write(f"  (e) / (c){'':<49}{c['e_last_patches_blobs_host']['median'] / c['c_last_segment_128']['median']:10.1f}\n\n")
        f.write(f"(a) and (d) returned the same histograms, (c) and (e) the same summaries and, for the hits not truncated at cap "
                f"{cap},\nthe same records: {out['found']['blobs_at_128']} blobs at threshold 128, {out['found']['truncated_hits']} "
                f"hits truncated.  Otsu's thresholds over the hits: {out['found']['otsu_thresholds']}.\nThe launches of one "
                f"(c), HIP events, summed per kernel over its {out['segment_128_labelling_launches']} labelling rounds: "
                + ", ".join(f"{k} {v:.3f} ms" for k, v in out["segment_128_kernel_ms"].items()) + ".\n")


if __name__ == "__main__":
    main()
