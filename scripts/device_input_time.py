"""Cost of getting a Src7-size frame (4024 x 3036, Dst7 template, +-180 deg, TargetNum 3: bench.py PARAMS and its
synthetic Src7) into a search from device memory against from host memory.  Needs a gfx950 device and torch.

(a) A lone search: match(host gray) against match_device for a gray, an interleaved BGR and a planar RGB device tensor
    and a gray one with rows padded to a multiple of 16 B.  Two figures per call: fpm_profile_last's device_ms (the
    search's device pass, the same work in every form) and a host clock around the synchronous call (upload or staging
    included).  The colour frames carry the gray frame in all three channels, so every form searches the same plane.
(b) Staging `--batch` sources: stage() from numpy arrays against stage_device(), by a host clock around the synchronous
    call, in GB/s on the algorithmic bytes per pixel below; and, in the same run over the same slab with the same
    1 + 1 bytes per pixel, k_bitwise_not (FPM_K_NOT, event-timed with profiling on) as the in-project yardstick of a
    streaming pass.  Staging has no profiling index, so a host clock it is, read three ways: around stage_device()
    (which also checks and describes every tensor in Python), around the C entry with the pointer table prebuilt
    (kernel + event, table copy, launch and stream wait), and that call for the whole batch minus the same call for one
    source, over the other sources' bytes (the fixed cost of a call drops out; the closest to the kernel's own rate
    and the figure to hold against k_bitwise_not's event time).

Every form is warmed up, the forms alternate within a series, and the whole series is repeated (`--series`): the spread
reported is that of the series' medians.  Prints one JSON line.

    python scripts/device_input_time.py [--batch 64] [--reps 20] [--series 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# algorithmic bytes per pixel of a staging pass: source bytes read + one gray byte written
BYTES_PER_PIXEL = {"gray": 1 + 1, "gray_padded": 1 + 1, "bgr": 3 + 1, "rgb_planar": 3 + 1, "bgra": 4 + 1, "host": 1 + 1}
DISTINCT = 8   # distinct scenes generated on the host; a larger batch repeats them (staging cost does not depend on content)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
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

    def device_forms(s):
        """name -> (tensor, channel_order, layout) of one scene; the colour forms hold it in every channel."""
        g = torch.from_numpy(s).cuda()
        wp = (w + 15) // 16 * 16
        padded = torch.zeros((h, wp), dtype=torch.uint8, device="cuda")[:, :w]
        padded.copy_(g)
        return {"gray": (g, "bgr", None),
                "gray_padded": (padded, "bgr", None),
                "bgr": (g[:, :, None].expand(h, w, 3).contiguous(), "bgr", "hwc"),
                "rgb_planar": (g[None].expand(3, h, w).contiguous(), "rgb", "chw"),
                "bgra": (g[:, :, None].expand(h, w, 4).contiguous(), "bgr", "hwc")}

    def path_of(form):
        """The kernel form a tensor gets: "fast" (16-byte loads) needs the base, the row stride and, for planar, the
        plane stride to be multiples of 16; anything else runs the general form."""
        t, _, layout = form
        strides = [t.stride(0), t.stride(1)] if layout == "chw" else [t.stride(0)]
        return "fast" if t.data_ptr() % 16 == 0 and all(st % 16 == 0 for st in strides) else "general"

    def spread(series_medians):
        return {"median": statistics.median(series_medians), "min": min(series_medians), "max": max(series_medians),
                "series": series_medians}

    out = {"frame": [w, h], "template": list(templ.shape[::-1]), "params": bench.PARAMS, "batch": args.batch,
           "reps": args.reps, "series": args.series, "bytes_per_pixel": BYTES_PER_PIXEL,
           "hbm_peak_gb_per_s": bench.HBM_PEAK_GBS}

    # ---- (a) a lone search -----------------------------------------------------------------------------------
    one = device_forms(scenes[0])
    lone_forms = ["host", "gray", "gray_padded", "bgr", "rgb_planar"]

    def lone_call(name):
        if name == "host":
            return m.match(scenes[0])
        t, order, layout = one[name]
        return m.match_device(t, order, layout)

    torch.cuda.synchronize()
    ref = [r.as_tuple() for r in lone_call("host")]
    assert len(ref) == bench.PARAMS["max_pos"], ref
    for name in lone_forms:
        for _ in range(3):
            assert [r.as_tuple() for r in lone_call(name)] == ref, name
    call_ms = {n: [] for n in lone_forms}
    dev_ms = {n: [] for n in lone_forms}
    for _ in range(args.series):
        c = {n: [] for n in lone_forms}
        d = {n: [] for n in lone_forms}
        for _ in range(args.reps):
            for name in lone_forms:
                t0 = time.perf_counter()
                lone_call(name)
                c[name].append((time.perf_counter() - t0) * 1e3)
                d[name].append(m.profile_last()[0])
        for name in lone_forms:
            call_ms[name].append(statistics.median(c[name]))
            dev_ms[name].append(statistics.median(d[name]))
    out["lone_search"] = {n: {"path": "upload" if n == "host" else path_of(one[n]), "call_ms": spread(call_ms[n]),
                              "device_pass_ms": spread(dev_ms[n])} for n in lone_forms}
    host_med = out["lone_search"]["host"]["call_ms"]["median"]
    for n in lone_forms[1:]:
        out["lone_search"][n]["call_over_host_call"] = out["lone_search"][n]["call_ms"]["median"] / host_med
    del one

    # ---- (b) staging a batch ---------------------------------------------------------------------------------
    B = args.batch
    host_batch = [scenes[i % len(scenes)] for i in range(B)]
    per_scene = [device_forms(s) for s in scenes]
    stage_forms = ["host", "gray", "gray_padded", "bgr", "rgb_planar", "bgra"]
    batches = {}
    for name in stage_forms[1:]:
        # separate allocations per source, as frames from a decoder are
        ts = []
        for i in range(B):
            t = per_scene[i % len(scenes)][name][0]
            if i >= len(scenes):   # a repeated scene gets memory of its own, laid out like the first copy
                t = (torch.zeros((h, t.stride(0)), dtype=torch.uint8, device="cuda")[:, :w].copy_(t)
                     if name == "gray_padded" else t.clone())
            ts.append(t)
        batches[name] = (ts, per_scene[0][name][1], per_scene[0][name][2])
    torch.cuda.synchronize()

    def c_args(name, count):
        """Arguments of a direct fpm_stage_sources_device call over the first `count` tensors of a batch."""
        ts, order, layout = batches[name]
        descs = [m._device_image(t, order, layout) for t in ts[:count]]
        _, hh, ww, row, plane, fmt = descs[0]
        ptrs = (C.c_void_p * count)(*[d[0] for d in descs])
        return (m._ctx, ptrs, count, ww, hh, row, plane, fmt, None)   # NULL = the null stream, torch's default

    prebuilt = {n: {c: c_args(n, c) for c in (1, B)} for n in stage_forms[1:]}

    def stage_c(name, count):
        """The C entry alone, pointer table prebuilt: staging kernel + its fixed cost (event, table copy, launch, wait)."""
        t0 = time.perf_counter()
        rc = m._lib.fpm_stage_sources_device(*prebuilt[name][count])
        t = (time.perf_counter() - t0) * 1e3
        assert rc == L.FPM_OK, (rc, m.last_error())
        m._staged = count
        return t

    def stage_py(name):
        """The Python entry: for device tensors it also checks and describes every tensor of the batch."""
        t0 = time.perf_counter()
        if name == "host":
            m.stage(host_batch)
        else:
            ts, order, layout = batches[name]
            m.stage_device(ts, order, layout)
        return (time.perf_counter() - t0) * 1e3

    def not_kernel_ms():
        """One k_bitwise_not over the staged slab's level 0: the pass after the switch flips carries the launch."""
        m.setBitwiseNot(not m.getBitwiseNot())
        m.profile_reset()
        m.match_staged_array()
        ms_, n, b = m.profile_get(L.K_NOT)
        assert n == 1 and b == 2 * B * w * h, (n, b)
        return ms_

    m.setBitwiseNot(False)
    m._push()
    for name in stage_forms:
        for _ in range(2):
            stage_py(name)
            if name != "host":
                stage_c(name, 1)
                stage_c(name, B)
    m.profile(True)
    m.match_staged_array()
    keys = ["host"] + [f"{n}:{k}" for n in stage_forms[1:] for k in ("py", "c1", "c")]
    stage_ms = {k: [] for k in keys}
    not_ms = []
    for _ in range(args.series):
        c = {k: [] for k in keys}
        k_not = []
        for _ in range(max(3, args.reps // 4)):
            m.setBitwiseNot(False)   # staging writes the plane as given: the yardstick below is a separate launch
            m._push()
            c["host"].append(stage_py("host"))
            for name in stage_forms[1:]:
                c[f"{name}:py"].append(stage_py(name))
                c[f"{name}:c1"].append(stage_c(name, 1))
                c[f"{name}:c"].append(stage_c(name, B))
            k_not.append(not_kernel_ms())   # over the B sources the last call staged
        for k in keys:
            stage_ms[k].append(statistics.median(c[k]))
        not_ms.append(statistics.median(k_not))
    m.setBitwiseNot(False)
    m.profile(False)

    def rate(name, ms_list, sources=B):
        gbs = [sources * w * h * BYTES_PER_PIXEL[name] / (t * 1e-3) / 1e9 for t in ms_list]
        r = {"ms": spread(ms_list), "gb_per_s": spread(gbs)}
        r["share_of_hbm_peak"] = r["gb_per_s"]["median"] / bench.HBM_PEAK_GBS
        return r

    st = {"host": dict(rate("host", stage_ms["host"]), path="upload", timed_by="host clock around stage()")}
    for n in stage_forms[1:]:
        # B sources against one source, call for call within a series: the fixed cost of a call drops out
        marginal = [a - b for a, b in zip(stage_ms[f"{n}:c"], stage_ms[f"{n}:c1"])]
        st[n] = {"path": path_of((batches[n][0][0],) + batches[n][1:]),
                 "python_call": dict(rate(n, stage_ms[f"{n}:py"]), timed_by="host clock around stage_device()"),
                 "c_call": dict(rate(n, stage_ms[f"{n}:c"]),
                                timed_by="host clock around fpm_stage_sources_device, pointer table prebuilt"),
                 "c_call_one_source_ms": spread(stage_ms[f"{n}:c1"]),
                 "marginal": dict(rate(n, marginal, B - 1), timed_by=f"c_call of {B} sources minus c_call of 1, over "
                                                                     f"{B - 1} sources' bytes")}
    st["k_bitwise_not"] = dict(rate("gray", not_ms), timed_by="HIP events around the kernel (FPM_K_NOT)")
    yard = st["k_bitwise_not"]["gb_per_s"]
    for n in ("gray", "gray_padded"):
        for how in ("c_call", "marginal"):
            st[n][how]["rate_over_bitwise_not"] = st[n][how]["gb_per_s"]["median"] / yard["median"]
    st["device_gray_over_host_stage_time"] = st["gray"]["python_call"]["ms"]["median"] / st["host"]["ms"]["median"]
    out["staging"] = st

    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
