"""Sources already in device memory (fpm_stage_sources_device / fpm_match_device / fpm_op_to_gray, k_stage_gray): the
gray plane byte for byte against a numpy restatement of the conversion, searches on device tensors (gray, interleaved,
planar, contiguous and views) against match() on the host array and against the oracle, batches, the polarity fused
into the staging, the producer-stream hand-over and the argument checks.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch as _torch   # at collection time, before any test loads libfpm_hip.so: one HIP runtime for both (_lib.hip_runtimes)

from fastest_image_pattern_matching_amd import _lib as L
from tests import oracle
from tests.cases import CASES
from tests.test_device_input_host import gray_restated
from tests.test_gpu_parity import assert_same_results

pytestmark = pytest.mark.gpu

FORMATS = {"gray": L.FMT_GRAY8, "bgr": L.FMT_BGR8, "rgb": L.FMT_RGB8, "bgra": L.FMT_BGRA8, "rgba": L.FMT_RGBA8,
           "bgr_planar": L.FMT_BGR8_PLANAR, "rgb_planar": L.FMT_RGB8_PLANAR}
COLOUR = [f for f in FORMATS if f != "gray"]
COLOUR_CASES = ("dst10_multi", "dst5_subpixel", "dst4_overlap")


@pytest.fixture(scope="module")
def torch():
    return _torch


def test_one_hip_runtime(hip, torch):
    """torch (imported when this module is collected, before any test loads libfpm_hip.so) and the library share one
    HIP runtime: a tensor's pointer and stream are the library's own kind."""
    torch.zeros(1, device="cuda")
    assert len(L.hip_runtimes()) == 1, L.hip_runtimes()


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


def _setup(m, t, prm, **extra):
    m.resetParams()
    for k, v in {**prm, **extra}.items():
        setattr(m._params, k, v)
    assert m.learnPattern(t)


def _tuples(res):
    return [r.as_tuple() for r in res]


def _inv(s):
    return np.ascontiguousarray(255 - s)


def lay_out(fmt, b, g, r, alpha_seed=0):
    """(image in the format's memory layout, channel_order, layout hint) from three channel planes."""
    if fmt == "gray":
        return np.ascontiguousarray(b), "bgr", None
    first, last = (r, b) if fmt.startswith("rgb") else (b, r)
    if fmt.endswith("_planar"):
        return np.ascontiguousarray(np.stack([first, g, last], 0)), fmt[:3], "chw"
    ch = [first, g, last]
    if fmt in ("bgra", "rgba"):
        ch.append(np.random.default_rng(alpha_seed).integers(0, 256, b.shape, dtype=np.uint8))
    return np.ascontiguousarray(np.stack(ch, -1)), fmt[:3], "hwc"


def expected_gray(fmt, b, g, r):
    return np.ascontiguousarray(b) if fmt == "gray" else gray_restated(b, g, r)


def colourise(s):
    """The issue's colour frame of a gray scene: B = s, G = s, R = (s >> 1) + 60."""
    return s, s, ((s >> 1) + 60).astype(np.uint8)


_case_cache = {}


def case_data(templates, case, colour=False):
    """(search plane, template, params, oracle results, records, stats) of a case, computed once per module: the
    scene itself, or the gray plane of its colourised frame."""
    key = (case, colour)
    if key not in _case_cache:
        make, prm = CASES[case]
        s, t = make(templates)
        plane = gray_restated(*colourise(s)) if colour else s
        o = oracle.OracleMatcher().set(**prm)
        assert o.learnPattern(t)
        exp = o.match(plane)
        _case_cache[key] = (s, t, prm, exp, o.candidates().tobytes(), o.stats())
    return _case_cache[key]


def check_search(m, got, exp, rec, stats, label):
    assert_same_results(got, exp, label)
    assert m.last_candidates(0).tobytes() == rec, f"{label}: records differ"
    assert m.search_stats() == stats, label


# ------------------------------------------------------------------------------------------------ the operator
SHAPES = [(1, 1), (3, 5), (2, 15), (2, 16), (2, 17), (9, 17), (33, 67), (64, 64), (5, 4099)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_to_gray_operator(hip, fmt, shape):
    rng = np.random.default_rng(shape[0] * 131 + shape[1] + 7 * FORMATS[fmt])
    b, g, r = (rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(3))
    img, order, layout = lay_out(fmt, b, g, r)
    exp = expected_gray(fmt, b, g, r)
    out = hip.to_gray(img, order, layout)
    assert out.dtype == np.uint8 and out.shape == shape and out.tobytes() == exp.tobytes()
    assert hip.to_gray(img, order, layout, invert=True).tobytes() == (255 - exp).tobytes()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_to_gray_constant_images(hip, fmt):
    for (cb, cg, cr), want in [((255, 0, 0), 29), ((0, 255, 0), 150), ((0, 0, 255), 76), ((255, 255, 255), 255),
                               ((0, 0, 0), 0)]:
        b, g, r = (np.full((6, 37), v, np.uint8) for v in (cb, cg, cr))
        img, order, layout = lay_out(fmt, b, g, r)
        want = cb if fmt == "gray" else want
        assert np.array_equal(hip.to_gray(img, order, layout), np.full((6, 37), want, np.uint8)), (fmt, cb, cg, cr)
        assert np.array_equal(hip.to_gray(img, order, layout, invert=True), np.full((6, 37), 255 - want, np.uint8))


@pytest.mark.parametrize("offset", [1, 3, 13])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_to_gray_strided_views_at_odd_offsets(hip, fmt, offset):
    """Row-strided (and plane-strided) host views that start at an odd byte offset: the kernel's general path, with
    every source alignment modulo 4 and strides that are no multiple of 4."""
    h, w = 9, 67
    c = {"gray": 1, "bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4}.get(fmt, 1)
    row = w * c + 5
    plane = row * h + 7
    rng = np.random.default_rng(offset * 17 + FORMATS[fmt])
    flat = rng.integers(0, 256, offset + 3 * plane + 64, dtype=np.uint8)
    assert flat.ctypes.data % 16 == 0
    as_strided = np.lib.stride_tricks.as_strided
    if fmt == "gray":
        v = as_strided(flat[offset:], (h, w), (row, 1))
        exp, order, layout = v, "bgr", None
    elif fmt.endswith("_planar"):
        v = as_strided(flat[offset:], (3, h, w), (plane, row, 1))
        exp = gray_restated(v[2], v[1], v[0]) if fmt.startswith("rgb") else gray_restated(v[0], v[1], v[2])
        order, layout = fmt[:3], "chw"
    else:
        v = as_strided(flat[offset:], (h, w, c), (row, c, 1))
        exp = gray_restated(v[..., 2], v[..., 1], v[..., 0]) if fmt.startswith("rgb") else \
            gray_restated(v[..., 0], v[..., 1], v[..., 2])
        order, layout = fmt[:3], "hwc"
    assert v.ctypes.data % 16 == offset
    assert hip.to_gray(v, order, layout).tobytes() == np.ascontiguousarray(exp).tobytes()
    assert hip.to_gray(v, order, layout, invert=True).tobytes() == np.ascontiguousarray(255 - exp).tobytes()


@pytest.mark.parametrize("shape", [(3, 5), (2, 16), (9, 17), (33, 67), (5, 4099)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", ["gray", "bgr", "rgba", "rgb_planar"])
def test_to_gray_leaves_the_row_gap_alone(hip, fmt, shape):
    """With a destination stride wider than the width, the bytes between the width and the stride keep a sentinel: the
    kernel writes exactly w bytes per row (the rows travel to the device and back with their gap)."""
    h, w = shape
    rng = np.random.default_rng(w)
    b, g, r = (rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(3))
    img, order, layout = lay_out(fmt, b, g, r)
    wide = np.full((h, w + 29), 0xA5, np.uint8)
    hip.to_gray(img, order, layout, dst=wide[:, :w])
    assert np.array_equal(wide[:, :w], expected_gray(fmt, b, g, r))
    assert np.all(wide[:, w:] == 0xA5)


# ------------------------------------------------------------------------------------------------ searches
@pytest.mark.parametrize("case", sorted(CASES))
def test_match_device_gray(hip, torch, templates, case):
    """A gray device tensor: match_device == match on the host array == the oracle (results, records, stats)."""
    s, t, prm, exp, rec, stats = case_data(templates, case)
    _setup(hip, t, prm)
    check_search(hip, hip.match(s), exp, rec, stats, f"{case} host")
    d = torch.from_numpy(s).cuda()
    check_search(hip, hip.match_device(d), exp, rec, stats, f"{case} device")


@pytest.mark.parametrize("case", COLOUR_CASES)
@pytest.mark.parametrize("fmt", COLOUR)
def test_match_device_colour(hip, torch, templates, fmt, case):
    """A colour device tensor in every format: the search equals the oracle on the numpy gray plane.  (A wrong channel
    order changes most gray pixels and the scores in the 5th-6th decimal, so it fails the exact comparison.)"""
    s, t, prm, exp, rec, stats = case_data(templates, case, colour=True)
    assert len(exp) >= 1
    img, order, layout = lay_out(fmt, *colourise(s), alpha_seed=3)
    _setup(hip, t, prm)
    d = torch.from_numpy(img).cuda()
    check_search(hip, hip.match_device(d, order, layout), exp, rec, stats, f"{case} {fmt}")


def test_match_device_views(hip, torch, templates):
    """Views into wider tensors (misaligned base, strides that are no multiple of 16, plane stride > stride x height)
    equal the contiguous run."""
    s, t, prm, exp, rec, stats = case_data(templates, "dst10_multi")
    cs, _, _, cexp, crec, cstats = case_data(templates, "dst10_multi", colour=True)
    h, w = s.shape
    _setup(hip, t, prm)
    # gray: a column slice, base + 11, row stride w + 100
    wide = torch.zeros((h, w + 100), dtype=torch.uint8, device="cuda")
    v = wide[:, 11:11 + w]
    v.copy_(torch.from_numpy(s))
    assert v.stride() == (w + 100, 1) and v.data_ptr() % 16 == 11 and (w + 100) % 16 != 0
    check_search(hip, hip.match_device(v), exp, rec, stats, "gray column slice")
    # interleaved with padded rows, starting three pixels in
    b, g, r = colourise(cs)
    hwc = torch.zeros((h, w + 10, 3), dtype=torch.uint8, device="cuda")
    v = hwc[:, 3:3 + w]
    v.copy_(torch.from_numpy(np.stack([b, g, r], -1)))
    assert v.stride() == (3 * (w + 10), 3, 1) and not v.is_contiguous()
    check_search(hip, hip.match_device(v, "bgr"), cexp, crec, cstats, "hwc padded rows")
    # planar, cut from a larger tensor
    chw = torch.zeros((3, h + 5, w + 13), dtype=torch.uint8, device="cuda")
    v = chw[:, 2:2 + h, 5:5 + w]
    v.copy_(torch.from_numpy(np.stack([r, g, b], 0)))
    assert v.stride() == ((h + 5) * (w + 13), w + 13, 1) and v.stride(0) > v.stride(1) * h
    check_search(hip, hip.match_device(v, "rgb"), cexp, crec, cstats, "chw cut")


def test_match_device_rejects_before_any_library_call(hip, torch, templates):
    s, t, prm, exp, _, _ = case_data(templates, "dst10_multi")
    _setup(hip, t, prm)
    d = torch.from_numpy(s).cuda()
    for bad, err in [(s, TypeError), (torch.from_numpy(s), ValueError), (d.to(torch.int16), TypeError),
                     (d[:, ::2], ValueError), (d.t(), ValueError), (d[None], ValueError),
                     (torch.zeros((3, 8, 3), dtype=torch.uint8, device="cuda"), ValueError)]:
        with pytest.raises(err):
            hip.match_device(bad)
    assert_same_results(hip.match_device(d), exp, "after the rejections")


# ------------------------------------------------------------------------------------------------ batch
def test_stage_device_batch(gpu_matcher_factory, torch, templates):
    """Three sources in separate allocations, one a strided view: match_staged == the three lone searches; then a host
    stage() and a plain match() on the same context (slab re-layout, staged bookkeeping)."""
    s, t, prm, exp, rec, stats = case_data(templates, "dst10_multi")
    srcs = [s, np.ascontiguousarray(s[::-1]), np.ascontiguousarray(s[:, ::-1])]
    h, w = s.shape
    m = gpu_matcher_factory()
    _setup(m, t, prm)
    lone = [_tuples(m.match(x)) for x in srcs]
    assert lone[0] == exp and all(len(x) >= 1 for x in lone)
    wide = torch.zeros((h, w + 37), dtype=torch.uint8, device="cuda")
    view = wide[:, 5:5 + w]
    view.copy_(torch.from_numpy(srcs[1]))
    # one stride for the whole batch: the other two sit in allocations of their own with the same row stride
    devs = []
    for x in (srcs[0], srcs[2]):
        own = torch.zeros((h, w + 37), dtype=torch.uint8, device="cuda")
        own[:, :w].copy_(torch.from_numpy(x))
        devs.append(own[:, :w])
    batch = [devs[0], view, devs[1]]
    assert len({b.data_ptr() % 16 for b in batch}) == 2
    m.stage_device(batch)
    assert [_tuples(x) for x in m.match_staged()] == lone
    assert [_tuples(x) for x in m.match_staged()] == lone   # the graph replay over the same slab
    with pytest.raises(ValueError):   # different strides in one batch
        m.stage_device([devs[0], torch.from_numpy(srcs[1]).cuda()])
    assert [_tuples(x) for x in m.match_staged()] == lone   # a rejected call leaves the staged batch alone
    m.stage(srcs)
    assert [_tuples(x) for x in m.match_staged()] == lone
    check_search(m, m.match(s), exp, rec, stats, "plain match after the batches")
    check_search(m, m.match_device(devs[0]), exp, rec, stats, "match_device after the batches")
    with pytest.raises(RuntimeError):   # a lone search replaces the staged batch
        m.match_staged()


# ------------------------------------------------------------------------------------------------ polarity
def test_polarity_fused_at_staging(gpu_matcher_factory, torch, templates):
    """bitwise_not set before stage_device: the kernel writes 255 - gray and the search launches no k_bitwise_not;
    flipping the parameter afterwards inverts the slab once (the pattern of test_polarity_tracking)."""
    make, prm = CASES["dst1_rot30"]
    s, t = make(templates)
    srcs = [s, _inv(s)]
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    plain = [o.match(x) for x in srcs]
    inverted = [o.match(_inv(x)) for x in srcs]
    assert len(plain[0]) >= 1 and len(inverted[1]) >= 1
    m = gpu_matcher_factory()
    _setup(m, t, prm, bitwise_not=1)
    m.profile(True)
    m.profile_reset()
    m.stage_device([torch.from_numpy(x).cuda() for x in srcs])
    first = m.match_staged()
    assert m.profile_get(L.K_NOT)[1] == 0
    m._params.bitwise_not = 0
    second = m.match_staged()
    assert m.profile_get(L.K_NOT)[1] == 1
    m._params.bitwise_not = 1
    third = m.match_staged()
    assert m.profile_get(L.K_NOT)[1] == 2
    for i in range(2):
        assert_same_results(first[i], inverted[i], f"pass 1 source {i}")
        assert_same_results(second[i], plain[i], f"pass 2 source {i}")
        assert _tuples(third[i]) == _tuples(first[i])
    # staged plain, searched inverted: one launch; a lone device search under each setting
    m._params.bitwise_not = 0
    m.profile_reset()
    m.stage_device([torch.from_numpy(x).cuda() for x in srcs])
    assert [_tuples(r) for r in m.match_staged()] == [_tuples(r) for r in second]
    assert m.profile_get(L.K_NOT)[1] == 0
    m._params.bitwise_not = 1
    assert [_tuples(r) for r in m.match_staged()] == [_tuples(r) for r in first]
    assert m.profile_get(L.K_NOT)[1] == 1
    d = torch.from_numpy(s).cuda()
    assert_same_results(m.match_device(d), inverted[0], "lone, on")
    assert m.profile_get(L.K_NOT)[1] == 1
    m._params.bitwise_not = 0
    assert_same_results(m.match_device(d), plain[0], "lone, off")
    assert m.profile_get(L.K_NOT)[1] == 1


# ------------------------------------------------------------------------------------------------ producer stream
def test_producer_stream(hip, torch, templates):
    """The frame is written on a side stream behind a few hundred MB of queued copies and handed over with that stream
    and no host synchronisation; then the same on the default stream.  This guards the plumbing -- the handle is
    passed and the wait is issued, so a search that ran ahead of the copies would see the zeros the frame held
    before -- and cannot prove the absence of a race."""
    s, t, prm, exp, rec, stats = case_data(templates, "dst10_multi")
    assert len(exp) >= 1
    _setup(hip, t, prm)
    host = torch.from_numpy(s).pin_memory()
    ballast = torch.zeros(64 << 20, dtype=torch.uint8).pin_memory()
    sink = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    for stream in (torch.cuda.Stream(), None):
        frame = torch.zeros(s.shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream()):
            for _ in range(4):
                sink.copy_(ballast, non_blocking=True)
            frame.copy_(host, non_blocking=True)
        got = hip.match_device(frame, stream=stream)
        check_search(hip, got, exp, rec, stats, "side stream" if stream is not None else "default stream")
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(gpu_matcher_factory, torch, templates):
    s, t, prm, exp, _, _ = case_data(templates, "dst10_multi")
    h, w = s.shape
    m = gpu_matcher_factory()
    lib, ctx = m._lib, m._ctx
    d = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")   # room for every description below
    d[0].copy_(torch.from_numpy(s))
    ptr = d.data_ptr()
    n = C.c_int32()
    out = (L.Result * 64)()

    def lone(width, height, stride, plane, fmt):
        return lib.fpm_match_device(ctx, ptr, width, height, stride, plane, fmt, None, out, 64, C.byref(n), None)

    def stage(count, width, height, stride, plane, fmt):
        return lib.fpm_stage_sources_device(ctx, (C.c_void_p * 1)(ptr), count, width, height, stride, plane, fmt, None)

    assert m.match_device(d[0]) == []   # unlearned
    assert lone(w, h, w, 0, L.FMT_GRAY8) == L.FPM_E_NOT_LEARNED
    _setup(m, t, prm)
    bad = [(lambda: lone(w, h, w - 1, 0, L.FMT_GRAY8), "stride below"),
           (lambda: lone(100, h, 299, 0, L.FMT_BGR8), "stride below"),
           (lambda: lone(100, h, 399, 0, L.FMT_RGBA8), "stride below"),
           (lambda: stage(1, w, h, w - 1, 0, L.FMT_GRAY8), "stride below"),
           (lambda: lone(w, h, w, w * h - 1, L.FMT_RGB8_PLANAR), "plane stride"),
           (lambda: stage(1, w, h, w + 16, (w + 16) * h - 1, L.FMT_BGR8_PLANAR), "plane stride"),
           (lambda: stage(0, w, h, w, 0, L.FMT_GRAY8), "must be positive"),
           (lambda: stage(-1, w, h, w, 0, L.FMT_GRAY8), "must be positive"),
           (lambda: lone(0, h, w, 0, L.FMT_GRAY8), "must be positive"),
           (lambda: lone(w, -3, w, 0, L.FMT_GRAY8), "must be positive"),
           (lambda: lone(w, h, w, 0, L.FMT_COUNT), "unknown pixel format"),
           (lambda: lone(w, h, w, 0, -1), "unknown pixel format"),
           (lambda: stage(1, w, h, w, 0, 99), "unknown pixel format"),
           (lambda: lib.fpm_match_device(ctx, None, w, h, w, 0, L.FMT_GRAY8, None, out, 64, C.byref(n), None), "empty source"),
           (lambda: lib.fpm_stage_sources_device(ctx, None, 1, w, h, w, 0, L.FMT_GRAY8, None), "null image table"),
           (lambda: lib.fpm_stage_sources_device(ctx, (C.c_void_p * 1)(None), 1, w, h, w, 0, L.FMT_GRAY8, None),
            "null pointer")]
    for i, (call, text) in enumerate(bad):
        assert call() == L.FPM_E_INVALID_ARG, i
        assert text in m.last_error(), (i, m.last_error())
    assert lone(8, 8, 8, 0, L.FMT_GRAY8) == L.FPM_E_SIZE and m.last_error()
    assert stage(1, 8, 8, 8, 0, L.FMT_GRAY8) == L.FPM_E_SIZE
    # a staged search in flight
    m.stage_device([d[0]])
    m.match_staged_launch()
    assert stage(1, w, h, w, 0, L.FMT_GRAY8) == L.FPM_E_INVALID_ARG and "in flight" in m.last_error()
    assert lone(w, h, w, 0, L.FMT_GRAY8) == L.FPM_E_INVALID_ARG and "in flight" in m.last_error()
    counts, _ = m.match_staged_finish_array()
    assert counts[0] == len(exp)
    assert_same_results(m.match_device(d[0]), exp, "after the errors")
