"""Match patches on the HIP path (fpm_last_patches / fpm_last_patches_device / fpm_patches_at): the upright crop of
every result, sampled on the device from level 0 of the staged sources, against the oracle's getRotatedROI and
warpAffine.  Every comparison is exact (bytes, and the f64 matrices)."""
import ctypes as C

import numpy as np
import pytest
import torch   # at collection time, before any test loads libfpm_hip.so: one HIP runtime for both (_lib.hip_runtimes)

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import synth
from fastest_image_pattern_matching_amd.matcher import merge_candidates, patch_matrix
from tests import oracle
from tests.cases import CASES, _run_both
from tests.fast_mode_ref import fast_reference
from tests.test_patch_host import ANGLES, poses

pytestmark = pytest.mark.gpu

# the cases of the results-parity test with the hits their scenes paste
PARITY = {"dst10_multi": 3, "dst5_subpixel": 1, "top_is_layer0": 2, "dst4_overlap": 2}
SEMANTICS_MFC = 1   # FPM_SEMANTICS_MFC (include/fpm.h)


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


_scenes = {}


def _scene(templates, case):
    if case not in _scenes:
        make, prm = CASES[case]
        _scenes[case] = make(templates) + (prm,)
    return _scenes[case]


def _tuples(res):
    return [r.as_tuple() for r in res]


def _margin(t):
    th, tw = t.shape
    return (-3, -3, tw + 6, th + 6)


def _expect_rois(s, t, results):
    """getRotatedROI at every result's reported pose (Qt semantics: ptLT is the f32 point, the angle dMatchAngle)."""
    th, tw = t.shape
    return [oracle.rotated_roi(s, tw, th, r.ptLT, r.dMatchedAngle) for r in results]


def _assert_patches(got, exp, label):
    assert got.dtype == np.uint8 and len(got) == len(exp), f"{label}: {len(got)} patches vs {len(exp)}"
    for i, e in enumerate(exp):
        assert got[i].shape == e.shape, (label, i, got[i].shape, e.shape)
        bad = np.argwhere(got[i] != e)
        assert bad.size == 0, f"{label}: patch {i} differs at {len(bad)} pixels, first (y, x) = {bad[0]}"


# ---- 1. results parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PARITY))
def test_patches_of_results(hip, templates, case):
    s, t, prm = _scene(templates, case)
    th, tw = t.shape
    gpu, orc, _, _ = _run_both(hip, s, t, **prm)
    assert len(orc) >= PARITY[case] and _tuples(gpu) == orc
    assert hip.patch_size() == (tw, th) and hip.patch_size(_margin(t)) == (tw + 6, th + 6)
    _assert_patches(hip.last_patches(0, _margin(t)), _expect_rois(s, t, gpu), case)
    got, mats = hip.last_patches(0, matrices=True)
    assert mats.shape == (len(gpu), 2, 3)
    for i, r in enumerate(gpu):
        assert np.array_equal(mats[i], patch_matrix(s.shape[1], s.shape[0], r.ptLT, r.dMatchedAngle))
    _assert_patches(got, [oracle.warp_affine(s, m, (tw, th)) for m in mats], case + " default rect")
    # the user-defined rectangle is the default one once set (the reference tool's use of it)
    hip.setUserDefinedRect(_margin(t))
    try:
        _assert_patches(hip.last_patches(0), _expect_rois(s, t, gpu), case + " user rect")
    finally:
        hip._user_rect = None


# ---- 5. both forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PARITY))
def test_warp_form_gives_the_same_bytes(hip, gpu_matcher_factory, templates, monkeypatch, case):
    s, t, prm = _scene(templates, case)
    monkeypatch.setenv("FPM_PATCH_TILED", "0")
    other = gpu_matcher_factory()          # the switch is read when the matcher is made
    monkeypatch.delenv("FPM_PATCH_TILED")
    a, _, _, _ = _run_both(hip, s, t, **prm)
    b, _, _, _ = _run_both(other, s, t, **prm)
    assert _tuples(a) == _tuples(b) and len(a) >= PARITY[case]
    for rect in (None, _margin(t), (-40, 7, 101, 50)):
        pa, pb = hip.last_patches(0, rect), other.last_patches(0, rect)
        assert pa.shape == pb.shape and pa.tobytes() == pb.tobytes(), (case, rect)
    _assert_patches(other.last_patches(0, _margin(t)), _expect_rois(s, t, b), case + " k_warp form")


# ---- 2. switches -----------------------------------------------------------------------------------------------------
def test_mfc_semantics_uses_the_raw_pose(hip, templates):
    s, t, prm = _scene(templates, "dst3_range")
    th, tw = t.shape
    # under MFC semantics tolerance_range takes the angle list from the ranges [t1, t2] + [t3, t4] (MatchToolDlg.cpp:
    # 805-815), not from tolerance_angle: the case's +-40 degrees as two ranges
    o = oracle.OracleMatcher()
    hip.resetParams()
    for k, v in {**prm, "semantics": SEMANTICS_MFC}.items():
        setattr(o.params, k, v)
        setattr(hip._params, k, v)
    for k, v in enumerate((-40.0, -1.0, 0.0, 40.0)):
        o.params.tolerance[k] = v
        hip._params.tolerance[k] = v
    assert o.learnPattern(t) and hip.learnPattern(t)
    gpu, orc = hip.match(s), o.match(s)
    assert len(orc) >= 2 and _tuples(gpu) == orc
    assert all(abs(r.dMatchedAngle) < 40 for r in gpu)   # so the reported angle is the exact negation of dMatchAngle
    exp = [oracle.rotated_roi(s, tw, th, (np.float32(r.ptLT[0]), np.float32(r.ptLT[1])), -r.dMatchedAngle) for r in gpu]
    _assert_patches(hip.last_patches(0, _margin(t)), exp, "mfc")


def test_fast_mode_patches(hip, templates):
    s, t, prm = _scene(templates, "dst10_multi")
    th, tw = t.shape
    rec = fast_reference(t, s, prm)[0]
    hip.resetParams()
    for k, v in {**prm, "stop_layer": 1}.items():
        setattr(hip._params, k, v)
    assert hip.learnPattern(t)
    got = hip.match(s)
    exp = merge_candidates(hip._params, tw, th, rec)
    assert len(exp) >= 3 and _tuples(got) == _tuples(exp)
    _assert_patches(hip.last_patches(0, _margin(t)), _expect_rois(s, t, exp), "fast mode")


def test_bitwise_not_patches_sample_the_inverted_plane(hip, templates):
    s, t, prm = _scene(templates, "dst10_multi")
    inv = np.ascontiguousarray(255 - s)
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    orc = o.match(s)
    hip.resetParams()
    for k, v in {**prm, "bitwise_not": 1}.items():
        setattr(hip._params, k, v)
    assert hip.learnPattern(t)
    got = hip.match(inv)
    assert len(orc) >= 3 and _tuples(got) == orc
    _assert_patches(hip.last_patches(0, _margin(t)), _expect_rois(np.ascontiguousarray(255 - inv), t, got), "bitwise not")


# ---- 3. tile edges ---------------------------------------------------------------------------------------------------
EDGE_W = [1, 3, 4, 5, 63, 64, 65, 130]
EDGE_H = [1, 15, 16, 17, 33]


@pytest.mark.parametrize("sw", [161, 164])
def test_tile_edges(hip, sw):
    sh = 119
    rng = np.random.default_rng(sw)
    src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    tmpl = rng.integers(0, 256, (29, 37), dtype=np.uint8)
    hip.resetParams()
    assert hip.learnPattern(tmpl)
    hip.stage([src])
    ps = poses()
    lts, angs = [p[0] for p in ps], [p[1] for p in ps]
    for w in EDGE_W:
        for h in EDGE_H:
            rect = (-2, 1, w, h)
            exp = [oracle.warp_affine(src, patch_matrix(sw, sh, lt, a, rect[:2]), (w, h)) for lt, a in ps]
            # a canary-filled buffer wider and taller than the patches; even widths also pad between the patches
            pad = 1 if w % 2 == 0 else 0
            buf = np.full((len(ps), h + pad, w + 7), 0xA5, np.uint8)
            view = buf[:, :h, 3:3 + w]
            got, mats = hip.patches_at(0, lts, angs, rect, matrices=True, out=view)
            assert got is view
            _assert_patches(view, exp, f"{w}x{h}")
            for (lt, a), m in zip(ps, mats):
                assert np.array_equal(m, patch_matrix(sw, sh, lt, a, rect[:2]))
            view[...] = 0xA5
            assert (buf == 0xA5).all(), f"{w}x{h}: bytes outside the patches were written"
    assert len(ANGLES) == len(ps) == 8


# ---- 4. borders ------------------------------------------------------------------------------------------------------
def test_patches_leave_the_image_on_all_sides(hip, templates):
    s, t, prm = _scene(templates, "top_is_layer0")
    assert s.shape == (160, 220)
    th, tw = t.shape
    hip.resetParams()
    assert hip.learnPattern(t)
    hip.stage([s])
    rect = (-100, -100, tw + 200, th + 200)
    lts, angs = [(93.0, 70.0), (101.5, 72.25)], [0.0, 37.0]
    got = hip.patches_at([0, 0], lts, angs, rect)
    exp = [oracle.warp_affine(s, patch_matrix(220, 160, lt, a, rect[:2]), rect[2:]) for lt, a in zip(lts, angs)]
    for e, a in zip(exp, angs):   # the scene itself: zero fill at all four corners (upright: along all four edges)
        assert e.any() and not (e[0, 0] or e[0, -1] or e[-1, 0] or e[-1, -1])
        assert a != 0.0 or not (e[0].any() or e[-1].any() or e[:, 0].any() or e[:, -1].any())
        for edge in (e[0], e[-1], e[:, 0], e[:, -1]):
            assert (edge == 0).any()
    _assert_patches(got, exp, "borders")


# ---- 6. batch --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(templates):
    """5 sources of 320 x 240 with 2, 0, 2, 1, 1 pasted hits, and the oracle's results for each."""
    t = templates["Dst10"]
    hits = [[(80, 70, 25.0), (230, 160, -140.0)], [], [(90, 160, 100.0), (240, 80, -10.0)], [(160, 120, 61.0)],
            [(200, 150, -77.0)]]
    prm = dict(max_pos=3, tolerance_angle=180.0)
    srcs = []
    for k, hs in enumerate(hits):
        s = synth.noise(320, 240, 128, 10, 300 + k)
        for cx, cy, a in hs:
            synth.paste_rotated(s, t, cx, cy, a)
        srcs.append(s)
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    orc = [o.match(s) for s in srcs]
    assert [len(r) for r in orc] == [2, 0, 2, 1, 1]
    return t, prm, srcs, orc


def _search_batch(hip, batch):
    t, prm, srcs, orc = batch
    hip.resetParams()
    for k, v in prm.items():
        setattr(hip._params, k, v)
    assert hip.learnPattern(t)
    hip.stage(srcs)
    res = hip.match_staged()
    assert [_tuples(r) for r in res] == orc
    return res


def test_batch_all_sources(hip, batch):
    t, prm, srcs, orc = batch
    res = _search_batch(hip, batch)
    rect = _margin(t)
    allp, counts = hip.last_patches(-1, rect)
    assert counts.tolist() == [2, 0, 2, 1, 1] and len(allp) == 6
    per = [hip.last_patches(k, rect) for k in range(5)]
    assert [len(p) for p in per] == [2, 0, 2, 1, 1]
    assert np.array_equal(allp, np.concatenate(per))
    for k in range(5):
        _assert_patches(per[k], _expect_rois(srcs[k], t, res[k]), f"source {k}")
    # a buffer one patch too small: the count needed, FPM_E_CAPACITY, and no pixel written
    pw, ph = hip.patch_size(rect)
    buf = np.full((6, ph, pw), 0x5A, np.uint8)
    n = C.c_int32()
    r = L.PatchRect(*rect)
    rc = hip._lib.fpm_last_patches(hip._ctx, C.byref(r), -1, L.u8ptr(buf), pw, pw * ph, 5, C.byref(n), None)
    assert rc == L.FPM_E_CAPACITY and n.value == 6 and (buf == 0x5A).all()
    with pytest.raises(ValueError):
        hip.last_patches(5, rect)


# ---- 7. device output ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0,extra", [(3, 9), (4, 12)], ids=["unaligned", "aligned"])
def test_device_output_into_a_view(hip, batch, x0, extra):
    t = batch[0]
    _search_batch(hip, batch)
    rect = (-4, -3, 60, 58)          # 60 pixels wide: whole dwords where the view is aligned
    host, counts = hip.last_patches(-1, rect)
    n, ph, pw = host.shape
    assert n == 6 and (pw, ph) == (60, 58)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        big = torch.full((n, ph + 2, pw + extra), 0xA5, dtype=torch.uint8, device="cuda:0")
        view = big[:, 1:1 + ph, x0:x0 + pw]
        out, cnt = hip.last_patches_device(-1, rect, out=view, stream=side)
        got = big.cpu().numpy()      # on the side stream: ordered after the launch by the library's event
    assert out is view and cnt.tolist() == counts.tolist()
    assert np.array_equal(got[:, 1:1 + ph, x0:x0 + pw], host)
    got[:, 1:1 + ph, x0:x0 + pw] = 0xA5
    assert (got == 0xA5).all()
    # no `out`: a fresh tensor, on torch's current stream
    fresh = hip.last_patches_device(2, rect)
    assert fresh.dtype == torch.uint8 and fresh.is_cuda and tuple(fresh.shape) == (2, ph, pw)
    assert np.array_equal(fresh.cpu().numpy(), host[2:4])
    with pytest.raises(ValueError):
        hip.last_patches_device(-1, rect, out=big[:, :ph, :pw + 1])   # not (n, ph, pw)
    with pytest.raises((ValueError, TypeError)):
        hip.last_patches_device(0, rect, out=torch.zeros((2, ph, pw), dtype=torch.uint8))


# ---- 8. state --------------------------------------------------------------------------------------------------------
def test_state_rules(gpu_matcher_factory, batch):
    t, prm, srcs, orc = batch
    m = gpu_matcher_factory(**prm)
    with pytest.raises(ValueError):
        m.last_patches()                               # no template
    assert m.learnPattern(t)
    with pytest.raises(ValueError, match="no staged sources"):
        m.last_patches()
    m.stage(srcs)
    with pytest.raises(ValueError, match="no search has run"):
        m.last_patches()
    m.match_staged_launch()
    with pytest.raises(ValueError, match="in flight"):
        m.last_patches()
    with pytest.raises(ValueError, match="in flight"):
        m.patches_at(0, [(10.0, 10.0)], [0.0])
    counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [2, 0, 2, 1, 1]
    assert len(m.last_patches(0)) == 2
    for bad in [(0, 0, 0, 4), (0, 0, 4, 8193)]:
        with pytest.raises(ValueError):
            m.last_patches(0, bad)
        n = C.c_int32(-1)   # and the library's own check of the rectangle
        assert m._lib.fpm_last_patches(m._ctx, C.byref(L.PatchRect(*bad)), 0, None, 0, 0, 0, C.byref(n), None) == \
            L.FPM_E_INVALID_ARG and n.value == 0
    m.stage(srcs)                                      # staged again, not searched
    with pytest.raises(ValueError, match="no search has run"):
        m.last_patches()
    assert len(m.patches_at(4, [(10.0, 10.0)], [5.0])) == 1   # poses of the caller's need no search
    with pytest.raises(ValueError):
        m.patches_at(5, [(10.0, 10.0)], [5.0])         # source index past the batch
    m.match_staged_candidates()                        # a search without results (the angle-sharded rank's step)
    th, tw = t.shape
    none, counts = m.last_patches(-1)
    assert none.shape == (0, th, tw) and counts.tolist() == [0] * 5
    m.clearPattern()
    with pytest.raises(ValueError):
        m.last_patches(0, (0, 0, 8, 8))
