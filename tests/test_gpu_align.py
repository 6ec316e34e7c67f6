"""Pose alignment on the HIP path (fpm_align_sums_at / fpm_align_at / fpm_align_last): k_patch_align's eleven sums
against the numpy restatement of tests/align_ref.py (the oracle's warpAffine of fpm_patch_matrix's matrix, then exact
integers), the iteration against the reference loop, and what adopting the aligned poses does to the later entries.
Every comparison of sums and of results is ==."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import synth
from fastest_image_pattern_matching_amd.matcher import ALIGN_DTYPE, ALIGN_SUMS_DTYPE
from tests import align_ref as ref
from tests.cases import CASES
from tests.test_patch_host import poses as host_poses

pytestmark = pytest.mark.gpu

EDGE_W = [1, 2, 3, 4, 5, 63, 64, 65]          # tests/test_gpu_compare.py's setting
EDGE_H = [1, 15, 16, 17]
EDGE_POSES = [((40.0, 30.0), 0.0), ((52.25, 41.5), 30.0), ((70.5, 66.125), -137.5)]


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


def _expect_sums(src, t, poses, rect, normalize):
    th, tw = t.shape
    rect = rect if rect is not None else (0, 0, tw, th)
    return [ref.sums(ref.patch(src, rect, lt, a), t, rect, ref.table(src, t, rect, lt, a) if normalize else None)
            for lt, a in poses]


def _check_sums(hip, src, t, poses, rect, normalize, label, source=0):
    got = hip.align_sums_at(source, [p[0] for p in poses], [p[1] for p in poses], rect, normalize=normalize)
    assert got.dtype == ALIGN_SUMS_DTYPE
    exp = _expect_sums(src, t, poses, rect, normalize)
    ref.assert_rows(got, exp, ref.SUM_FIELDS, f"{label} rect={rect} norm={normalize}")
    return exp


# ---- tile, lane-group and gradient-mask edges -----------------------------------------------------------------------
@pytest.mark.parametrize("sw", [161, 164])
def test_tile_lane_group_and_gradient_mask_edges(hip, sw):
    sh, tw, th = 119, 71, 23
    rng = np.random.default_rng(sw)
    src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    tmpl = rng.integers(0, 256, (th, tw), dtype=np.uint8)
    hip.resetParams()
    assert hip.learnPattern(tmpl)
    hip.stage([src])
    ps = EDGE_POSES + host_poses()      # the patch tests' poses too: some start left of / above the source
    rects = []
    for w in EDGE_W:
        for h in EDGE_H:
            for x in (0, 1, 2, 3):      # the alignment of the template reads; x = 0, y = 0 touch the left and top sides
                rects.append((x, (0, 1, 3)[(x + w + h) % 3], w, h))
            # touching the right / bottom side, and one pixel inside each (the gradient then reads outside the rectangle)
            rects += [(tw - w, 1, w, h), (tw - w - 1, 0, w, h), (2, th - h, w, h), (1, th - h - 1, w, h)]
    assert {r[1] for r in rects} >= {0, 1, 3} and any(r[0] == 1 and r[1] == 1 for r in rects)
    for k, rect in enumerate(rects):
        _check_sums(hip, src, tmpl, ps, rect, k % 2 == 1, "edges")
    for norm in (False, True):          # the whole template, and a single used pixel
        exp = _check_sums(hip, src, tmpl, ps, None, norm, "whole")
        assert all(e["n_used"] == (tw - 2) * (th - 2) for e in exp)
        assert all(e["n_used"] == 1 for e in _check_sums(hip, src, tmpl, ps, (0, 0, 2, 2), norm, "one pixel"))
        assert all(e["n_used"] == 0 and e["ssd"] == 0 for e in _check_sums(hip, src, tmpl, ps, (0, 0, 71, 1), norm, "row 0"))


# ---- the per-pixel terms at their extremes --------------------------------------------------------------------------
def _checker(h, w, period=3, phase=0):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx + phase) // period + yy // period) % 2 == 1, 255, 0).astype(np.uint8)


def test_checker_template_and_source(hip):
    """A 0 / 255 checker of period 3 on both sides: Tx, Ty and r sit at +-255 over whole tiles, so a fold that wraps at
    32 bits shows up.  1021 x 300 is the largest the few seconds of this test afford the numpy reference."""
    tw, th = 1021, 300
    tmpl, src = _checker(th, tw), _checker(400, 1100, phase=1)
    hip.resetParams()
    assert hip.learnPattern(tmpl)
    hip.stage([src])
    ps = [((30.0, 40.0), 0.0), ((31.0, 41.0), 0.0), ((33.5, 42.25), 0.0), ((60.25, 70.5), 3.0)]
    for rect, norm in [(None, False), (None, True), ((2, 1, 1019, 299), False)]:
        exp = _check_sums(hip, src, tmpl, ps, rect, norm, "checker")
        assert all(e["h_tt"] > 2 ** 32 for e in exp) and max(e["h_tt"] for e in exp) > 2 ** 50
        assert norm or exp[0]["ssd"] > 2 ** 32


# ---- border path ----------------------------------------------------------------------------------------------------
def test_patches_that_leave_the_source(hip, templates):
    make, prm = CASES["top_is_layer0"]
    s, t = make(templates)
    assert s.shape == (160, 220)
    th, tw = t.shape
    hip.resetParams()
    assert hip.learnPattern(t)
    hip.stage([s])
    ps = [((-tw / 2.0, 70.0), 0.0), ((220.0 - tw / 2.0, 70.0), 0.0), ((93.0, -th / 2.0), 0.0), ((93.0, 160.0 - th / 2.0), 0.0),
          ((-10.5, 150.25), 37.0), ((1000.0, 1000.0), 0.0), ((101.5, 72.25), 37.0)]   # test_gpu_compare.py's list
    for norm in (False, True):
        exp = _check_sums(hip, s, t, ps, None, norm, "borders")
        # the patch wholly outside the source is all zeros: r = -T there
        inner = t[1:-1, 1:-1].astype(np.int64)
        assert norm or exp[5]["ssd"] == int((inner * inner).sum())


# ---- batch, determinism -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(templates):
    """3 sources of 320 x 240 with 2, 0, 1 pasted hits (tests/test_gpu_compare.py's)."""
    t = templates["Dst10"]
    hits = [[(80, 70, 25.0), (230, 160, -140.0)], [], [(160, 120, 61.0)]]
    srcs = []
    for k, hs in enumerate(hits):
        s = synth.noise(320, 240, 128, 10, 300 + k)
        for cx, cy, a in hs:
            synth.paste_rotated(s, t, cx, cy, a)
        srcs.append(s)
    return t, dict(max_pos=3, tolerance_angle=180.0), srcs


def _search_batch(m, batch):
    t, prm, srcs = batch
    m.resetParams()
    for k, v in prm.items():
        setattr(m._params, k, v)
    assert m.learnPattern(t)
    m.stage(srcs)
    res = m.match_staged()
    assert [len(r) for r in res] == [2, 0, 1]
    return res


def _poses(res):
    idx = [k for k in range(len(res)) for _ in res[k]]
    ps = [(r.ptLT, r.dMatchedAngle) for k in range(len(res)) for r in res[k]]     # Qt semantics: the raw pose
    return idx, [p[0] for p in ps], [p[1] for p in ps]


def test_order_independence_over_a_batch(hip, batch):
    t, prm, srcs = batch
    idx, lts, angs = _poses(_search_batch(hip, batch))
    idx, lts, angs = idx * 5, lts * 5, [a + 0.1 * k for k in range(5) for a in angs]
    for norm in (False, True):
        a = hip.align_sums_at(idx, lts, angs, normalize=norm)
        b = hip.align_sums_at(idx, lts, angs, normalize=norm)
        assert a.tobytes() == b.tobytes() and (a["n_used"] > 0).all()
        for i in (0, 7, 14):
            e = _expect_sums(srcs[idx[i]], t, [(lts[i], angs[i])], None, norm)
            ref.assert_rows(a[i:i + 1], e, ref.SUM_FIELDS, f"batch row {i}")
        r1 = hip.align_at(idx, lts, angs, iters=2, normalize=norm)
        r2 = hip.align_at(idx, lts, angs, iters=2, normalize=norm)
        assert r1.tobytes() == r2.tobytes()


# ---- the loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 3])
def test_loop_equals_the_reference_loop(hip, iters):
    s, plants = ref.planted()
    hip.resetParams()
    for k, (T, lt, a) in enumerate(plants):
        assert hip.learnPattern(T)
        hip.stage([s])
        for rect in [None, (3, 2, 60, 40)]:
            full = rect if rect is not None else (0, 0, ref.TW, ref.TH)
            starts = ref.starts(lt, a) + [(lt, a), ((lt[0] + 40.0, lt[1]), a)]
            for norm in (False, True):
                got = hip.align_at(0, [p[0] for p in starts], [p[1] for p in starts], rect, iters=iters, normalize=norm)
                assert got.dtype == ALIGN_DTYPE
                exp = [ref.loop(s, T, full, slt, sa, iters, 2.0, norm) for slt, sa in starts]
                ref.assert_rows(got, exp, ref.RESULT_FIELDS, f"plant {k} rect {rect} iters {iters} norm {norm}")
                assert (got["ssd"] <= got["ssd_start"]).all()
                c_true = ref.centre(s.shape, full, lt, a)
                for i in (0, 1):
                    e0 = np.linalg.norm(ref.centre(s.shape, full, *starts[i]) - c_true)
                    e1 = np.linalg.norm(ref.centre(s.shape, full, (got[i]["lt_x"], got[i]["lt_y"]), got[i]["angle"]) - c_true)
                    print(f"plant {k} rect {rect} iters {iters} norm {norm}: {e0:.4f} -> {e1:.5f} px")
                    assert e1 < e0 and (iters < 3 or e1 < 1.0 / 16.0)
                # the planted pose itself; another rectangle origin rounds the matrix's f32 terms differently
                assert got[2]["ssd_start"] == 0 or rect is not None
                if k == 0:      # 40 px off on the first scene: stopped at once (tests/test_align_host.py)
                    assert got[3]["flags"] & (L.ALIGN_STEP_CLAMPED | L.ALIGN_KEPT_START)


def test_max_step_freezes_a_hit(hip):
    s, plants = ref.planted()
    T, lt, a = plants[0]
    hip.resetParams()
    assert hip.learnPattern(T)
    hip.stage([s])
    slt, sa = ref.starts(lt, a)[0]
    got = hip.align_at(0, [slt], [sa], iters=3, max_step=0.05)[0]     # the first step is about 0.4 px
    exp = ref.loop(s, T, (0, 0, ref.TW, ref.TH), slt, sa, 3, 0.05)
    ref.assert_rows([got], [exp], ref.RESULT_FIELDS, "max_step")
    assert got["flags"] == L.ALIGN_STEP_CLAMPED | L.ALIGN_KEPT_START and got["evals"] == 1 and got["angle"] == sa


# ---- adopt ----------------------------------------------------------------------------------------------------------
def _last_results(m, n_src):
    n = (C.c_int32 * n_src)()
    m._lib.fpm_last_results(m._ctx, None, 0, n)
    out = (L.Result * max(sum(n), 1))()
    assert m._lib.fpm_last_results(m._ctx, out, sum(n), n) == L.FPM_OK
    return bytes(out), list(n)


def test_adopt(hip, batch):
    t, prm, srcs = batch
    res = _search_batch(hip, batch)
    idx, lts, angs = _poses(res)
    before, results = hip.last_compare(-1), _last_results(hip, 3)
    cands = [hip.last_candidates(k).tobytes() for k in range(3)]
    for norm in (False, True):
        got = hip.align_last(-1, normalize=norm)
        assert got.tobytes() == hip.align_at(idx, lts, angs, normalize=norm).tobytes()
        assert len(got) == 3 and (got["ssd"] <= got["ssd_start"]).all() and (got["evals"] >= 1).all()
        assert hip.last_compare(-1).tobytes() == before.tobytes()      # nothing in the context changed
    assert [len(hip.align_last(k)) for k in range(3)] == [2, 0, 1]
    hip.model_clear()
    hip.model_train_at(idx, lts, angs)                                   # a model to inspect against
    got = hip.align_last(-1, adopt=True)
    assert (got["best_eval"] > 0).any(), "no hit moved: the test shows nothing"
    alt, aang = np.stack([got["lt_x"], got["lt_y"]], 1), got["angle"]
    for norm in (False, True):
        st, img = hip.last_compare(-1, normalize=norm, diff=True)
        st2, img2 = hip.compare_at(idx, alt, aang, normalize=norm, diff=True)
        assert st.tobytes() == st2.tobytes() and np.array_equal(img, img2)
        assert hip.last_inspect(-1, normalize=norm).tobytes() == hip.inspect_at(idx, alt, aang, normalize=norm).tobytes()
    assert hip.last_compare(-1).tobytes() != before.tobytes()
    assert np.array_equal(hip.last_patches(-1)[0], hip.patches_at(idx, alt, aang))
    assert np.array_equal(hip.last_patches(0), hip.patches_at(idx[:2], alt[:2], aang[:2]))
    # a second alignment starts from the adopted poses
    assert hip.align_last(-1).tobytes() == hip.align_at(idx, alt, aang).tobytes()
    # one source only: the others keep their poses
    one = hip.align_last(2, iters=1, adopt=True)
    assert len(one) == 1
    st = hip.last_compare(-1)
    assert st[:2].tobytes() == hip.compare_at(idx[:2], alt[:2], aang[:2]).tobytes()
    assert st[2:].tobytes() == hip.compare_at([2], [(one[0]["lt_x"], one[0]["lt_y"])], [one[0]["angle"]]).tobytes()
    # the search's own records never change
    assert _last_results(hip, 3) == results and [hip.last_candidates(k).tobytes() for k in range(3)] == cands
    # the next search drops the adopted poses
    assert [len(r) for r in hip.match_staged()] == [2, 0, 1]
    assert hip.last_compare(-1).tobytes() == before.tobytes()


# ---- state ----------------------------------------------------------------------------------------------------------
def test_state_rules(gpu_matcher_factory, batch):
    t, prm, srcs = batch
    th, tw = t.shape
    m = gpu_matcher_factory(**prm)
    n = C.c_int32(-1)
    assert m._lib.fpm_align_last(m._ctx, None, 0, 3, 2.0, 0, None, 0, C.byref(n)) == L.FPM_E_NOT_LEARNED and n.value == 0
    with pytest.raises(ValueError):
        m.align_last()                                 # no template
    assert m.learnPattern(t)
    with pytest.raises(ValueError, match="no staged sources"):
        m.align_last()
    with pytest.raises(ValueError, match="no staged sources"):
        m.align_sums_at(0, [(10.0, 10.0)], [0.0])
    m.stage(srcs)
    with pytest.raises(ValueError, match="no search has run"):
        m.align_last()
    assert len(m.align_at(2, [(10.0, 10.0)], [5.0])) == 1     # poses of the caller's need no search
    m.match_staged_launch()
    for call in (lambda: m.align_last(), lambda: m.align_at(0, [(10.0, 10.0)], [0.0]),
                 lambda: m.align_sums_at(0, [(10.0, 10.0)], [0.0])):
        with pytest.raises(ValueError, match="in flight"):
            call()
    counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [2, 0, 1]
    assert len(m.align_last(0)) == 2 and len(m.align_last(1)) == 0 and len(m.align_last(-1)) == 3
    before = m.last_compare(-1).tobytes()
    # capacity: the count, FPM_E_CAPACITY, nothing written, nothing adopted
    out = np.zeros(3, ALIGN_DTYPE)
    pout = out.ctypes.data_as(C.POINTER(L.AlignResult))
    rc = m._lib.fpm_align_last(m._ctx, None, -1, 3, 2.0, L.ALIGN_ADOPT, pout, 2, C.byref(n))
    assert rc == L.FPM_E_CAPACITY and n.value == 3 and out.tobytes() == bytes(out.nbytes)
    assert m.last_compare(-1).tobytes() == before
    # arguments out of range: FPM_E_INVALID_ARG, nothing launched, nothing adopted
    m.profile(True)
    try:
        m.profile_reset()
        for iters, step, flags in [(0, 2.0, 0), (9, 2.0, 0), (3, 0.0, 0), (3, -1.0, 0), (3, float("nan"), 0),
                                   (3, float("inf"), 0), (3, 1025.0, 0), (3, 2.0, 4), (3, 2.0, 8 | L.ALIGN_ADOPT)]:
            rc = m._lib.fpm_align_last(m._ctx, None, -1, iters, step, flags | L.ALIGN_ADOPT, pout, 3, C.byref(n))
            assert rc == L.FPM_E_INVALID_ARG and n.value == 0, (iters, step, flags)
        idx, lt, ang = np.zeros(1, np.int32), np.full((1, 2), 10.0, np.float32), np.zeros(1, np.float64)
        pi, pl, pa = (idx.ctypes.data_as(C.POINTER(C.c_int32)), lt.ctypes.data_as(C.POINTER(C.c_float)),
                      ang.ctypes.data_as(C.POINTER(C.c_double)))
        assert m._lib.fpm_align_at(m._ctx, None, pi, pl, pa, 1, 3, 2.0, L.ALIGN_ADOPT, pout) == L.FPM_E_INVALID_ARG
        sums = np.zeros(1, ALIGN_SUMS_DTYPE)
        assert m._lib.fpm_align_sums_at(m._ctx, None, pi, pl, pa, 1, 2, sums.ctypes.data_as(C.POINTER(L.AlignSums))) == \
            L.FPM_E_INVALID_ARG
        for bad in [(0, 0, 0, 4), (-1, 0, 4, 4), (0, 0, tw + 1, th), (1, 0, tw, th), (0, 1, tw, th), (0, 0, tw, th + 1)]:
            with pytest.raises(ValueError):
                m.align_last(0, bad)
            rc = m._lib.fpm_align_last(m._ctx, C.byref(L.PatchRect(*bad)), 0, 3, 2.0, L.ALIGN_ADOPT, pout, 3, C.byref(n))
            assert rc == L.FPM_E_INVALID_ARG and n.value == 0
        with pytest.raises(ValueError):
            m.align_last(3)                            # source index past the batch
        with pytest.raises(ValueError):
            m.align_at(3, [(10.0, 10.0)], [5.0])
        with pytest.raises(ValueError):
            m.align_last(iters=0)
        with pytest.raises(ValueError):
            m.align_last(max_step=0.0)
        assert m.align_profile()[1] == 0 and m.profile_get(L.K_COMPARE)[1] == 0
    finally:
        m.profile(False)
    assert m.last_compare(-1).tobytes() == before and out.tobytes() == bytes(out.nbytes)
    m.stage(srcs)                                      # staged again, not searched
    with pytest.raises(ValueError, match="no search has run"):
        m.align_last()
    m.match_staged_candidates()                        # a search without results
    none = m.align_last(-1, adopt=True)
    assert none.shape == (0,) and none.dtype == ALIGN_DTYPE
    m.clearPattern()
    with pytest.raises(ValueError):
        m.align_last(0)


def test_rectangle_caps(gpu_matcher_factory):
    """A template beyond the caps: NULL is FPM_E_INVALID_ARG, a rectangle within them runs."""
    rng = np.random.default_rng(3)
    t = rng.integers(0, 256, (1030, 1040), dtype=np.uint8)
    s = np.zeros((1100, 1100), np.uint8)
    s[20:1050, 30:1070] = t
    m = gpu_matcher_factory()
    assert m.learnPattern(t)
    m.stage([s])
    with pytest.raises(ValueError):
        m.align_sums_at(0, [(30.0, 20.0)], [0.0])
    sums = np.zeros(1, ALIGN_SUMS_DTYPE)
    idx, lt, ang = np.zeros(1, np.int32), np.array([[30.0, 20.0]], np.float32), np.zeros(1, np.float64)
    args = (idx.ctypes.data_as(C.POINTER(C.c_int32)), lt.ctypes.data_as(C.POINTER(C.c_float)),
            ang.ctypes.data_as(C.POINTER(C.c_double)), 1, 0, sums.ctypes.data_as(C.POINTER(L.AlignSums)))
    assert m._lib.fpm_align_sums_at(m._ctx, None, *args) == L.FPM_E_INVALID_ARG
    assert m._lib.fpm_align_sums_at(m._ctx, C.byref(L.PatchRect(0, 0, 1024, 1025)), *args) == L.FPM_E_INVALID_ARG
    got = m.align_sums_at(0, [(30.0, 20.0)], [0.0], (8, 3, 1024, 1024))[0]     # 2^20 pixels, planted exactly: r = 0
    assert got["n_used"] == 1 << 20 and got["ssd"] == 0 and got["g_t"] == 0 and got["h_tt"] > 2 ** 50
    ref.assert_rows([got], [ref.sums(t[3:1027, 8:1032], t, (8, 3, 1024, 1024))], ref.SUM_FIELDS, "area cap")


# ---- profile --------------------------------------------------------------------------------------------------------
def test_profile_counts_the_launches(hip, batch):
    t, prm, srcs = batch
    th, tw = t.shape
    idx, lts, angs = _poses(_search_batch(hip, batch))
    hip.profile(True)
    try:
        for iters in (1, 3, 8):
            hip.profile_reset()
            hip.align_last(-1, iters=iters)
            ms, launches, nbytes = hip.align_profile()
            assert launches == iters + 1 and nbytes == (iters + 1) * 2 * 3 * tw * th and ms > 0
            assert hip.profile_get(L.K_COMPARE)[1] == 0 and hip.profile_get(L.K_PATCH)[1] == 0
        hip.profile_reset()
        hip.align_last(-1, iters=3, normalize=True, adopt=True)
        assert hip.align_profile()[1] == 4 and hip.profile_get(L.K_COMPARE)[1] == 1    # the one sums launch
        hip.profile_reset()
        hip.align_sums_at(idx, lts, angs)
        assert hip.align_profile()[1] == 1 and hip.profile_get(L.K_COMPARE)[1] == 0
        hip.align_sums_at(idx, lts, angs, normalize=True)
        assert hip.align_profile()[1] == 2 and hip.profile_get(L.K_COMPARE)[1] == 1
        hip.profile_reset()
        assert hip.align_profile() == (0.0, 0, 0)
        assert len(L.KERNEL_NAMES) == 15 and len(L.PROFILE_NAMES) == 16     # no FPM_K_* index was added
    finally:
        hip.profile(False)
