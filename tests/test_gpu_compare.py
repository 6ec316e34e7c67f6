"""Patch comparison on the HIP path (fpm_last_compare / fpm_compare_at): every hit against the learned template, reduced
on the device.  The expectation is the oracle's warpAffine of fpm_patch_matrix's matrix, then numpy on integers
(tests/compare_ref.py).  Every comparison is exact: the integers by construction, the f64 by the fixed operation order."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import synth
from fastest_image_pattern_matching_amd.matcher import COMPARE_DTYPE, merge_candidates, patch_matrix
from tests import compare_ref as ref
from tests import oracle
from tests.cases import CASES, _run_both
from tests.fast_mode_ref import fast_reference
from tests.test_patch_host import poses as host_poses

pytestmark = pytest.mark.gpu

PARITY = {"dst10_multi": 3, "dst5_subpixel": 1, "top_is_layer0": 2, "dst4_overlap": 2}   # tests/test_gpu_patches.py's
SEMANTICS_MFC = 1


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


def _qt_poses(results):
    """(ptLT, angle) of results under the Qt semantics: the reported fields are the raw pose."""
    return [(r.ptLT, r.dMatchedAngle) for r in results]


def _expect(src, t, poses, rect, threshold, normalize):
    """Rows and difference images for `poses` [(lt, angle)] on `src`; rect None = the whole template."""
    th, tw = t.shape
    x, y, w, h = rect if rect is not None else (0, 0, tw, th)
    T = np.ascontiguousarray(t[y:y + h, x:x + w])
    rows, diffs = [], []
    for lt, a in poses:
        I = oracle.warp_affine(src, patch_matrix(src.shape[1], src.shape[0], lt, a, (x, y)), (w, h))
        row, d = ref.stats(I, T, threshold, normalize)
        rows.append(row)
        diffs.append(d)
    return rows, np.array(diffs, np.uint8).reshape(len(poses), h, w)


def _check_last(hip, src, t, poses, label, rects=(None,), thresholds=(16,), source=0):
    for rect in rects:
        for thr in thresholds:
            for norm in (False, True):
                rows, diffs = _expect(src, t, poses, rect, thr, norm)
                got, img = hip.last_compare(source, rect, threshold=thr, normalize=norm, diff=True)
                tag = f"{label} rect={rect} thr={thr} norm={norm}"
                assert got.dtype == COMPARE_DTYPE
                ref.assert_rows(got, rows, tag)
                assert img.shape == diffs.shape and np.array_equal(img, diffs), tag
                ref.assert_rows(hip.last_compare(source, rect, threshold=thr, normalize=norm), rows, tag + " no diff")


# ---- tile and lane-group edges ------------------------------------------------------------------------------------
EDGE_W = [1, 2, 3, 4, 5, 63, 64, 65]
EDGE_H = [1, 15, 16, 17]
EDGE_POSES = [((40.0, 30.0), 0.0), ((52.25, 41.5), 30.0), ((70.5, 66.125), -137.5)]


@pytest.mark.parametrize("sw", [161, 164])
def test_tile_and_lane_group_edges(hip, sw):
    sh = 119
    rng = np.random.default_rng(sw)
    src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    tmpl = rng.integers(0, 256, (23, 71), dtype=np.uint8)
    hip.resetParams()
    assert hip.learnPattern(tmpl)
    hip.stage([src])
    ps = EDGE_POSES + host_poses()      # the patch tests' poses too: some start left of / above the source
    lts, angs = [p[0] for p in ps], [p[1] for p in ps]
    for w in EDGE_W:
        for h in EDGE_H:
            for x in (0, 1, 2, 3):     # the alignment of the template read
                rect = (x, (x + h) % 5, w, h)
                norm = (w + h + x) % 2 == 1
                rows, diffs = _expect(src, tmpl, ps, rect, 16, norm)
                got, img = hip.compare_at(0, lts, angs, rect, threshold=16, normalize=norm, diff=True)
                ref.assert_rows(got, rows, f"{rect} norm={norm}")
                assert np.array_equal(img, diffs), rect


# ---- border path ----------------------------------------------------------------------------------------------------
def test_patches_that_leave_the_source(hip, templates):
    s, t, prm = _scene(templates, "top_is_layer0")
    assert s.shape == (160, 220)
    th, tw = t.shape
    hip.resetParams()
    assert hip.learnPattern(t)
    hip.stage([s])
    ps = [((-tw / 2.0, 70.0), 0.0), ((220.0 - tw / 2.0, 70.0), 0.0), ((93.0, -th / 2.0), 0.0), ((93.0, 160.0 - th / 2.0), 0.0),
          ((-10.5, 150.25), 37.0), ((1000.0, 1000.0), 0.0), ((101.5, 72.25), 37.0)]
    for norm in (False, True):
        rows, diffs = _expect(s, t, ps, None, 16, norm)
        assert all(0 < r["sum_i"] for r in rows[:5]) and rows[5]["sum_i"] == 0 and rows[5]["zncc"] == 0.0
        # the scene itself: each of the first four patches is cut by one side of the source (a zero column or row there)
        I = [oracle.warp_affine(s, patch_matrix(220, 160, lt, a), (tw, th)) for lt, a in ps[:4]]
        assert not I[0][:, 0].any() and not I[1][:, -1].any() and not I[2][0].any() and not I[3][-1].any()
        got, img = hip.compare_at(0, [p[0] for p in ps], [p[1] for p in ps], threshold=16, normalize=norm, diff=True)
        ref.assert_rows(got, rows, f"borders norm={norm}")
        assert np.array_equal(img, diffs)


# ---- after a search -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PARITY))
def test_compare_of_results(hip, templates, case):
    s, t, prm = _scene(templates, case)
    th, tw = t.shape
    gpu, orc, _, _ = _run_both(hip, s, t, **prm)
    assert len(orc) >= PARITY[case] and _tuples(gpu) == orc
    _check_last(hip, s, t, _qt_poses(gpu), case, rects=(None, (3, 2, tw - 5, th - 4)), thresholds=(16, 0, 255))
    # threshold 255: nothing can exceed it -- the empty box's encoding
    got = hip.last_compare(0, threshold=255)
    assert (got["n_over"] == 0).all() and (got["x0"] == tw).all() and (got["y0"] == th).all()
    assert (got["x1"] == -1).all() and (got["y1"] == -1).all()
    # the user-defined rectangle is the default once set and inside the template; one that is not is ignored
    try:
        hip.setUserDefinedRect((3, 2, tw - 5, th - 4))
        ref.assert_rows(hip.last_compare(0), _expect(s, t, _qt_poses(gpu), (3, 2, tw - 5, th - 4), 16, False)[0], "user rect")
        hip.setUserDefinedRect((-3, -3, tw + 6, th + 6))
        ref.assert_rows(hip.last_compare(0), _expect(s, t, _qt_poses(gpu), None, 16, False)[0], "user rect outside")
    finally:
        hip._user_rect = None


def test_mfc_semantics_uses_the_raw_pose(hip, templates):
    s, t, prm = _scene(templates, "dst3_range")
    o = oracle.OracleMatcher()
    hip.resetParams()
    for k, v in {**prm, "semantics": SEMANTICS_MFC}.items():
        setattr(o.params, k, v)
        setattr(hip._params, k, v)
    for k, v in enumerate((-40.0, -1.0, 0.0, 40.0)):   # as tests/test_gpu_patches.py: the case's +-40 degrees as two ranges
        o.params.tolerance[k] = v
        hip._params.tolerance[k] = v
    assert o.learnPattern(t) and hip.learnPattern(t)
    gpu, orc = hip.match(s), o.match(s)
    assert len(orc) >= 2 and _tuples(gpu) == orc
    assert all(abs(r.dMatchedAngle) < 40 for r in gpu)   # so the reported angle is the exact negation of dMatchAngle
    _check_last(hip, s, t, [(r.ptLT, -r.dMatchedAngle) for r in gpu], "mfc")


def test_fast_mode_uses_the_doubled_layer1_pose(hip, templates):
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
    _check_last(hip, s, t, _qt_poses(exp), "fast mode")


def test_bitwise_not_compares_the_inverted_plane(hip, templates):
    s, t, prm = _scene(templates, "dst10_multi")
    inv = np.ascontiguousarray(255 - s)
    hip.resetParams()
    for k, v in {**prm, "bitwise_not": 1}.items():
        setattr(hip._params, k, v)
    assert hip.learnPattern(t)
    got = hip.match(inv)
    assert len(got) >= 3
    _check_last(hip, s, t, _qt_poses(got), "bitwise not")   # 255 - inv = s is what was searched, and what is compared


# ---- normalisation --------------------------------------------------------------------------------------------------
def test_normalisation_absorbs_gain_and_offset(hip, templates):
    s, t, prm = _scene(templates, "dst10_multi")
    dim = np.clip(np.rint(0.8 * s.astype(np.float64) + 20.0), 0, 255).astype(np.uint8)
    hip.resetParams()
    for k, v in prm.items():
        setattr(hip._params, k, v)
    assert hip.learnPattern(t)
    res = hip.match(dim)
    assert len(res) >= 3
    _check_last(hip, dim, t, _qt_poses(res), "dimmed")
    raw, nrm = hip.last_compare(0), hip.last_compare(0, normalize=True)
    assert (nrm["sum_abs"] < raw["sum_abs"]).all(), (nrm["sum_abs"], raw["sum_abs"])
    assert (raw["gain"] == 1.0).all() and (raw["offset"] == 0.0).all()
    assert ((nrm["gain"] > 1.1) & (nrm["gain"] < 1.4)).all() and (nrm["offset"] < 0).all()   # about 1 / 0.8 and -20 / 0.8


# ---- planted defect -------------------------------------------------------------------------------------------------
def test_planted_defect(hip, templates):
    t = templates["Dst10"]
    th, tw = t.shape
    # a 6 x 5 block of the template none of whose pixels is within 16 of its own inversion
    far = np.abs(255 - 2 * t.astype(np.int32)) > 16
    spots = [(bx, by) for by in range(4, th - 9) for bx in range(4, tw - 10) if far[by:by + 5, bx:bx + 6].all()]
    assert spots
    bx, by = spots[len(spots) // 2]
    s = synth.noise(320, 240, 128, 10, 41)
    px, py = 130, 90
    synth.paste(s, t, px, py)
    blk = s[py + by:py + by + 5, px + bx:px + bx + 6]
    blk[...] = 255 - blk
    hip.resetParams()
    hip._params.max_pos = 1
    assert hip.learnPattern(t)
    res = hip.match(s)
    assert len(res) == 1 and res[0].ptLT == (float(px), float(py)) and res[0].dMatchedAngle == 0.0
    _check_last(hip, s, t, _qt_poses(res), "defect")
    got = hip.last_compare(0, threshold=16)[0]
    assert got["n_over"] == 30 and got["max_abs"] == int(np.abs(255 - 2 * t[by:by + 5, bx:bx + 6].astype(np.int32)).max())
    assert (got["x0"], got["y0"], got["x1"], got["y1"]) == (bx, by, bx + 5, by + 4)
    inner = (2, 3, tw - 4, th - 5)    # in rectangle coordinates the box moves with the rectangle's origin
    got = hip.last_compare(0, inner, threshold=16)[0]
    assert (got["x0"], got["y0"], got["x1"], got["y1"]) == (bx - 2, by - 3, bx + 3, by + 1)


# ---- batch, determinism, strides --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(templates):
    """3 sources of 320 x 240 with 2, 0, 1 pasted hits."""
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


def test_batch_all_sources_and_compare_at(hip, batch):
    t, prm, srcs = batch
    res = _search_batch(hip, batch)
    for norm in (False, True):
        allr, alld = hip.last_compare(-1, normalize=norm, diff=True)
        exp = [_expect(srcs[k], t, _qt_poses(res[k]), None, 16, norm) for k in range(3)]
        ref.assert_rows(allr, exp[0][0] + exp[1][0] + exp[2][0], f"all sources norm={norm}")
        assert np.array_equal(alld, np.concatenate([e[1] for e in exp]))
        per = [hip.last_compare(k, normalize=norm) for k in range(3)]
        assert [len(p) for p in per] == [2, 0, 1] and np.concatenate(per).tobytes() == allr.tobytes()
        idx = [k for k in range(3) for _ in res[k]]
        ps = [p for k in range(3) for p in _qt_poses(res[k])]
        at, atd = hip.compare_at(idx, [p[0] for p in ps], [p[1] for p in ps], normalize=norm, diff=True)
        assert at.tobytes() == allr.tobytes() and np.array_equal(atd, alld)
        # determinism: the record does not depend on the order in which the workgroups add to it
        again, againd = hip.last_compare(-1, normalize=norm, diff=True)
        assert again.tobytes() == allr.tobytes() and np.array_equal(againd, alld)


def test_difference_image_strides_and_capacity(hip, batch):
    t, prm, srcs = batch
    _search_batch(hip, batch)
    rect = (1, 2, 49, 18)
    x, y, w, h = rect
    stats, dense = hip.last_compare(-1, rect, diff=True)
    r = L.PatchRect(*rect)
    n = C.c_int32()
    for norm in (0, L.COMPARE_NORMALIZE):
        exp_s, exp_d = hip.last_compare(-1, rect, normalize=bool(norm), diff=True)
        buf = np.full((3, h + 1, w + 7), 0xA5, np.uint8)    # rows 7 bytes wider than w, a spare row per image
        out = np.zeros(3, COMPARE_DTYPE)
        rc = hip._lib.fpm_last_compare(hip._ctx, C.byref(r), -1, 16, norm, out.ctypes.data_as(C.POINTER(L.CompareStats)), 3,
                                       C.byref(n), L.u8ptr(buf), w + 7, (w + 7) * (h + 1))
        assert rc == L.FPM_OK and n.value == 3 and out.tobytes() == exp_s.tobytes()
        assert np.array_equal(buf[:, :h, :w], exp_d)
        buf[:, :h, :w] = 0xA5
        assert (buf == 0xA5).all(), "bytes outside the difference images were written"
    # one row too few: the count, FPM_E_CAPACITY, nothing written
    out = np.zeros(3, COMPARE_DTYPE)
    buf = np.full((3, h, w), 0x5A, np.uint8)
    rc = hip._lib.fpm_last_compare(hip._ctx, C.byref(r), -1, 16, 0, out.ctypes.data_as(C.POINTER(L.CompareStats)), 2,
                                   C.byref(n), L.u8ptr(buf), w, w * h)
    assert rc == L.FPM_E_CAPACITY and n.value == 3 and (buf == 0x5A).all() and out.tobytes() == bytes(out.nbytes)
    # bad strides, threshold, flags
    for args in [(16, 0, w - 1, w * h), (16, 0, w, w * h - 1), (256, 0, w, w * h), (-1, 0, w, w * h), (16, 2, w, w * h)]:
        rc = hip._lib.fpm_last_compare(hip._ctx, C.byref(r), -1, args[0], args[1],
                                       out.ctypes.data_as(C.POINTER(L.CompareStats)), 3, C.byref(n), L.u8ptr(buf), args[2],
                                       args[3])
        assert rc == L.FPM_E_INVALID_ARG and (buf == 0x5A).all(), args


# ---- state ----------------------------------------------------------------------------------------------------------
def test_state_rules(gpu_matcher_factory, batch):
    t, prm, srcs = batch
    th, tw = t.shape
    m = gpu_matcher_factory(**prm)
    n = C.c_int32(-1)
    assert m._lib.fpm_last_compare(m._ctx, None, 0, 16, 0, None, 0, C.byref(n), None, 0, 0) == L.FPM_E_NOT_LEARNED
    with pytest.raises(ValueError):
        m.last_compare()                               # no template
    assert m.learnPattern(t)
    with pytest.raises(ValueError, match="no staged sources"):
        m.last_compare()
    m.stage(srcs)
    with pytest.raises(ValueError, match="no search has run"):
        m.last_compare()
    m.match_staged_launch()
    with pytest.raises(ValueError, match="in flight"):
        m.last_compare()
    with pytest.raises(ValueError, match="in flight"):
        m.compare_at(0, [(10.0, 10.0)], [0.0])
    counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [2, 0, 1]
    assert len(m.last_compare(0)) == 2 and len(m.last_compare(1)) == 0
    for bad in [(0, 0, 0, 4), (-1, 0, 4, 4), (0, 0, tw + 1, th), (1, 0, tw, th), (0, 1, tw, th), (0, 0, tw, th + 1)]:
        with pytest.raises(ValueError):
            m.last_compare(0, bad)
        n = C.c_int32(-1)   # and the library's own check of the rectangle
        assert m._lib.fpm_last_compare(m._ctx, C.byref(L.PatchRect(*bad)), 0, 16, 0, None, 0, C.byref(n), None, 0, 0) == \
            L.FPM_E_INVALID_ARG and n.value == 0
    with pytest.raises(ValueError):
        m.last_compare(3)                              # source index past the batch
    m.stage(srcs)                                      # staged again, not searched
    with pytest.raises(ValueError, match="no search has run"):
        m.last_compare()
    assert len(m.compare_at(2, [(10.0, 10.0)], [5.0])) == 1   # poses of the caller's need no search
    with pytest.raises(ValueError):
        m.compare_at(3, [(10.0, 10.0)], [5.0])
    m.match_staged_candidates()                        # a search without results
    none, img = m.last_compare(-1, diff=True)
    assert none.shape == (0,) and none.dtype == COMPARE_DTYPE and img.shape == (0, th, tw)
    m.clearPattern()
    with pytest.raises(ValueError):
        m.last_compare(0)


# ---- profile --------------------------------------------------------------------------------------------------------
def test_profile_counts_the_launches(hip, batch):
    t, prm, srcs = batch
    th, tw = t.shape
    _search_batch(hip, batch)
    hip.profile(True)
    try:
        hip.profile_reset()
        hip.last_compare(-1)
        ms, launches, nbytes = hip.profile_get(L.K_COMPARE)
        assert launches == 1 and nbytes == 2 * 3 * tw * th and ms > 0
        assert hip.profile_get(L.K_PATCH)[1] == 0      # no patch is written: k_patch_warp does not run
        hip.profile_reset()
        hip.last_compare(-1, normalize=True, diff=True)
        ms, launches, nbytes = hip.profile_get(L.K_COMPARE)
        assert launches == 2 and nbytes == (2 + 3) * 3 * tw * th
        assert L.KERNEL_NAMES[L.K_COMPARE] == "patch_compare" and len(L.KERNEL_NAMES) == 15
    finally:
        hip.profile(False)
