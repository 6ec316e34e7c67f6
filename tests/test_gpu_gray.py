"""The gray-value tools on the HIP path (fpm_histogram_at / fpm_last_histogram / fpm_segment_at / fpm_last_segment):
k_patch_hist's histograms and k_patch_threshold's images, with the blobs cut from them, against the restatement of
tests/gray_ref.py (the oracle's warpAffine of fpm_patch_matrix's matrix, np.bincount, Otsu in Python floats in the
header's order, blobs_ref).  Every comparison is ==; a truncated hit goes through blobs_ref.accept."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import gray_ref as ref
from tests.cases import CASES
from tests.test_gpu_align import EDGE_POSES

pytestmark = pytest.mark.gpu

SW, SH = 203, 157
TEMPLATES = [(67, 35), (130, 33)]
WIDTHS = [1, 3, 4, 5, 63, 64, 65]
HEIGHTS = [1, 15, 16, 17, 33]
# the template's rectangle across each side of the 203 x 157 source, and one pose wholly outside
SIDE_POSES = [((-20.0, 50.0), 0.0), ((180.0, 60.25), 0.0), ((60.5, -15.0), 0.0), ((40.0, 140.0), 0.0)]
FAR_POSE = ((5000.0, 5000.0), 0.0)
POSES = EDGE_POSES + SIDE_POSES + [FAR_POSE]
MASKS = ["none", "ones", "zeros", "ellipse", "checker", "tile", "mixed"]


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


def _source(seed=203):
    return np.random.default_rng(seed).integers(0, 256, (SH, SW), dtype=np.uint8)


def _template(tw, th):
    return np.random.default_rng(tw).integers(0, 256, (th, tw), dtype=np.uint8)


def rects_for(tw, th):
    """The whole template, every x & 3, every width with every height, the last column and the last row."""
    rs = [(0, 0, tw, th)] + [(x, x % 2, 9, 7) for x in range(4)]
    for i, w in enumerate(WIDTHS):
        for j, h in enumerate(HEIGHTS):
            rs.append((min((i + j) % 4, tw - w), min((2 * i + j) % 3, th - h), w, h))
    rs += [(tw - 1, 0, 1, th), (0, th - 1, tw, 1), (tw - 5, th - 3, 5, 3)]
    assert {r[0] & 3 for r in rs} == {0, 1, 2, 3} and all(r[0] + r[2] <= tw and r[1] + r[3] <= th for r in rs)
    return rs


def mask_for(name, tw, th):
    v, u = np.mgrid[0:th, 0:tw]
    if name == "none":
        return None
    if name == "ones":
        return np.ones((th, tw), np.uint8)
    if name == "zeros":
        return np.zeros((th, tw), np.uint8)
    if name == "ellipse":
        return ((((u - (tw - 1) / 2) / (tw / 2.2)) ** 2 + ((v - (th - 1) / 2) / (th / 2.2)) ** 2) <= 1).astype(np.uint8)
    if name == "checker":
        return ((u + v) % 2).astype(np.uint8)
    if name == "tile":                      # the first 64 x 16 tile of the whole-template rectangle ignored
        m = np.ones((th, tw), np.uint8)
        m[:16, :64] = 0
        return m
    m = np.array([0, 1, 128, 255], np.uint8)[(u * 7 + v * 3) % 4]     # every non-zero byte counts alike
    return np.ascontiguousarray(m)


_patches = {}


def _patch(key, src, rect, pose):
    """The reference patch of (source key, rectangle, pose): computed once, shared, left unchanged."""
    k = (key, rect, pose)
    if k not in _patches:
        p = ref.patch(src, rect, *pose)
        p.setflags(write=False)
        _patches[k] = p
    return _patches[k]


def _expect_hist(key, src, rects, poses, mask):
    out = np.zeros((len(poses), len(rects), 256), np.uint32)
    for i, pose in enumerate(poses):
        for k, r in enumerate(rects):
            out[i, k] = ref.histogram(_patch(key, src, r, pose), ref.used(mask, r))
    return out


def _setup(hip, tw, th, srcs, mask=None):
    hip.resetParams()
    hip.gray_set_run(0)
    assert hip.learnPattern(_template(tw, th))
    hip.stage(srcs)
    if mask is not None:
        hip.set_mask(mask)


def _at(poses):
    return [0] * len(poses), [p[0] for p in poses], [p[1] for p in poses]


# ---- histograms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("tw,th", TEMPLATES)
def test_histogram_parity(hip, tw, th, mask_name):
    src, mask = _source(), mask_for(mask_name, tw, th)
    _setup(hip, tw, th, [src], mask)
    rects = rects_for(tw, th)
    got = hip.histogram_at(*_at(POSES), rects=rects)
    exp = _expect_hist("rand", src, rects, POSES, mask)
    assert got.dtype == np.uint32 and got.shape == exp.shape
    bad = np.argwhere((got != exp).any(axis=2))
    assert not len(bad), f"{mask_name}: (pose, rect) {bad[:6].tolist()} of {len(bad)}: rect {rects[bad[0][1]]}"
    n = np.array([int(ref.used(mask, r).sum()) for r in rects])
    assert (got.sum(axis=2) == n[None, :]).all()
    if mask is not None:
        assert n.tolist() == [hip.mask_count(r) for r in rects]
    assert (got[-1, :, 0] == n).all()                              # wholly outside: every used pixel in bin 0
    if mask_name == "zeros":
        assert not got.any()
    # the whole template by default, and results do not depend on the run length
    whole = hip.histogram_at(*_at(POSES))
    assert whole.shape == (len(POSES), 1, 256) and np.array_equal(whole[:, 0], exp[:, 0])
    for run in (1, 2, 0):
        hip.gray_set_run(run)
        assert hip.histogram_at(*_at(POSES), rects=rects).tobytes() == got.tobytes(), f"run {run}"


def test_rect_counts_and_permutation(hip):
    tw, th = TEMPLATES[0]
    src = _source()
    _setup(hip, tw, th, [src])
    rects = rects_for(tw, th)
    rects += [(k % 7, k % 5, 10 + 2 * k, 3 + k % 20) for k in range(64 - len(rects))]
    assert len(rects) == 64 and len({(r[2], r[3]) for r in rects}) > 40
    poses = POSES[:5]
    exp = _expect_hist("rand", src, rects, poses, None)
    for sel in ([7], [0, 40, 12], list(range(64))):
        got = hip.histogram_at(*_at(poses), rects=[rects[k] for k in sel])
        assert np.array_equal(got, exp[:, sel]), f"n_rects {len(sel)}"
    perm = list(np.random.default_rng(9).permutation(64))
    got = hip.histogram_at(*_at(poses), rects=[rects[k] for k in perm])
    assert np.array_equal(got, exp[:, perm])
    one = hip.histogram_at(*_at(poses), rects=rects[7])            # a single (x, y, w, h)
    assert np.array_equal(one[:, 0], exp[:, 7])


def test_contention_and_counter_width(hip):
    """Flat and few-valued regions, where every lane of a wave meets one bin, and a region of 70 720 equal pixels,
    which no 16-bit partial count survives."""
    tw, th = TEMPLATES[1]
    vv, uu = np.mgrid[0:SH, 0:SW]
    srcs = [np.zeros((SH, SW), np.uint8), np.full((SH, SW), 255, np.uint8),
            np.where(uu % 2 == 0, 17, 240).astype(np.uint8), ((uu + vv) % 256).astype(np.uint8)]
    _setup(hip, tw, th, srcs)
    rects = [(0, 0, tw, th), (1, 0, 64, 33), (3, 1, 65, 17), (2, 2, 5, 15)]
    poses = [POSES[0], POSES[1], SIDE_POSES[0]]
    for s, src in enumerate(srcs):
        got = hip.histogram_at([s] * len(poses), [p[0] for p in poses], [p[1] for p in poses], rects=rects)
        assert np.array_equal(got, _expect_hist(("flat", s), src, rects, poses, None)), f"source {s}"
    inside = hip.histogram_at([0, 1, 2], [POSES[0][0]] * 3, [0.0] * 3)[:, 0]
    assert inside[0, 0] == tw * th and inside[1, 255] == tw * th and inside[2, 17] + inside[2, 240] == tw * th
    # 520 x 136 = 70 720 pixels of one value
    big = np.full((200, 600), 200, np.uint8)
    hip.resetParams()
    assert hip.learnPattern(np.random.default_rng(3).integers(0, 256, (136, 520), dtype=np.uint8))
    hip.stage([big])
    for run in (1, 2, 0):
        hip.gray_set_run(run)
        h = hip.histogram_at([0], [(40.0, 30.0)], [0.0])[0, 0]
        assert h[200] == 70720 and h.sum() == 70720, f"run {run}: {h[200]}"
    hip.gray_set_run(0)
    h = hip.histogram_at([0], [(40.25, 30.5)], [10.0])[0, 0]      # rotated: border zeros beside the 200s
    assert np.array_equal(h, ref.histogram(ref.patch(big, (0, 0, 520, 136), (40.25, 30.5), 10.0), np.ones((136, 520), bool)))


# ---- segmentation ---------------------------------------------------------------------------------------------------
def _bimodal(seed=31):
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(0, 2, (20, 26)), np.ones((8, 8), np.int64))[:SH, :SW]
    img = np.where(blocks == 1, 190, 60) + rng.integers(-25, 26, (SH, SW))
    salt = rng.random((SH, SW)) < 0.03
    img[salt] = rng.integers(0, 256, int(salt.sum()))
    img[5:9, 5:9] = [[0, 1, 254, 255]] * 4
    return np.clip(img, 0, 255).astype(np.uint8)


SEG_POSES = EDGE_POSES + [SIDE_POSES[0], ((5.0, 5.0), 0.0)]


def _segment_at(hip, srcs, idx, poses, rect, threshold, polarity, connectivity, min_area, cap, mask, label):
    lts, angs = [p[0] for p in poses], [p[1] for p in poses]
    got = hip.segment_at(idx, lts, angs, rect=rect, threshold=threshold, polarity=polarity, min_area=min_area,
                         connectivity=connectivity, cap=cap, image=True)
    ref.assert_segment(got, srcs, idx, lts, angs, rect, threshold, polarity, connectivity, min_area, cap, mask, label)
    return got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("polarity", [1, -1])
def test_fixed_thresholds(hip, polarity, connectivity):
    tw, th = TEMPLATES[0]
    src = _bimodal()
    _setup(hip, tw, th, [src])
    rect, cap = (0, 0, tw, th), (tw * th + 1) // 2
    fg = 0
    for t in (0, 1, 127, 254, 255):
        for min_area in (1, 4):
            info, summary, blobs, img = _segment_at(hip, [src], [0] * len(SEG_POSES), SEG_POSES, rect, t, polarity,
                                                    connectivity, min_area, cap, None, f"t {t} min_area {min_area}")
            assert (info["threshold"] == t).all() and not (summary["flags"] & L.BLOBS_TRUNCATED).any()
            fg += int(summary["fg_pixels"].sum())
            # a fixed threshold takes no histogram: only the outside flag, on the poses that leave the source (the
            # rectangle turned by -137.5 degrees about its corner, and the one across the left side)
            assert info["flags"].tolist() == [0, 0, L.GRAY_OUTSIDE, L.GRAY_OUTSIDE, 0]
            if (t, polarity) in ((255, 1), (0, -1)):
                assert not img.any() and not summary["n_components"].any()
    assert fg > 1000
    # without the images the records are the same bytes
    a = hip.segment_at(*_at(SEG_POSES), rect=rect, threshold=127, polarity=polarity, connectivity=connectivity, cap=cap)
    b = hip.segment_at(*_at(SEG_POSES), rect=rect, threshold=127, polarity=polarity, connectivity=connectivity, cap=cap,
                       image=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("mask_name", ["none", "ellipse", "zeros"])
def test_otsu_per_hit(hip, mask_name):
    tw, th = TEMPLATES[0]
    srcs = [_bimodal(), np.full((SH, SW), 77, np.uint8), _bimodal(32) // 2]
    mask = mask_for(mask_name, tw, th)
    _setup(hip, tw, th, srcs, mask)
    rect = (2, 1, 64, 33)
    poses = SEG_POSES + [((40.0, 30.0), 0.0), ((50.5, 40.25), 12.0), ((60.0, 50.0), -30.0)]
    idx = [0] * len(SEG_POSES) + [1, 1, 2]
    hist = hip.histogram_at(idx, [p[0] for p in poses], [p[1] for p in poses], rects=[rect])[:, 0]
    stats = M.hist_derive(hist)
    for polarity in (1, -1):
        info, summary, blobs, img = _segment_at(hip, srcs, idx, poses, rect, "otsu", polarity, 8, 4,
                                                (rect[2] * rect[3] + 1) // 2, mask, f"otsu {polarity} {mask_name}")
        assert info["threshold"].tolist() == (stats["otsu"] + (polarity < 0)).tolist()
        assert (info["flags"] & 3).tolist() == stats["flags"].tolist() and (info["n"] == stats["n"]).all()
        flagged = (info["flags"] & (L.HIST_EMPTY | L.HIST_FLAT)) != 0
        assert not img[flagged].any() and not summary["fg_pixels"][flagged].any()
        if mask_name == "zeros":
            assert ((info["flags"] & 3) == L.HIST_EMPTY).all() and not info["n"].any()
        else:
            # the constant source's hits are flat (the rotated ones too: they lie inside it), the others are not
            assert ((info["flags"] & 3) != 0).tolist() == [False] * len(SEG_POSES) + [True, True, False]
            assert (info["flags"][5:7] & 3 == L.HIST_FLAT).all() and summary["fg_pixels"][:3].all()
        out = ((info["flags"] & L.GRAY_OUTSIDE) != 0).tolist()
        assert out == [ref.outside(SW, SH, rect, *p) for p in poses] and out[:2] == [False, False] and out[3] and not any(out[4:])


def test_more_blobs_than_capacity(hip):
    tw, th = TEMPLATES[0]
    vv, uu = np.mgrid[0:SH, 0:SW]
    src = np.where((uu % 2 == 0) & (vv % 2 == 0), 20, 220).astype(np.uint8)     # isolated dark pixels
    _setup(hip, tw, th, [src])
    rect = (0, 0, tw, th)
    for cap in (1, 8):
        info, summary, blobs, _ = _segment_at(hip, [src], [0, 0], [((40.0, 30.0), 0.0), ((41.0, 31.0), 0.0)], rect, 128, -1,
                                              4, 1, cap, None, f"cap {cap}")
        assert (summary["flags"] == L.BLOBS_TRUNCATED).all() and (summary["n_returned"] == cap).all()
        assert summary["n_blobs"].min() > 500 and all(len(b) == cap for b in blobs)
    info, summary, blobs, _ = _segment_at(hip, [src], [0], [((40.0, 30.0), 0.0)], rect, "otsu", -1, 8, 1, 64, None, "otsu")
    assert info["threshold"][0] == 21 and summary["flags"][0] == L.BLOBS_TRUNCATED


# ---- over the hits of a search ----------------------------------------------------------------------------------------
def _search(m, templates, bitwise_not=False):
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    m.resetParams()
    m.gray_set_run(0)
    for k, v in prm.items():
        setattr(m._params, k, v)
    m.setBitwiseNot(bitwise_not)
    assert m.learnPattern(t)
    m.stage([np.ascontiguousarray(255 - s) if bitwise_not else s])
    res = m.match_staged()
    assert len(res[0]) == 3
    ps = [(r.ptLT, r.dMatchedAngle) for r in res[0]]     # Qt semantics: the raw pose
    return s, t, [p[0] for p in ps], [p[1] for p in ps]


def _hit_rects(t):
    th, tw = t.shape
    return [(0, 0, tw, th), (3, 2, tw // 2, th // 2), (tw - 9, th - 7, 9, 7)]


def _check_last(m, s, t, lts, angs, mask, label):
    rects = _hit_rects(t)
    got = m.last_histogram(rects, source=0)
    exp = np.stack([np.stack([ref.histogram(ref.patch(s, r, lt, a), ref.used(mask, r)) for r in rects])
                    for lt, a in zip(lts, angs)])
    assert np.array_equal(got, exp), label
    assert got.tobytes() == m.histogram_at(0, lts, angs, rects=rects).tobytes()
    assert got.tobytes() == m.last_histogram(rects, source=-1).tobytes()
    rect, cap = rects[1], (rects[1][2] * rects[1][3] + 1) // 2
    seg = m.last_segment(rect, source=0, threshold="otsu", polarity=-1, min_area=2, connectivity=8, cap=cap, image=True)
    ref.assert_segment(seg, [s], [0, 0, 0], lts, angs, rect, "otsu", -1, 8, 2, cap, mask, label)
    at = m.segment_at(0, lts, angs, rect=rect, threshold="otsu", polarity=-1, min_area=2, connectivity=8, cap=cap, image=True)
    assert seg[0].tobytes() == at[0].tobytes() and seg[1].tobytes() == at[1].tobytes() and seg[3].tobytes() == at[3].tobytes()
    return got, seg


def test_last_histogram_and_segment_after_a_search(hip, templates):
    s, t, lts, angs = _search(hip, templates)
    got, seg = _check_last(hip, s, t, lts, angs, None, "raw poses")
    assert seg[1]["fg_pixels"].all()
    # a mask: honoured while enabled; disabled or cleared, the unmasked bytes
    th, tw = t.shape
    mask = mask_for("ellipse", tw, th)
    hip.set_mask(mask)
    masked, _ = _check_last(hip, s, t, lts, angs, mask, "masked")
    assert masked.tobytes() != got.tobytes()
    hip.mask_enable(False)
    assert hip.last_histogram(_hit_rects(t)).tobytes() == got.tobytes()
    off = hip.last_segment(_hit_rects(t)[1], threshold="otsu", min_area=2, cap=len(seg[2][0]) + 64, image=True)
    assert off[0].tobytes() == seg[0].tobytes() and off[3].tobytes() == seg[3].tobytes()
    hip.mask_enable(True)
    hip.clear_mask()
    assert hip.last_histogram(_hit_rects(t)).tobytes() == got.tobytes()
    # after adoption both sample at the aligned poses
    al = hip.align_last(0, adopt=True)
    assert (al["best_eval"] > 0).any(), "no hit moved: the test shows nothing"
    alt, aang = np.stack([al["lt_x"], al["lt_y"]], 1), al["angle"]
    got2, _ = _check_last(hip, s, t, [tuple(p) for p in alt.tolist()], aang.tolist(), None, "adopted")
    assert got2.tobytes() != got.tobytes()


def test_last_histogram_under_bitwise_not(hip, templates):
    s, t, lts, angs = _search(hip, templates, bitwise_not=True)     # staged: 255 - s; sampled: the inverted plane, s
    try:
        _check_last(hip, s, t, lts, angs, None, "bitwise_not")
    finally:
        hip.setBitwiseNot(False)


# ---- state ----------------------------------------------------------------------------------------------------------
def _results(m, n_src):
    n = (C.c_int32 * n_src)()
    m._lib.fpm_last_results(m._ctx, None, 0, n)
    out = (L.Result * max(sum(n), 1))()
    assert m._lib.fpm_last_results(m._ctx, out, sum(n), n) == L.FPM_OK
    return bytes(out), list(n)


def test_state_rules(gpu_matcher_factory, templates):
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    th, tw = t.shape
    m = gpu_matcher_factory(**prm)
    one = [(10.0, 10.0)]
    for call in (lambda: m.last_histogram(), lambda: m.histogram_at(0, one, [0.0]), lambda: m.last_segment(),
                 lambda: m.segment_at(0, one, [0.0])):
        with pytest.raises((ValueError, RuntimeError)):
            call()                                              # no template
    n = C.c_int32(-1)
    assert m._lib.fpm_last_histogram(m._ctx, None, 1, 0, None, 0, C.byref(n)) == L.FPM_E_NOT_LEARNED
    assert m.learnPattern(t)
    for call in (lambda: m.last_histogram(), lambda: m.histogram_at(0, one, [0.0]), lambda: m.segment_at(0, one, [0.0])):
        with pytest.raises(ValueError, match="no staged sources"):
            call()
    m.stage([s])
    for call in (lambda: m.last_histogram(), lambda: m.last_segment()):
        with pytest.raises(ValueError, match="no search has run"):
            call()
    assert m.histogram_at(0, one, [5.0]).shape == (1, 1, 256)   # poses of the caller's need no search
    assert len(m.segment_at(0, one, [5.0])[0]) == 1
    m.match_staged_launch()
    for call in (lambda: m.last_histogram(), lambda: m.histogram_at(0, one, [0.0]), lambda: m.last_segment(),
                 lambda: m.segment_at(0, one, [0.0])):
        with pytest.raises(ValueError, match="in flight"):
            call()
    counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [3]
    mask = mask_for("ellipse", tw, th)
    m.set_mask(mask)
    m.model_train_last(source=0)
    results, cands = _results(m, 1), m.last_candidates(0).tobytes()
    patches, model = m.last_patches(0).tobytes(), [a.tobytes() for a in m.model_sums()]
    rects = (L.PatchRect * 2)(L.PatchRect(0, 0, tw, th), L.PatchRect(1, 2, 9, 7))
    hist = np.zeros((3, 2, 256), np.uint32)
    ph = hist.ctypes.data_as(C.POINTER(C.c_uint32))
    info, summary, recs = np.zeros(3, M.SEGMENT_INFO_DTYPE), np.zeros(3, M.BLOB_SUMMARY_DTYPE), np.zeros((3, 8), M.BLOB_DTYPE)
    img = np.zeros((3, th, tw), np.uint8)
    pi, ps, pr = (info.ctypes.data_as(C.POINTER(L.SegmentInfo)), summary.ctypes.data_as(C.POINTER(L.BlobSummary)),
                  recs.ctypes.data_as(C.POINTER(L.Blob)))
    pimg = L.u8ptr(img)

    def untouched():
        return not any(a.tobytes().strip(b"\0") for a in (hist, info, summary, recs, img))

    def last_seg(source=0, rect=None, t=128, pol=-1, conn=8, min_area=4, i=pi, sm=ps, r=pr, cap_per=8, cap=3, im=pimg,
                 row=tw, patch=tw * th):
        return m._lib.fpm_last_segment(m._ctx, source, rect, t, pol, conn, min_area, i, sm, r, cap_per, cap, C.byref(n), im,
                                       row, patch)

    # the count-only calls, then a capacity below the count: FPM_E_CAPACITY, nothing written
    assert m._lib.fpm_last_histogram(m._ctx, rects, 2, 0, None, 0, C.byref(n)) == L.FPM_E_CAPACITY and n.value == 3
    assert last_seg(i=None, sm=None, r=None, cap=0, im=None, row=0, patch=0) == L.FPM_E_CAPACITY and n.value == 3
    assert m._lib.fpm_last_histogram(m._ctx, rects, 2, 0, ph, 2, C.byref(n)) == L.FPM_E_CAPACITY and n.value == 3
    assert last_seg(cap=2) == L.FPM_E_CAPACITY and n.value == 3 and untouched()
    m.profile(True)
    try:
        m.profile_reset()
        # arguments out of range: FPM_E_INVALID_ARG, nothing launched, nothing written
        bad_rects = [L.PatchRect(-1, 0, 5, 5), L.PatchRect(0, 0, tw + 1, th), L.PatchRect(0, 0, 0, 5), L.PatchRect(1, 1, tw, th)]
        for nr, src_i, pr_, buf in [(0, 0, rects, ph), (65, 0, rects, ph), (2, 0, None, ph), (2, 1, rects, ph), (2, -2, rects, ph),
                                    (2, 0, rects, None)]:
            assert m._lib.fpm_last_histogram(m._ctx, pr_, nr, src_i, buf, 3, C.byref(n)) == L.FPM_E_INVALID_ARG, (nr, src_i)
        for b in bad_rects:
            two = (L.PatchRect * 2)(L.PatchRect(0, 0, tw, th), b)
            assert m._lib.fpm_last_histogram(m._ctx, two, 2, 0, ph, 3, C.byref(n)) == L.FPM_E_INVALID_ARG
            assert last_seg(rect=C.byref(b)) == L.FPM_E_INVALID_ARG
        for kw in (dict(t=-2), dict(t=256), dict(pol=0), dict(pol=2), dict(conn=6), dict(min_area=0), dict(cap_per=0),
                   dict(cap_per=65537), dict(i=None), dict(sm=None), dict(r=None), dict(source=1), dict(row=tw - 1),
                   dict(patch=tw * th - 1)):
            assert last_seg(**kw) == L.FPM_E_INVALID_ARG and untouched(), kw
        with pytest.raises(ValueError):
            m.histogram_at(1, one, [5.0])                       # source index past the batch
        with pytest.raises(ValueError):
            m.histogram_at(0, [(2e6, 10.0)], [5.0])             # beyond the samplers' range
        with pytest.raises(ValueError):
            m.segment_at(0, [(2e6, 10.0)], [5.0])
        with pytest.raises(ValueError):
            m.last_histogram([(0, 0, 5, 5)] * 65)
        with pytest.raises(ValueError):
            m.last_segment(threshold="mean")
        with pytest.raises(ValueError):
            m.gray_set_run(-1)
        assert untouched() and m.gray_profile(L.GRAY_HIST) == (0.0, 0, 0) and m.gray_profile(L.GRAY_THRESHOLD) == (0.0, 0, 0)
        # a fixed threshold: no histogram launch and one threshold launch; Otsu: one and one; a histogram call: one and none
        m.last_segment(threshold=128)
        assert m.gray_profile(L.GRAY_HIST)[1] == 0 and m.gray_profile(L.GRAY_THRESHOLD)[1] == 1
        ms, launches, nbytes = m.gray_profile(L.GRAY_THRESHOLD)
        assert ms > 0 and nbytes == 3 * 3 * tw * th              # source, mask and e bytes of three hits
        m.profile_reset()
        m.last_segment(threshold="otsu")
        assert m.gray_profile(L.GRAY_HIST)[1] == 1 and m.gray_profile(L.GRAY_THRESHOLD)[1] == 1
        assert m.gray_profile(L.GRAY_HIST)[2] == 3 * 2 * tw * th + 3 * 1024
        m.profile_reset()
        m.last_histogram([(0, 0, tw, th), (1, 2, 9, 7)])
        m.histogram_at(0, one * 4, [5.0] * 4)
        assert m.gray_profile(L.GRAY_HIST)[1] == 2 and m.gray_profile(L.GRAY_THRESHOLD)[1] == 0
        assert m.profile_get(L.K_PATCH)[1] == 0 and m.profile_get(L.K_COMPARE)[1] == 0
        assert len(L.KERNEL_NAMES) == 15 and len(L.PROFILE_NAMES) == 16     # no FPM_K_* index was added
        m.profile_reset()
        assert m.gray_profile(L.GRAY_HIST) == (0.0, 0, 0)
    finally:
        m.profile(False)
    assert untouched()
    assert m._lib.fpm_last_histogram(m._ctx, rects, 2, 0, ph, 3, C.byref(n)) == L.FPM_OK and n.value == 3
    assert hist.sum(axis=2).tolist() == [[m.mask_count(), m.mask_count((1, 2, 9, 7))]] * 3
    assert last_seg(t=L.SEG_OTSU) == L.FPM_OK and n.value == 3 and info["n"].tolist() == [m.mask_count()] * 3 and img.any()
    # the search's records, the poses, the model and the mask are what they were, and a following search returns the same
    assert _results(m, 1) == results and m.last_candidates(0).tobytes() == cands and m.last_patches(0).tobytes() == patches
    assert [a.tobytes() for a in m.model_sums()] == model and np.array_equal(m.mask() != 0, mask != 0)
    assert len(m.match_staged()[0]) == 3 and _results(m, 1) == results and m.last_candidates(0).tobytes() == cands
    m.stage([s])                                                # staged again, not searched
    with pytest.raises(ValueError, match="no search has run"):
        m.last_histogram()
    m.match_staged_candidates()                                 # a search without results
    assert m.last_histogram(source=-1).shape == (0, 1, 256)
    none = m.last_segment(source=-1, image=True)
    assert len(none[0]) == 0 and len(none[1]) == 0 and none[2] == [] and none[3].shape == (0, th, tw)
