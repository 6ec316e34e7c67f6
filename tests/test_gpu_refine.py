"""The refinement kernels at ROI level (fpm_op_refine: k_roi_small, or k_roi_tables -> k_roi_warp / k_roi_warp3 ->
k_roi_corr -> k_roi_eval, by the search's own form selection) on ROIs a search never produces, bit for bit against the
oracle's refine_roi: every record field (scores as f32 bit patterns) and, where the form materialises them, every
sampled ROI pixel.  tests/test_oracle_refine.py pins refine_roi itself on the CPU."""
import ctypes as C

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from tests import cases, oracle, refine_cases as rc

pytestmark = pytest.mark.gpu

SMALL, THREE = "small", "three-kernel"


def assert_same_records(got, exp, what=""):
    assert got.shape == exp.shape
    for f in ("mx", "my", "on_border"):
        assert np.array_equal(got[f], exp[f]), (what, f, np.argwhere(got[f] != exp[f])[:5].tolist())
    for f in ("score", "vec"):
        g, e = np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(exp[f]).view(np.uint32)
        bad = np.argwhere(g != e)
        assert not len(bad), (what, f, bad[:5].tolist(), got[f][tuple(bad[0])], exp[f][tuple(bad[0])])
    assert got.tobytes() == exp.tobytes(), what


def assert_same_pixels(got, exp, what=""):
    assert got.shape == exp.shape
    bad = np.argwhere(got != exp)
    assert not len(bad), (what, len(bad), bad[:5].tolist())


def run_refine(m, levels, lt, ang, fold, round_rois=0):
    """refine_rois with the profile counters around it: (records, pixels or None, form that ran, launches)."""
    m.profile(True)
    m.profile_reset()
    rec, px = m.refine_rois(levels, 0, lt, ang, fold, round_rois)
    n = {k: m.profile_get(k)[1] for k in (L.K_ROI_TABLES, L.K_ROI_WARP, L.K_ROI_CORR, L.K_ROI_EVAL, L.K_ROI_SMALL,
                                          L.K_CAND_STEP)}
    m.profile(False)
    assert n[L.K_CAND_STEP] == 0
    if n[L.K_ROI_SMALL]:
        assert n[L.K_ROI_TABLES] == n[L.K_ROI_WARP] == n[L.K_ROI_CORR] == n[L.K_ROI_EVAL] == 0
        return rec, px, SMALL, n[L.K_ROI_SMALL]
    assert n[L.K_ROI_TABLES] == n[L.K_ROI_WARP] == n[L.K_ROI_CORR] == n[L.K_ROI_EVAL] > 0
    return rec, px, THREE, n[L.K_ROI_EVAL]


def check(m, o, levels, lt, ang, fold, what, round_rois=0, equal1=False):
    """One op call against refine_roi; asserts the form the shape's rule (roi_small_fits) names.  Returns the form."""
    th, tw = o.template_levels()[0][0][0].shape
    S = len(levels)
    lt = np.asarray(lt, np.float32).reshape(S, -1, 2)
    ang = np.asarray(ang, np.float64).reshape(S, lt.shape[1], -1)
    rec, px, form, launches = run_refine(m, levels, lt, ang, fold, round_rois)
    assert form == (SMALL if rc.roi_small_fits(tw, th) else THREE), (what, tw, th)
    total = ang.size
    assert launches == (1 if not round_rois else -(-total // round_rois)), what
    exp_rec, exp_px = rc.oracle_refine(o, levels, 0, lt, ang, fold)
    assert_same_records(rec, exp_rec, what)
    if form == THREE and not equal1:
        assert px is not None, what
        assert_same_pixels(px, exp_px, what)
    else:
        assert px is None, what
    return form


def pair(gpu_matcher_factory, t):
    o = rc.learn_one_level(oracle.OracleMatcher(), t)
    m = rc.learn_one_level(gpu_matcher_factory(), t)
    assert m.template_info()[0] == 1 and len(o.template_levels()[0]) == 1
    return m, o


def source_for(tw, th, seed):
    """A textured level image a few hundred pixels on a side, wider than the template so that ROIs lie inside it."""
    return rc.texture(max(360, tw + 160), max(260, th + 120), seed)


def rois_for(rng, s, tw, th, n, n3, wide=False):
    """random_rois plus n // 3 ROIs centred within 20 px of the image centre (inside the image where the template fits),
    so every case has interior, partly off-image and wholly off-image ROIs."""
    h, w = s.shape
    lt, ang = rc.random_rois(rng, w, h, tw, th, n, n3, wide)
    for i in range(n // 3):
        c = ang[i, n3 // 2]
        lt[i] = rc.pasted_lt(w / 2 + rng.uniform(-20, 20), h / 2 + rng.uniform(-20, 20), tw, th, c)
    return lt, ang


# ---- map-position sweep -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tw,th", [(40, 30), (300, 65)])   # k_roi_small / the three-kernel path
@pytest.mark.parametrize("angle", [0.0, 30.0, -137.5])
def test_position_sweep(gpu_matcher_factory, tw, th, angle):
    """The maximum driven to every position of the 7x7 map (tests/test_oracle_refine.py asserts the coverage for the
    unrotated 40 x 30 sweep): every score that can become a maximum, the border ring and on_border."""
    size = (260, 220) if tw < 100 else (520, 300)
    s, t, lt, ang, _ = rc.sweep_case(tw, th, angle, 21, size)
    m, o = pair(gpu_matcher_factory, t)
    check(m, o, [s], lt, ang, True, f"sweep {tw}x{th} at {angle}")
    if angle == 0.0:
        rec, _ = m.refine_rois([s], 0, lt, ang, True)
        assert {(int(r["mx"]), int(r["my"])) for r in rec[0, :, 1]} == {(x, y) for x in range(7) for y in range(7)}
        assert int(rec[0, :, 1]["on_border"].sum()) == 24


# ---- random ROIs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("n3", [1, 3])
@pytest.mark.parametrize("tw,th", [(45, 37), (180, 120)])
def test_random_rois(gpu_matcher_factory, tw, th, n3, fold, S):
    """ptLT anywhere on the image grown by the template diagonal, centre angles over +-180: partly off-image ROIs
    (kTileInterior-clear tiles), wholly off-image ones (kTileAny-clear: all zeros, score 0 at (0, 0)); S = 3 takes the
    batch forms (k_roi_eval<40>, the two- / four-wave k_roi_small)."""
    rng = np.random.default_rng(100 * tw + 10 * n3 + 2 * fold + S)
    t = rc.texture(tw, th, 31)
    levels = [source_for(tw, th, 40 + k) for k in range(S)]
    m, o = pair(gpu_matcher_factory, t)
    n = 30 // (n3 * S) + 2
    lts, angs = zip(*[rois_for(rng, levels[k], tw, th, n, n3) for k in range(S)])
    lt, ang = np.stack(lts), np.stack(angs)
    check(m, o, levels, lt, ang, bool(fold), f"random {tw}x{th} n3={n3} fold={fold} S={S}")
    # the wholly off-image ROI of every source: all zeros, flat windows, score 0, first maximum at (0, 0)
    for k in range(S):
        assert not any(o.refine_roi(levels[k], 0, lt[k, -1], a, bool(fold))[0].any() for a in ang[k, -1])
    rec, _ = m.refine_rois(levels, 0, lt, ang, bool(fold))
    off = rec[:, -1, :]
    assert not off["score"].any() and not off["mx"].any() and not off["my"].any() and off["on_border"].all()


# ---- wide triples: k_roi_warp3's per-ROI fallback ------------------------------------------------------------------
@pytest.mark.parametrize("warp3", ["1", "0"])
def test_wide_triples(gpu_matcher_factory, monkeypatch, warp3):
    """Angle triples (a, a + 20, a - 35): the three boxes of a tile position spread over more than the wave buffer's
    64 px x 60 rows (asserted from the tile descriptors' rule), so k_roi_warp3 stages each ROI's own box; FPM_WARP3=0
    samples the same ROIs one at a time (k_roi_warp)."""
    monkeypatch.setenv("FPM_WARP3", warp3)
    tw, th = 180, 120   # 6 x 4 tiles, past what k_roi_small takes
    rng = np.random.default_rng(7)
    t = rc.texture(tw, th, 33)
    s = source_for(tw, th, 44)
    m, o = pair(gpu_matcher_factory, t)
    lt, ang = rois_for(rng, s, tw, th, 12, 3, wide=True)
    h, w = s.shape
    fallback = [rc.warp3_fallback_tiles(w, h, tw, th, lt[i], ang[i]) for i in range(len(lt))]
    assert sum(1 for f in fallback if f > 0) >= 4 and sum(fallback) >= 20, fallback
    # ... and the search's own triples (one layer step apart) never leave the union path at this shape
    near = np.stack([ang[:, 0] - rc.layer_step(tw, th), ang[:, 0], ang[:, 0] + rc.layer_step(tw, th)], 1)
    assert not any(rc.warp3_fallback_tiles(w, h, tw, th, lt[i], near[i]) for i in range(len(lt)))
    assert check(m, o, [s], lt, ang, True, f"wide triples warp3={warp3}") == THREE


# ---- shape edges ---------------------------------------------------------------------------------------------------
def _shape_case(gpu_matcher_factory, tw, th, seed, n=4, S=1, fold=True, what=""):
    rng = np.random.default_rng(seed)
    t = rc.texture(tw, th, seed)
    levels = [source_for(tw, th, seed + 1 + k) for k in range(S)]
    m, o = pair(gpu_matcher_factory, t)
    lts, angs = zip(*[rois_for(rng, levels[k], tw, th, n, 3) for k in range(S)])
    return check(m, o, levels, np.stack(lts), np.stack(angs), fold, what or f"shape {tw}x{th}")


@pytest.mark.parametrize("tw", [63, 64, 65, 256, 257, 512, 513, 768, 769, 1024, 1025])
def test_corr_k_steps(gpu_matcher_factory, tw):
    """64-column k-steps and k_roi_corr's NK = 4 / 8 / 12 / 16 register-A and slot-major forms (switching at tw = 256, 512,
    768, 1024); th = 33: one full 32-row band plus one row.  Up to tw = 512 this shape fits k_roi_small (its own banded
    correlation over the same k-steps); test_corr_k_steps_tall takes those widths to k_roi_corr."""
    assert _shape_case(gpu_matcher_factory, tw, 33, 500 + tw) == (SMALL if tw <= 512 else THREE)


@pytest.mark.parametrize("tw", [63, 64, 65, 256, 257, 512])
def test_corr_k_steps_tall(gpu_matcher_factory, tw):
    """The widths of test_corr_k_steps that k_roi_small takes at th = 33, at th = 257 (eight bands plus one row): the
    NK = 4 and 8 forms of k_roi_corr and their k-step padding."""
    assert _shape_case(gpu_matcher_factory, tw, 257, 550 + tw, n=3) == THREE


@pytest.mark.parametrize("th", [31, 32, 39, 40, 41, 47, 48, 49, 64, 65, 97, 257, 271, 288, 289])
def test_bands_and_eval_blocks(gpu_matcher_factory, th):
    """32-row bands (kBandRows) and k_roi_eval's 48-row blocks at tw = 300; the th <= 64 shapes fit k_roi_small, so
    th = 257 .. 289 reach k_roi_eval's block edges (240 + 17, 6 x 48 - 17, 6 x 48, 6 x 48 + 1)."""
    form = _shape_case(gpu_matcher_factory, 300, th, 600 + th, n=3)
    assert form == (SMALL if th <= 64 else THREE)


@pytest.mark.parametrize("th", [79, 80, 81, 257])
def test_eval_blocks_batch(gpu_matcher_factory, th):
    """k_roi_eval<40> (batches of more than two sources): block edges at 2 x 40 - 1, 2 x 40, 2 x 40 + 1, and th > 256."""
    assert _shape_case(gpu_matcher_factory, 300, th, 650 + th, n=2, S=3) == THREE


@pytest.mark.parametrize("tw", [26, 27, 58, 59])
@pytest.mark.parametrize("th", [26, 27, 58, 59])
def test_roi_tile_edges(gpu_matcher_factory, tw, th):
    """ROI sizes tw + 6, th + 6 in {32, 33, 64, 65}: one whole tile, one pixel into the next, two, two and one."""
    assert _shape_case(gpu_matcher_factory, tw, th, 700 + 64 * tw + th) == SMALL


@pytest.mark.parametrize("tw,th", [(26, 257), (27, 300), (59, 257)])
def test_roi_tile_edges_three_kernel(gpu_matcher_factory, tw, th):
    """The samplers' column-tile edges (tw + 6 = 32, 33, 65) where th > 256 takes the three-kernel path."""
    assert _shape_case(gpu_matcher_factory, tw, th, 800 + tw) == THREE


# shapes whose footprint bound (small_footprint_bound) lies just below / just above nw * ROI_FT bytes, 4 : 3
SMALL_FOOTPRINT = {128: ((55, 41), (56, 42)), 256: ((86, 64), (87, 65)), 512: ((129, 96), (130, 97))}


@pytest.mark.parametrize("nt", [128, 256, 512])
@pytest.mark.parametrize("side", [0, 1])
def test_small_footprint_paths(gpu_matcher_factory, monkeypatch, nt, side):
    """k_roi_small's U region: sized to the footprint bound below nw * ROI_FT (the whole footprint staged), capped at
    one tile buffer per wave above it (rotated ROIs then stage per-wave tiles); each of the two- / four- / eight-wave
    forms forced at its own boundary."""
    nw = nt // 64
    tw, th = SMALL_FOOTPRINT[nt][side]
    fb = rc.small_footprint_bound(tw + 6, th + 6)
    assert (fb < nw * rc.ROI_FT) == (side == 0) and abs(fb - nw * rc.ROI_FT) < 800
    assert rc.roi_small_fits(tw, th)
    monkeypatch.setenv("FPM_SMALL_NT", str(nt))
    assert _shape_case(gpu_matcher_factory, tw, th, 900 + nt + side, n=6) == SMALL


def test_small_fits_boundary(gpu_matcher_factory):
    """The largest 4 : 3 shape k_roi_small takes and the smallest it does not; the tallest narrow one (its LDS runs out
    at th = 230, below the rule's th <= 256) and the next; th = 256 and 257."""
    assert rc.roi_small_fits(150, 112) and not rc.roi_small_fits(151, 113)
    assert _shape_case(gpu_matcher_factory, 150, 112, 1001) == SMALL
    assert _shape_case(gpu_matcher_factory, 151, 113, 1002) == THREE
    assert rc.roi_small_fits(16, 230) and not rc.roi_small_fits(16, 231)
    assert _shape_case(gpu_matcher_factory, 16, 230, 1003) == SMALL
    assert _shape_case(gpu_matcher_factory, 16, 231, 1004) == THREE
    assert _shape_case(gpu_matcher_factory, 16, 256, 1005) == THREE
    assert _shape_case(gpu_matcher_factory, 16, 257, 1006) == THREE


@pytest.mark.parametrize("tw,th", [(40, 30), (60, 300)])
def test_constant_template(gpu_matcher_factory, tw, th):
    """matResult = 1 (vecResultEqual1): a map of ones, so score 1 at (0, 0), on the border, for every ROI."""
    t = np.full((th, tw), 77, np.uint8)
    s = source_for(tw, th, 55)
    m, o = pair(gpu_matcher_factory, t)
    assert o.template_levels()[0][0][4] and m.template_level(0)[4]
    lt, ang = rois_for(np.random.default_rng(3), s, tw, th, 5, 3)
    check(m, o, [s], lt, ang, True, f"constant {tw}x{th}", equal1=True)
    rec, px = m.refine_rois([s], 0, lt, ang, True)
    assert px is None
    assert (rec["score"] == 1).all() and not rec["mx"].any() and not rec["my"].any() and rec["on_border"].all()
    assert not rec["vec"].any()


# ---- rounds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tw,th", [(45, 37), (180, 120)])
def test_rounds(gpu_matcher_factory, tw, th):
    """Bounded-scratch rounds (slot_base > 0): 21 ROIs in rounds of 9 (9, 9, 3) give the one-round call's records."""
    rng = np.random.default_rng(17)
    t = rc.texture(tw, th, 35)
    s = source_for(tw, th, 46)
    m, o = pair(gpu_matcher_factory, t)
    lt, ang = rois_for(rng, s, tw, th, 7, 3)
    one, px1 = m.refine_rois([s], 0, lt, ang, True)
    check(m, o, [s], lt, ang, True, f"rounds {tw}x{th}", round_rois=9)
    three, px3 = m.refine_rois([s], 0, lt, ang, True, 9)
    assert one.tobytes() == three.tobytes()
    assert (px1 is None) == (px3 is None) and (px1 is None or np.array_equal(px1, px3))


# ---- the layers of a search ----------------------------------------------------------------------------------------
def test_search_layers(gpu_matcher_factory, templates):
    """Every refinement ROI of a real search (dst10_multi), taken from the oracle's trace: the op on the oracle's own
    pyramid level gives the trace's score and location."""
    build, prm = cases.CASES["dst10_multi"]
    s, t = build(templates)
    o = oracle.OracleMatcher().set(**prm).set_trace(True)
    assert o.learnPattern(t) and o.match(s)
    tr = o.trace()
    m = gpu_matcher_factory(**prm)
    assert m.learnPattern(t)
    level = s
    layers = sorted(set(int(l) for l in tr["layer"]))
    assert layers == list(range(m.template_info()[0] - 1))
    for layer in layers:
        rows = tr[tr["layer"] == layer]
        rec, _ = m.refine_rois([level], layer, rows["lt"], rows["angle"], True)
        assert np.array_equal(rec[0]["score"].astype(np.float64), rows["score"]), layer
        assert np.array_equal(rec[0]["mx"], rows["x"]) and np.array_equal(rec[0]["my"], rows["y"]), layer
        exp = np.zeros(rec.shape, oracle.ROI_RECORD_DTYPE)
        for i, row in enumerate(rows):
            for j in range(3):
                exp[0, i, j] = o.refine_roi(level, layer, row["lt"], row["angle"][j], True)[2]
        assert_same_records(rec, exp, f"search layer {layer}")
        level = oracle.pyr_down(level)


# ---- argument validation (needs a context, so a device) -------------------------------------------------------------
def test_argument_validation(gpu_matcher_factory):
    m = gpu_matcher_factory()
    s = rc.texture(64, 48, 1)
    lt, ang = np.zeros((1, 1, 2), np.float32), np.zeros((1, 1, 3))

    def call(layer=0, lt=lt, ang=ang, rounds=0):
        lt = np.ascontiguousarray(lt, np.float32)
        ang = np.ascontiguousarray(ang, np.float64)
        rec = np.zeros(ang.shape, oracle.ROI_RECORD_DTYPE)
        wrote = C.c_int32()
        ptrs = (L._U8P * 1)(L.u8ptr(s))
        return m._lib.fpm_op_refine(m._ctx, ptrs, 1, 64, 48, s.strides[0], layer, lt.ctypes.data_as(C.POINTER(C.c_float)),
                                    ang.ctypes.data_as(C.POINTER(C.c_double)), lt.shape[1], ang.shape[2], 1, rounds,
                                    rec.ctypes.data_as(C.POINTER(L.RoiRecord)), None, C.byref(wrote))

    assert call() == L.FPM_E_NOT_LEARNED
    rc.learn_one_level(m, rc.texture(20, 16, 2))
    assert call() == L.FPM_OK
    assert call(layer=1) == call(layer=-1) == L.FPM_E_INVALID_ARG
    assert call(ang=np.zeros((1, 1, 2))) == L.FPM_E_INVALID_ARG            # n3 = 2
    assert call(rounds=2) == call(rounds=-3) == L.FPM_E_INVALID_ARG        # not a multiple of n3
    assert call(rounds=3) == L.FPM_OK
    for bad in (np.nan, np.inf, -np.inf):
        assert call(lt=np.array([[[bad, 0]]])) == L.FPM_E_INVALID_ARG
        assert call(ang=np.array([[[0, bad, 0]]])) == L.FPM_E_INVALID_ARG
    assert call(lt=np.array([[[1e6, 0]]])) == L.FPM_E_INVALID_ARG          # beyond the fixed-point tables' range
