"""k_roi_corr's window sums as band totals and edge rows (RoiArgs::wtot / wtotq / wedge) and k_roi_eval's rebuild of the
49 sums from them: fpm_op_refine on the large-template path, every record field bit for bit against the oracle's
refine_roi, at the smallest shapes that reach each form of k_roi_corr and each edge of the bookkeeping.

No shape with th < 6 reaches a register-A form: roi_small_fits takes every th <= 5 up to tw = 1344, past the widest
register-A template (960); 1345 x 5 takes the slot-major form and is the head / tail overlap case here."""
import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from tests import oracle, refine_cases as rc

pytestmark = pytest.mark.gpu

N_ROIS = 24        # per call: 24 candidates at n3 = 1, 8 triples at n3 = 3
ROUND_ROIS = 15    # two rounds: 15 + 9 ROIs (whole candidates at n3 = 3)


def corr_form(tw):
    """launch_roi_corr restated: the register-A form's NK (4 / 8 / 12 / 16), or 0 for the slot-major form."""
    pitch, nk = rc.roi_pitch(tw), (tw + 63) // 64
    src_rows = rc.BAND_ROWS + 6
    lds = src_rows * pitch + 4 * (2 * src_rows + 14 * src_rows + 2 * rc.MMA_ROWS + 2 * rc.MMA_ROWS * 49) + 64
    if pitch // 16 <= 64 and nk <= 16 and lds <= 65536:
        return 4 if nk <= 4 else 8 if nk <= 8 else 12 if nk <= 12 else 16
    return 0


# (tw, th, form, what the shape reaches); rb: the last band's template rows, th - 32 (nband - 1)
SHAPES = [
    (8, 257, 4, "NK 4; last band rb = 1: its tail rows 1 .. 6 in N tile 0"),
    (8, 272, 4, "rb = 16: N tile 1 holds only the 6 trailing rows"),
    (8, 288, 4, "rb = 32: the tail rows are N tile 2"),
    (8, 262, 4, "rb = 6: tail rows 6 .. 11 right after the head rows' indices"),
    (8, 270, 4, "rb = 14: tail rows 14 .. 19 straddle N tiles 0 and 1"),
    (8, 284, 4, "rb = 28: tail rows 28 .. 33 straddle N tiles 1 and 2"),
    (260, 257, 8, "NK 8, RS 3, LDS-DMA staging"),
    (520, 257, 12, "NK 12, RS 4, LDS-DMA staging"),
    (900, 257, 16, "NK 16 (13 .. 15 k-steps; register staging with prefetch)"),
    # 17 k-steps: the launcher's rule (nk <= 16, pitch / 16 <= 64) gives this shape the slot-major form, not NK 16
    (1030, 257, 0, "slot-major form (NK 0, RS 1), wider than 1024"),
    (1345, 5, 0, "th < 6: head and tail rows overlap (row 5 is both); one band, slot-major form"),
]


def level_for(tw, th, seed):
    return rc.texture(max(360, tw + 160), max(260, th + 120), seed)


def rois(rng, s, tw, th, n3):
    """random_rois (partly and wholly off-image ROIs among them) with a third of the candidates moved inside the image."""
    h, w = s.shape
    n = N_ROIS // n3
    lt, ang = rc.random_rois(rng, w, h, tw, th, n, n3)
    for i in range(n // 3):
        lt[i] = rc.pasted_lt(w / 2 + rng.uniform(-20, 20), h / 2 + rng.uniform(-20, 20), tw, th, ang[i, n3 // 2])
    return lt, ang


def refine(m, levels, lt, ang, fold, round_rois):
    """refine_rois and the launches it made: (records, k_roi_corr launches, k_roi_small launches)."""
    m.profile(True)
    m.profile_reset()
    rec, _ = m.refine_rois(levels, 0, lt, ang, fold, round_rois)
    n = {k: m.profile_get(k)[1] for k in (L.K_ROI_CORR, L.K_ROI_EVAL, L.K_ROI_SMALL)}
    m.profile(False)
    return rec, n[L.K_ROI_CORR], n[L.K_ROI_EVAL], n[L.K_ROI_SMALL]


def assert_same_records(got, exp, what):
    assert got.shape == exp.shape, what
    for f in ("mx", "my", "on_border"):
        assert np.array_equal(got[f], exp[f]), (what, f, np.argwhere(got[f] != exp[f])[:5].tolist())
    for f in ("score", "vec"):   # f32 bit patterns: score and the 9 vec values
        g, e = np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(exp[f]).view(np.uint32)
        bad = np.argwhere(g != e)
        assert not len(bad), (what, f, len(bad), bad[:5].tolist(), got[f][tuple(bad[0])], exp[f][tuple(bad[0])])
    assert got.tobytes() == exp.tobytes(), what


def test_shapes_reach_their_forms():
    """The table's own claims, from the layout rules' host mirrors (no device work)."""
    for tw, th, form, _ in SHAPES:
        assert not rc.roi_small_fits(tw, th), (tw, th)
        assert corr_form(tw) == form, (tw, th)
    assert {f for _, _, f, _ in SHAPES} == {0, 4, 8, 12, 16}
    # th < 6 and the register-A forms: k_roi_small takes every such shape the register-A forms could
    widest_a = max(tw for tw in range(8, 1100) if corr_form(tw))
    assert widest_a == 960 and all(rc.roi_small_fits(tw, th) for th in range(1, 6) for tw in (8, 64, 512, widest_a))
    assert rc.roi_small_fits(1344, 5) and not rc.roi_small_fits(1345, 5)


@pytest.mark.parametrize("n3", [1, 3])
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("tw,th,form,what", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_window_sums(gpu_matcher_factory, tw, th, form, what, fold, n3):
    assert not rc.roi_small_fits(tw, th) and corr_form(tw) == form
    rng = np.random.default_rng(7 * tw + 13 * th + 2 * n3 + fold)
    t = rc.texture(tw, th, 61)
    s = level_for(tw, th, 62)
    o = rc.learn_one_level(oracle.OracleMatcher(), t)
    m = rc.learn_one_level(gpu_matcher_factory(), t)
    assert m.template_info()[0] == 1 and len(o.template_levels()[0]) == 1
    lt, ang = rois(rng, s, tw, th, n3)
    exp, _ = rc.oracle_refine(o, [s], 0, lt, ang, bool(fold), pixels=False)
    label = f"{tw}x{th} ({what}) fold={fold} n3={n3}"
    for round_rois, launches in ((0, 1), (ROUND_ROIS, 2)):
        rec, n_corr, n_eval, n_small = refine(m, [s], lt[None], ang[None], bool(fold), round_rois)
        assert n_small == 0 and n_corr == n_eval == launches, (label, round_rois, n_corr, n_eval, n_small)
        assert_same_records(rec, exp, f"{label} rounds of {round_rois}")
    # the wholly off-image ROI (random_rois' last): all zeros, flat windows, score 0 at (0, 0)
    off = rec[0, -1, :]
    assert not off["score"].any() and not off["mx"].any() and not off["my"].any() and off["on_border"].all()
