"""The refinement kernels' row statistics (full-row sums of I and I^2 on the matrix cores in k_roi_corr's register-A
forms, tile_row_sums; k_roi_small's row sums) at ROI level, bit for bit against the oracle's refine_roi: the relations
between the ROI width RW = tw + 6 and the 64-column k-steps the sums cover, in every NK form; the bench's own level
shapes; sources of extreme bytes, where the signed operands' corrections wrap; the batch forms.  Each case asserts the
form it ran (tests/test_gpu_refine.py's check against roi_small_fits) and takes a handful of ROI triples."""
import numpy as np
import pytest

from tests import refine_cases as rc
from tests.test_gpu_refine import SMALL, THREE, check, pair, rois_for, source_for

pytestmark = pytest.mark.gpu


def shape_case(gpu_matcher_factory, tw, th, seed, n=4, S=1, levels=None, template=None):
    """n ROI triples per source (interior, partly and wholly off the image) of a tw x th template.  Returns the form
    that ran and the oracle's records."""
    rng = np.random.default_rng(seed)
    t = rc.texture(tw, th, seed) if template is None else template
    levels = [source_for(tw, th, seed + 1 + k) for k in range(S)] if levels is None else levels
    m, o = pair(gpu_matcher_factory, t)
    lts, angs = zip(*[rois_for(rng, lv, tw, th, n, 3) for lv in levels])
    lt, ang = np.stack(lts), np.stack(angs)
    form = check(m, o, levels, lt, ang, True, f"rowstats {tw}x{th}")
    exp, _ = rc.oracle_refine(o, levels, 0, lt, ang, True)
    return form, exp


# ---- k_roi_corr: column coverage ----------------------------------------------------------------------------------
# per NK form, RW - 64 nk = 0, 1, 5, 6 (the k-steps end at, or up to 6 columns before, the ROI's right edge: the
# window's right-edge pixels partly outside the full sums) and -57 (16-byte chunks past the ROI's tiles inside the
# k-steps, which no staging load writes); th = 257 keeps the narrow shapes out of k_roi_small.  At 16 k-steps the row
# pitch passes the register-A form's 64 chunks and the slot-major form runs, so the NK = 16 instantiation is reached
# at 15 k-steps (0 and 6)
CORR_EDGES = [(122, 257), (123, 257), (127, 257), (128, 257), (129, 257),      # NK 4
              (314, 113), (319, 113), (320, 113), (321, 113),                  # NK 8
              (570, 33), (575, 33), (576, 33), (577, 33),                      # NK 12
              (1018, 33), (1024, 33),                                          # 16 k-steps: the slot-major form
              (954, 33), (960, 33)]                                            # NK 16 (15 k-steps, the widest)


@pytest.mark.parametrize("tw,th", CORR_EDGES)
def test_corr_column_coverage(gpu_matcher_factory, tw, th):
    nk = (tw + 63) // 64
    assert tw + 6 - 64 * nk in (0, 1, 5, 6, -57)
    assert shape_case(gpu_matcher_factory, tw, th, 2000 + tw, n=3)[0] == THREE


@pytest.mark.parametrize("tw,th", [(762, 65), (381, 113), (191, 131)])
def test_corr_bench_levels(gpu_matcher_factory, tw, th):
    """The widths of the Src7 bench's three lowest layers (12, 6 and 3 k-steps; 381 and 191 end 3 columns short of RW)."""
    assert shape_case(gpu_matcher_factory, tw, th, 2100 + tw, n=3)[0] == THREE


# ---- k_roi_small ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tw,th", [(58, 40), (59, 40), (63, 40), (64, 40), (65, 40), (122, 60), (127, 60), (128, 60),
                                   (129, 60), (96, 66), (48, 33), (24, 17)])
def test_small_column_coverage(gpu_matcher_factory, tw, th):
    """The same relations between RW and the k-steps at one and two k-steps, and the bench's upper layers."""
    assert shape_case(gpu_matcher_factory, tw, th, 2200 + tw)[0] == SMALL


@pytest.mark.parametrize("nt,tw,th", [(128, 58, 40), (256, 96, 66), (512, 129, 60)])
def test_small_workgroup_sizes(gpu_matcher_factory, monkeypatch, nt, tw, th):
    """The two- / four- / eight-wave forms of k_roi_small forced (FPM_SMALL_NT)."""
    monkeypatch.setenv("FPM_SMALL_NT", str(nt))
    assert shape_case(gpu_matcher_factory, tw, th, 2300 + nt, n=6)[0] == SMALL


# ---- extreme bytes ---------------------------------------------------------------------------------------------------
def checkerboard(w, h):
    """0 / 255 squares of 8 pixels: every window mixes both extremes (I' = -128 and 127)."""
    yy, xx = np.mgrid[:h, :w]
    return ((((xx >> 3) + (yy >> 3)) & 1) * 255).astype(np.uint8)


def white_with_patch(w, h, pw, ph, seed):
    """All 255 with a textured patch at the centre (where rois_for centres a third of the ROIs)."""
    s = np.full((h, w), 255, np.uint8)
    y0, x0 = (h - ph) // 2, (w - pw) // 2
    s[y0:y0 + ph, x0:x0 + pw] = rc.texture(pw, ph, seed)
    return s


@pytest.mark.parametrize("tw,th,form", [(321, 113, THREE), (65, 40, SMALL)])
@pytest.mark.parametrize("kind", ["checkerboard", "white"])
def test_extreme_bytes(gpu_matcher_factory, tw, th, form, kind):
    """Row sums at the ends of the byte range: S1' = -128 C .. 127 C and their 256 S1' + 16384 C correction.  The
    centred ROIs' scores are non-zero (no flat windows there); the last ROI is wholly off the image, I' = -128."""
    w, h = max(360, tw + 160), max(260, th + 120)
    s = checkerboard(w, h) if kind == "checkerboard" else white_with_patch(w, h, tw + 40, th + 40, 77)
    n = 6
    got, exp = shape_case(gpu_matcher_factory, tw, th, 2400 + tw, n=n, levels=[s])
    assert got == form
    assert (exp[0, :n // 3]["score"] != 0).all() and not exp[0, -1]["score"].any()


# ---- batch forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tw,th,form", [(319, 113, THREE), (63, 40, SMALL)])
def test_batch_forms(gpu_matcher_factory, tw, th, form):
    """S = 3 sources: k_roi_eval<40> after k_roi_corr, and the batch forms of k_roi_small."""
    assert shape_case(gpu_matcher_factory, tw, th, 2500 + tw, n=2, S=3)[0] == form
