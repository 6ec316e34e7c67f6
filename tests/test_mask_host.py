"""The template-mask restatement (tests/mask_ref.py) against hand-made cases and against the references it is built on,
and the planted scene of DESIGN.md section 22 on the CPU reference (oracle.warp_affine through align_ref.patch): an
elliptic part on a foreign background, aligned and inspected with and without the mask.  No GPU."""
import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from tests import align_ref
from tests import blobs_ref
from tests import compare_ref
from tests import mask_ref as ref
from tests import model_ref


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_one_used_pixel_by_hand():
    I = np.array([[10, 200], [30, 40]], np.uint8)
    T = np.array([[12, 100], [90, 41]], np.uint8)
    m = np.array([[False, True], [False, False]])
    row, d = ref.compare(I, T, m, 16, False)
    assert (row["n"], row["sum_i"], row["sum_ii"], row["sum_t"], row["sum_tt"], row["sum_it"]) == (1, 200, 40000, 100, 10000, 20000)
    assert (row["sum_abs"], row["max_abs"], row["n_over"]) == (100, 100, 1)
    assert (row["x0"], row["y0"], row["x1"], row["y1"]) == (1, 0, 1, 0)
    assert (row["zncc"], row["gain"], row["offset"]) == (0.0, 1.0, 0.0)      # one pixel: both variances are 0
    assert np.array_equal(d, [[0, 100], [0, 0]])
    # normalised: the variance of I is 0, so gain 1 and offset = (100 - 200) / 1: the used pixel no longer deviates,
    # and the ignored ones, which do under that table, stay 0
    row, d = ref.compare(I, T, m, 16, True)
    assert (row["gain"], row["offset"], row["sum_abs"], row["n_over"]) == (1.0, -100.0, 0, 0) and not d.any()
    assert (row["x0"], row["y0"], row["x1"], row["y1"]) == (2, 2, -1, -1)


def test_two_used_pixels_by_hand():
    I = np.array([[10, 20, 30]], np.uint8)
    T = np.array([[50, 0, 90]], np.uint8)
    row, _ = ref.compare(I, T, np.array([[True, False, True]]), 0, True)
    # I = 10, 30 against T = 50, 90: gain 2, offset 30, correlation 1
    assert (row["n"], row["sum_i"], row["sum_t"], row["sum_it"]) == (2, 40, 140, 3200)
    assert (row["zncc"], row["gain"], row["offset"], row["sum_abs"]) == (1.0, 2.0, 30.0, 0)


def test_no_used_pixel():
    I, T = _rand((5, 7), 1), _rand((5, 7), 2)
    for norm in (False, True):
        row, d = ref.compare(I, T, np.zeros((5, 7), bool), 0, norm)
        assert [row[f] for f in compare_ref.FIELDS] == [0] * 9 + [7, 5, -1, -1, 0.0, 1.0, 0.0] and not d.any()
    assert np.array_equal(ref.table(I, T, np.zeros((5, 7), bool)), np.arange(256))
    s = ref.align_sums(I, _rand((9, 11), 3), (2, 2, 7, 5), np.zeros((9, 11), np.uint8))
    assert not any(s.values())
    lo, hi = np.full((5, 7), 100, np.uint8), np.full((5, 7), 120, np.uint8)
    row, e = ref.inspect(I, lo, hi, np.zeros((5, 7), bool))
    assert [row[f] for f in model_ref.FIELDS] == [0, 0, 0, 0, 0, 7, 5, -1, -1, 1.0, 0.0] and not e.any()


@pytest.mark.parametrize("norm", [False, True])
def test_all_ones_is_the_unmasked_reference(norm):
    T = _rand((35, 67), 4)
    rect = (3, 2, 41, 30)
    x, y, w, h = rect
    I = _rand((h, w), 5)
    Tc = np.ascontiguousarray(T[y:y + h, x:x + w])
    ones = np.ones(T.shape, np.uint8)
    row, d = ref.compare(I, Tc, ref.crop(ones, rect), 16, norm)
    row0, d0 = compare_ref.stats(I, Tc, 16, norm)
    assert row == row0 and np.array_equal(d, d0)
    lut = compare_ref.derive(*compare_ref.sums(I, Tc), True)[3] if norm else None
    assert ref.align_sums(I, T, rect, ones, lut) == align_ref.sums(I, T, rect, lut) == ref.align_sums(I, T, rect, None, lut)
    lo, hi = _rand((h, w), 6) // 2, _rand((h, w), 7) // 2 + 128
    v, g, o = ref.sample(I, Tc, ref.crop(ones, rect), norm)
    v0, g0, o0 = model_ref.sample(I, Tc, norm)
    assert np.array_equal(v, v0) and (g, o) == (g0, o0)
    row, e = ref.inspect(v, lo, hi, ref.crop(ones, rect), g, o)
    row0, e0 = model_ref.inspect(v0, lo, hi, g0, o0)
    assert row == row0 and np.array_equal(e, e0)


def test_masked_sums_are_the_sums_of_the_used_pixels():
    T = _rand((35, 67), 8)
    rect = (1, 3, 60, 29)
    x, y, w, h = rect
    I = _rand((h, w), 9)
    mask = (_rand(T.shape, 10) < 128).astype(np.uint8) * np.uint8(7)       # any non-zero byte counts
    m = ref.crop(mask, rect)
    Tc = T[y:y + h, x:x + w]
    row, d = ref.compare(I, Tc, m, 16, False)
    i, t = I.astype(np.int64), Tc.astype(np.int64)
    assert row["n"] == m.sum() and row["sum_it"] == (i * t * m).sum() and row["sum_ii"] == (i * i * m).sum()
    assert row["sum_abs"] == (np.abs(i - t) * m).sum() and not d[~m].any()
    # a pixel's own byte decides, not its neighbours': masking everything but one interior pixel keeps its gradient
    one = np.zeros(T.shape, np.uint8)
    one[10, 20] = 1
    s = ref.align_sums(I, T, rect, one)
    gx, gy = int(T[10, 21]) - int(T[10, 19]), int(T[11, 20]) - int(T[9, 20])
    assert (s["n_used"], s["h_xx"], s["h_yy"], s["h_xy"]) == (1, gx * gx, gy * gy, gx * gy)
    # and a border pixel of the template stays unused whatever the mask says
    one[:] = 0
    one[0, 5] = 1
    assert ref.align_sums(I, T, (0, 0, 60, 29), one)["n_used"] == 0


# ---- planted truth: an elliptic part on a foreign background ---------------------------------------------------------------
RECT = ref.PLANT_RECT


def test_planted_alignment_needs_the_mask():
    errs = ref.planted_alignments()
    assert len(errs) == 4
    for start, unmasked, masked in errs:
        print(f"start {start:.4f} px  unmasked {unmasked:.4f} px  masked {masked:.4f} px")
        assert masked < start           # the masked alignment ends nearer the planted centre than its start
        assert masked < unmasked        # and nearer than the unmasked one, on all four starts
    print(f"largest masked error of the reference: {max(e[2] for e in errs):.4f} px")


def test_planted_inspection_needs_the_mask():
    mask, scenes = ref.planted()
    part = align_ref.smooth_scene(seed=13)
    for scene, t, lt, a in scenes:
        taught = align_ref.patch(part, RECT, lt, a)            # one sample: the template frame from the seed-13 scene
        n, S, Q = model_ref.accumulate([taught])
        _, lo, hi = model_ref.derive_fast(n, S, Q, 8, model_ref.kq_of(3.0))
        I = align_ref.patch(scene, RECT, lt, a)
        row, e = model_ref.inspect(I, lo, hi)
        assert row["n_low"] + row["n_high"] > 0
        # the box reaches a corner of the rectangle: a corner of the box IS a corner pixel of the 71 x 45 frame
        assert ref.box_reaches_a_corner(row, align_ref.TW, align_ref.TH), row
        mrow, me = ref.inspect(I, lo, hi, mask)
        assert mrow["n_low"] + mrow["n_high"] == 0 and mrow["n"] == int(mask.sum()) and not me.any()
        _, recs, summary = blobs_ref.blobs(me, 0, 8, 1, 64)
        assert len(recs) == 0 and summary["n_blobs"] == 0
        assert len(blobs_ref.blobs(e, 0, 8, 1, 64)[1]) > 0
