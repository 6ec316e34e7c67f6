"""Match patches, host side (no GPU): fpm_patch_matrix against the oracle's getRotatedROI, the rectangle's float-rounded
translation terms, and the pure argument checks of the Python wrappers."""
import math

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import matcher as M
from tests import oracle

ANGLES = [0.0, 90.0, 180.0, -90.0, 37.0, 0.001, 179.999, -100.0]
SW, SH, TW, TH = 161, 119, 37, 29


def poses():
    """One pose per angle: fractional ptLT, some of them left of / above the source."""
    rng = np.random.default_rng(20260)
    lts = rng.uniform([-25.0, -20.0], [SW - 10.0, SH - 10.0], size=(len(ANGLES), 2)).astype(np.float32)
    lts[1] = (-7.375, 40.5)
    lts[4] = (60.25, -11.0625)
    return [(tuple(float(v) for v in lt), a) for lt, a in zip(lts, ANGLES)]


@pytest.fixture(scope="module")
def source():
    return np.random.default_rng(7).integers(0, 256, (SH, SW), dtype=np.uint8)


@pytest.mark.parametrize("lt,angle", poses(), ids=[f"a{a:g}" for a in ANGLES])
def test_margin_rect_is_get_rotated_roi(source, lt, angle, fpm_lib, oracle_lib):
    m = M.patch_matrix(SW, SH, lt, angle, (-3, -3))
    got = oracle.warp_affine(source, m, (TW + 6, TH + 6))
    exp = oracle.rotated_roi(source, TW, TH, lt, angle)
    assert got.shape == exp.shape and np.array_equal(got, exp)
    if angle in (37.0, -100.0):
        assert exp.any() and (exp == 0).sum() < exp.size   # a real crop, not an all-border one


def rotate_pt_f32(lt, c, rad):
    """ptRotatePt2f (TemplateMatcher.cpp:971-982) with the reference's types and operation order: the x difference of
    two floats is a float, everything else f64; the result rounded to f32."""
    cs, sn = math.cos(rad), math.sin(rad)
    iy = float(np.float32(lt[1]))
    ox, oy = float(c[0]), float(c[1])
    dx = float(np.float32(lt[0]) - np.float32(c[0]))
    h = oy * 2
    y1, y2 = h - iy, h - oy
    x = dx * cs - (y1 - oy) * sn + ox
    y = dx * sn + (y1 - oy) * cs + y2
    y = -y + h
    return np.float32(x), np.float32(y)


@pytest.mark.parametrize("lt,angle", poses(), ids=[f"a{a:g}" for a in ANGLES])
@pytest.mark.parametrize("rx,ry", [(0, 0), (-3, -3), (5, -11), (-100, 250)])
def test_rect_origin_moves_the_translation_by_float_rounded_terms(lt, angle, rx, ry, fpm_lib, oracle_lib):
    c = (np.float32((SW - 1) / 2.0), np.float32((SH - 1) / 2.0))
    rot = oracle.rotation_matrix(float(c[0]), float(c[1]), angle)
    ltr = rotate_pt_f32(lt, c, angle * (math.pi / 180.0))
    exp = rot.copy()
    exp[0, 2] -= float(np.float32(ltr[0] + np.float32(rx)))
    exp[1, 2] -= float(np.float32(ltr[1] + np.float32(ry)))
    got = M.patch_matrix(SW, SH, lt, angle, (rx, ry))
    assert np.array_equal(got, exp), (got, exp)


def test_patch_matrix_rejects_bad_arguments(fpm_lib):
    import ctypes as C

    m = (C.c_double * 6)()
    assert fpm_lib.fpm_patch_matrix(0, 10, 0.0, 0.0, 0.0, 0, 0, m) != 0
    assert fpm_lib.fpm_patch_matrix(10, 10, 0.0, 0.0, 0.0, 0, 0, None) != 0
    assert fpm_lib.fpm_last_patches(None, None, 0, None, 0, 0, 0, None, None) != 0
    assert fpm_lib.fpm_set_patch_form(None, 0) != 0


def test_normalize_rect():
    assert M.normalize_rect((-3, -3, 43, 35)) == (-3, -3, 43, 35)
    assert M.normalize_rect(np.array([1, 2, 8192, 1])) == (1, 2, 8192, 1)
    for bad in [(0, 0, 0, 5), (0, 0, 5, 0), (0, 0, 8193, 5), (0, 0, 5, -1), (0, 0, 5), None, (0.5, 0, 4, 4), "abcd"]:
        with pytest.raises(ValueError):
            M.normalize_rect(bad)


def test_patch_out_layout():
    n, ph, pw = 3, 5, 7
    assert M.patch_out_layout((n, ph, pw), (35, 7, 1), n, ph, pw) == (7, 35)
    assert M.patch_out_layout((n, ph, pw), (400, 20, 1), n, ph, pw) == (20, 400)      # a column slice of a wider tensor
    assert M.patch_out_layout((1, ph, pw), (1, 9, 1), 1, ph, pw) == (9, 45)           # one patch: its stride is free
    assert M.patch_out_layout((n, 1, pw), (10, 123, 1), n, 1, pw) == (7, 10)          # one row: its stride is free
    assert M.patch_out_layout((0, ph, pw), (35, 7, 1), 0, ph, pw) == (7, 35)
    for shape, strides in [((n, ph, pw + 1), (40, 8, 1)),    # wrong shape
                           ((n, ph), (35, 7)),
                           ((n, ph, pw), (35, 7, 2)),        # pixel stride
                           ((n, ph, pw), (35, 6, 1)),        # rows overlap
                           ((n, ph, pw), (34, 7, 1)),        # patches overlap
                           ((n, ph, pw), (35, -7, 1))]:
        with pytest.raises(ValueError):
            M.patch_out_layout(shape, strides, n, ph, pw)


def test_patch_poses():
    idx, lt, ang = M.patch_poses(0, [(1.5, 2.5), (3, 4)], [10, -20])
    assert idx.dtype == np.int32 and idx.tolist() == [0, 0]
    assert lt.dtype == np.float32 and lt.shape == (2, 2) and ang.dtype == np.float64 and ang.tolist() == [10.0, -20.0]
    idx, lt, ang = M.patch_poses([2], (1.0, 2.0), [5.0])
    assert idx.tolist() == [2] and lt.shape == (1, 2)
    for args in [(0, [(1, 2)], [1, 2]), ([0, 1, 2], [(1, 2), (3, 4)], [1, 2]), (0, [(1, 2, 3)], [1]),
                 (0, [(float("nan"), 2)], [1]), (0, [(1, 2)], [float("inf")]), ([-1], [(1, 2)], [1])]:
        with pytest.raises(ValueError):
            M.patch_poses(*args)
