"""Patch comparison, host side (no GPU): fpm_compare_derive -- what the engine derives from a hit's integer sums --
against the numpy restatement of tests/compare_ref.py, and the pure argument checks.  Every expectation is equality."""
import ctypes as C

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from fastest_image_pattern_matching_amd import synth
from tests import compare_ref as ref
from tests import oracle


def _check(sums, normalize):
    z, g, o, lut = M.compare_derive(*sums, normalize=normalize)
    ez, eg, eo, elut = ref.derive(*sums, normalize)
    assert (z, g, o) == (ez, eg, eo), (sums, normalize, (z, g, o), (ez, eg, eo))
    assert np.array_equal(lut, elut), (sums, normalize)
    return z, g, o, lut


@pytest.fixture(scope="module")
def real_pairs(templates, oracle_lib):
    """(patch, template crop) pairs as the device forms them: warp_affine of a scene at (near) the pasted poses."""
    t = templates["Dst10"]
    th, tw = t.shape
    s = synth.noise(320, 240, 128, 10, 77)
    synth.paste_rotated(s, t, 150, 120, 25.0)
    dim = np.clip(np.rint(0.8 * s.astype(np.float64) + 20.0), 0, 255).astype(np.uint8)
    o = oracle.OracleMatcher().set(max_pos=1, tolerance_angle=180.0)
    assert o.learnPattern(t)
    hit = o.match(s)[0]                      # as_tuple: ptLT first, the angle last but one
    lt0, ang0 = (hit[0], hit[1]), hit[10]
    pairs = []
    for img in (s, dim):
        for lt, ang, rect in [(lt0, ang0, (0, 0, tw, th)), ((lt0[0] + 1.5, lt0[1] - 0.75), ang0 - 1.0, (3, 2, tw - 5, th - 7)),
                              ((10.0, 200.0), -137.5, (1, 0, 17, 9))]:
            m = M.patch_matrix(320, 240, lt, ang, rect[:2])
            I = oracle.warp_affine(img, m, rect[2:])
            pairs.append((I, t[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]))
    return pairs


@pytest.mark.parametrize("normalize", [False, True])
def test_derive_on_real_pairs(real_pairs, normalize, fpm_lib):
    zs = [_check(ref.sums(I, T), normalize)[0] for I, T in real_pairs]
    assert max(zs) > 0.5 and all(-1.0 <= z <= 1.0 for z in zs)   # real correlations among them, not only noise


@pytest.mark.parametrize("normalize", [False, True])
def test_derive_on_random_images(normalize, fpm_lib):
    rng = np.random.default_rng(15)
    for k in range(200):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        lo, hi = sorted(int(v) for v in rng.integers(0, 256, 2))
        I = rng.integers(lo, hi + 1, (h, w), dtype=np.uint8)
        T = rng.integers(0, 256, (h, w), dtype=np.uint8) if k % 2 else \
            np.clip(np.rint(I * rng.uniform(0.2, 3.0) + rng.uniform(-60, 60)), 0, 255).astype(np.uint8)
        _check(ref.sums(I, T), normalize)


@pytest.mark.parametrize("normalize", [False, True])
def test_zero_variance(normalize, fpm_lib):
    flat_a, flat_b = np.full((5, 7), 90, np.uint8), np.full((5, 7), 201, np.uint8)
    ramp = np.arange(35, dtype=np.uint8).reshape(5, 7)
    z, g, o, _ = _check(ref.sums(flat_a, ramp), normalize)       # Di == 0
    assert z == 0.0 and g == 1.0
    assert o == ((int(ramp.sum()) - 90 * 35) / 35 if normalize else 0.0)
    z, g, o, lut = _check(ref.sums(ramp, flat_b), normalize)     # Dt == 0: gain 0, every value maps onto the template's
    assert z == 0.0 and (g, o) == ((0.0, 201.0) if normalize else (1.0, 0.0))
    assert not normalize or (lut == 201).all()
    z, g, o, _ = _check(ref.sums(flat_a, flat_b), normalize)     # both
    assert z == 0.0 and (g, o) == ((1.0, 111.0) if normalize else (1.0, 0.0))


def test_identity_table_without_normalisation(fpm_lib):
    _, g, o, lut = M.compare_derive(4, 10, 30, 500, 70000, 1400, normalize=False)
    assert (g, o) == (1.0, 0.0) and np.array_equal(lut, np.arange(256, dtype=np.uint8))


def test_gain_clamps_at_both_ends(fpm_lib):
    I = np.array([[100, 110, 100, 110]], np.uint8)
    T = np.array([[0, 255, 0, 255]], np.uint8)
    _, g, o, lut = _check(ref.sums(I, T), True)
    assert g == 25.5 and o < 0
    assert (lut[:101] == 0).all() and (lut[110:] == 255).all() and 0 < lut[105] < 255


def test_half_way_ties_round_to_even(fpm_lib):
    """gain = 1 and offset = 0.5 exactly: Di == Dt and sum_t - sum_i == n / 2.  Integer sums give it: n = 8,
    I = 0 0 0 0 2 2 2 2, T = 0 0 1 2 2 2 2 3 (Di = Dt = 64)."""
    I = np.array([[0, 0, 0, 0, 2, 2, 2, 2]], np.uint8)
    T = np.array([[0, 0, 1, 2, 2, 2, 2, 3]], np.uint8)
    s = ref.sums(I, T)
    assert s == (8, 8, 16, 12, 26, 18)
    _, g, o, lut = _check(s, True)
    assert (g, o) == (1.0, 0.5)
    assert lut[:6].tolist() == [0, 2, 2, 4, 4, 6] and lut[253:].tolist() == [254, 254, 255]   # rint(255.5) = 256 -> 255


@pytest.mark.parametrize("normalize", [False, True])
def test_sums_at_the_area_cap(normalize, fpm_lib):
    n = M.COMPARE_MAX_AREA
    half = n // 2
    # half 0, half 255 on both sides, in phase / in antiphase / template shifted by a quarter; then everything 255
    for si, sii, st, stt, sit in [(255 * half, 65025 * half, 255 * half, 65025 * half, 65025 * half),
                                  (255 * half, 65025 * half, 255 * half, 65025 * half, 0),
                                  (255 * half, 65025 * half, 255 * half, 65025 * half, 65025 * (half // 2)),
                                  (255 * n, 65025 * n, 255 * n, 65025 * n, 65025 * n),
                                  (255 * n - 255, 65025 * n - 65025, 254 * n, 64516 * n, 254 * (255 * n - 255))]:
        z, _, _, _ = _check((n, si, sii, st, stt, sit), normalize)
        assert -1.0 <= z <= 1.0
    assert M.compare_derive(n, 255 * half, 65025 * half, 255 * half, 65025 * half, 65025 * half)[0] == 1.0
    assert M.compare_derive(n, 255 * half, 65025 * half, 255 * half, 65025 * half, 0)[0] == -1.0


def test_derive_rejects_bad_arguments(fpm_lib):
    z, g, o = C.c_double(), C.c_double(), C.c_double()
    lut = (C.c_uint8 * 256)()
    ok = (8, 8, 16, 12, 26, 18)
    assert fpm_lib.fpm_compare_derive(*ok, 1, C.byref(z), C.byref(g), C.byref(o), lut) == L.FPM_OK
    assert fpm_lib.fpm_compare_derive(*ok, 1, C.byref(z), C.byref(g), C.byref(o), None) == L.FPM_OK   # the table is optional
    for args in [(None, C.byref(g), C.byref(o)), (C.byref(z), None, C.byref(o)), (C.byref(z), C.byref(g), None)]:
        assert fpm_lib.fpm_compare_derive(*ok, 1, *args, lut) == L.FPM_E_INVALID_ARG
    for bad in [(0, 0, 0, 0, 0, 0), (M.COMPARE_MAX_AREA + 1, 0, 0, 0, 0, 0), (8, -1, 16, 12, 26, 20),
                (8, 8 * 255 + 1, 16, 12, 26, 20), (8, 8, 16, 12, 8 * 65025 + 1, 20), (8, 8, 16, 12, 26, -1),
                (8, 8, 7, 12, 26, 20),      # Di < 0: the sums of no 8 pixels
                (8, 8, 16, 12, 17, 20)]:    # Dt < 0
        assert fpm_lib.fpm_compare_derive(*bad, 1, C.byref(z), C.byref(g), C.byref(o), lut) == L.FPM_E_INVALID_ARG, bad
        with pytest.raises(ValueError):
            M.compare_derive(*bad, normalize=True)


def test_entries_reject_null_arguments_without_a_device(fpm_lib):
    n = C.c_int32()
    assert fpm_lib.fpm_last_compare(None, None, 0, 16, 0, None, 0, C.byref(n), None, 0, 0) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_compare_at(None, None, None, None, None, 0, 16, 0, None, None, 0, 0) == L.FPM_E_INVALID_ARG


def test_compare_rect():
    tw, th = 40, 30
    assert M.compare_rect(None, tw, th) == (0, 0, 40, 30)
    assert M.compare_rect((0, 0, 40, 30), tw, th) == (0, 0, 40, 30)
    assert M.compare_rect(np.array([39, 29, 1, 1]), tw, th) == (39, 29, 1, 1)
    assert M.compare_rect((3, 2, 37, 28), tw, th) == (3, 2, 37, 28)
    for bad in [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 41, 30), (0, 0, 40, 31), (1, 0, 40, 30), (0, 1, 40, 30),
                (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, 4, -2), (0, 0, 4), (0.5, 0, 4, 4), "abcd", (40, 0, 1, 1)]:
        with pytest.raises(ValueError):
            M.compare_rect(bad, tw, th)
    # the area cap: 2^22 pixels pass, one row more does not
    assert M.compare_rect((0, 0, 2048, 2048), 4096, 4096) == (0, 0, 2048, 2048)
    with pytest.raises(ValueError):
        M.compare_rect((0, 0, 2048, 2049), 4096, 4096)


def test_stats_record_layout():
    assert M.COMPARE_DTYPE.itemsize == C.sizeof(L.CompareStats) == 104
    assert list(M.COMPARE_DTYPE.names) == [f[0] for f in L.CompareStats._fields_] == list(ref.FIELDS)
    for name, _ in L.CompareStats._fields_:
        assert M.COMPARE_DTYPE.fields[name][1] == getattr(L.CompareStats, name).offset
