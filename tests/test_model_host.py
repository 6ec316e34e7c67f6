"""Variation model, host side (no GPU): fpm_model_derive -- the per-pixel rule the device runs, compiled for the host --
against Python integers (tests/model_ref.py), and the pure argument checks.  Every expectation is equality."""
import ctypes as C
import itertools
import math

import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import model_ref as ref


def _derive(lib, n, S, Q, a, kq):
    mean, lo, hi = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    rc = lib.fpm_model_derive(n, S, Q, a, kq, C.byref(mean), C.byref(lo), C.byref(hi))
    return rc, (mean.value, lo.value, hi.value)


def _check(lib, n, S, Q, a, kq):
    rc, got = _derive(lib, n, S, Q, a, kq)
    exp = ref.derive1(n, S, Q, a, kq)
    assert rc == L.FPM_OK and got == exp, ((n, S, Q, a, kq), rc, got, exp)
    mean, lo, hi = got
    # the interval is the rule |n u - S| <= B, value by value
    B = max(n * a, math.isqrt((kq * kq * (n * Q - S * S)) >> 8))
    inside = [u for u in range(256) if abs(n * u - S) <= B]
    assert inside == list(range(lo, hi + 1)), (n, S, Q, a, kq)
    return got


def test_small_inputs(fpm_lib):
    vals = (0, 1, 127, 128, 254, 255)
    seen = 0
    for n in (1, 2, 3):
        for vs in itertools.combinations_with_replacement(vals, n):
            S, Q = sum(vs), sum(v * v for v in vs)
            for a in (0, 1, 255):
                for kq in (0, 1, 16, 48, 255):
                    _check(fpm_lib, n, S, Q, a, kq)
                    seen += 1
    assert seen == (6 + 21 + 56) * 15


def test_empty_interval(fpm_lib):
    assert _check(fpm_lib, 2, 21, 10 * 10 + 11 * 11, 0, 0) == (11, 11, 10)   # mean 10.5 rounds half up; no value is inside
    assert M.model_derive(2, 21, 221, 0, 0.0) == (11, 11, 10)


def test_cap_and_isqrt_correction(fpm_lib):
    # 65535 samples, 32767 of them 0 and 32768 of them 255: V and kq^2 V near their caps (2^46, 2^62)
    n, m = 65535, 32768
    S, Q = 255 * m, 65025 * m
    V = n * Q - S * S
    assert 2 ** 45 < V < 2 ** 46 and 2 ** 61 < 255 * 255 * V < 2 ** 62
    for kq in (255, 254, 16, 1):
        for a in (0, 255):
            _check(fpm_lib, n, S, Q, a, kq)
    # the other way round, and all at one value (V = 0)
    _check(fpm_lib, n, 255 * (n - m), 65025 * (n - m), 0, 255)
    _check(fpm_lib, n, 255 * n, 65025 * n, 0, 255)
    _check(fpm_lib, n, 0, 0, 0, 255)


def test_isqrt_boundary(fpm_lib):
    # x = (kq^2 V) >> 8 at a perfect square t^2 and at its two neighbours: isqrt gives t - 1, t, t.  Three samples of
    # small bytes and the even kq from 4 to 38 reach every such triple for many t.
    found = {}
    for vs in itertools.combinations_with_replacement(range(48), 3):
        S, Q = sum(vs), sum(v * v for v in vs)
        for kq in range(4, 40, 2):
            found.setdefault((kq * kq * (3 * Q - S * S)) >> 8, (3, S, Q, kq))
    roots = [t for t in range(2, 60) if all(t * t + d in found for d in (-1, 0, 1))]
    assert len(roots) >= 10, roots
    for t in roots:
        for d, root in ((-1, t - 1), (0, t), (1, t)):
            n, S, Q, kq = found[t * t + d]
            assert math.isqrt((kq * kq * (n * Q - S * S)) >> 8) == root
            mean, lo, hi = _check(fpm_lib, n, S, Q, 0, kq)
            assert hi == min(255, (S + root) // n) and lo == max(0, -((root - S) // n))
    # two samples 0 and 2 r at kq = 16: x = V = 4 r^2 exactly, hi = floor((2 r + 2 r) / 2) = 2 r
    for r in (1, 7, 50, 127):
        assert _check(fpm_lib, 2, 2 * r, 4 * r * r, 0, 16) == (r, 0, 2 * r)
    # near the cap, where the f64 root alone is not exact: x around 2^61
    n = 65535
    for m in (1, 2, 3, 1000, 32767, 32768, 65534):
        S, Q = 255 * m, 65025 * m
        for kq in (16, 255):
            x = (kq * kq * (n * Q - S * S)) >> 8
            t = math.isqrt(x)
            assert t * t <= x < (t + 1) * (t + 1)
            _check(fpm_lib, n, S, Q, 0, kq)


def test_mean_rounding(fpm_lib):
    # (2 S + n) / (2 n): exact means, halves (rounded up) and the values either side of a half
    for n, S, exp in [(2, 21, 11), (2, 20, 10), (2, 19, 10), (4, 10, 3), (4, 9, 2), (4, 11, 3), (3, 4, 1), (3, 5, 2),
                      (65535, 65535 * 255, 255), (65534, 32767, 1), (65534, 32766, 0)]:
        # any Q that n bytes of sum S can have: S = q n + r -> r samples of q + 1 and n - r of q
        q, r = divmod(S, n)
        Q = r * (q + 1) ** 2 + (n - r) * q * q
        assert _check(fpm_lib, n, S, Q, 0, 0)[0] == exp, (n, S)


def test_rejects_what_no_samples_give(fpm_lib):
    ok = (3, 30, 300, 8, 48)
    assert _derive(fpm_lib, *ok)[0] == L.FPM_OK
    bad = [(0, 0, 0, 8, 48), (-1, 0, 0, 8, 48), (65536, 0, 0, 8, 48),          # n outside 1 .. 65535
           (3, -1, 1, 8, 48), (3, 3 * 255 + 1, 3 * 65025, 8, 48),              # sum outside 0 .. 255 n
           (3, 30, 29, 8, 48), (3, 30, 30 * 255 + 2, 8, 48), (3, 30, 301, 8, 48),   # Q below S, above 255 S, odd against even
           (1, 255, 65025 + 2, 8, 48), (3, 30, -300, 8, 48),
           (3, 30, 298, 8, 48),                                                # n Q < S^2: 894 < 900
           (3, 30, 300, -1, 48), (3, 30, 300, 256, 48), (3, 30, 300, 8, -1), (3, 30, 300, 8, 256)]
    for args in bad:
        rc, out = _derive(fpm_lib, *args)
        assert rc == L.FPM_E_INVALID_ARG and out == (-7, -7, -7), args
    m = C.c_int32()
    assert fpm_lib.fpm_model_derive(3, 30, 300, 8, 48, None, C.byref(m), C.byref(m)) == L.FPM_E_INVALID_ARG


def test_python_argument_checks():
    assert M.model_thresholds(8, 3.0) == (8, 48) and M.model_thresholds(0, 0) == (0, 0)
    assert M.model_thresholds(255, 15.9375) == (255, 255) and M.model_thresholds(1, 0.03) == (1, 0)
    assert M.model_thresholds(1, 0.04) == (1, 1)
    for a, k in [(-1, 3.0), (256, 3.0), (8.5, 3.0), (8, -0.04), (8, 15.97), (8, float("nan")), (8, float("inf"))]:
        with pytest.raises(ValueError):
            M.model_thresholds(a, k)
    with pytest.raises(ValueError):
        M.model_derive(3, 30, 298)
    assert M.INSPECT_DTYPE.itemsize == C.sizeof(L.InspectStats) == 64
    assert M.INSPECT_DTYPE.names == ref.FIELDS
