"""Learning on the device, host side (no GPU): the five new entries are declared and exported, and fpm_learn_derive --
what the engine derives for a template level from its pixel count and exact sums -- gives the CPU oracle's mean, norm,
inv_area and vecResultEqual1 bit for bit.  Every expectation is equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from fastest_image_pattern_matching_amd import synth
from tests import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fpm_learn_device", "fpm_learn_at", "fpm_learn_hit", "fpm_learn_derive", "fpm_template_operands")


def test_header_declares_and_library_exports_the_entries(fpm_lib):
    hdr = open(os.path.join(REPO, "include", "fpm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(fpm_lib, name), name
        assert name in L.SIGNATURES, name
    assert int(re.search(r"#define FPM_K_LEARN (\d+)", hdr).group(1)) == L.K_LEARN == 15
    assert int(re.search(r"#define FPM_K_COUNT (\d+)", hdr).group(1)) == len(L.PROFILE_NAMES) == 16
    assert L.PROFILE_NAMES[L.K_LEARN] == "tmpl_prep" and L.KERNEL_SYMBOLS["tmpl_prep"] == ["k_tmpl_prep"]
    # an additive change: the ABI version of the three features before
    assert int(re.search(r"#define FPM_ABI_VERSION (\d+)", hdr).group(1)) == 11


def _sums(px):
    v = px.astype(np.int64)
    return int(v.size), int(v.sum()), int((v * v).sum())


def _check_levels(t, **params):
    o = oracle.OracleMatcher().set(**params)
    assert o.learnPattern(t)
    levels, border = o.template_levels()
    for px, mean, norm, inv_area, equal1 in levels:
        got = M.learn_derive(*_sums(px))
        assert got == (mean, norm, inv_area, equal1), (px.shape, got, (mean, norm, inv_area, equal1))
    # the border colour comes from level 0's mean (TemplateMatcher.cpp:58-59)
    assert border == (255 if M.learn_derive(*_sums(levels[0][0]))[0] < 128 else 0)
    return levels


def test_derive_equals_the_oracle_on_every_template_level(templates, oracle_lib, fpm_lib):
    n = 0
    for name, t in sorted(templates.items()):
        n += len(_check_levels(t))
        n += len(_check_levels(t, min_reduce_area=64))   # deeper pyramids, odd level sizes
    assert n > 2 * len(templates)   # pyramids, not only level 0


def test_derive_on_a_constant_image(oracle_lib, fpm_lib):
    levels = _check_levels(np.full((20, 20), 77, np.uint8))
    assert all(lv[4] for lv in levels)   # vecResultEqual1 on every level
    mean, norm, inv_area, equal1 = M.learn_derive(400, 77 * 400, 77 * 77 * 400)
    assert (mean, norm, inv_area, equal1) == (77.0, 0.0, 1.0 / 400.0, True)


def test_derive_on_random_images(oracle_lib, fpm_lib):
    rng = np.random.default_rng(16)
    for _ in range(40):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        lo, hi = sorted(int(v) for v in rng.integers(0, 256, 2))
        _check_levels(rng.integers(lo, hi + 1, (h, w), dtype=np.uint8), min_reduce_area=64)


def test_derive_rejects_sums_of_no_pixels(fpm_lib):
    M.learn_derive(4, 4 * 255, 4 * 65025)            # the largest sums of four bytes
    for n, s, q in [(0, 0, 0), (-3, 0, 0),           # n <= 0
                    (4, 4 * 255 + 1, 4 * 65025),     # sum > 255 n
                    (4, 4 * 255, 4 * 65025 + 1),     # sum_sq > 65025 n
                    (4, -1, 10), (4, 10, -1),
                    (4, 40, 399)]:                   # n sum_sq < sum^2: the sums of no four numbers
        with pytest.raises(ValueError):
            M.learn_derive(n, s, q)
    d = C.c_double()
    e = C.c_int32()
    assert fpm_lib.fpm_learn_derive(4, 40, 400, None, C.byref(d), C.byref(d), C.byref(e)) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_learn_derive(4, 40, 400, C.byref(d), C.byref(d), C.byref(d), None) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_learn_derive(4, 40, 400, C.byref(d), C.byref(d), C.byref(d), C.byref(e)) == L.FPM_OK


def test_null_contexts_are_rejected_without_a_device(fpm_lib):
    assert fpm_lib.fpm_learn_device(None, None, 8, 8, 8, 0, L.FMT_GRAY8, None) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_learn_at(None, None, 0, 0.0, 0.0, 0.0) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_learn_hit(None, None, 0, 0) == L.FPM_E_INVALID_ARG
    n = C.c_size_t()
    assert fpm_lib.fpm_template_operands(None, None, C.byref(n), None, C.byref(n)) == L.FPM_E_INVALID_ARG
