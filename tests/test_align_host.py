"""Pose alignment, host side (no GPU): fpm_align_solve against the numpy restatement of tests/align_ref.py with ==,
fpm_align_update by its two properties (a zero step returns the pose; the new pose's patch map is the composed map), the
reference loop's convergence on planted scenes, and the pure argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import align_ref as ref
from tests.test_patch_host import SH, SW
from tests.test_patch_host import poses as host_poses

EDGE_POSES = [((40.0, 30.0), 0.0), ((52.25, 41.5), 30.0), ((70.5, 66.125), -137.5)]   # tests/test_gpu_compare.py's


def _sums(**kw):
    s = dict.fromkeys(ref.SUM_FIELDS, 0)
    s.update(kw)
    return s


def _check(s):
    got, exp = M.align_solve(s), ref.solve(s)
    assert got == exp, (s, got, exp)
    return got


# ---- fpm_align_solve ----------------------------------------------------------------------------------------------
def test_solve_diagonal(fpm_lib):
    du, dv, dphi, singular = _check(_sums(n_used=100, h_xx=400, h_yy=900, h_tt=250000, g_x=-100, g_y=90, g_t=500))
    assert not singular and (du, dv, dphi) == (0.5, -0.2, -0.008)    # q = -g / h; du = 2 q0, dv = 2 q1, dphi = 4 q2
    # with cross terms, against the restatement and against numpy's own solver
    s = _sums(n_used=50, h_xx=5000, h_xy=-1200, h_yy=7000, h_xt=30000, h_yt=-41000, h_tt=9000000, g_x=700, g_y=-300, g_t=12000)
    du, dv, dphi, singular = _check(s)
    H = np.array([[5000, -1200, 30000], [-1200, 7000, -41000], [30000, -41000, 9000000]], np.float64)
    q = np.linalg.solve(H, -np.array([700, -300, 12000], np.float64))
    assert not singular and np.allclose([du, dv, dphi], [2 * q[0], 2 * q[1], 4 * q[2]], rtol=1e-12, atol=0)


def test_solve_singular(fpm_lib):
    # Tx == 0 everywhere (a template of horizontal stripes): no x information
    assert _check(_sums(n_used=100, h_yy=900, h_yt=30, h_tt=250000, g_y=90, g_t=500)) == (0.0, 0.0, 0.0, True)
    # two used pixels
    assert _check(_sums(n_used=2, h_xx=400, h_yy=900, h_tt=250000, g_x=-100, g_y=90, g_t=500)) == (0.0, 0.0, 0.0, True)
    assert not _check(_sums(n_used=3, h_xx=400, h_yy=900, h_tt=250000, g_x=-100, g_y=90, g_t=500))[3]
    # everything zero, and an indefinite matrix (det < 0)
    assert _check(_sums(n_used=100))[3]
    assert _check(_sums(n_used=100, h_xx=1, h_xy=2, h_yy=1, h_tt=1, g_x=1))[3]


def test_solve_at_the_caps(fpm_lib):
    n, w, h = ref.MAX_AREA, ref.MAX_SIDE, ref.MAX_AREA // ref.MAX_SIDE      # 2^20 pixels as 4096 x 256: w + h = 4352
    j = 255 * (w + h)                                                       # above any |Jt|
    cap = dict(n_used=n, h_xx=65025 * n, h_xy=0, h_yy=65025 * n, h_xt=0, h_yt=0, h_tt=n * j * j, g_x=65025 * n,
               g_y=-65025 * n, g_t=n * j * 255, ssd=65025 * n)
    for s in (cap, dict(cap, h_xy=65025 * n // 2, h_xt=255 * j * n // 3, h_yt=-255 * j * n // 5),
              dict(cap, h_xy=65025 * n, h_xt=255 * j * n, h_yt=255 * j * n)):     # the last: rank 1, singular
        assert all(abs(v) < 2 ** 62 for v in s.values()), s
        _check(s)
    assert not M.align_solve(cap)[3] and M.align_solve(dict(cap, h_xy=65025 * n, h_xt=255 * j * n, h_yt=255 * j * n))[3]


def test_solve_on_real_sums(fpm_lib, oracle_lib):
    s, plants = ref.planted()
    seen = 0
    for T, lt, a in plants:
        for rect in [(0, 0, ref.TW, ref.TH), (3, 2, 60, 40), (0, 0, 2, 2), (1, 1, 1, 1), (0, 0, 1, 45)]:
            for slt, sa in ref.starts(lt, a) + [(lt, a)]:
                sm = ref.sums(ref.patch(s, rect, slt, sa), T, rect)
                seen += not _check(sm)[3]
    assert seen >= 12


def test_solve_rejects_null_arguments(fpm_lib):
    rec, d = L.AlignSums(), C.c_double()
    assert fpm_lib.fpm_align_solve(None, C.byref(d), C.byref(d), C.byref(d)) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_align_solve(C.byref(rec), None, C.byref(d), C.byref(d)) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_align_solve(C.byref(rec), C.byref(d), C.byref(d), C.byref(d)) == 1      # all zero: singular
    with pytest.raises(ValueError):
        M.align_solve([1, 2, 3])


# ---- fpm_align_update ---------------------------------------------------------------------------------------------
RECTS = [(0, 0, 71, 23), (3, 2, 60, 17), (5, 1, 1, 1), (0, 0, 64, 16)]


def test_update_zero_step_returns_the_pose(fpm_lib):
    for sw, sh in [(SW, SH), (4096, 3000)]:
        for lt, a in EDGE_POSES + host_poses() + [((3000.7, 2500.2), 77.0), ((0.3, 0.0004), -12.5)]:
            for rect in RECTS:
                (x2, y2), a2 = M.align_update(sw, sh, rect, lt, a, 0.0, 0.0, 0.0)
                assert a2 == a
                for got, was in ((x2, lt[0]), (y2, lt[1])):
                    was = np.float32(was)
                    assert abs(np.float64(got) - np.float64(was)) <= np.spacing(np.abs(was)), (lt, a, rect, got)


def _full(m):
    return np.vstack([m, [0.0, 0.0, 1.0]])


COMPOSED_STEPS = [(0.3, -0.2, 0.004), (-1.25, 0.75, -0.02), (0.0, 0.0, 0.01), (1.9, 1.9, 0.0), (-0.01, 0.02, 1e-5)]
COMPOSED_ULPS = 4.56     # 4 x the worst case measured on the CPU, 1.14 f32 ulp (profiles/align/README.txt)


def test_update_gives_the_composed_map(fpm_lib):
    """fpm_patch_matrix of the new pose, inverted, against A o D at the four corners of the rectangle.  Both maps carry
    f32 roundings -- the new ptLT, and the rotated ptLT inside either matrix -- so the bound is a few f32 ulp at the
    largest coordinate involved."""
    worst = 0.0
    for sw, sh in [(SW, SH), (4096, 3000)]:
        for lt, a in EDGE_POSES + host_poses() + [((3000.7, 2500.2), 77.0)]:
            for rect in RECTS:
                x, y, w, h = rect
                A = np.linalg.inv(_full(M.patch_matrix(sw, sh, lt, a, (x, y))))
                cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
                for du, dv, dphi in COMPOSED_STEPS:
                    c, s = math.cos(dphi), math.sin(dphi)
                    D = np.array([[c, -s, cx - c * cx + s * cy + du], [s, c, cy - s * cx - c * cy + dv], [0.0, 0.0, 1.0]])
                    lt2, a2 = M.align_update(sw, sh, rect, lt, a, du, dv, dphi)
                    assert a2 == a + dphi * (180.0 / math.pi)
                    A2 = np.linalg.inv(_full(M.patch_matrix(sw, sh, lt2, a2, (x, y))))
                    for px, py in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]:
                        p = np.array([px, py, 1.0])
                        want, got = (A @ D @ p)[:2], (A2 @ p)[:2]
                        big = max(np.abs(want).max(), abs(lt[0]), abs(lt[1]), abs(lt2[0]), abs(lt2[1]), sw, sh)
                        ulps = np.abs(want - got).max() / float(np.spacing(np.float32(big)))
                        worst = max(worst, ulps)
                        assert ulps <= COMPOSED_ULPS, (sw, lt, a, rect, (du, dv, dphi), ulps)
    print(f"composed map: worst {worst:.3f} f32 ulp")


def test_update_rejects_bad_arguments(fpm_lib):
    f, d, r = C.c_float(), C.c_double(), L.PatchRect(0, 0, 4, 4)
    ok = (100, 80, C.byref(r), 1.0, 2.0, 3.0, 0.0, 0.0, 0.0)
    assert fpm_lib.fpm_align_update(*ok, C.byref(f), C.byref(f), C.byref(d)) == L.FPM_OK
    assert fpm_lib.fpm_align_update(*ok, None, C.byref(f), C.byref(d)) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_align_update(100, 80, None, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, C.byref(f), C.byref(f), C.byref(d)) == \
        L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_align_update(0, 80, C.byref(r), 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, C.byref(f), C.byref(f), C.byref(d)) == \
        L.FPM_E_INVALID_ARG


# ---- the reference loop converges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", range(len(ref.PLANTED)))
def test_reference_loop_converges(plant, fpm_lib, oracle_lib):
    s, plants = ref.planted()
    T, lt, a = plants[plant]
    assert np.array_equal(ref.patch(s, (0, 0, ref.TW, ref.TH), lt, a), T)
    for rect in [(0, 0, ref.TW, ref.TH), (3, 2, 60, 40)]:
        c_true = ref.centre(s.shape, rect, lt, a)
        for slt, sa in ref.starts(lt, a):
            o = ref.loop(s, T, rect, slt, sa, 3)
            e0 = float(np.linalg.norm(ref.centre(s.shape, rect, slt, sa) - c_true))
            e1 = float(np.linalg.norm(ref.centre(s.shape, rect, (o["lt_x"], o["lt_y"]), o["angle"]) - c_true))
            print(f"plant {plant} rect {rect} start {e0:.4f} px -> {e1:.5f} px, {sa - a:+.3f} -> {o['angle'] - a:+.5f} deg, "
                  f"ssd {o['ssd_start']} -> {o['ssd']}")
            assert e1 < e0 and e1 < 1.0 / 16.0      # two steps of warpAffine's 1/32-pixel sampling grid
            assert o["ssd"] <= o["ssd_start"] and o["flags"] == 0 and o["evals"] == 4
    # at the planted pose itself nothing is left to do: the residual is zero, so is the step
    o = ref.loop(s, T, (0, 0, ref.TW, ref.TH), lt, a, 2)
    assert o["ssd_start"] == 0 and o["ssd"] == 0 and o["best_eval"] == 0 and o["flags"] == L.ALIGN_KEPT_START
    assert (o["lt_x"], o["lt_y"], o["angle"]) == (float(np.float32(lt[0])), float(np.float32(lt[1])), a)


def test_a_far_start_is_stopped(fpm_lib, oracle_lib):
    """40 px off there is nothing to converge to: on the first planted scene the first step is far beyond max_step.  (No
    law makes it so -- on other texture a far start can find small steps that lower ssd -- but ssd never rises.)"""
    s, plants = ref.planted()
    for k, (T, lt, a) in enumerate(plants):
        o = ref.loop(s, T, (0, 0, ref.TW, ref.TH), (lt[0] + 40.0, lt[1]), a, 3)
        assert o["ssd"] <= o["ssd_start"]
        if k == 0:
            assert o["flags"] & (L.ALIGN_STEP_CLAMPED | L.ALIGN_KEPT_START) and o["evals"] == 1


# ---- argument rules -------------------------------------------------------------------------------------------------
def test_align_rect():
    tw, th = 40, 30
    assert M.align_rect(None, tw, th) == (0, 0, 40, 30)
    assert M.align_rect(np.array([39, 29, 1, 1]), tw, th) == (39, 29, 1, 1)
    assert M.align_rect((3, 2, 37, 28), tw, th) == (3, 2, 37, 28)
    for bad in [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 41, 30), (0, 0, 40, 31), (1, 0, 40, 30), (0, 1, 40, 30),
                (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, 4), (0.5, 0, 4, 4), "abcd", (40, 0, 1, 1)]:
        with pytest.raises(ValueError):
            M.align_rect(bad, tw, th)
    # the caps: 2^20 pixels pass, one row more does not; a side of 4096 passes, 4097 does not; NULL over a large template
    assert M.align_rect((0, 0, 1024, 1024), 5000, 5000) == (0, 0, 1024, 1024)
    assert M.align_rect((7, 9, 4096, 256), 5000, 5000) == (7, 9, 4096, 256)
    assert M.align_rect((0, 0, 762, 521), 762, 521) == (0, 0, 762, 521)
    for bad in [(0, 0, 1024, 1025), (0, 0, 4097, 1), (0, 0, 1, 4097), (0, 0, 4096, 257)]:
        with pytest.raises(ValueError):
            M.align_rect(bad, 5000, 5000)
    with pytest.raises(ValueError):
        M.align_rect(None, 1025, 1024)
    assert M.compare_rect((0, 0, 1024, 1025), 5000, 5000)      # a comparison's cap is the wider one


def test_entries_reject_null_arguments_without_a_device(fpm_lib):
    n = C.c_int32()
    assert fpm_lib.fpm_align_last(None, None, 0, 3, 2.0, 0, None, 0, C.byref(n)) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_align_at(None, None, None, None, None, 0, 3, 2.0, 0, None) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_align_sums_at(None, None, None, None, None, 0, 0, None) == L.FPM_E_INVALID_ARG
    d, i = C.c_double(), C.c_int64()
    assert fpm_lib.fpm_align_profile(None, C.byref(d), C.byref(i), C.byref(i)) == L.FPM_E_INVALID_ARG


def test_record_layouts():
    assert M.ALIGN_SUMS_DTYPE.itemsize == C.sizeof(L.AlignSums) == 88
    assert M.ALIGN_DTYPE.itemsize == C.sizeof(L.AlignResult) == 56
    assert list(M.ALIGN_SUMS_DTYPE.names) == [f[0] for f in L.AlignSums._fields_] == list(ref.SUM_FIELDS)
    assert list(M.ALIGN_DTYPE.names) == [f[0] for f in L.AlignResult._fields_] == list(ref.RESULT_FIELDS)
    for struct, dtype in ((L.AlignSums, M.ALIGN_SUMS_DTYPE), (L.AlignResult, M.ALIGN_DTYPE)):
        for name, _ in struct._fields_:
            assert dtype.fields[name][1] == getattr(struct, name).offset


def test_library_holds_the_kernel(fpm_lib):
    from tests.test_abi import _kernel_symbols

    ks = [k for k in _kernel_symbols() if k.startswith("fpm::" + L.ALIGN_KERNEL_SYMBOL + "<")]
    assert sorted(ks) == ["fpm::k_patch_align<false>", "fpm::k_patch_align<true>"], ks
