"""The C-ABI library builds, loads and exports every entry point include/fpm.h declares (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

from fastest_image_pattern_matching_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(REPO, "include", "fpm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fpm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_boundary():
    syms = declared_symbols()
    for must in ("fpm_create", "fpm_destroy", "fpm_set_params", "fpm_learn", "fpm_match", "fpm_last_error"):
        assert must in syms


def test_library_exports_every_declared_symbol(fpm_lib):
    missing = [s for s in declared_symbols() if not hasattr(fpm_lib, s)]
    assert not missing, missing


def test_python_binding_covers_header(fpm_lib):
    assert set(declared_symbols()) == set(_lib.SIGNATURES)


def test_result_struct_is_s_single_target_match_layout():
    # five cv::Point2d + dMatchedAngle + dMatchScore = 12 doubles (DataStructures.h:97-115)
    assert C.sizeof(_lib.Result) == 12 * 8


def test_defaults_equal_reference_constructor(fpm_lib):
    p = _lib.Params()
    fpm_lib.fpm_params_default(C.byref(p))
    assert (p.max_pos, p.max_overlap, p.score, p.tolerance_angle, p.min_reduce_area, p.use_simd, p.subpixel) == \
        (70, 0.0, 0.7, 0.0, 256, 1, 0)


def test_abi_version(fpm_lib):
    hdr = open(os.path.join(REPO, "include", "fpm.h")).read()
    assert fpm_lib.fpm_abi_version() == int(re.search(r"#define FPM_ABI_VERSION (\d+)", hdr).group(1))


def test_null_arguments_are_rejected_without_a_device(fpm_lib):
    assert fpm_lib.fpm_create(0, None) == _lib.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_destroy(None) == _lib.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_set_params(None, None) == _lib.FPM_E_INVALID_ARG


def test_library_is_gfx950_code_object():
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"gfx942" not in blob and b"gfx90a" not in blob


def _kernel_symbols():
    import shutil
    import subprocess

    so = os.path.join(REPO, "fastest_image_pattern_matching_amd", "lib", "libfpm_hip.so")
    nm = shutil.which("nm")
    if not (nm and os.path.exists(so)):
        pytest.skip("nm or libfpm_hip.so missing")
    out = subprocess.run([nm, "-C", so], capture_output=True, text=True, check=True).stdout
    return sorted({m.group(1) for m in re.finditer(r"(fpm::k_[a-z0-9_]+(?:<[^>]*>)?)\(", out)})


def test_product_library_holds_no_measurement_kernels():
    """The product library carries only result-path kernels: no fused K6+K7 experiment and no 16-row-item
    correlation (scripts/roi_fused.hip / roi_corr16.hip, built only into fused_bench / corr16_bench), and every ablation template parameter of k_roi_corr / k_roi_small (MODE) and
    k_roi_warp (ABL) at its product value 0 -- the profiling instantiations exist only in scripts/*.hip."""
    ks = _kernel_symbols()
    assert any(k.startswith("fpm::k_roi_warp3") for k in ks) and any(k.startswith("fpm::k_roi_corr<") for k in ks)
    assert not [k for k in ks if "k_roi_fused" in k]
    assert not [k for k in ks if "k_roi_corr16" in k]   # measured slower (round 5): scripts/corr16_bench.hip only
    for k in ks:
        args = k[k.index("<") + 1:-1].split(", ") if "<" in k else []
        if k.startswith(("fpm::k_roi_corr<", "fpm::k_roi_small<", "fpm::k_pyr_down<")):
            assert args[0] == "0", k
        if k.startswith("fpm::k_roi_warp<"):
            assert args[1] == "0", k
        if k.startswith("fpm::k_roi_warp3<"):
            assert args[2] == "0" and len(args) == 3, k   # <WPE, PITCH, ABL>: no ablation, no measurement-only form
        if k.startswith("fpm::k_roi_corr<"):
            assert len(args) == 7, k   # <MODE, WPE, NK, PFR, RS, SE, DMA>: no double-buffered measurement form


def test_product_sources_hold_no_measurement_kernels():
    """No file under csrc/ mentions the measurement-only kernels or the define that once guarded them: they live in
    scripts/roi_fused.hip and scripts/roi_corr16.hip."""
    csrc = os.path.join(REPO, "fastest_image_pattern_matching_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if os.path.isfile(os.path.join(csrc, f)))
    assert any(f.endswith(".hip") for f in files)
    for f in files:
        text = open(os.path.join(csrc, f), errors="replace").read()
        for word in ("FPM_EXPERIMENTAL", "k_roi_fused", "k_roi_corr16"):
            assert word not in text, (f, word)


def test_product_switches_are_result_neutral():
    """Every environment switch the product library reads is a schedule or diagnostic knob whose both settings are
    parity-tested (DESIGN.md section 1 lists them); none selects an ablation."""
    csrc = os.path.join(REPO, "fastest_image_pattern_matching_amd", "csrc")
    names = set()
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".cpp", ".h")):
            names |= set(re.findall(r'getenv\("(FPM_[A-Z0-9_]+)"\)', open(os.path.join(csrc, f)).read()))
    assert names <= {"FPM_SCRATCH_MB", "FPM_TOP_FUSED", "FPM_OVERLAP_DEVICE_MIN", "FPM_TAIL_TIMES", "FPM_PYR_WGS",
                     "FPM_PYR_OH", "FPM_PYR2_OH", "FPM_STEP_PROLOGUE", "FPM_STEP_TABLES", "FPM_PYR2", "FPM_WARP3", "FPM_HOST_THREADS", "FPM_POOL_TRACE",
                     "FPM_HOST_WARM", "FPM_GRID_WARP", "FPM_GRID_CORR", "FPM_GRID_SMALL", "FPM_GRID_TOP", "FPM_SMALL_NT",
                     "FPM_TOP_MMA", "FPM_TOP_LIST_CAP"}, names
