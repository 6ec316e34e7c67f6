"""The device blob entries at the boundary (no GPU needed): exported by libfpm_hip.so, bound in Python, additive."""
import ctypes as C

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd.matcher import TemplateMatcher

ENTRIES = ("fpm_last_blobs", "fpm_blobs_at", "fpm_op_blobs", "fpm_blobs_set_round", "fpm_blobs_profile")


def test_library_exports_the_entries(fpm_lib):
    for name in ENTRIES:
        assert hasattr(fpm_lib, name), name
        assert name in L.SIGNATURES, name
        assert getattr(fpm_lib, name).restype is C.c_int


def test_python_wrappers_exist():
    for name in ("last_blobs", "blobs_at", "op_blobs", "blobs_set_round", "blobs_profile"):
        assert callable(getattr(TemplateMatcher, name)), name
    assert (L.BLOB_TILE, L.BLOB_MERGE, L.BLOB_FLATTEN, L.BLOB_SLOTS, L.BLOB_FEATURES) == (0, 1, 2, 3, 4)
    assert len(L.BLOB_KERNEL_SYMBOLS) == 5


def test_abi_version_is_unchanged(fpm_lib):
    assert fpm_lib.fpm_abi_version() == 11


def test_null_context_is_refused(fpm_lib):
    n = C.c_int32(5)
    assert fpm_lib.fpm_last_blobs(None, 0, 8, 48, 0, 0, 8, 4, None, None, None, 64, 0, C.byref(n)) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_blobs_at(None, None, None, None, 0, 8, 48, 0, 0, 8, 4, None, None, None, 64) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_op_blobs(None, None, 1, 1, 1, 1, 0, 8, 1, None, None, 1, None) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_blobs_set_round(None, 0) == L.FPM_E_INVALID_ARG
    ms, k, b = C.c_double(), C.c_int64(), C.c_int64()
    assert fpm_lib.fpm_blobs_profile(None, 0, C.byref(ms), C.byref(k), C.byref(b)) == L.FPM_E_INVALID_ARG
