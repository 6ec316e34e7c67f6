"""Device-memory input (fpm_stage_sources_device / fpm_match_device / fpm_op_to_gray), the parts that need no GPU: the
format constants, the null-context guard of the three entries, the layout rule of the torch entries on bare
(shape, strides) tuples, and the gray conversion's integer formula."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib, images
from fastest_image_pattern_matching_amd.matcher import device_format, device_layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gray_restated(b, g, r):
    """gray = (1868 B + 9617 G + 4899 R + 8192) >> 14 in exact integers (include/fpm.h)."""
    b, g, r = (np.asarray(v).astype(np.int64) for v in (b, g, r))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def test_format_constants_equal_the_header():
    hdr = open(os.path.join(REPO, "include", "fpm.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define FPM_FMT_([A-Z0-9_]+) (\d+)", hdr)}
    assert got == {"GRAY8": _lib.FMT_GRAY8, "BGR8": _lib.FMT_BGR8, "RGB8": _lib.FMT_RGB8, "BGRA8": _lib.FMT_BGRA8,
                   "RGBA8": _lib.FMT_RGBA8, "BGR8_PLANAR": _lib.FMT_BGR8_PLANAR, "RGB8_PLANAR": _lib.FMT_RGB8_PLANAR,
                   "COUNT": _lib.FMT_COUNT}
    assert sorted(v for k, v in got.items() if k != "COUNT") == list(range(got["COUNT"]))


def test_entries_reject_a_null_context(fpm_lib):
    n = C.c_int32()
    ptrs = (C.c_void_p * 1)(16)
    out = (C.c_uint8 * 16)()
    assert fpm_lib.fpm_stage_sources_device(None, ptrs, 1, 4, 4, 4, 0, _lib.FMT_GRAY8, None) == _lib.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_match_device(None, 16, 4, 4, 4, 0, _lib.FMT_GRAY8, None, None, 0, C.byref(n), None) == \
        _lib.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_op_to_gray(None, out, 4, 4, 4, 0, _lib.FMT_GRAY8, 0, out, 4) == _lib.FPM_E_INVALID_ARG


def test_hip_runtimes_lists_the_loaded_runtime(fpm_lib):
    rts = _lib.hip_runtimes()
    assert rts and all(os.path.basename(p).startswith("libamdhip64.so") and os.path.exists(p) for p in rts)


# ---- the layout rule ------------------------------------------------------------------------------------------
H, W = 7, 10


def test_layout_contiguous():
    assert device_layout((H, W), (W, 1)) == ("gray", H, W, 1, W, 0)
    assert device_layout((H, W, 3), (3 * W, 3, 1)) == ("hwc", H, W, 3, 3 * W, 0)
    assert device_layout((H, W, 4), (4 * W, 4, 1)) == ("hwc", H, W, 4, 4 * W, 0)
    assert device_layout((3, H, W), (H * W, W, 1)) == ("chw", H, W, 3, W, H * W)


def test_layout_views():
    # row-padded and column-sliced: the row stride is the parent's
    assert device_layout((H, W), (64, 1)) == ("gray", H, W, 1, 64, 0)
    assert device_layout((H, W, 3), (200, 3, 1)) == ("hwc", H, W, 3, 200, 0)
    assert device_layout((H, W, 4), (4 * W + 4, 4, 1)) == ("hwc", H, W, 4, 4 * W + 4, 0)
    # planar cut from a larger (3, H + 5, 37) tensor: plane stride > row stride x height
    assert device_layout((3, H, W), ((H + 5) * 37, 37, 1)) == ("chw", H, W, 3, 37, (H + 5) * 37)
    # one plane of a planar tensor, one row of a gray one
    assert device_layout((H, W), (37, 1)) == ("gray", H, W, 1, 37, 0)
    assert device_layout((1, W), (12345, 1)) == ("gray", 1, W, 1, W, 0)
    # numpy hands over byte strides of real views the same way
    wide = np.zeros((H, 50, 3), np.uint8)
    v = wide[:, 5:5 + W]
    assert device_layout(v.shape, v.strides) == ("hwc", H, W, 3, 150, 0)


def test_layout_channel_slice_is_rejected():
    bgra = np.zeros((H, W, 4), np.uint8)
    for v in (bgra[..., :3], bgra[..., 1:]):   # three channels of a four-byte pixel: pixel stride 4, not 3
        with pytest.raises(ValueError, match="pixel stride"):
            device_layout(v.shape, v.strides)
    with pytest.raises(ValueError, match="pixel stride"):   # one channel of an interleaved image as "gray"
        device_layout(bgra[..., 0].shape, bgra[..., 0].strides)


def test_layout_ambiguous_shape_needs_a_hint():
    for c in (3, 4):
        shape, strides = (3, H, c), (H * c, c, 1)
        with pytest.raises(ValueError, match="layout="):
            device_layout(shape, strides)
        assert device_layout(shape, strides, "hwc") == ("hwc", 3, H, c, H * c, 0)
        assert device_layout(shape, strides, "chw") == ("chw", H, c, 3, c, H * c)
    assert device_layout((3, H, 5), (H * 5, 5, 1)) == ("chw", H, 5, 3, 5, H * 5)   # only one rule fits


@pytest.mark.parametrize("shape,strides,layout", [
    ((H, W), (W, 2), None),                 # column step
    ((H, W), (-W, 1), None),                # flipped rows
    ((H, W), (W, -1), None),                # flipped columns
    ((H, W), (W - 1, 1), None),             # overlapping rows
    ((H, W, 3), (3 * W, 3, 2), None),       # channel step
    ((H, W, 3), (3 * W, 6, 1), None),       # every second pixel
    ((H, W, 3), (3 * W - 1, 3, 1), None),   # overlapping rows
    ((H, W, 3), (3, 3 * H, 1), None),       # transposed
    ((3, H, W), (H * W, W, 2), None),       # planar with a column step
    ((3, H, W), (H * W - 1, W, 1), None),   # overlapping planes
    ((3, H, W), (-H * W, W, 1), None),      # planes in reverse
    ((H, W, 2), (2 * W, 2, 1), None),       # two channels
    ((4, H, W), (H * W, W, 1), None),       # four planes
    ((H, W, 3), (3 * W, 3, 1), "chw"),      # hint that does not fit
    ((H, W), (W, 1), "hwc"),                # hint on a gray image
    ((H, W, 3), (3 * W, 3, 1), "nhwc"),     # unknown hint
    ((W,), (1,), None),                     # 1-D
    ((2, 3, H, W), (3 * H * W, H * W, W, 1), None),   # batch dimension
    ((0, W), (W, 1), None),                 # empty
])
def test_layout_rejections(shape, strides, layout):
    with pytest.raises(ValueError):
        device_layout(shape, strides, layout)


def test_format_of_layout_and_channel_order():
    assert device_format("gray", 1, "bgr") == device_format("gray", 1, "rgb") == _lib.FMT_GRAY8
    assert device_format("hwc", 3, "bgr") == _lib.FMT_BGR8 and device_format("hwc", 3, "rgb") == _lib.FMT_RGB8
    assert device_format("hwc", 4, "bgr") == _lib.FMT_BGRA8 and device_format("hwc", 4, "rgba") == _lib.FMT_RGBA8
    assert device_format("chw", 3, "bgr") == _lib.FMT_BGR8_PLANAR and device_format("chw", 3, "RGB") == _lib.FMT_RGB8_PLANAR
    for bad in [("hwc", 3, "gbr"), ("hwc", 3, "bgra"), ("chw", 3, "rgba")]:
        with pytest.raises(ValueError):
            device_format(*bad)


# ---- the formula ----------------------------------------------------------------------------------------------
def test_restatement_agrees_with_the_load_path():
    rgb = np.random.default_rng(11).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert np.array_equal(gray_restated(rgb[..., 2], rgb[..., 1], rgb[..., 0]), images.bgr_to_gray(rgb))


@pytest.mark.parametrize("bgr,gray", [((255, 0, 0), 29), ((0, 255, 0), 150), ((0, 0, 255), 76), ((255, 255, 255), 255),
                                      ((0, 0, 0), 0)])
def test_restatement_hand_values(bgr, gray):
    assert int(gray_restated(*bgr)) == gray
