"""Python mirror of the reference's ``TemplateMatcher`` (include/TemplateMatcher.h:9-90) over the C ABI.

Same method names, argument meaning and error behaviour as the C++ class: ``learnPattern`` returns False on an
empty image (TemplateMatcher.cpp:47-49); ``match`` returns an empty list on an empty source, an unlearned
template or a size mismatch (:99-114); ``getLastExecutionTime`` keeps its previous value when a search finds
nothing (:398-404).  All pixel work runs in libfpm_hip.so on a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


@dataclass
class SingleTargetMatch:
    """s_SingleTargetMatch (DataStructures.h:97-115)."""

    ptLT: Tuple[float, float]
    ptRT: Tuple[float, float]
    ptRB: Tuple[float, float]
    ptLB: Tuple[float, float]
    ptCenter: Tuple[float, float]
    dMatchedAngle: float
    dMatchScore: float

    @staticmethod
    def from_c(r: "L.Result") -> "SingleTargetMatch":
        return SingleTargetMatch((r.lt_x, r.lt_y), (r.rt_x, r.rt_y), (r.rb_x, r.rb_y), (r.lb_x, r.lb_y),
                                 (r.cx, r.cy), r.angle, r.score)

    @staticmethod
    def from_row(r) -> "SingleTargetMatch":
        v = [float(x) for x in r]
        return SingleTargetMatch((v[0], v[1]), (v[2], v[3]), (v[4], v[5]), (v[6], v[7]), (v[8], v[9]), v[10], v[11])

    def getCenterQPoint(self):
        return self.ptCenter

    def getBoundingRect(self):
        xs = [self.ptLT[0], self.ptRT[0], self.ptRB[0], self.ptLB[0]]
        ys = [self.ptLT[1], self.ptRT[1], self.ptRB[1], self.ptLB[1]]
        return (min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys))

    def as_tuple(self):
        return (*self.ptLT, *self.ptRT, *self.ptRB, *self.ptLB, *self.ptCenter, self.dMatchedAngle,
                self.dMatchScore)


# fpm_candidate as a numpy record (include/fpm.h), 56 bytes
CANDIDATE_DTYPE = np.dtype([("top_score", "<f8"), ("x", "<f8"), ("y", "<f8"), ("score", "<f8"), ("angle", "<f8"),
                            ("angle_index", "<i4"), ("peak_rank", "<i4"), ("source", "<i4"), ("kept", "<i4")])
assert CANDIDATE_DTYPE.itemsize == C.sizeof(L.Candidate)


# fpm_roi_record as a numpy record (include/fpm.h), 52 bytes
ROI_RECORD_DTYPE = np.dtype([("score", "<f4"), ("mx", "<i4"), ("my", "<i4"), ("on_border", "<i4"), ("vec", "<f4", 9)])
assert ROI_RECORD_DTYPE.itemsize == C.sizeof(L.RoiRecord)

# fpm_peak as a numpy record (include/fpm.h), 12 bytes
PEAK_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("score", "<f4")])
assert PEAK_DTYPE.itemsize == C.sizeof(L.Peak)


def merge_candidates(params: "L.Params", tmpl_w: int, tmpl_h: int, cands: np.ndarray) -> List[SingleTargetMatch]:
    """fpm_merge_candidates: the coupled tail of TemplateMatcher::match (TemplateMatcher.cpp:214, 262-432) over one
    source's candidate records in push order (all shards concatenated in shard order).  Host only (no device)."""
    lib = L.load()
    c = np.ascontiguousarray(cands, CANDIDATE_DTYPE)
    cap = max(16, len(c))
    out = (L.Result * cap)()
    n = C.c_int32()
    rc = lib.fpm_merge_candidates(C.byref(params), int(tmpl_w), int(tmpl_h),
                                  c.ctypes.data_as(C.POINTER(L.Candidate)), len(c), out, cap, C.byref(n))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_merge_candidates failed with {rc} (records not in push order?)")
    return [SingleTargetMatch.from_c(out[i]) for i in range(n.value)]


def _gray(img) -> np.ndarray:
    a = np.asarray(img)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise TypeError("expected a 2-D uint8 (CV_8UC1) image")
    return np.ascontiguousarray(a)


_one_runtime = False   # torch and libfpm_hip.so were seen to share one HIP runtime (_lib.hip_runtimes, checked once)


def device_layout(shape, strides, layout=None):
    """How a uint8 image with this ``shape`` and these ``strides`` (in elements = bytes) lies in memory, for the
    device-memory entries (fpm_match_device, fpm_stage_sources_device, fpm_op_to_gray).  Pure: works on the two tuples,
    needs neither torch nor a device.  Returns ``(kind, height, width, channels, row_stride, plane_stride)`` with kind
    "gray", "hwc" (interleaved) or "chw" (planar; plane_stride is 0 otherwise).

    * 2-D (H, W) is gray: unit pixel stride.
    * 3-D (H, W, C) with C in (3, 4), unit channel stride and pixel stride C is interleaved.
    * 3-D (3, H, W) with unit pixel stride is planar: strides[1] is the row stride, strides[0] the plane stride.
    * A shape both rules fit, (3, H, 3) or (3, H, 4), needs ``layout="hwc"`` or ``"chw"``.

    Row strides wider than a row, plane strides wider than a plane and any base offset are fine (views into larger
    tensors).  Everything else raises ValueError: a non-unit pixel or channel stride (a channel slice of a wider pixel,
    a column step), negative strides, rows or planes that overlap.  The stride of a dimension of size 1 is not looked
    at."""
    shape = tuple(int(v) for v in shape)
    strides = tuple(int(v) for v in strides)
    if layout not in (None, "hwc", "chw"):
        raise ValueError(f"layout must be 'hwc', 'chw' or None, not {layout!r}")
    if len(shape) != len(strides) or len(shape) not in (2, 3):
        raise ValueError(f"expected a 2-D (H, W) or 3-D (H, W, C) / (3, H, W) image, got shape {shape}")
    if any(n <= 0 for n in shape):
        raise ValueError(f"empty image: shape {shape}")
    if any(st < 0 for n, st in zip(shape, strides) if n > 1):
        raise ValueError(f"negative strides {strides} are not supported")

    def unit(d):
        return shape[d] == 1 or strides[d] == 1

    def at_least(d, least):   # a stride that must clear the extent below it; free when the dimension has one entry
        return least if shape[d] == 1 else (strides[d] if strides[d] >= least else None)

    if len(shape) == 2:
        if layout is not None:
            raise ValueError("layout applies to 3-D images only")
        h, w = shape
        if not unit(1):
            raise ValueError(f"pixel stride {strides[1]} of a gray image must be 1 (no column steps or channel slices)")
        row = at_least(0, w)
        if row is None:
            raise ValueError(f"row stride {strides[0]} below the width {w}")
        return "gray", h, w, 1, row, 0

    def hwc():
        h, w, c = shape
        if c not in (3, 4):
            return f"{c} channels (3 or 4 expected)"
        if not unit(2):
            return f"channel stride {strides[2]} must be 1"
        if w > 1 and strides[1] != c:
            return f"pixel stride {strides[1]} must equal the channel count {c} (no channel slices of wider pixels)"
        row = at_least(0, w * c)
        if row is None:
            return f"row stride {strides[0]} below width x channels = {w * c}"
        return "hwc", h, w, c, row, 0

    def chw():
        c, h, w = shape
        if c != 3:
            return f"{c} planes (3 expected)"
        if not unit(2):
            return f"pixel stride {strides[2]} must be 1"
        row = at_least(1, w)
        if row is None:
            return f"row stride {strides[1]} below the width {w}"
        plane = at_least(0, row * h)
        if plane is None:
            return f"plane stride {strides[0]} below row stride x height = {row * h}"
        return "chw", h, w, 3, row, plane

    fits_hwc, fits_chw = shape[2] in (3, 4), shape[0] == 3
    if layout is None and fits_hwc and fits_chw:
        raise ValueError(f"shape {shape} reads as interleaved (H, W, C) and as planar (3, H, W): pass layout='hwc' or "
                         f"layout='chw'")
    if layout is None and not (fits_hwc or fits_chw):
        raise ValueError(f"shape {shape} is neither (H, W, 3 or 4) nor (3, H, W)")
    got = hwc() if (layout == "hwc" or (layout is None and fits_hwc)) else chw()
    if isinstance(got, str):
        raise ValueError(f"shape {shape}, strides {strides}: {got}")
    return got


def device_format(kind: str, channels: int, channel_order: str = "bgr") -> int:
    """The FPM_FMT_* of a device_layout kind and a channel order ("bgr" or "rgb"; "bgra" / "rgba" say the same for four
    channels).  The order does not matter for gray."""
    order = str(channel_order).lower()
    if order not in ("bgr", "rgb", "bgra", "rgba"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', not {channel_order!r}")
    if kind == "gray":
        return L.FMT_GRAY8
    rgb = order.startswith("rgb")
    if len(order) == 4 and (kind != "hwc" or channels != 4):
        raise ValueError(f"channel_order {channel_order!r} needs a four-channel interleaved image")
    if kind == "chw":
        return L.FMT_RGB8_PLANAR if rgb else L.FMT_BGR8_PLANAR
    if channels == 4:
        return L.FMT_RGBA8 if rgb else L.FMT_BGRA8
    return L.FMT_RGB8 if rgb else L.FMT_BGR8


# -- match patches (fpm_last_patches* / fpm_patches_at): pure argument checks, no device needed ----------------------
PATCH_MAX_SIDE = 8192


def normalize_rect(rect) -> Tuple[int, int, int, int]:
    """A patch rectangle (x, y, w, h) in template coordinates as four ints.  It may reach outside the template; width
    and height must be 1 .. 8192 (include/fpm.h).  Raises ValueError otherwise."""
    try:
        x, y, w, h = (int(v) for v in rect)
    except (TypeError, ValueError):
        raise ValueError(f"expected a rectangle (x, y, w, h), got {rect!r}") from None
    if any(float(v) != i for v, i in zip(rect, (x, y, w, h))):
        raise ValueError(f"rectangle {tuple(rect)!r} must hold whole numbers")
    if not (1 <= w <= PATCH_MAX_SIDE and 1 <= h <= PATCH_MAX_SIDE):
        raise ValueError(f"rectangle {(x, y, w, h)}: width and height must be 1 .. {PATCH_MAX_SIDE}")
    return x, y, w, h


def patch_out_layout(shape, strides, n: int, ph: int, pw: int) -> Tuple[int, int]:
    """(row_stride, patch_stride) in bytes of a uint8 output of ``shape`` and ``strides`` (in elements = bytes) that is to
    receive ``n`` patches of ``ph`` x ``pw`` (last_patches_device's ``out``).  The shape must be (n, ph, pw); the pixel
    stride must be 1, rows must not overlap, patches must not overlap (views into larger tensors are fine: a column
    slice, a row slice, every k-th patch slot).  The stride of a dimension of size 1 is not looked at.  Raises
    ValueError otherwise."""
    shape = tuple(int(v) for v in shape)
    strides = tuple(int(v) for v in strides)
    if shape != (n, ph, pw) or len(strides) != 3:
        raise ValueError(f"out must have shape {(n, ph, pw)}, got {shape}")
    if pw > 1 and strides[2] != 1:
        raise ValueError(f"pixel stride {strides[2]} of out must be 1")
    row = strides[1] if ph > 1 else pw   # one row per patch: only the patch stride matters
    if row < pw:
        raise ValueError(f"row stride {row} of out below the patch width {pw}")
    patch = strides[0] if n > 1 else row * ph
    if patch < row * ph:
        raise ValueError(f"patch stride {patch} of out below row stride x height = {row * ph}")
    return row, patch


def patch_poses(src_index, lts, angles):
    """(src_index int32 [n], lt float32 [n, 2], angles float64 [n]) for patches_at, from array-likes of matching
    lengths; a scalar src_index stands for every pose.  Raises ValueError on a mismatch or a non-finite value."""
    lt = np.ascontiguousarray(lts, np.float32)
    if lt.ndim == 1 and lt.size == 2:
        lt = lt.reshape(1, 2)
    if lt.ndim != 2 or lt.shape[1] != 2:
        raise ValueError(f"lts must be (n, 2) points (x, y), got shape {lt.shape}")
    n = lt.shape[0]
    ang = np.ascontiguousarray(angles, np.float64).reshape(-1)
    if ang.size != n:
        raise ValueError(f"{n} points but {ang.size} angles")
    idx = np.asarray(src_index)
    if idx.ndim == 0:
        idx = np.full(n, int(idx))
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
    if idx.size != n:
        raise ValueError(f"{n} points but {idx.size} source indices")
    if not (np.isfinite(lt).all() and np.isfinite(ang).all()):
        raise ValueError("poses must be finite")
    if n and idx.min() < 0:
        raise ValueError("negative source index")
    return idx, lt, ang


def _ptr(a, ctype):
    """``a``'s data as a ``ctype`` pointer (None stays NULL); the pointer keeps the array alive."""
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _pose_args(src_index, lts, angles):
    """``(src_index*, lt*, angles*, n)`` as every fpm_*_at entry takes them, from patch_poses' arrays, which the
    pointers keep alive."""
    idx, lt, ang = patch_poses(src_index, lts, angles)
    return _ptr(idx, C.c_int32), _ptr(lt, C.c_float), _ptr(ang, C.c_double), len(idx)


def patch_matrix(src_w: int, src_h: int, lt, angle: float, rect_xy=(0, 0)) -> np.ndarray:
    """fpm_patch_matrix: the forward 2x3 matrix of the patch of a pose (ptLT ``lt`` as f32, ``angle`` in degrees) on a
    ``src_w`` x ``src_h`` source, for a rectangle whose origin is ``rect_xy`` in template coordinates.  Host only (no
    device): cv::warpAffine(source, m, (w, h), INTER_LINEAR, BORDER_CONSTANT 0) is the patch."""
    m = (C.c_double * 6)()
    rc = L.load().fpm_patch_matrix(int(src_w), int(src_h), float(np.float32(lt[0])), float(np.float32(lt[1])),
                                   float(angle), int(rect_xy[0]), int(rect_xy[1]), m)
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_patch_matrix failed with {rc}")
    return np.array(m[:], np.float64).reshape(2, 3)


# -- patch comparison (fpm_last_compare / fpm_compare_at / fpm_compare_derive) ---------------------------------------
COMPARE_MAX_AREA = 1 << 22
# one row per hit: fpm_compare_stats, field for field
COMPARE_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.CompareStats._fields_], align=True)
assert COMPARE_DTYPE.itemsize == C.sizeof(L.CompareStats)


def compare_rect(rect, tw: int, th: int) -> Tuple[int, int, int, int]:
    """A comparison rectangle (x, y, w, h) for a ``tw`` x ``th`` template as four ints; None = the whole template.
    Unlike a patch rectangle it must lie inside the template, and hold at most 2^22 pixels (include/fpm.h).  Raises
    ValueError otherwise.  Pure: no device."""
    if rect is None:
        x, y, w, h = 0, 0, int(tw), int(th)
    else:
        try:
            x, y, w, h = (int(v) for v in rect)
        except (TypeError, ValueError):
            raise ValueError(f"expected a rectangle (x, y, w, h), got {rect!r}") from None
        if any(float(v) != i for v, i in zip(rect, (x, y, w, h))):
            raise ValueError(f"rectangle {tuple(rect)!r} must hold whole numbers")
    if x < 0 or y < 0 or w < 1 or h < 1 or x + w > tw or y + h > th:
        raise ValueError(f"rectangle {(x, y, w, h)} must lie inside the {tw} x {th} template")
    if w * h > COMPARE_MAX_AREA:
        raise ValueError(f"rectangle {(x, y, w, h)} holds more than 2^22 pixels")
    return x, y, w, h


def compare_derive(n: int, sum_i: int, sum_ii: int, sum_t: int, sum_tt: int, sum_it: int, normalize: bool = False):
    """fpm_compare_derive: ``(zncc, gain, offset, lut)`` -- what the comparison derives from a hit's integer sums, by the
    engine's own code (f64 in the order include/fpm.h states; ``lut`` the uint8 [256] table).  Host only (no device).
    Raises ValueError for sums that are those of no ``n`` bytes."""
    z, g, o = C.c_double(), C.c_double(), C.c_double()
    lut = np.zeros(256, np.uint8)
    rc = L.load().fpm_compare_derive(int(n), int(sum_i), int(sum_ii), int(sum_t), int(sum_tt), int(sum_it),
                                     1 if normalize else 0, C.byref(z), C.byref(g), C.byref(o), L.u8ptr(lut))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_compare_derive failed with {rc}")
    return z.value, g.value, o.value, lut


class LearnError(ValueError):
    """A device learn (learn_device / learn_at / learn_hit) the library rejected; ``code`` is its FPM_E_* status."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = int(code)


class MaskError(ValueError):
    """A template-mask call (set_mask, clear_mask, mask_enable, mask, mask_count) the library rejected; ``code`` is its
    FPM_E_* status."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = int(code)


def learn_derive(n: int, total: int, total_sq: int):
    """fpm_learn_derive: ``(mean, norm, inv_area, equal1)`` of a template level from its pixel count and the exact sums of
    its pixels and of their squares, by the engine's own code (fpm_learn's f64 expressions in their order).  Host only
    (no device).  Raises ValueError for sums that are those of no ``n`` bytes."""
    mean, norm, inv = C.c_double(), C.c_double(), C.c_double()
    eq = C.c_int32()
    rc = L.load().fpm_learn_derive(int(n), int(total), int(total_sq), C.byref(mean), C.byref(norm), C.byref(inv),
                                   C.byref(eq))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_learn_derive failed with {rc}")
    return mean.value, norm.value, inv.value, bool(eq.value)


# -- variation model (fpm_model_* / fpm_last_inspect / fpm_inspect_at / fpm_model_derive) -----------------------------
# one row per hit: fpm_inspect_stats, field for field
INSPECT_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.InspectStats._fields_], align=True)
assert INSPECT_DTYPE.itemsize == C.sizeof(L.InspectStats)


def model_thresholds(abs_threshold, k) -> Tuple[int, int]:
    """(a, kq) of the library for an absolute threshold 0 .. 255 and a sigma multiple ``k`` (a float, taken to
    sixteenths by round; 0 .. 255 sixteenths).  Raises ValueError outside those ranges.  Pure: no device."""
    a = int(abs_threshold)
    if a != abs_threshold or not 0 <= a <= 255:
        raise ValueError(f"abs_threshold {abs_threshold!r} must be a whole number 0 .. 255")
    kf = float(k)
    if not np.isfinite(kf):
        raise ValueError(f"k {k!r} must be finite")
    kq = int(round(kf * 16.0))
    if not 0 <= kq <= 255:
        raise ValueError(f"k {k!r} is {kq} sixteenths: 0 .. 255 expected")
    return a, kq


def model_derive(n: int, total: int, total_sq: int, abs_threshold: int = 8, k: float = 3.0):
    """fpm_model_derive: ``(mean, lo, hi)`` of one pixel of a variation model from its sample count and the exact sums of
    the samples and of their squares, by the code the device runs (exact integers; ``lo == hi + 1`` is the empty
    interval).  Host only (no device).  Raises ValueError for sums that are those of no ``n`` bytes."""
    a, kq = model_thresholds(abs_threshold, k)
    mean, lo, hi = C.c_int32(), C.c_int32(), C.c_int32()
    if not (-2 ** 31 <= int(n) < 2 ** 31 and -2 ** 63 <= int(total) < 2 ** 63 and -2 ** 63 <= int(total_sq) < 2 ** 63):
        raise ValueError("fpm_model_derive: argument out of range")
    rc = L.load().fpm_model_derive(int(n), int(total), int(total_sq), a, kq, C.byref(mean), C.byref(lo), C.byref(hi))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_model_derive failed with {rc}")
    return mean.value, lo.value, hi.value


# -- defect blobs (fpm_blobs_host) --------------------------------------------------------------------------------------
# one row per component / per hit: fpm_blob and fpm_blob_summary, field for field
BLOB_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.Blob._fields_], align=True)
BLOB_SUMMARY_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.BlobSummary._fields_], align=True)
assert BLOB_DTYPE.itemsize == C.sizeof(L.Blob) == 56 and BLOB_SUMMARY_DTYPE.itemsize == C.sizeof(L.BlobSummary) == 32


def _blob_images(images):
    """(n, h, w) uint8, C-contiguous, from one (h, w) image or a stack of them."""
    a = np.ascontiguousarray(images, np.uint8)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.size == 0:
        raise ValueError("images: a (h, w) or (n, h, w) uint8 array with at least one pixel expected")
    return a


def _blob_buffers(n, h, w, cap, labels):
    if not 1 <= int(cap) <= L.BLOBS_MAX_CAP or n * int(cap) > L.BLOBS_MAX_SLOTS:
        raise ValueError(f"cap {cap!r}: 1 .. 65536 with n x cap <= 2^22 expected")
    summary = np.zeros(n, BLOB_SUMMARY_DTYPE)
    recs = np.zeros((n, int(cap)), BLOB_DTYPE)
    lab = np.zeros((n, h, w), np.int32) if labels else None
    plab = lab.ctypes.data_as(C.POINTER(C.c_int32)) if labels else None
    return summary, recs, lab, plab


def _blob_result(summary, recs, lab, labels):
    blobs = [recs[i, :summary["n_returned"][i]].copy() for i in range(len(summary))]
    return (summary, blobs, lab) if labels else (summary, blobs)


def blobs_host(images, level: int = 0, min_area: int = 4, connectivity: int = 8, cap: int = 64, labels: bool = False):
    """fpm_blobs_host: the connected components of the pixels above ``level`` in each of the uint8 ``images`` ((h, w)
    or (n, h, w)) -- the excess images last_inspect(image=True) returns, for one -- on the host (no device), by the
    contract in include/fpm.h: ``(summary, blobs)`` with ``summary`` a BLOB_SUMMARY_DTYPE array, one row per image,
    and ``blobs`` one BLOB_DTYPE array per image, the components of at least ``min_area`` pixels in ascending seed
    (the smallest row-major index of the component), at most ``cap`` of them (the first by seed).  ``labels=True``: a
    third item, int32 (n, h, w), seed + 1 per foreground pixel and 0 elsewhere."""
    a = _blob_images(images)
    n, h, w = a.shape
    summary, recs, lab, plab = _blob_buffers(n, h, w, cap, labels)
    rc = L.load().fpm_blobs_host(L.u8ptr(a), n, w, h, w, int(level), int(connectivity), int(min_area),
                                 summary.ctypes.data_as(C.POINTER(L.BlobSummary)),
                                 recs.ctypes.data_as(C.POINTER(L.Blob)), int(cap), plab)
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_blobs_host failed with {rc}")
    return _blob_result(summary, recs, lab, labels)


# -- pose alignment (fpm_align_*): least-squares polish of every hit's pose against the template ----------------------
# one row per hit: fpm_align_sums / fpm_align_result, field for field
ALIGN_SUMS_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.AlignSums._fields_], align=True)
ALIGN_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.AlignResult._fields_], align=True)
assert ALIGN_SUMS_DTYPE.itemsize == C.sizeof(L.AlignSums) and ALIGN_DTYPE.itemsize == C.sizeof(L.AlignResult)


def align_rect(rect, tw: int, th: int) -> Tuple[int, int, int, int]:
    """An alignment rectangle (x, y, w, h) for a ``tw`` x ``th`` template as four ints; None = the whole template.  A
    comparison rectangle (inside the template) under two narrower caps: at most 2^20 pixels, sides of at most 4096
    (include/fpm.h: they keep every sum below 2^62).  Raises ValueError otherwise.  Pure: no device."""
    x, y, w, h = compare_rect(rect, tw, th)
    if w > L.ALIGN_MAX_SIDE or h > L.ALIGN_MAX_SIDE:
        raise ValueError(f"rectangle {(x, y, w, h)}: sides of at most {L.ALIGN_MAX_SIDE}")
    if w * h > L.ALIGN_MAX_AREA:
        raise ValueError(f"rectangle {(x, y, w, h)} holds more than 2^20 pixels")
    return x, y, w, h


def align_solve(sums):
    """fpm_align_solve: ``(du, dv, dphi, singular)`` -- the Gauss-Newton step of one record of ALIGN_SUMS_DTYPE (or a
    mapping / sequence of its eleven integers in order), by the engine's own code: du, dv in patch pixels, dphi in
    radians; a singular step is (0, 0, 0, True).  Host only (no device)."""
    names = [f[0] for f in L.AlignSums._fields_]
    if isinstance(sums, dict) or (hasattr(sums, "dtype") and getattr(sums.dtype, "names", None)):
        vals = [int(sums[k]) for k in names]
    else:
        vals = [int(v) for v in sums]
    if len(vals) != len(names) or not all(-2 ** 63 <= v < 2 ** 63 for v in vals):
        raise ValueError("fpm_align_solve: eleven int64 sums expected")
    rec = L.AlignSums(*vals)
    du, dv, dphi = C.c_double(), C.c_double(), C.c_double()
    rc = L.load().fpm_align_solve(C.byref(rec), C.byref(du), C.byref(dv), C.byref(dphi))
    if rc not in (0, 1):
        raise ValueError(f"fpm_align_solve failed with {rc}")
    return du.value, dv.value, dphi.value, bool(rc)


def align_update(src_w: int, src_h: int, rect, lt, angle: float, du: float, dv: float, dphi: float):
    """fpm_align_update: ``((lt_x, lt_y), angle)`` -- the pose after the step (du, dv, dphi) of a pose (ptLT ``lt`` as
    f32, ``angle`` in degrees) on a ``src_w`` x ``src_h`` source for the rectangle ``rect`` (x, y, w, h): the pose whose
    patch map is the current one composed with the rotation by dphi about the rectangle's centre and the shift (du,
    dv).  ``lt`` comes back as float32 values.  Host only (no device)."""
    x, y, w, h = (int(v) for v in rect)
    r = L.PatchRect(x, y, w, h)
    ox, oy, oa = C.c_float(), C.c_float(), C.c_double()
    rc = L.load().fpm_align_update(int(src_w), int(src_h), C.byref(r), float(np.float32(lt[0])), float(np.float32(lt[1])),
                                   float(angle), float(du), float(dv), float(dphi), C.byref(ox), C.byref(oy),
                                   C.byref(oa))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_align_update failed with {rc}")
    return (ox.value, oy.value), oa.value


# -- edge calipers (fpm_caliper_* / fpm_last_calipers / fpm_calipers_at): edges measured across every hit -------------
# fpm_caliper, fpm_edge_raw, fpm_edge and fpm_caliper_summary, field for field
CALIPER_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.Caliper._fields_], align=True)
EDGE_RAW_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.EdgeRaw._fields_], align=True)
EDGE_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.Edge._fields_], align=True)
CALIPER_SUMMARY_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.CaliperSummary._fields_], align=True)
assert CALIPER_DTYPE.itemsize == C.sizeof(L.Caliper) == 48 and EDGE_DTYPE.itemsize == C.sizeof(L.Edge) == 64
assert CALIPER_SUMMARY_DTYPE.itemsize == C.sizeof(L.CaliperSummary) == 32 and EDGE_RAW_DTYPE.itemsize == 16


def caliper(cx: float, cy: float, phi: float, length: int, width: int, half: int = 2, contrast: int = 12,
            polarity: int = 0) -> np.ndarray:
    """One caliper as a CALIPER_DTYPE record: the centre (cx, cy) of its sample grid in template coordinates, the scan
    direction ``phi`` in degrees in the template's frame (0 = along +x), ``length`` samples along the scan and ``width``
    across it, ``half`` samples summed on each side of a boundary, the least step ``contrast`` in gray levels, and
    ``polarity`` +1 (dark to bright along the scan), -1 or 0 (both).  Raises ValueError outside the ranges of
    include/fpm.h.  Pure: no device."""
    vals = [int(v) for v in (length, width, half, contrast, polarity)]
    if vals != [length, width, half, contrast, polarity]:
        raise ValueError("length, width, half, contrast and polarity must be whole numbers")
    length, width, half, contrast, polarity = vals
    if not (np.isfinite(cx) and np.isfinite(cy) and np.isfinite(phi)):
        raise ValueError("cx, cy and phi must be finite")
    if not 2 <= length <= L.CALIPER_MAX_LENGTH or not 1 <= width <= L.CALIPER_MAX_WIDTH:
        raise ValueError(f"length {length} must be 2 .. {L.CALIPER_MAX_LENGTH}, width {width} 1 .. {L.CALIPER_MAX_WIDTH}")
    if not 1 <= half <= L.CALIPER_MAX_HALF or 2 * half > length:
        raise ValueError(f"half {half} must be 1 .. {L.CALIPER_MAX_HALF} with 2 half <= length")
    if not 1 <= contrast <= 255 or polarity not in (-1, 0, 1):
        raise ValueError("contrast must be 1 .. 255 and polarity +1, -1 or 0")
    rec = np.zeros((), CALIPER_DTYPE)
    rec["cx"], rec["cy"], rec["phi"] = float(cx), float(cy), float(phi)
    rec["length"], rec["width"], rec["half"], rec["contrast"], rec["polarity"] = length, width, half, contrast, polarity
    return rec


def _calipers(cals) -> np.ndarray:
    """A contiguous CALIPER_DTYPE array of one or more calipers (records of caliper(), or such an array)."""
    if isinstance(cals, np.ndarray) and cals.dtype == CALIPER_DTYPE:
        arr = np.ascontiguousarray(cals).reshape(-1)
    else:
        arr = np.array([np.asarray(c, CALIPER_DTYPE).reshape(()) for c in cals], CALIPER_DTYPE).reshape(-1)
    if not 1 <= arr.size <= L.CALIPER_MAX_CALS:
        raise ValueError(f"1 .. {L.CALIPER_MAX_CALS} calipers expected, got {arr.size}")
    return arr


def _caliper_ptr(cal):
    arr = _calipers([cal] if not (isinstance(cal, np.ndarray) and cal.ndim >= 1) else cal)
    if arr.size != 1:
        raise ValueError("one caliper expected")
    return arr, arr.ctypes.data_as(C.POINTER(L.Caliper))


def caliper_pose(lt, angle: float, cal):
    """fpm_caliper_pose: ``((lt_x, lt_y), angle)`` -- the pose at which caliper ``cal`` samples on a hit at ptLT ``lt``
    (as f32) and ``angle`` (degrees): its rectangle (0, 0, length, width) at that pose is the caliper's sample grid.
    ``lt`` comes back as float32 values.  Host only (no device)."""
    arr, p = _caliper_ptr(cal)
    ox, oy, oa = C.c_float(), C.c_float(), C.c_double()
    rc = L.load().fpm_caliper_pose(float(np.float32(lt[0])), float(np.float32(lt[1])), float(angle), p, C.byref(ox),
                                   C.byref(oy), C.byref(oa))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_caliper_pose failed with {rc}")
    return (ox.value, oy.value), oa.value


def caliper_edges_host(profile, cal, cap: int = 8):
    """fpm_caliper_edges_host: the step filter and edge rules of include/fpm.h on a profile of ``cal['length']`` integers
    (each 0 .. 255 width): ``(raw, n_edges, flags)`` with ``raw`` an EDGE_RAW_DTYPE array of the first min(n_edges, cap)
    edges in ascending index and ``flags`` L.CALIPER_TRUNCATED when there are more.  Host only (no device)."""
    arr, p = _caliper_ptr(cal)
    prof = np.ascontiguousarray(profile, np.int32).reshape(-1)
    if prof.size != int(arr[0]["length"]) or not np.array_equal(prof, np.asarray(profile).reshape(-1)):
        raise ValueError("profile must hold cal['length'] int32 values")
    if int(cap) != cap or not 1 <= int(cap) <= L.CALIPER_MAX_CAP:
        raise ValueError(f"cap {cap!r} must be a whole number 1 .. {L.CALIPER_MAX_CAP}")
    raw = np.zeros(int(cap), EDGE_RAW_DTYPE)
    n, flags = C.c_int32(), C.c_int32()
    rc = L.load().fpm_caliper_edges_host(prof.ctypes.data_as(C.POINTER(C.c_int32)), p, int(cap),
                                         raw.ctypes.data_as(C.POINTER(L.EdgeRaw)), C.byref(n), C.byref(flags))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_caliper_edges_host failed with {rc}")
    return raw[:min(n.value, int(cap))], n.value, flags.value


def caliper_derive(cal, lt_k, angle_k: float, raw) -> np.ndarray:
    """fpm_caliper_derive: the raw records ``raw`` (EDGE_RAW_DTYPE, or rows of index, d_prev, d, d_next) of caliper
    ``cal`` sampled at the pose (``lt_k`` as f32, ``angle_k``) as an EDGE_DTYPE array: the sub-sample position t, the
    contrast in gray levels, the edge point in template (tx, ty) and source (sx, sy) coordinates.  Host only."""
    arr, p = _caliper_ptr(cal)
    if isinstance(raw, np.ndarray) and raw.dtype == EDGE_RAW_DTYPE:
        r = np.ascontiguousarray(raw).reshape(-1)
    else:
        rows = np.asarray(raw, np.int64).reshape(-1, 4)
        r = np.zeros(len(rows), EDGE_RAW_DTYPE)
        for i, name in enumerate(EDGE_RAW_DTYPE.names):
            r[name] = rows[:, i]
    out = np.zeros(len(r), EDGE_DTYPE)
    rc = L.load().fpm_caliper_derive(p, float(np.float32(lt_k[0])), float(np.float32(lt_k[1])), float(angle_k),
                                     r.ctypes.data_as(C.POINTER(L.EdgeRaw)), len(r),
                                     out.ctypes.data_as(C.POINTER(L.Edge)))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_caliper_derive failed with {rc}")
    return out


# -- edge probes (fpm_probe_* / fpm_last_probes / fpm_probes_at / fpm_fit_*): an outline measured on every hit --------
# fpm_probe, fpm_probe_params, fpm_probe_raw, fpm_probe_result and fpm_probe_summary, field for field
PROBE_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.Probe._fields_], align=True)
PROBE_PARAMS_DTYPE = np.dtype([("length", "<i4"), ("width", "<i4"), ("half", "<i4"), ("contrast", "<i4"),
                               ("polarity", "<i4"), ("select", "<i4"), ("reserved", "<i4", (2,))], align=True)
PROBE_RAW_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.ProbeRaw._fields_], align=True)
PROBE_RESULT_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.ProbeResult._fields_], align=True)
PROBE_SUMMARY_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.ProbeSummary._fields_], align=True)
assert PROBE_DTYPE.itemsize == C.sizeof(L.Probe) == 24 and PROBE_PARAMS_DTYPE.itemsize == C.sizeof(L.ProbeParams) == 32
assert PROBE_RAW_DTYPE.itemsize == C.sizeof(L.ProbeRaw) == 24 and PROBE_RESULT_DTYPE.itemsize == C.sizeof(L.ProbeResult) == 64
assert PROBE_SUMMARY_DTYPE.itemsize == C.sizeof(L.ProbeSummary) == 64
_PROBE_SELECT = {"nearest": L.PROBE_NEAREST, "strongest": L.PROBE_STRONGEST, "first": L.PROBE_FIRST, "last": L.PROBE_LAST}


def probe(x: float, y: float, phi: float) -> np.ndarray:
    """One edge probe as a PROBE_DTYPE record: the nominal edge point (x, y) in template coordinates, which is the
    centre of the probe's sample grid, and the scan direction ``phi`` in degrees in the template's frame (0 = along
    +x).  Raises ValueError for a value that is not finite.  Pure: no device."""
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(phi)):
        raise ValueError("x, y and phi must be finite")
    rec = np.zeros((), PROBE_DTYPE)
    rec["x"], rec["y"], rec["phi"] = float(x), float(y), float(phi)
    return rec


def probe_params(length: int, width: int, half: int = 2, contrast: int = 12, polarity: int = 0,
                 select="nearest") -> np.ndarray:
    """The size and rules all probes of a call share, as a PROBE_PARAMS_DTYPE record: ``length`` 4 .. 64 samples along
    the scan and ``width`` 1 .. 16 across it, ``half`` 1 .. 8 samples summed on each side of a boundary (2 half <=
    length), the least step ``contrast`` 1 .. 255 in gray levels, ``polarity`` +1 (dark to bright along the scan), -1
    or 0 (both), and ``select``: "nearest" (to the nominal point), "strongest", "first" or "last" along the scan, or
    the L.PROBE_* code.  Raises ValueError outside the ranges of include/fpm.h.  Pure: no device."""
    sel = _PROBE_SELECT.get(select, select) if isinstance(select, str) else select
    vals = [int(v) for v in (length, width, half, contrast, polarity)]
    if vals != [length, width, half, contrast, polarity]:
        raise ValueError("length, width, half, contrast and polarity must be whole numbers")
    length, width, half, contrast, polarity = vals
    if not L.PROBE_MIN_LENGTH <= length <= L.PROBE_MAX_LENGTH or not 1 <= width <= L.PROBE_MAX_WIDTH:
        raise ValueError(f"length {length} must be {L.PROBE_MIN_LENGTH} .. {L.PROBE_MAX_LENGTH}, "
                         f"width {width} 1 .. {L.PROBE_MAX_WIDTH}")
    if not 1 <= half <= L.PROBE_MAX_HALF or 2 * half > length:
        raise ValueError(f"half {half} must be 1 .. {L.PROBE_MAX_HALF} with 2 half <= length")
    if not 1 <= contrast <= 255 or polarity not in (-1, 0, 1):
        raise ValueError("contrast must be 1 .. 255 and polarity +1, -1 or 0")
    if sel not in _PROBE_SELECT.values():
        raise ValueError(f"select {select!r} must be one of {sorted(_PROBE_SELECT)}")
    rec = np.zeros((), PROBE_PARAMS_DTYPE)
    rec["length"], rec["width"], rec["half"], rec["contrast"], rec["polarity"] = length, width, half, contrast, polarity
    rec["select"] = int(sel)
    return rec


def _probes(probes, most=L.PROBE_MAX) -> np.ndarray:
    """A contiguous PROBE_DTYPE array of one or more probes (records of probe(), or such an array)."""
    if isinstance(probes, np.ndarray) and probes.dtype == PROBE_DTYPE:
        arr = np.ascontiguousarray(probes).reshape(-1)
    else:
        arr = np.array([np.asarray(p, PROBE_DTYPE).reshape(()) for p in probes], PROBE_DTYPE).reshape(-1)
    if not 1 <= arr.size <= most:
        raise ValueError(f"1 .. {most} probes expected, got {arr.size}")
    return arr


def _probe_params_ptr(params):
    arr = np.ascontiguousarray(np.asarray(params, PROBE_PARAMS_DTYPE)).reshape(-1)
    if arr.size != 1:
        raise ValueError("one probe_params record expected")
    return arr, arr.ctypes.data_as(C.POINTER(L.ProbeParams))


def probe_matrix(src_w: int, src_h: int, lt, angle: float, prb, params) -> np.ndarray:
    """fpm_probe_matrix: the 2x3 matrix that takes sample (u, v) of probe ``prb`` on a hit at ptLT ``lt`` (as f32) and
    ``angle`` (degrees) of a ``src_w`` x ``src_h`` source to source coordinates -- the hit's inverted patch matrix
    composed with the probe's frame in the header's order.  Host only (no device)."""
    arr = _probes([prb] if not (isinstance(prb, np.ndarray) and prb.ndim >= 1) else prb, 1)
    pa, pp = _probe_params_ptr(params)
    n = (C.c_double * 6)()
    rc = L.load().fpm_probe_matrix(int(src_w), int(src_h), float(np.float32(lt[0])), float(np.float32(lt[1])),
                                   float(angle), _ptr(arr, L.Probe), pp, n)
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_probe_matrix failed with {rc}")
    return np.array(n[:], np.float64).reshape(2, 3)


def probe_edges_host(profile, params) -> np.ndarray:
    """fpm_probe_edges_host: the step, edge and select rules of include/fpm.h on a profile of ``params['length']``
    integers (each 0 .. 255 width), as one PROBE_RAW_DTYPE record: index (0: no edge), n_edges (the true count), the
    three steps, flags 0.  Host only (no device)."""
    pa, pp = _probe_params_ptr(params)
    prof = np.ascontiguousarray(profile, np.int32).reshape(-1)
    if prof.size != int(pa[0]["length"]) or not np.array_equal(prof, np.asarray(profile).reshape(-1)):
        raise ValueError("profile must hold params['length'] int32 values")
    raw = np.zeros((), PROBE_RAW_DTYPE)
    rc = L.load().fpm_probe_edges_host(_ptr(prof, C.c_int32), pp, raw.ctypes.data_as(C.POINTER(L.ProbeRaw)))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_probe_edges_host failed with {rc}")
    return raw


def probe_derive(probes, params, lt, angle: float, raw) -> np.ndarray:
    """fpm_probe_derive: raw record i (PROBE_RAW_DTYPE, or rows of index, n_edges, d_prev, d, d_next, flags) of probe i
    on a hit at ptLT ``lt`` (as f32) and ``angle`` as a PROBE_RESULT_DTYPE array: dev (the edge's signed displacement
    from nominal along phi, template pixels), the contrast in gray levels, the edge point in template (tx, ty) and
    source (sx, sy) coordinates.  Host only."""
    arr = _probes(probes)
    pa, pp = _probe_params_ptr(params)
    if isinstance(raw, np.ndarray) and raw.dtype == PROBE_RAW_DTYPE:
        r = np.ascontiguousarray(raw).reshape(-1)
    else:
        rows = np.asarray(raw, np.int64).reshape(-1, 6)
        r = np.zeros(len(rows), PROBE_RAW_DTYPE)
        for i, name in enumerate(PROBE_RAW_DTYPE.names):
            r[name] = rows[:, i]
    if len(r) != len(arr):
        raise ValueError("one raw record per probe expected")
    out = np.zeros(len(r), PROBE_RESULT_DTYPE)
    rc = L.load().fpm_probe_derive(_ptr(arr, L.Probe), pp, float(np.float32(lt[0])), float(np.float32(lt[1])),
                                   float(angle), _ptr(r, L.ProbeRaw), len(r), _ptr(out, L.ProbeResult))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_probe_derive failed with {rc}")
    return out


def _fit(entry, ctype, pts, trim, what):
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
    out = ctype()
    rc = entry(_ptr(p, C.c_double), len(p), float(trim), C.byref(out))
    if rc != L.FPM_OK:
        raise ValueError(f"{what} failed with {rc}")
    return {name: getattr(out, name) for name, _ in ctype._fields_}


def fit_line(pts, trim: float = 0.0) -> dict:
    """fpm_fit_line: the total-least-squares line through the (n, 2) points ``pts`` -- (sx, sy) or (tx, ty) of found
    probes -- as a dict: angle (the direction in degrees, in (-90, 90]), px, py (the point of the line nearest the
    origin), rms and max_resid of the point distances, n_used, flags.  ``trim`` > 0 drops the points farther than
    that from the first fit and fits the rest once more.  ValueError below 2 points or for non-finite input."""
    return _fit(L.load().fpm_fit_line, L.LineFit, pts, trim, "fpm_fit_line")


def fit_circle(pts, trim: float = 0.0) -> dict:
    """fpm_fit_circle: the circle through the (n, 2) points ``pts`` -- Kasa's algebraic fit, then at most 8
    Gauss-Newton steps on the geometric residual -- as a dict: cx, cy, r, rms and max_resid of the radial residuals,
    n_used, flags (L.FIT_COLLINEAR: no circle, the numbers are 0; L.FIT_NOT_CONVERGED).  ``trim`` as fit_line.
    ValueError below 3 points or for non-finite input."""
    return _fit(L.load().fpm_fit_circle, L.CircleFit, pts, trim, "fpm_fit_circle")


def circle_probes(cx: float, cy: float, r: float, n: int, outward: bool = True) -> np.ndarray:
    """``n`` radial probes on the circle of centre (cx, cy) and radius ``r`` in template coordinates, evenly spaced
    from 0 degrees on: probe k sits at the angle 360 k / n and scans outward (phi = that angle) or inward (phi + 180).
    A PROBE_DTYPE array.  Pure numpy."""
    if int(n) != n or n < 1 or not r > 0:
        raise ValueError("n must be a whole number >= 1 and r > 0")
    a = 360.0 * np.arange(int(n), dtype=np.float64) / int(n)
    out = np.zeros(int(n), PROBE_DTYPE)
    out["x"] = cx + r * np.cos(np.deg2rad(a))
    out["y"] = cy + r * np.sin(np.deg2rad(a))
    out["phi"] = a if outward else a + 180.0
    return out


def line_probes(p0, p1, n: int, normal_side: int = +1) -> np.ndarray:
    """``n`` probes along the segment ``p0`` -> ``p1`` (template coordinates), at the fractions (k + 0.5) / n, each
    scanning across it: phi = the segment's direction + 90 degrees for ``normal_side`` +1, - 90 for -1.  A PROBE_DTYPE
    array.  Pure numpy."""
    if int(n) != n or n < 1 or normal_side not in (-1, 1):
        raise ValueError("n must be a whole number >= 1 and normal_side +1 or -1")
    (x0, y0), (x1, y1) = (float(p0[0]), float(p0[1])), (float(p1[0]), float(p1[1]))
    if x0 == x1 and y0 == y1:
        raise ValueError("p0 and p1 must differ")
    f = (np.arange(int(n), dtype=np.float64) + 0.5) / int(n)
    out = np.zeros(int(n), PROBE_DTYPE)
    out["x"] = x0 + f * (x1 - x0)
    out["y"] = y0 + f * (y1 - y0)
    out["phi"] = float(np.rad2deg(np.arctan2(y1 - y0, x1 - x0))) + 90.0 * normal_side
    return out


def contour_probes(template, step: float, min_contrast: float, mask=None) -> np.ndarray:
    """Probes along the edges of the taught image ``template`` (2-D uint8), a PROBE_DTYPE array in row-major order of
    the kept pixels.  The gradient is the 3 x 3 Sobel (gx, gy) / 8, in gray levels per pixel, on the interior pixels; a
    pixel is an edge point when its gradient magnitude is at least ``min_contrast`` and a local maximum along the
    gradient: not below the magnitude at the neighbour the gradient points to (its direction rounded to the nearest of
    the 8), and above that of the opposite neighbour.  Edge points are thinned greedily in row-major order: one is
    kept when it is at least ``step`` pixels from every point kept before.  phi = atan2(gy, gx) in degrees, the
    direction from dark to bright.  ``mask`` (same shape, non-zero = use) only skips pixels while teaching.
    Deterministic; pure numpy."""
    t = np.asarray(template)
    if t.ndim != 2 or t.dtype != np.uint8 or min(t.shape) < 3:
        raise ValueError("template must be a 2-D uint8 image of at least 3 x 3")
    if not step > 0 or not min_contrast > 0:
        raise ValueError("step and min_contrast must be positive")
    f = t.astype(np.int32)
    h, w = f.shape
    gx = np.zeros((h, w), np.int32)
    gy = np.zeros((h, w), np.int32)
    gx[1:-1, 1:-1] = (f[:-2, 2:] + 2 * f[1:-1, 2:] + f[2:, 2:]) - (f[:-2, :-2] + 2 * f[1:-1, :-2] + f[2:, :-2])
    gy[1:-1, 1:-1] = (f[2:, :-2] + 2 * f[2:, 1:-1] + f[2:, 2:]) - (f[:-2, :-2] + 2 * f[:-2, 1:-1] + f[:-2, 2:])
    mag2 = gx.astype(np.int64) ** 2 + gy.astype(np.int64) ** 2          # (8 |g|)^2, exact
    ok = mag2 >= (8.0 * float(min_contrast)) ** 2
    ok[0, :] = ok[-1, :] = ok[:, 0] = ok[:, -1] = False
    if mask is not None:
        mk = np.asarray(mask)
        if mk.shape != t.shape:
            raise ValueError("mask must have the template's shape")
        ok &= mk != 0
    ys, xs = np.nonzero(ok)
    ang = np.arctan2(gy[ys, xs], gx[ys, xs])
    k = np.rint(ang / (np.pi / 4)).astype(np.int64) % 8
    dxs = np.array([1, 1, 0, -1, -1, -1, 0, 1])[k]
    dys = np.array([0, 1, 1, 1, 0, -1, -1, -1])[k]
    m = mag2[ys, xs]
    peak = (m >= mag2[ys + dys, xs + dxs]) & (m > mag2[ys - dys, xs - dxs])
    ys, xs = ys[peak], xs[peak]
    kept_x, kept_y = [], []
    s2 = float(step) ** 2
    cell = max(int(np.ceil(step)), 1)
    grid = {}
    for y, x in zip(ys.tolist(), xs.tolist()):                          # nonzero's order is row-major
        cy, cx = y // cell, x // cell
        near = False
        for gy_ in (cy - 1, cy, cy + 1):
            for gx_ in (cx - 1, cx, cx + 1):
                for (py, px) in grid.get((gy_, gx_), ()):
                    if (py - y) ** 2 + (px - x) ** 2 < s2:
                        near = True
        if not near:
            grid.setdefault((cy, cx), []).append((y, x))
            kept_x.append(x)
            kept_y.append(y)
    out = np.zeros(len(kept_x), PROBE_DTYPE)
    if kept_x:
        ky, kx = np.array(kept_y), np.array(kept_x)
        out["x"], out["y"] = kx, ky
        out["phi"] = np.rad2deg(np.arctan2(gy[ky, kx].astype(np.float64), gx[ky, kx].astype(np.float64)))
    return out


# -- sub-pattern locators (fpm_locate_host / fpm_locate_derive / fpm_last_locate / fpm_locate_at) ---------------------
# fpm_feature, fpm_locate_raw and fpm_locate_result, field for field
FEATURE_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.Feature._fields_], align=True)
LOCATE_RAW_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.LocateRaw._fields_], align=True)
LOCATE_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.LocateResult._fields_], align=True)
assert FEATURE_DTYPE.itemsize == C.sizeof(L.Feature) == 32 and LOCATE_RAW_DTYPE.itemsize == C.sizeof(L.LocateRaw) == 160
assert LOCATE_DTYPE.itemsize == C.sizeof(L.LocateResult) == 80


def feature(x: int, y: int, w: int, h: int, rx: int = 8, ry: Optional[int] = None) -> np.ndarray:
    """One feature as a FEATURE_DTYPE record: the region (x, y, w, h) of the template to find again on a hit, w and h
    1 .. 128, and the search radii rx, ry (``ry=None``: rx) in pixels, 0 .. 16.  Whether the region lies inside the
    learned template is checked by the call that uses it.  Raises ValueError outside the ranges.  Pure: no device."""
    ry = rx if ry is None else ry
    vals = [int(v) for v in (x, y, w, h, rx, ry)]
    if vals != [x, y, w, h, rx, ry]:
        raise ValueError("x, y, w, h, rx and ry must be whole numbers")
    x, y, w, h, rx, ry = vals
    if not (1 <= w <= L.LOCATE_MAX_SIDE and 1 <= h <= L.LOCATE_MAX_SIDE):
        raise ValueError(f"w {w} and h {h} must be 1 .. {L.LOCATE_MAX_SIDE}")
    if not (0 <= rx <= L.LOCATE_MAX_RADIUS and 0 <= ry <= L.LOCATE_MAX_RADIUS):
        raise ValueError(f"rx {rx} and ry {ry} must be 0 .. {L.LOCATE_MAX_RADIUS}")
    if x < 0 or y < 0 or abs(x) > 1 << 20 or abs(y) > 1 << 20:
        raise ValueError("x and y must not be negative")
    rec = np.zeros((), FEATURE_DTYPE)
    rec["x"], rec["y"], rec["w"], rec["h"], rec["rx"], rec["ry"] = x, y, w, h, rx, ry
    return rec


def _features(feats) -> np.ndarray:
    """A contiguous FEATURE_DTYPE array of one or more features (records of feature(), or such an array)."""
    if isinstance(feats, np.ndarray) and feats.dtype == FEATURE_DTYPE:
        arr = np.ascontiguousarray(feats).reshape(-1)
    else:
        arr = np.array([np.asarray(f, FEATURE_DTYPE).reshape(()) for f in feats], FEATURE_DTYPE).reshape(-1)
    if not 1 <= arr.size <= L.LOCATE_MAX_FEATURES:
        raise ValueError(f"1 .. {L.LOCATE_MAX_FEATURES} features expected, got {arr.size}")
    return arr


def locate_host(window, tmpl, rx: int, ry: int, maps: bool = False):
    """fpm_locate_host: the template region ``tmpl`` (uint8, h x w) searched in ``window`` (uint8, (h + 2 ry) x (w + 2
    rx)) by the rules of include/fpm.h.  Returns the LOCATE_RAW_DTYPE record; with ``maps=True`` also the int32 sums
    (3, 2 ry + 1, 2 rx + 1): S_i, S_ii, S_it per offset.  Host only (no device)."""
    t = np.ascontiguousarray(tmpl, np.uint8)
    win = np.ascontiguousarray(window, np.uint8)
    if t.ndim != 2 or win.ndim != 2 or int(rx) != rx or int(ry) != ry:
        raise ValueError("two uint8 images and whole radii expected")
    h, w = t.shape
    rx, ry = int(rx), int(ry)
    if win.shape != (h + 2 * ry, w + 2 * rx):
        raise ValueError(f"window {win.shape} must be {(h + 2 * ry, w + 2 * rx)}")
    raw = np.zeros(1, LOCATE_RAW_DTYPE)
    m = np.zeros((3, 2 * max(ry, 0) + 1, 2 * max(rx, 0) + 1), np.int32) if maps else None
    rc = L.load().fpm_locate_host(win.ctypes.data_as(C.POINTER(C.c_uint8)), win.strides[0],
                                  t.ctypes.data_as(C.POINTER(C.c_uint8)), t.strides[0], w, h, rx, ry,
                                  raw.ctypes.data_as(C.POINTER(L.LocateRaw)),
                                  m.ctypes.data_as(C.POINTER(C.c_int32)) if maps else None)
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_locate_host failed with {rc}")
    return (raw[0], m) if maps else raw[0]


def locate_derive(feat, lt, angle: float, raw) -> np.ndarray:
    """fpm_locate_derive: one raw record ``raw`` (LOCATE_RAW_DTYPE) of feature ``feat`` on a hit at ptLT ``lt`` (as
    f32) and ``angle`` (degrees) as a LOCATE_DTYPE record: score, score_nominal, the sub-pixel displacement (ox, oy),
    the found centre in template (tx, ty) and source (sx, sy) coordinates, and flags.  Host only (no device)."""
    f = _features([feat] if not (isinstance(feat, np.ndarray) and feat.ndim >= 1) else feat)
    r = np.ascontiguousarray(raw, LOCATE_RAW_DTYPE).reshape(-1)
    if f.size != 1 or r.size != 1:
        raise ValueError("one feature and one raw record expected")
    out = np.zeros(1, LOCATE_DTYPE)
    rc = L.load().fpm_locate_derive(f.ctypes.data_as(C.POINTER(L.Feature)), float(np.float32(lt[0])),
                                    float(np.float32(lt[1])), float(angle), r.ctypes.data_as(C.POINTER(L.LocateRaw)),
                                    out.ctypes.data_as(C.POINTER(L.LocateResult)))
    if rc != L.FPM_OK:
        raise ValueError(f"fpm_locate_derive failed with {rc}")
    return out[0]


# -- gray-value tools (fpm_hist_derive / fpm_last_histogram / fpm_last_segment ..): the hit's own gray values ---------
# fpm_hist_stats and fpm_segment_info, field for field
HIST_STATS_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.HistStats._fields_], align=True)
SEGMENT_INFO_DTYPE = np.dtype([(name, np.dtype(ct)) for name, ct in L.SegmentInfo._fields_], align=True)
assert HIST_STATS_DTYPE.itemsize == C.sizeof(L.HistStats) == 64
assert SEGMENT_INFO_DTYPE.itemsize == C.sizeof(L.SegmentInfo) == 16


def hist_derive(hist) -> np.ndarray:
    """fpm_hist_derive: the statistics of 256-bin histograms (uint32, shape (256,) or (..., 256), as last_histogram
    returns them) as a HIST_STATS_DTYPE array of shape ``hist.shape[:-1]``: n, sum, sum_sq, min, max, median, mean,
    stddev, Otsu's threshold (class 0 is I <= otsu) and flags (L.HIST_EMPTY: no pixel, every field 0; L.HIST_FLAT: one
    occupied bin, otsu = min).  Raises ValueError for a histogram of more than 2^22 pixels.  Host only (no device)."""
    h = np.ascontiguousarray(hist, np.uint32)
    if h.ndim < 1 or h.shape[-1] != 256 or not np.array_equal(h, np.asarray(hist)):
        raise ValueError("hist: uint32 values, 256 in the last dimension, expected")
    flat = h.reshape(-1, 256)
    out = np.zeros(len(flat), HIST_STATS_DTYPE)
    lib = L.load()
    for i in range(len(flat)):
        rc = lib.fpm_hist_derive(flat[i].ctypes.data_as(C.POINTER(C.c_uint32)),
                                 out[i:i + 1].ctypes.data_as(C.POINTER(L.HistStats)))
        if rc != L.FPM_OK:
            raise ValueError(f"fpm_hist_derive failed with {rc}")
    return out.reshape(h.shape[:-1])


def _segment_threshold(threshold) -> int:
    if isinstance(threshold, str):
        if threshold != "otsu":
            raise ValueError(f"threshold {threshold!r}: 0 .. 255 or 'otsu' expected")
        return L.SEG_OTSU
    if int(threshold) != threshold or not 0 <= int(threshold) <= 255:
        raise ValueError(f"threshold {threshold!r}: 0 .. 255 or 'otsu' expected")
    return int(threshold)


class TemplateMatcher:
    """Drop-in for the reference TemplateMatcher, one context (one HIP stream) per instance."""

    def __init__(self, device: int = 0):
        self._lib = L.load()
        self._ctx = C.c_void_p()
        rc = self._lib.fpm_create(device, C.byref(self._ctx))
        if rc != L.FPM_OK:
            raise RuntimeError(f"fpm_create(device={device}) failed with {rc}: no gfx950 device / HIP runtime")
        self._device = int(device)
        self._params = L.Params()
        self._lib.fpm_params_default(C.byref(self._params))
        self._last_time = 0.0
        self._user_rect = None
        self._cap = 64                 # results per source; grown on FPM_E_CAPACITY
        self._staged = 0               # sources of the last stage() (0 after a plain match())
        self._bufs = None              # reusable ctypes result buffers for match_staged
        # FPM_PATCH_TILED=0: the match patches through k_warp instead of k_patch_warp (same bytes; the comparison and
        # the fallback).  Read once, here; setPatchForm changes it afterwards.
        env = os.environ.get("FPM_PATCH_TILED")
        if env is not None and env.strip() != "":
            self.setPatchForm(L.PATCH_FORM_WARP if int(env) == 0 else L.PATCH_FORM_TILED)

    def __del__(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is not None and ctx.value:
            self._lib.fpm_destroy(ctx)
            self._ctx = None

    # -- error plumbing ---------------------------------------------------------------------------------
    def last_error(self) -> str:
        s = self._lib.fpm_last_error(self._ctx)
        return s.decode() if s else ""

    def _check(self, rc: int, what: str):
        if rc == L.FPM_E_DEVICE or rc == L.FPM_E_INTERNAL:
            raise RuntimeError(f"{what}: device error {rc}: {self.last_error()}")
        return rc

    def _push(self):
        self._lib.fpm_set_params(self._ctx, C.byref(self._params))

    # -- template -----------------------------------------------------------------------------------------
    def learnPattern(self, templateImage) -> bool:
        a = np.asarray(templateImage)
        if a.size == 0:
            return False
        g = _gray(a)
        self._push()
        rc = self._check(self._lib.fpm_learn(self._ctx, L.u8ptr(g), g.shape[1], g.shape[0], g.strides[0]),
                         "learnPattern")
        return rc == L.FPM_OK

    def isPatternLearned(self) -> bool:
        return bool(self._lib.fpm_is_learned(self._ctx))

    def clearPattern(self):
        self._lib.fpm_clear_pattern(self._ctx)

    # -- learning on the device (fpm_learn_device / fpm_learn_at / fpm_learn_hit) -------------------------------------
    def _learn_done(self, rc, what):
        self._check(rc, what)
        if rc != L.FPM_OK:
            raise LearnError(rc, f"{what} failed with {rc}: {self.last_error()}")

    def learn_device(self, img, channel_order: str = "bgr", layout=None, stream=None):
        """learnPattern on an image already in device memory (fpm_learn_device): a uint8 torch tensor as match_device
        takes it (gray, interleaved or planar, contiguous or a view), converted as match_device converts a frame.  Nothing
        crosses the host but the level statistics' sums and the top level's pixels; the learned template equals
        learnPattern's for the same gray pixels in every byte and every double.  setBitwiseNot is not looked at.  Staged
        sources survive when the new template has the top layer they were staged for (see learn_at).  Raises LearnError
        (a ValueError with the status in ``code``) when the call is rejected."""
        ptr, h, w, row, plane, fmt = self._device_image(img, channel_order, layout)
        prod = self._producer_stream(stream)
        self._push()
        rc = self._lib.fpm_learn_device(self._ctx, ptr, w, h, row, plane, fmt, prod)
        self._learn_done(rc, "learn_device")

    def learn_at(self, source: int, lt, angle: float, rect=None):
        """learnPattern on the patch patches_at gives for (``source``, ``lt``, ``angle``, ``rect``), sampled on the device
        straight into the template (fpm_learn_at): teach from a region of a staged frame.  ``rect`` None = the
        user-defined rectangle when one is set, else the frame of the template learned now.  Needs staged sources (stage
        / stage_device, or the source of the last match).  They stay staged when the new template's top layer equals the
        one they were staged for: match_staged, patches_at and compare_at then work without restaging; otherwise stage
        again, as after learnPattern.  The poses of the last search are dropped either way."""
        r = self._patch_rect(rect)
        self._push()
        rc = self._lib.fpm_learn_at(self._ctx, C.byref(r) if r is not None else None, int(source),
                                    float(np.float32(lt[0])), float(np.float32(lt[1])), float(angle))
        self._learn_done(rc, "learn_at")

    def learn_hit(self, index: int, source: int = 0, rect=None):
        """learn_at at the raw pose of result ``index`` of ``source`` of the last search, the pose last_patches uses
        (fpm_learn_hit): re-teach on what the matcher just found.  Needs a finished search on the staged sources."""
        r = self._patch_rect(rect)
        self._push()
        rc = self._lib.fpm_learn_hit(self._ctx, C.byref(r) if r is not None else None, int(source), int(index))
        self._learn_done(rc, "learn_hit")

    def template_operands(self):
        """(t8 int8 [bytes], tsum int32 [rows]): the matrix-core operand slab (T ^ 0x80 per level, zero padded, slack
        included) and the per-row sums as they lie in device memory (fpm_template_operands); for parity tests."""
        nb, ns = C.c_size_t(), C.c_size_t()
        rc = self._check(self._lib.fpm_template_operands(self._ctx, None, C.byref(nb), None, C.byref(ns)),
                         "template_operands")
        if rc != L.FPM_OK:
            raise ValueError("template not learned")
        t8 = np.zeros(nb.value, np.int8)
        ts = np.zeros(ns.value, np.int32)
        rc = self._check(self._lib.fpm_template_operands(self._ctx, t8.ctypes.data_as(C.POINTER(C.c_int8)), C.byref(nb),
                                                         ts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ns)),
                         "template_operands")
        if rc != L.FPM_OK:
            raise ValueError(f"fpm_template_operands failed with {rc}")
        return t8, ts

    # -- search ---------------------------------------------------------------------------------------------
    def match(self, sourceImage) -> List[SingleTargetMatch]:
        a = np.asarray(sourceImage)
        self._staged = 0   # fpm_match replaces a staged batch (fpm_match_staged_launch then fails loudly)
        if a.size == 0 or not self.isPatternLearned():
            # an argument-less fpm_match fails its checks and drops the previous search's candidate records
            self._lib.fpm_match(self._ctx, None, 0, 0, 0, None, 0, C.byref(C.c_int32()), None)
            return []
        g = _gray(a)
        self._push()
        out = (L.Result * self._cap)()
        n = C.c_int32()
        sec = C.c_double(self._last_time)
        rc = self._check(self._lib.fpm_match(self._ctx, L.u8ptr(g), g.shape[1], g.shape[0], g.strides[0], out,
                                             self._cap, C.byref(n), C.byref(sec)), "match")
        if rc == L.FPM_E_CAPACITY:   # fetch the results already computed into a larger buffer (no second search)
            self._cap = max(self._cap * 2, n.value)
            out = (L.Result * self._cap)()
            rc = self._check(self._lib.fpm_last_results(self._ctx, out, self._cap, C.byref(n)), "last_results")
        if rc != L.FPM_OK:
            return []
        self._last_time = sec.value
        return [SingleTargetMatch.from_c(out[i]) for i in range(n.value)]

    def match_batch(self, sources: Sequence[np.ndarray]) -> List[List[SingleTargetMatch]]:
        """Extension: all sources (same size) searched in one device pass (fpm_stage_sources + fpm_match_staged)."""
        self.stage(sources)
        return self.match_staged()

    def stage(self, sources: Sequence[np.ndarray]):
        gs = [_gray(s) for s in sources]
        h, w = gs[0].shape
        if any(g.shape != (h, w) for g in gs):
            raise ValueError("all staged sources must have the same size")
        self._push()
        ptrs = (L._U8P * len(gs))(*[L.u8ptr(g) for g in gs])
        rc = self._check(self._lib.fpm_stage_sources(self._ctx, ptrs, len(gs), w, h, gs[0].strides[0]), "stage")
        if rc != L.FPM_OK:
            raise ValueError(f"fpm_stage_sources failed with {rc}: {self.last_error()}")
        self._staged = len(gs)

    # -- sources already in device memory (fpm_match_device / fpm_stage_sources_device) ----------------------------
    def _device_image(self, img, channel_order, layout):
        """(data pointer, height, width, row stride, plane stride, FPM_FMT_*) of a uint8 torch tensor on this
        context's device, as it lies in memory: no copy is made, a layout the kernel cannot read raises instead."""
        import torch   # only the device-memory entries need torch

        if not isinstance(img, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor on cuda:{self._device}, got {type(img).__name__}")
        if img.dtype != torch.uint8:
            raise TypeError(f"expected a uint8 tensor, got {img.dtype}")
        if img.device.type != "cuda":
            raise ValueError(f"expected a tensor on cuda:{self._device}, got one on {img.device} (match() takes host images)")
        if img.device.index != self._device:
            raise ValueError(f"tensor on {img.device}, context on cuda:{self._device}")
        self._check_one_runtime()
        kind, h, w, ch, row, plane = device_layout(tuple(img.shape), tuple(img.stride()), layout)
        return img.data_ptr(), h, w, row, plane, device_format(kind, ch, channel_order)

    @staticmethod
    def _check_one_runtime():
        global _one_runtime
        if not _one_runtime:
            rts = L.hip_runtimes()
            if len(rts) > 1:
                raise RuntimeError("torch and libfpm_hip.so run on separate HIP runtimes (" + ", ".join(rts) + "), so "
                                   "the tensor's pointer and stream are foreign to the library: import torch before "
                                   "the first TemplateMatcher is created (before libfpm_hip.so is loaded)")
            _one_runtime = True

    def _producer_stream(self, stream):
        import torch

        if stream is None:
            return torch.cuda.current_stream(torch.device("cuda", self._device)).cuda_stream
        return int(getattr(stream, "cuda_stream", stream))

    def match_device(self, img, channel_order: str = "bgr", layout=None, stream=None) -> List[SingleTargetMatch]:
        """match() on a frame already in device memory: a uint8 torch tensor on this context's device, gray (H, W),
        interleaved (H, W, 3 or 4) or planar (3, H, W), contiguous or a view (device_layout has the rules; nothing is
        copied or made contiguous).  Colour is converted as the reference's load path converts it
        (cv::imread(IMREAD_GRAYSCALE), images.bgr_to_gray); channel_order names the order of the channels in memory.
        stream is the stream the frame was written on (a torch stream or a raw handle; None = torch's current stream
        of the device): the search is ordered after it, no host synchronisation is needed."""
        ptr, h, w, row, plane, fmt = self._device_image(img, channel_order, layout)
        prod = self._producer_stream(stream)
        self._staged = 0
        if not self.isPatternLearned():
            # as match(): an argument-less fpm_match fails its checks and drops the previous search's records
            self._lib.fpm_match(self._ctx, None, 0, 0, 0, None, 0, C.byref(C.c_int32()), None)
            return []
        self._push()
        out = (L.Result * self._cap)()
        n = C.c_int32()
        sec = C.c_double(self._last_time)
        rc = self._check(self._lib.fpm_match_device(self._ctx, ptr, w, h, row, plane, fmt, prod, out, self._cap,
                                                    C.byref(n), C.byref(sec)), "match_device")
        if rc == L.FPM_E_CAPACITY:   # fetch the results already computed into a larger buffer (no second search)
            self._cap = max(self._cap * 2, n.value)
            out = (L.Result * self._cap)()
            rc = self._check(self._lib.fpm_last_results(self._ctx, out, self._cap, C.byref(n)), "last_results")
        if rc != L.FPM_OK:
            return []
        self._last_time = sec.value
        return [SingleTargetMatch.from_c(out[i]) for i in range(n.value)]

    def stage_device(self, imgs, channel_order: str = "bgr", layout=None, stream=None):
        """stage() for frames already in device memory (fpm_stage_sources_device): tensors as match_device takes them,
        all of one size, format and strides (separate allocations and views are fine).  match_staged* then work as
        after stage()."""
        descs = [self._device_image(t, channel_order, layout) for t in imgs]
        if not descs:
            raise ValueError("no sources")
        if any(d[1:] != descs[0][1:] for d in descs):
            raise ValueError("all staged sources must have the same size, format and strides")
        _, h, w, row, plane, fmt = descs[0]
        prod = self._producer_stream(stream)
        self._push()
        ptrs = (C.c_void_p * len(descs))(*[d[0] for d in descs])
        rc = self._check(self._lib.fpm_stage_sources_device(self._ctx, ptrs, len(descs), w, h, row, plane, fmt, prod),
                         "stage_device")
        if rc != L.FPM_OK:
            raise ValueError(f"fpm_stage_sources_device failed with {rc}: {self.last_error()}")
        self._staged = len(descs)

    def match_staged(self) -> List[List[SingleTargetMatch]]:
        counts, res = self.match_staged_array()
        return [[SingleTargetMatch.from_row(res[s, i]) for i in range(counts[s])] for s in range(len(counts))]

    def _views(self, n_src):
        if self._bufs is None or self._bufs[0] != (n_src, self._cap):
            out = (L.Result * (self._cap * n_src))()
            n = (C.c_int32 * n_src)()
            views = (np.frombuffer(n, dtype=np.int32), np.frombuffer(out, dtype=np.float64).reshape(n_src, self._cap, 12))
            self._bufs = ((n_src, self._cap), out, n, views)
        return self._bufs

    def match_staged_array(self):
        """Like match_staged, returning (counts[int32, n_src], results[f64, n_src, cap, 12]) views of reused buffers
        (fields in s_SingleTargetMatch order) instead of Python objects; valid until the next call."""
        self.match_staged_launch()
        return self.match_staged_finish_array()

    def match_staged_launch(self):
        """Enqueue the device pass over the staged sources and return (fpm_match_staged_launch)."""
        self._push()
        rc = self._check(self._lib.fpm_match_staged_launch(self._ctx), "match_staged_launch")
        if rc != L.FPM_OK:
            raise RuntimeError(f"fpm_match_staged_launch failed with {rc}: {self.last_error()}")

    def match_staged_finish_array(self):
        """Wait for the launched pass and post-process it (fpm_match_staged_finish); array views as
        match_staged_array.  On a full result buffer the results already computed are fetched into a larger one
        (fpm_last_results), without searching again."""
        n_src = self._staged
        _, out, n, views = self._views(n_src)
        rc = self._check(self._lib.fpm_match_staged_finish(self._ctx, out, self._cap, n), "match_staged_finish")
        if rc == L.FPM_E_CAPACITY:
            self._cap = max(self._cap * 2, max(n))
            _, out, n, views = self._views(n_src)
            rc = self._check(self._lib.fpm_last_results(self._ctx, out, self._cap, n), "last_results")
        if rc != L.FPM_OK:
            raise RuntimeError(f"fpm_match_staged_finish failed with {rc}: {self.last_error()}")
        return views

    # -- angle sharding of one search (fpm_set_angle_shard / fpm_last_candidates; sharding.match_angle_sharded) ----
    def setAngleShard(self, shard: int, shards: int):
        """Restrict searches to shard `shard` of `shards` contiguous blocks of the top-layer angle list."""
        rc = self._lib.fpm_set_angle_shard(self._ctx, int(shard), int(shards))
        if rc != L.FPM_OK:
            raise ValueError(f"fpm_set_angle_shard({shard}, {shards}) failed with {rc}: {self.last_error()}")

    def getAngleShard(self) -> Tuple[int, int]:
        a, b = C.c_int32(), C.c_int32()
        self._lib.fpm_get_angle_shard(self._ctx, C.byref(a), C.byref(b))
        return a.value, b.value

    def match_staged_candidates(self) -> List[np.ndarray]:
        """Search the staged sources and return each source's candidate records, skipping the host tail
        (fpm_match_staged_finish with out = NULL): the per-rank step of an angle-sharded search."""
        self.match_staged_launch()
        return self.match_staged_candidates_finish()

    def match_staged_candidates_finish(self) -> List[np.ndarray]:
        """Wait for a pass enqueued by match_staged_launch and return each source's candidate records (the second
        half of match_staged_candidates: a stream of passes over two contexts overlaps one's device pass with the
        other's record exchange and merge)."""
        n = (C.c_int32 * self._staged)()
        rc = self._check(self._lib.fpm_match_staged_finish(self._ctx, None, 0, n), "match_staged_finish")
        if rc != L.FPM_OK:
            raise RuntimeError(f"fpm_match_staged_finish failed with {rc}: {self.last_error()}")
        return [self.last_candidates(s) for s in range(self._staged)]

    def last_candidates_if_searched(self, source: int = 0):
        """last_candidates(source), or None when the last call ran no search for it (fpm_match returned before the
        device pass: empty source, unlearned template, size mismatch)."""
        n = C.c_int32()
        rc = self._lib.fpm_last_candidates(self._ctx, int(source), None, 0, C.byref(n))
        if rc not in (L.FPM_OK, L.FPM_E_CAPACITY):
            return None
        return self.last_candidates(source)

    def last_candidates(self, source: int = 0) -> np.ndarray:
        """Candidate records (CANDIDATE_DTYPE, push order) of `source` in the last search."""
        n = C.c_int32()
        rc = self._lib.fpm_last_candidates(self._ctx, int(source), None, 0, C.byref(n))
        if rc not in (L.FPM_OK, L.FPM_E_CAPACITY):
            raise ValueError(f"fpm_last_candidates({source}) failed with {rc}")
        out = np.zeros(n.value, CANDIDATE_DTYPE)
        if n.value:
            self._lib.fpm_last_candidates(self._ctx, int(source), out.ctypes.data_as(C.POINTER(L.Candidate)),
                                          n.value, C.byref(n))
        return out

    def search_bytes(self) -> Tuple[int, int, int]:
        """(B_pyr, B_top, B_ref): SURVEY.md §8(d) algorithmic bytes of the last search (fpm_search_bytes)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._lib.fpm_search_bytes(self._ctx, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def search_stats(self) -> List[int]:
        buf = (C.c_int64 * 64)()
        k = self._lib.fpm_search_stats(self._ctx, buf, 64)
        return list(buf[:k])

    # -- setters / getters (TemplateMatcher.h:22-37) --------------------------------------------------------
    def resetParams(self):
        """Back to the reference constructor defaults (TemplateMatcher.cpp:28-39)."""
        self._lib.fpm_params_default(C.byref(self._params))

    def setMaxPositions(self, v: int): self._params.max_pos = int(v)
    def setMaxOverlap(self, v: float): self._params.max_overlap = float(v)
    def setScore(self, v: float): self._params.score = float(v)
    def setToleranceAngle(self, v: float): self._params.tolerance_angle = float(v)
    def setMinReduceArea(self, v: int): self._params.min_reduce_area = int(v)
    def setUseSIMD(self, v: bool): self._params.use_simd = 1 if v else 0
    def setSubPixelEstimation(self, v: bool): self._params.subpixel = 1 if v else 0
    def getMaxPositions(self) -> int: return self._params.max_pos
    def getMaxOverlap(self) -> float: return self._params.max_overlap
    def getScore(self) -> float: return self._params.score
    def getToleranceAngle(self) -> float: return self._params.tolerance_angle
    def getMinReduceArea(self) -> int: return self._params.min_reduce_area
    def getUseSIMD(self) -> bool: return bool(self._params.use_simd)
    def getSubPixelEstimation(self) -> bool: return bool(self._params.subpixel)
    def getLastExecutionTime(self) -> float: return self._last_time

    # -- the MFC tool's two search switches (MatchToolDlg.cpp:936, :788-796), honoured under both semantics ---
    def setStopLayer1(self, v: bool):
        """Fast mode (m_bStopLayer1): stop the pyramid descent at layer 1.  Positions have layer-1 precision (the
        layer-1 ptLT times 2, no sub-pixel fit); a template whose top layer is 0 is searched as usual."""
        self._params.stop_layer = 1 if v else 0

    def getStopLayer1(self) -> bool: return bool(self._params.stop_layer)

    def setBitwiseNot(self, v: bool):
        """m_ckBitwiseNot: search 255 - source with the template as learned (patterns of inverted polarity)."""
        self._params.bitwise_not = 1 if v else 0

    def getBitwiseNot(self) -> bool: return bool(self._params.bitwise_not)

    # -- user rectangle (TemplateMatcher.cpp:1224-1238): unused by matching; the default rectangle of the match patches,
    # which is what the reference's tool does with it (MatchToolDialog.cpp:1216-1328 carries it onto every match) ----
    def setUserDefinedRect(self, rect): self._user_rect = tuple(rect)
    def getUserDefinedRect(self): return self._user_rect if self._user_rect is not None else (0, 0, 0, 0)
    def hasUserDefinedRect(self) -> bool: return self._user_rect is not None

    # -- match patches: upright crops of the results, sampled on the device (fpm_last_patches* / fpm_patches_at) -------
    def setPatchForm(self, form: int):
        """fpm_set_patch_form: L.PATCH_FORM_TILED (k_patch_warp, default) or L.PATCH_FORM_WARP (k_warp; same bytes)."""
        rc = self._lib.fpm_set_patch_form(self._ctx, int(form))
        if rc != L.FPM_OK:
            raise ValueError(f"fpm_set_patch_form({form}) failed with {rc}: {self.last_error()}")

    def _patch_rect(self, rect):
        """The fpm_patch_rect of ``rect``: None = the user-defined rectangle when one is set, else NULL (the whole
        template)."""
        r = rect if rect is not None else self._user_rect
        return None if r is None else L.PatchRect(*normalize_rect(r))

    def patch_size(self, rect=None) -> Tuple[int, int]:
        """(pw, ph) of the patches for ``rect`` ((x, y, w, h) in template coordinates; None = the user-defined rectangle
        when one is set, else the learned template's frame)."""
        r = self._patch_rect(rect)
        if r is not None:
            return r.w, r.h
        return self._template_size()

    def _template_size(self) -> Tuple[int, int]:
        """(tw, th) of the learned template."""
        w, h, eq = C.c_int32(), C.c_int32(), C.c_int32()
        d = C.c_double()
        if self._lib.fpm_template_level(self._ctx, 0, C.byref(w), C.byref(h), C.byref(d), C.byref(d), C.byref(d),
                                        C.byref(eq), None, 0) != L.FPM_OK:
            raise ValueError("template not learned")
        return w.value, h.value

    def _patch_fail(self, rc, what):
        self._check(rc, what)
        raise ValueError(f"{what} failed with {rc}: {self.last_error()}")

    def _last(self, what, call, nulls, alloc, count_what=None):
        """Count, then fill, of a last_* wrapper.  ``call(outs, cap, n)`` makes the C call with the output arguments
        ``outs``: first with ``nulls`` and capacity 0, which gives the count (FPM_OK or FPM_E_CAPACITY);
        ``alloc(count)`` then returns ``(results, outs)``, and the fill call runs only when there is a hit.  Returns
        ``results``.
        ``count_what``: the name in a failed count call's message when it is not ``what``."""
        n = C.c_int32()
        rc = call(nulls, 0, C.byref(n))
        if rc not in (L.FPM_OK, L.FPM_E_CAPACITY):
            self._patch_fail(rc, count_what or what)
        results, outs = alloc(n.value)
        if n.value:
            rc = call(outs, n.value, C.byref(n))
            if rc != L.FPM_OK:
                self._patch_fail(rc, what)
        return results

    def _profile(self, getter, *which, fail):
        """``(ms, launches, bytes)`` of one fpm_*_profile getter; ValueError(``fail``) when it is rejected."""
        ms, n, b = C.c_double(), C.c_int64(), C.c_int64()
        if getter(self._ctx, *which, C.byref(ms), C.byref(n), C.byref(b)) != L.FPM_OK:
            raise ValueError(fail)
        return ms.value, n.value, b.value

    def _last_counts(self) -> np.ndarray:
        n = (C.c_int32 * max(self._staged, 1))()
        self._lib.fpm_last_results(self._ctx, None, 0, n)
        return np.array(n[:], np.int32)

    @staticmethod
    def _host_patch_out(out, n, ph, pw):
        """(array, row_stride, patch_stride) of a host output: a fresh dense one, or the caller's checked."""
        if out is None:
            return np.zeros((n, ph, pw), np.uint8), pw, pw * ph
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8:
            raise TypeError("out must be a uint8 numpy array")
        row, patch = patch_out_layout(out.shape, out.strides, n, ph, pw)
        return out, row, patch

    def last_patches(self, source: int = 0, rect=None, matrices: bool = False, out=None):
        """The pixels behind the last search's results: for every result of ``source`` (result order) the matched region
        of level 0 turned upright and cropped to ``rect`` -- (x, y, w, h) in template coordinates, None = the
        user-defined rectangle when one is set, else the template's frame; (-3, -3, tw + 6, th + 6) is the reference's
        getRotatedROI (TemplateMatcher.cpp:1074-1090) bit for bit.  Returns a uint8 array (n, ph, pw); with
        ``matrices`` also the patches' forward 2x3 matrices (n, 2, 3).  ``source=-1``: the patches of all sources in
        source order and the per-source counts, ``(patches, counts[, matrices])``.  The plane sampled is the one the
        search ran on: 255 - source under setBitwiseNot.  ``out``: a uint8 array (n, ph, pw) to write instead of a new
        one (unit pixel stride, any row and patch strides; the bytes between the rows keep their values).  One device
        launch (fpm_last_patches)."""
        r = self._patch_rect(rect)
        pr = C.byref(r) if r is not None else None

        def call(o, cap, n):
            return self._lib.fpm_last_patches(self._ctx, pr, int(source), o[0], o[1], o[2], cap, n, o[3])

        def alloc(n):
            pw, ph = self.patch_size(rect)
            buf, row, patch = self._host_patch_out(out, n, ph, pw)
            mats = np.zeros((n, 2, 3), np.float64)
            return (buf, mats), (L.u8ptr(buf), row, patch, _ptr(mats, C.c_double))

        out, mats = self._last("last_patches", call, (None, 0, 0, None), alloc)
        res = (out,) if source >= 0 else (out, self._last_counts())
        res = res + (mats,) if matrices else res
        return res[0] if len(res) == 1 else res

    def last_patches_device(self, source: int = 0, rect=None, out=None, stream=None):
        """last_patches into device memory, for a consumer on the device: a uint8 cuda tensor (n, ph, pw), no pixel
        crossing the host (fpm_last_patches_device).  ``out``: the tensor to write, shape (n, ph, pw), unit pixel stride,
        any row and patch strides (a view into a larger tensor is written in place; its other bytes are untouched);
        None allocates one.  The launch is ordered after the work already enqueued on ``stream`` (a torch stream or a
        raw handle; None = torch's current stream of the device) and that stream's later work after the launch, without
        a host synchronisation: use the tensor on that stream.  ``source=-1``: ``(patches, counts)``."""
        import torch

        r = self._patch_rect(rect)
        pr = C.byref(r) if r is not None else None
        dev = torch.device("cuda", self._device)

        def call(o, cap, n):
            if o is None:                                   # the count comes from the host entry: no stream is touched
                return self._lib.fpm_last_patches(self._ctx, pr, int(source), None, 0, 0, 0, n, None)
            return self._lib.fpm_last_patches_device(self._ctx, pr, int(source), o[0], o[1], o[2], cap, n,
                                                     self._producer_stream(stream))

        def alloc(n):
            pw, ph = self.patch_size(rect)
            buf = out
            if buf is None:
                ctx = torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else torch.cuda.device(dev)
                with ctx:
                    buf = torch.empty((n, ph, pw), dtype=torch.uint8, device=dev)
            if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8:
                raise TypeError("out must be a uint8 torch.Tensor")
            if buf.device != dev:
                raise ValueError(f"out on {buf.device}, context on {dev}")
            self._check_one_runtime()
            row, patch = patch_out_layout(tuple(buf.shape), tuple(buf.stride()), n, ph, pw)
            return buf, (buf.data_ptr(), row, patch)

        out = self._last("last_patches_device", call, None, alloc, count_what="last_patches")
        return out if source >= 0 else (out, self._last_counts())

    def patches_at(self, src_index, lts, angles, rect=None, matrices: bool = False, out=None):
        """Patches at poses the caller supplies, on the staged sources (fpm_patches_at): ``lts`` (n, 2) ptLT as the
        search reports it, ``angles`` (n) dMatchedAngle of the Qt semantics in degrees, ``src_index`` (n) or one index
        for all.  For results that no context holds, such as the merged results of an angle-sharded search.  Needs
        staged sources (stage / stage_device, or the source of the last match), not a search.  Returns uint8
        (n, ph, pw), with ``matrices`` also (n, 2, 3); ``out`` as last_patches."""
        poses = _pose_args(src_index, lts, angles)
        r = self._patch_rect(rect)
        pw, ph = self.patch_size(rect)
        n = poses[3]
        out, row, patch = self._host_patch_out(out, n, ph, pw)
        mats = np.zeros((n, 2, 3), np.float64)
        rc = self._lib.fpm_patches_at(self._ctx, C.byref(r) if r is not None else None, *poses, L.u8ptr(out), row,
                                      patch, _ptr(mats, C.c_double))
        if rc != L.FPM_OK:
            self._patch_fail(rc, "patches_at")
        return (out, mats) if matrices else out

    # -- patch comparison: every hit against the template, reduced on the device (fpm_last_compare / fpm_compare_at) ---
    def _compare_rect(self, rect):
        """(fpm_patch_rect or None, w, h) of a comparison: ``rect``, else the user-defined rectangle when one is set and
        lies inside the template, else the whole template (NULL)."""
        tw, th = self._template_size()
        if rect is None and self._user_rect is not None:
            try:
                rect = compare_rect(self._user_rect, tw, th)
            except ValueError:
                rect = None
        if rect is None:
            return None, tw, th
        x, y, w, h = compare_rect(rect, tw, th)
        return L.PatchRect(x, y, w, h), w, h

    @staticmethod
    def _compare_diff(diff, n, h, w):
        """(array or None, pointer, row_stride, patch_stride) of the difference images asked for by ``diff``."""
        if not diff:
            return None, None, 0, 0
        img = np.zeros((n, h, w), np.uint8)
        return img, L.u8ptr(img), w, w * h

    def last_compare(self, source: int = 0, rect=None, threshold: int = 16, normalize: bool = False, diff: bool = False):
        """Every result of the last search compared with the learned template where the pixels are: a structured array
        (COMPARE_DTYPE), one row per result of ``source`` in result order (``source=-1``: all sources, in source order).
        Per row the exact integer sums over the rectangle (n, sum_i, sum_ii, sum_t, sum_tt, sum_it: I = the pixels
        last_patches gives, T = the template's), zncc, and the deviations d = |LUT[I] - T|: sum_abs, max_abs, n_over
        = pixels with d > ``threshold`` and their inclusive bounding box x0, y0, x1, y1 in rectangle coordinates (w, h,
        -1, -1 when there is none).  ``normalize`` first fits the hit's gain and offset to the template's (a change
        of lighting is then no deviation; gain and offset are reported).  ``rect``: (x, y, w, h) inside the template;
        None = the user-defined rectangle when one is set and lies inside the template, else the whole template.
        ``diff=True``: also d as uint8 images, ``(stats, (n, h, w))``.  No patch is written anywhere."""
        r, w, h = self._compare_rect(rect)
        pr = C.byref(r) if r is not None else None
        flags = L.COMPARE_NORMALIZE if normalize else 0

        def call(o, cap, n):
            return self._lib.fpm_last_compare(self._ctx, pr, int(source), int(threshold), flags, o[0], cap, n, *o[1:])

        def alloc(n):
            stats = np.zeros(n, COMPARE_DTYPE)
            img, pimg, row, patch = self._compare_diff(diff, n, h, w)
            return (stats, img), (_ptr(stats, L.CompareStats), pimg, row, patch)

        stats, img = self._last("last_compare", call, (None, None, 0, 0), alloc)
        return (stats, img) if diff else stats

    def compare_at(self, src_index, lts, angles, rect=None, threshold: int = 16, normalize: bool = False,
                   diff: bool = False):
        """last_compare at poses the caller supplies, on the staged sources (fpm_compare_at); poses as patches_at.
        Needs staged sources, not a search."""
        poses = _pose_args(src_index, lts, angles)
        r, w, h = self._compare_rect(rect)
        n = poses[3]
        stats = np.zeros(n, COMPARE_DTYPE)
        img, pimg, row, patch = self._compare_diff(diff, n, h, w)
        rc = self._lib.fpm_compare_at(self._ctx, C.byref(r) if r is not None else None, *poses, int(threshold),
                                      L.COMPARE_NORMALIZE if normalize else 0, _ptr(stats, L.CompareStats), pimg, row,
                                      patch)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "compare_at")
        return (stats, img) if diff else stats

    # -- variation model: per-pixel tolerances trained from hits, inspection on the device (fpm_model_* / fpm_*inspect*) --
    def model_clear(self):
        """Drops the variation model (fpm_model_clear)."""
        rc = self._lib.fpm_model_clear(self._ctx)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "model_clear")

    def model_set_chunk(self, jobs: int = 0):
        """fpm_model_set_chunk: samples per workgroup of the training kernel; 0 = the engine's choice.  The sums do not
        depend on it (parity tests and measurements)."""
        rc = self._lib.fpm_model_set_chunk(self._ctx, int(jobs))
        if rc != L.FPM_OK:
            self._patch_fail(rc, "model_set_chunk")

    def model_train_last(self, source: int = -1, rect=None, normalize: bool = False) -> int:
        """Adds the hits of the last search (``source=-1``: of all sources) to the variation model, where the pixels
        are: per pixel of ``rect`` the sum and the sum of squares of what last_patches gives there, in two uint32 planes
        on the device (fpm_model_train_last); returns the number of samples added.  ``rect``: as last_compare's, fixed
        by the first call after model_clear.  ``normalize``: the samples go through the hit's gain / offset table first,
        as in last_compare.  At most 65535 samples; restaging keeps the model, every learn entry but model_learn drops
        it."""
        r, _, _ = self._compare_rect(rect)
        n = C.c_int32()
        rc = self._lib.fpm_model_train_last(self._ctx, C.byref(r) if r is not None else None, int(source),
                                            L.COMPARE_NORMALIZE if normalize else 0, C.byref(n))
        if rc != L.FPM_OK:
            self._patch_fail(rc, "model_train_last")
        return n.value

    def model_train_at(self, src_index, lts, angles, rect=None, normalize: bool = False) -> int:
        """model_train_last at poses the caller supplies, on the staged sources (fpm_model_train_at); poses as
        patches_at.  Needs staged sources, not a search."""
        poses = _pose_args(src_index, lts, angles)
        r, _, _ = self._compare_rect(rect)
        rc = self._lib.fpm_model_train_at(self._ctx, C.byref(r) if r is not None else None, *poses,
                                          L.COMPARE_NORMALIZE if normalize else 0)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "model_train_at")
        return poses[3]

    def model_info(self):
        """``(n, (x, y, w, h))`` of the variation model: its sample count and rectangle; ``(0, None)`` without one."""
        n, r = C.c_int32(), L.PatchRect()
        self._lib.fpm_model_info(self._ctx, C.byref(n), C.byref(r))
        return (n.value, (r.x, r.y, r.w, r.h)) if n.value else (0, None)

    def _model_size(self, what):
        n, rect = self.model_info()
        if not n:
            raise ValueError(f"{what}: no variation model (model_train_last / model_train_at first)")
        return rect[2], rect[3]

    def model_sums(self):
        """``(S, Q)``: the model's per-pixel sum and sum of squares, uint32 (h, w) each (fpm_model_sums)."""
        w, h = self._model_size("model_sums")
        s, q = np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)
        rc = self._lib.fpm_model_sums(self._ctx, s.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      q.ctypes.data_as(C.POINTER(C.c_uint32)))
        if rc != L.FPM_OK:
            self._patch_fail(rc, "model_sums")
        return s, q

    def model_images(self, abs_threshold: int = 8, k: float = 3.0):
        """``(mean, lo, hi)``: uint8 (h, w) images of the model for an absolute threshold and a sigma multiple ``k``
        (model_thresholds), as the device derives them: a pixel value u is inside where lo <= u <= hi, which is mean +-
        max(abs_threshold, k sigma) in exact integers (include/fpm.h); lo == hi + 1 where no value is."""
        a, kq = model_thresholds(abs_threshold, k)
        w, h = self._model_size("model_images")
        out = [np.zeros((h, w), np.uint8) for _ in range(3)]
        rc = self._lib.fpm_model_images(self._ctx, a, kq, L.u8ptr(out[0]), L.u8ptr(out[1]), L.u8ptr(out[2]), w)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "model_images")
        return tuple(out)

    def last_inspect(self, source: int = 0, abs_threshold: int = 8, k: float = 3.0, normalize: bool = False,
                     image: bool = False):
        """Every result of the last search held against the variation model where the pixels are: a structured array
        (INSPECT_DTYPE), one row per result of ``source`` in result order (``source=-1``: all sources).  Per row, over
        the model's rectangle: n, sum_excess, n_low and n_high = the pixels below lo and above hi, max_excess, their
        inclusive bounding box x0, y0, x1, y1 in rectangle coordinates (w, h, -1, -1 when there is none), and the
        gain and offset of ``normalize`` (1 and 0 without).  ``image=True``: also the excess per pixel as uint8 images,
        ``(stats, (n, h, w))``.  No patch is written anywhere."""
        a, kq = model_thresholds(abs_threshold, k)
        w, h = self._model_size("last_inspect")
        flags = L.COMPARE_NORMALIZE if normalize else 0

        def call(o, cap, n):
            return self._lib.fpm_last_inspect(self._ctx, int(source), a, kq, flags, o[0], cap, n, *o[1:])

        def alloc(n):
            stats = np.zeros(n, INSPECT_DTYPE)
            img, pimg, row, patch = self._compare_diff(image, n, h, w)
            return (stats, img), (_ptr(stats, L.InspectStats), pimg, row, patch)

        stats, img = self._last("last_inspect", call, (None, None, 0, 0), alloc)
        return (stats, img) if image else stats

    def inspect_at(self, src_index, lts, angles, abs_threshold: int = 8, k: float = 3.0, normalize: bool = False,
                   image: bool = False):
        """last_inspect at poses the caller supplies, on the staged sources (fpm_inspect_at); poses as patches_at."""
        poses = _pose_args(src_index, lts, angles)
        a, kq = model_thresholds(abs_threshold, k)
        w, h = self._model_size("inspect_at")
        n = poses[3]
        stats = np.zeros(n, INSPECT_DTYPE)
        img, pimg, row, patch = self._compare_diff(image, n, h, w)
        rc = self._lib.fpm_inspect_at(self._ctx, *poses, a, kq, L.COMPARE_NORMALIZE if normalize else 0,
                                      _ptr(stats, L.InspectStats), pimg, row, patch)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "inspect_at")
        return (stats, img) if image else stats

    # -- defect blobs on the device (fpm_last_blobs / fpm_blobs_at / fpm_op_blobs) -----------------------------------
    def last_blobs(self, source: int = 0, abs_threshold: int = 8, k: float = 3.0, normalize: bool = False,
                   level: int = 0, min_area: int = 4, connectivity: int = 8, cap: int = 64, stats: bool = False):
        """The defect list of every result of the last search (fpm_last_blobs): last_inspect's excess images cut into
        connected components where they lie, on the device -- no image crosses the host.  Returns what
        ``blobs_host(last_inspect(..., image=True)[1], level, min_area, connectivity, cap)`` returns, ``(summary,
        blobs)``, one summary row and one BLOB_DTYPE array per result of ``source`` in result order (``source=-1``: all
        sources); of a truncated hit any ``cap`` of its qualifying components come back, in ascending seed.
        ``stats=True``: also last_inspect's rows, ``(summary, blobs, stats)``."""
        a, kq = model_thresholds(abs_threshold, k)
        self._model_size("last_blobs")
        flags = L.COMPARE_NORMALIZE if normalize else 0
        args = (int(level), int(connectivity), int(min_area))

        def call(o, hits, n):
            return self._lib.fpm_last_blobs(self._ctx, int(source), a, kq, flags, *args, *o, int(cap), hits, n)

        def alloc(n):
            rows = np.zeros(n, INSPECT_DTYPE)
            summary, recs, _, _ = _blob_buffers(n, 0, 0, cap, False)
            return (rows, summary, recs), (_ptr(rows, L.InspectStats), _ptr(summary, L.BlobSummary), _ptr(recs, L.Blob))

        rows, summary, recs = self._last("last_blobs", call, (None, None, None), alloc)
        out = _blob_result(summary, recs, None, False)
        return out + (rows,) if stats else out

    def blobs_at(self, src_index, lts, angles, abs_threshold: int = 8, k: float = 3.0, normalize: bool = False,
                 level: int = 0, min_area: int = 4, connectivity: int = 8, cap: int = 64, stats: bool = False):
        """last_blobs at poses the caller supplies, on the staged sources (fpm_blobs_at); poses as patches_at."""
        poses = _pose_args(src_index, lts, angles)
        a, kq = model_thresholds(abs_threshold, k)
        self._model_size("blobs_at")
        n = poses[3]
        rows = np.zeros(n, INSPECT_DTYPE)
        summary, recs, _, _ = _blob_buffers(n, 0, 0, cap, False)
        rc = self._lib.fpm_blobs_at(self._ctx, *poses, a, kq, L.COMPARE_NORMALIZE if normalize else 0, int(level),
                                    int(connectivity), int(min_area), _ptr(rows, L.InspectStats),
                                    _ptr(summary, L.BlobSummary), _ptr(recs, L.Blob), int(cap))
        if rc != L.FPM_OK:
            self._patch_fail(rc, "blobs_at")
        out = _blob_result(summary, recs, None, False)
        return out + (rows,) if stats else out

    def op_blobs(self, images, level: int = 0, min_area: int = 4, connectivity: int = 8, cap: int = 64,
                 labels: bool = False):
        """blobs_host's arguments and results through the labelling kernels (fpm_op_blobs, parity vehicle): needs no
        template, sources or model and changes none of them.  ``images``: (h, w) or (n, h, w) uint8; a view with unit
        pixel stride whose rows and images are evenly spaced (a padded batch cut to its width) is uploaded with its row
        stride as it is, padding included."""
        a = np.asarray(images)
        if a.dtype != np.uint8:
            a = _blob_images(a)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.size == 0:
            raise ValueError("images: a (h, w) or (n, h, w) uint8 array with at least one pixel expected")
        n, h, w = a.shape
        stride = a.strides[1]
        if a.strides[2] != 1 or stride < w or (n > 1 and a.strides[0] != stride * h) or h == 1:
            a = np.ascontiguousarray(a)
            stride = w
        summary, recs, lab, plab = _blob_buffers(n, h, w, cap, labels)
        rc = self._lib.fpm_op_blobs(self._ctx, C.cast(a.ctypes.data, C.POINTER(C.c_uint8)), n, w, h, stride, int(level),
                                    int(connectivity), int(min_area), summary.ctypes.data_as(C.POINTER(L.BlobSummary)),
                                    recs.ctypes.data_as(C.POINTER(L.Blob)), int(cap), plab)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "op_blobs")
        return _blob_result(summary, recs, lab, labels)

    def blobs_set_round(self, images: int = 0):
        """Images per round of the labelling launches (fpm_blobs_set_round); 0 = the engine's choice.  The results do
        not depend on it: it is there for tests."""
        if self._lib.fpm_blobs_set_round(self._ctx, int(images)) != L.FPM_OK:
            raise ValueError(f"blobs_set_round({images!r}): a count >= 0 expected")

    def blobs_profile(self, which: int):
        """``(ms, launches, bytes)`` of L.BLOB_TILE .. L.BLOB_FEATURES, collected under profile(True) and cleared by
        profile_reset (fpm_blobs_profile)."""
        return self._profile(self._lib.fpm_blobs_profile, int(which), fail=f"fpm_blobs_profile({which}) failed")

    def model_learn(self):
        """Learns the model's mean image as the new template, on the device (fpm_model_learn): re-teach from many good
        parts instead of one.  State afterwards as after learn_at; the model survives with the rectangle (0, 0, w, h).
        A template mask survives too, cropped to the model's rectangle -- the new template's frame -- so that it keeps
        covering the same pixels, and keeps its enabled state (every other learn entry drops the mask).
        Raises LearnError when the call is rejected."""
        self._push()
        self._learn_done(self._lib.fpm_model_learn(self._ctx), "model_learn")

    # -- template mask: compare, align, inspect and cut blobs on the part only (fpm_mask_*) --------------------------
    def _mask_done(self, rc, what):
        self._check(rc, what)
        if rc != L.FPM_OK:
            raise MaskError(rc, f"{what} failed with {rc}: {self.last_error()}")

    def set_mask(self, mask, stream=None):
        """Sets the template mask (fpm_mask_set / fpm_mask_set_device): ``mask`` of shape (th, tw), the learned
        template's, bool or uint8, nonzero = use the pixel, 0 = ignore it (background, a date code, a hole).  A numpy
        array, or a uint8 / bool torch tensor on this context's device, contiguous or a view with unit column stride
        (``stream``: the stream it was written on, as match_device).  With a mask set last_compare / compare_at,
        align_* and last_inspect / inspect_at / last_blobs / blobs_at run over the used pixels only, and the normalising
        tables are fitted to them; the search, the patches, the calipers and the training planes do not look at it.  The
        mask starts enabled and lives as long as the template (model_learn crops it).  Raises MaskError (a ValueError
        with the status in ``code``) when the call is rejected; the previous mask then stays in force."""
        if isinstance(mask, np.ndarray) or not hasattr(mask, "data_ptr"):
            a = np.asarray(mask)
            if a.dtype == np.bool_:
                a = a.view(np.uint8)
            if a.dtype != np.uint8 or a.ndim != 2:
                raise TypeError(f"expected a 2-D bool or uint8 mask, got {a.dtype} with shape {a.shape}")
            if a.size and (a.strides[1] != 1 or a.strides[0] < a.shape[1]):
                a = np.ascontiguousarray(a)
            rc = self._lib.fpm_mask_set(self._ctx, L.u8ptr(a), a.shape[1], a.shape[0], a.strides[0] if a.size else 0)
            return self._mask_done(rc, "set_mask")
        import torch

        t = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        if t.dim() != 2:
            raise TypeError(f"expected a 2-D mask, got shape {tuple(t.shape)}")
        ptr, h, w, row, _, _ = self._device_image(t, "bgr", None)
        rc = self._lib.fpm_mask_set_device(self._ctx, ptr, w, h, row, self._producer_stream(stream))
        self._mask_done(rc, "set_mask")

    def clear_mask(self):
        """Drops the template mask (fpm_mask_clear)."""
        self._mask_done(self._lib.fpm_mask_clear(self._ctx), "clear_mask")

    def mask_enable(self, flag: bool = True):
        """Switches a set mask on or off; a disabled mask stays resident and every tool behaves as without one."""
        self._mask_done(self._lib.fpm_mask_enable(self._ctx, 1 if flag else 0), "mask_enable")

    def mask_info(self):
        """``(w, h, count, enabled)`` of the template mask: its size, its used pixels, whether it is enabled;
        ``(0, 0, 0, False)`` without one (fpm_mask_info)."""
        w, h, e, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        if self._lib.fpm_mask_info(self._ctx, C.byref(w), C.byref(h), C.byref(n), C.byref(e)) != L.FPM_OK:
            raise ValueError("fpm_mask_info failed")
        return w.value, h.value, n.value, bool(e.value)

    def mask(self):
        """The mask as stored, uint8 (th, tw) of 0 / 255, or None without one (fpm_mask_get)."""
        w, h, _, _ = self.mask_info()
        if w == 0:
            return None
        out = np.zeros((h, w), np.uint8)
        self._mask_done(self._lib.fpm_mask_get(self._ctx, L.u8ptr(out), w), "mask")
        return out

    def mask_count(self, rect=None) -> int:
        """Used pixels of the mask inside ``rect`` (x, y, w, h), None = the whole template (fpm_mask_count): the ``n``
        of a masked last_compare over that rectangle."""
        r = None
        if rect is not None:
            x, y, w, h = normalize_rect(rect)
            r = L.PatchRect(x, y, w, h)
        n = C.c_int64()
        self._mask_done(self._lib.fpm_mask_count(self._ctx, C.byref(r) if r is not None else None, C.byref(n)),
                        "mask_count")
        return n.value

    def model_profile(self, which: int):
        """``(ms, launches, bytes)`` of L.MODEL_TRAIN / L.MODEL_PREPARE / L.MODEL_INSPECT, collected under profile(True)
        and cleared by profile_reset (fpm_model_profile)."""
        return self._profile(self._lib.fpm_model_profile, int(which), fail=f"fpm_model_profile({which}) failed")

    # -- pose alignment: every hit polished by least squares against the template (fpm_align_*) ---------------------
    def _align_rect(self, rect):
        """(fpm_patch_rect or None, (x, y, w, h)) of an alignment: ``rect``, else the user-defined rectangle when one is
        set and passes align_rect, else the whole template (NULL)."""
        tw, th = self._template_size()
        if rect is None and self._user_rect is not None:
            try:
                rect = align_rect(self._user_rect, tw, th)
            except ValueError:
                rect = None
        r = align_rect(rect, tw, th)
        return (None if rect is None else L.PatchRect(*r)), r

    @staticmethod
    def _align_args(iters, max_step):
        if int(iters) != iters or not 1 <= int(iters) <= L.ALIGN_MAX_ITERS:
            raise ValueError(f"iters {iters!r} must be a whole number 1 .. {L.ALIGN_MAX_ITERS}")
        if not 0.0 < float(max_step) <= L.ALIGN_MAX_STEP:
            raise ValueError(f"max_step {max_step!r} must be above 0 and at most {L.ALIGN_MAX_STEP} pixels")
        return int(iters), float(max_step)

    def align_sums_at(self, src_index, lts, angles, rect=None, normalize: bool = False) -> np.ndarray:
        """The sums of one Gauss-Newton step of the pose at every pose supplied, on the staged sources
        (fpm_align_sums_at): a structured array (ALIGN_SUMS_DTYPE) of exact integers -- n_used, the six entries of the
        normal matrix, the three of the gradient, ssd (include/fpm.h).  One launch of k_patch_align; poses as
        patches_at."""
        poses = _pose_args(src_index, lts, angles)
        r, _ = self._align_rect(rect)
        out = np.zeros(poses[3], ALIGN_SUMS_DTYPE)
        rc = self._lib.fpm_align_sums_at(self._ctx, C.byref(r) if r is not None else None, *poses,
                                         L.COMPARE_NORMALIZE if normalize else 0, _ptr(out, L.AlignSums))
        if rc != L.FPM_OK:
            self._patch_fail(rc, "align_sums_at")
        return out

    def align_at(self, src_index, lts, angles, rect=None, iters: int = 3, max_step: float = 2.0,
                 normalize: bool = False) -> np.ndarray:
        """align_last from poses the caller supplies, on the staged sources (fpm_align_at); poses as patches_at.  Needs
        staged sources, not a search; nothing in the matcher changes."""
        poses = _pose_args(src_index, lts, angles)
        iters, max_step = self._align_args(iters, max_step)
        r, _ = self._align_rect(rect)
        out = np.zeros(poses[3], ALIGN_DTYPE)
        rc = self._lib.fpm_align_at(self._ctx, C.byref(r) if r is not None else None, *poses, iters, max_step,
                                    L.COMPARE_NORMALIZE if normalize else 0, _ptr(out, L.AlignResult))
        if rc != L.FPM_OK:
            self._patch_fail(rc, "align_at")
        return out

    def align_last(self, source: int = 0, rect=None, iters: int = 3, max_step: float = 2.0, normalize: bool = False,
                   adopt: bool = False) -> np.ndarray:
        """Every result of the last search polished by least squares against the learned template, where the pixels
        are: ``iters`` Gauss-Newton steps of shift and rotation, ``iters + 1`` launches, no crop written
        (fpm_align_last).  Returns a structured array (ALIGN_DTYPE), one row per result of ``source`` in result order
        (``source=-1``: all sources): the aligned pose lt_x, lt_y (f32), angle (degrees), ssd_start and ssd (the sum of
        squared differences at the start and at the returned pose: ssd <= ssd_start), n_used, evals, best_eval and flags
        (L.ALIGN_SINGULAR, L.ALIGN_STEP_CLAMPED: the hit stopped early; L.ALIGN_KEPT_START: no step improved it).  A step
        that would move a corner of the rectangle by more than ``max_step`` source pixels stops the hit.
        ``normalize``: the pixels go through the hit's gain / offset table, built once at the start pose.
        ``adopt=True``: the aligned poses replace the matcher's last poses -- last_patches, last_compare, last_inspect,
        model_train_last and learn_hit sample at them until the next search; the results of the search are unchanged."""
        iters, max_step = self._align_args(iters, max_step)
        r, _ = self._align_rect(rect)
        pr = C.byref(r) if r is not None else None
        flags = (L.COMPARE_NORMALIZE if normalize else 0) | (L.ALIGN_ADOPT if adopt else 0)

        def call(o, cap, n):
            return self._lib.fpm_align_last(self._ctx, pr, int(source), iters, max_step, flags, o, cap, n)

        def alloc(n):
            out = np.zeros(n, ALIGN_DTYPE)
            return out, _ptr(out, L.AlignResult)

        return self._last("align_last", call, None, alloc)

    def align_profile(self):
        """``(ms, launches, bytes)`` of k_patch_align, collected under profile(True) and cleared by profile_reset
        (fpm_align_profile)."""
        return self._profile(self._lib.fpm_align_profile, fail="fpm_align_profile failed")

    # -- edge calipers: edges measured across every hit, on the device (fpm_last_calipers / fpm_calipers_at) --------
    @staticmethod
    def _caliper_buffers(n, cals, cap, profiles):
        if int(cap) != cap or not 1 <= int(cap) <= L.CALIPER_MAX_CAP:
            raise ValueError(f"cap {cap!r} must be a whole number 1 .. {L.CALIPER_MAX_CAP}")
        K, cap = len(cals), int(cap)
        if n * K * cap > L.CALIPER_MAX_SLOTS:
            raise ValueError(f"{n} hits x {K} calipers x cap {cap} above {L.CALIPER_MAX_SLOTS} records")
        summary = np.zeros((n, K), CALIPER_SUMMARY_DTYPE)
        edges = np.zeros((n, K, cap), EDGE_DTYPE)
        stride = int(cals["length"].max())
        prof = np.zeros((n, K, stride), np.int32) if profiles else None
        return summary, edges, prof, stride

    def last_calipers(self, cals, source: int = 0, cap: int = 8, profiles: bool = False):
        """The calipers ``cals`` (records of caliper()) measured on every result of the last search, where the pixels
        are: one launch of k_caliper, no image crosses the host (fpm_last_calipers).  Returns ``(summary, edges)``: a
        CALIPER_SUMMARY_DTYPE array (n_hits, K) -- n_edges (the true count), n_returned, strongest (index of the
        returned edge with the largest step, -1: none), flags (L.CALIPER_TRUNCATED: more than ``cap`` edges, the first
        ``cap`` by index returned; L.CALIPER_OUTSIDE: the caliper leaves the source, border zeros are in its profile)
        and the sampling pose -- and an EDGE_DTYPE array (n_hits, K, cap), the records behind n_returned zero: index,
        the three steps d_prev, d, d_next, the sub-sample position t along the scan, the contrast in gray levels and
        the edge point in template (tx, ty) and source (sx, sy) coordinates.  Hits come in result order of ``source``
        (``source=-1``: all sources, in source order), sampled at the raw poses, or the aligned ones after
        align_last(adopt=True).  ``profiles=True`` adds the int32 profiles, (n_hits, K, the largest length), zero
        from a caliper's length on.  Under setBitwiseNot(True) the polarities are those of the inverted plane."""
        arr = _calipers(cals)
        pc = arr.ctypes.data_as(C.POINTER(L.Caliper))
        if int(cap) != cap or not 1 <= int(cap) <= L.CALIPER_MAX_CAP:
            raise ValueError(f"cap {cap!r} must be a whole number 1 .. {L.CALIPER_MAX_CAP}")

        def call(o, hits, n):
            return self._lib.fpm_last_calipers(self._ctx, int(source), pc, len(arr), int(cap), *o, hits, n)

        def alloc(n):
            summary, edges, prof, stride = self._caliper_buffers(n, arr, cap, profiles)
            return (summary, edges, prof), (_ptr(summary, L.CaliperSummary), _ptr(edges, L.Edge),
                                            _ptr(prof, C.c_int32), stride)

        summary, edges, prof = self._last("last_calipers", call, (None, None, None, 0), alloc)
        return (summary, edges, prof) if profiles else (summary, edges)

    def calipers_at(self, src_index, lts, angles, cals, cap: int = 8, profiles: bool = False):
        """last_calipers at poses the caller supplies, on the staged sources (fpm_calipers_at); poses as patches_at.
        Needs staged sources, not a search; nothing in the matcher changes."""
        poses = _pose_args(src_index, lts, angles)
        arr = _calipers(cals)
        summary, edges, prof, stride = self._caliper_buffers(poses[3], arr, cap, profiles)
        rc = self._lib.fpm_calipers_at(self._ctx, *poses, _ptr(arr, L.Caliper), len(arr), int(cap),
                                       _ptr(summary, L.CaliperSummary), _ptr(edges, L.Edge), _ptr(prof, C.c_int32),
                                       stride)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "calipers_at")
        return (summary, edges, prof) if profiles else (summary, edges)

    def caliper_profile(self):
        """``(ms, launches, bytes)`` of k_caliper, collected under profile(True) and cleared by profile_reset
        (fpm_caliper_profile)."""
        return self._profile(self._lib.fpm_caliper_profile, fail="fpm_caliper_profile failed")

    # -- edge probes: an outline measured on every hit, on the device (fpm_last_probes / fpm_probes_at) --------------
    @staticmethod
    def _probe_buffers(n, probes, params, profiles):
        K = len(probes)
        if n * K > L.PROBE_MAX_SLOTS:
            raise ValueError(f"{n} hits x {K} probes above {L.PROBE_MAX_SLOTS} records")
        summary = np.zeros(n, PROBE_SUMMARY_DTYPE)
        results = np.zeros((n, K), PROBE_RESULT_DTYPE)
        stride = int(params[0]["length"])
        prof = np.zeros((n, K, stride), np.int32) if profiles else None
        return summary, results, prof, stride

    def last_probes(self, probes, params, source: int = -1, profiles: bool = False):
        """The probes ``probes`` (records of probe(), or circle_probes / line_probes / contour_probes) with the shared
        ``params`` (probe_params()) measured on every result of the last search, where the pixels are: one launch of
        k_probe for all hits and probes, a job table of one entry per hit and one per probe (fpm_last_probes).
        Returns ``(summary, results)``: a PROBE_SUMMARY_DTYPE array (n_hits,) -- n_found, n_missing, n_ambiguous (more
        than one edge qualified), n_outside, worst (the probe with the largest |dev|, -1: none), sum_dev, sum_dev_sq,
        max_abs_dev and the hit's pose -- and a PROBE_RESULT_DTYPE array (n_hits, K): index (0: no edge; the doubles
        are then 0), n_edges, the step d, flags (L.PROBE_OUTSIDE: the probe leaves the source, border zeros may be in
        its profile), dev (the edge's signed displacement from the nominal point along phi, in template pixels), the
        contrast in gray levels and the edge point in template (tx, ty) and source (sx, sy) coordinates -- what
        fit_line and fit_circle take.  Hits come in result order of ``source`` (-1: all sources, in source order),
        sampled at the raw poses, or the aligned ones after align_last(adopt=True).  ``profiles=True`` adds the int32
        profiles, (n_hits, K, length).  Under setBitwiseNot(True) the polarities are those of the inverted plane."""
        arr = _probes(probes)
        pa, pp = _probe_params_ptr(params)
        pk = _ptr(arr, L.Probe)

        def call(o, hits, n):
            return self._lib.fpm_last_probes(self._ctx, int(source), pk, len(arr), pp, *o, hits, n)

        def alloc(n):
            summary, results, prof, stride = self._probe_buffers(n, arr, pa, profiles)
            return (summary, results, prof), (_ptr(summary, L.ProbeSummary), _ptr(results, L.ProbeResult),
                                              _ptr(prof, C.c_int32), stride)

        summary, results, prof = self._last("last_probes", call, (None, None, None, 0), alloc)
        return (summary, results, prof) if profiles else (summary, results)

    def probes_at(self, src_index, lts, angles, probes, params, profiles: bool = False):
        """last_probes at poses the caller supplies, on the staged sources (fpm_probes_at); poses as patches_at.
        Needs staged sources, not a template or a search; nothing in the matcher changes."""
        poses = _pose_args(src_index, lts, angles)
        arr = _probes(probes)
        pa, pp = _probe_params_ptr(params)
        summary, results, prof, stride = self._probe_buffers(poses[3], arr, pa, profiles)
        rc = self._lib.fpm_probes_at(self._ctx, *poses, _ptr(arr, L.Probe), len(arr), pp, _ptr(summary, L.ProbeSummary),
                                     _ptr(results, L.ProbeResult), _ptr(prof, C.c_int32), stride)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "probes_at")
        return (summary, results, prof) if profiles else (summary, results)

    def probe_profile(self):
        """``(ms, launches, bytes)`` of k_probe, collected under profile(True) and cleared by profile_reset
        (fpm_probe_profile)."""
        return self._profile(self._lib.fpm_probe_profile, fail="fpm_probe_profile failed")

    # -- gray-value tools: histograms, Otsu and threshold blobs of every hit (fpm_*histogram* / fpm_*segment*) --------
    def _gray_rects(self, rects):
        """(array of fpm_patch_rect or None, K) of a histogram call: ``rects`` a list of (x, y, w, h) inside the
        template (one such tuple also does); None = one rectangle, chosen as last_compare chooses its own."""
        if rects is None:
            r, _, _ = self._compare_rect(None)
            return (None, 1) if r is None else ((L.PatchRect * 1)(r), 1)
        tw, th = self._template_size()
        rl = list(rects)
        if len(rl) == 4 and all(np.ndim(v) == 0 for v in rl):
            rl = [tuple(rl)]
        if not 1 <= len(rl) <= L.GRAY_MAX_RECTS:
            raise ValueError(f"1 .. {L.GRAY_MAX_RECTS} rectangles expected, got {len(rl)}")
        arr = (L.PatchRect * len(rl))(*[L.PatchRect(*compare_rect(r, tw, th)) for r in rl])
        return arr, len(rl)

    def last_histogram(self, rects=None, source: int = 0) -> np.ndarray:
        """The 256-bin gray-value histograms of the rectangles ``rects`` (template coordinates) on every result of the
        last search, counted where the pixels are by one launch of k_patch_hist (fpm_last_histogram): uint32
        (n_hits, K, 256), the pixels those of last_patches for that rectangle, under an enabled template mask the used
        ones only.  Hits come in result order of ``source`` (``source=-1``: all sources), at the raw poses, or the aligned
        ones after align_last(adopt=True).  hist_derive turns them into mean, median, Otsu's threshold and so on."""
        arr, K = self._gray_rects(rects)

        def call(o, cap, n):
            return self._lib.fpm_last_histogram(self._ctx, arr, K, int(source), o, cap, n)

        def alloc(n):
            hist = np.zeros((n, K, 256), np.uint32)
            return hist, _ptr(hist, C.c_uint32)

        return self._last("last_histogram", call, None, alloc)

    def histogram_at(self, src_index, lts, angles, rects=None) -> np.ndarray:
        """last_histogram at poses the caller supplies, on the staged sources (fpm_histogram_at); poses as patches_at.
        Needs staged sources and a template, not a search."""
        poses = _pose_args(src_index, lts, angles)
        arr, K = self._gray_rects(rects)
        hist = np.zeros((poses[3], K, 256), np.uint32)
        rc = self._lib.fpm_histogram_at(self._ctx, arr, K, *poses, _ptr(hist, C.c_uint32))
        if rc != L.FPM_OK:
            self._patch_fail(rc, "histogram_at")
        return hist

    def last_segment(self, rect=None, source: int = 0, threshold="otsu", polarity: int = -1, min_area: int = 4,
                     connectivity: int = 8, cap: int = 64, image: bool = False):
        """Every result of the last search thresholded inside ``rect`` and cut into connected regions, on the device
        (fpm_last_segment).  ``polarity`` -1 takes the dark pixels (I < t, e = t - I), +1 the bright ones (I > t, e =
        I - t); ``threshold`` is 0 .. 255 or "otsu": each hit's own Otsu threshold of the rectangle (t = otsu for
        bright, otsu + 1 for dark).  Returns ``(info, summary, blobs)``: a SEGMENT_INFO_DTYPE array (n, the threshold
        used, flags L.HIST_EMPTY / L.HIST_FLAT -- such a hit has no foreground -- and L.GRAY_OUTSIDE: the rectangle
        leaves the source, border zeros are in it), and what ``blobs_host(e, 0, min_area, connectivity, cap)`` gives for
        the images e; of a truncated hit any ``cap`` of its qualifying regions come back.  ``image=True``: also e as
        uint8 (n_hits, h, w).  Under an enabled template mask ignored pixels are background."""
        r, w, h = self._compare_rect(rect)
        pr = C.byref(r) if r is not None else None
        t = _segment_threshold(threshold)
        args = (t, int(polarity), int(connectivity), int(min_area))

        def call(o, hits, n):
            return self._lib.fpm_last_segment(self._ctx, int(source), pr, *args, *o[:3], int(cap), hits, n, *o[3:])

        def alloc(n):
            info = np.zeros(n, SEGMENT_INFO_DTYPE)
            summary, recs, _, _ = _blob_buffers(n, 0, 0, cap, False)
            img, pimg, row, patch = self._compare_diff(image, n, h, w)
            return (info, summary, recs, img), (_ptr(info, L.SegmentInfo), _ptr(summary, L.BlobSummary),
                                                _ptr(recs, L.Blob), pimg, row, patch)

        info, summary, recs, img = self._last("last_segment", call, (None, None, None, None, 0, 0), alloc)
        out = (info,) + _blob_result(summary, recs, None, False)
        return out + (img,) if image else out

    def segment_at(self, src_index, lts, angles, rect=None, threshold="otsu", polarity: int = -1, min_area: int = 4,
                   connectivity: int = 8, cap: int = 64, image: bool = False):
        """last_segment at poses the caller supplies, on the staged sources (fpm_segment_at); poses as patches_at."""
        poses = _pose_args(src_index, lts, angles)
        r, w, h = self._compare_rect(rect)
        n = poses[3]
        info = np.zeros(n, SEGMENT_INFO_DTYPE)
        summary, recs, _, _ = _blob_buffers(n, 0, 0, cap, False)
        img, pimg, row, patch = self._compare_diff(image, n, h, w)
        rc = self._lib.fpm_segment_at(self._ctx, *poses, C.byref(r) if r is not None else None,
                                      _segment_threshold(threshold), int(polarity), int(connectivity), int(min_area),
                                      _ptr(info, L.SegmentInfo), _ptr(summary, L.BlobSummary), _ptr(recs, L.Blob),
                                      int(cap), pimg, row, patch)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "segment_at")
        out = (info,) + _blob_result(summary, recs, None, False)
        return out + (img,) if image else out

    def gray_set_run(self, tiles: int = 0):
        """Tiles per workgroup of k_patch_hist; 0 = the engine's choice.  For tests and measurements: results never
        depend on it (fpm_gray_set_run)."""
        if self._lib.fpm_gray_set_run(self._ctx, int(tiles)) != L.FPM_OK:
            raise ValueError(f"gray_set_run({tiles!r}): {self.last_error()}")

    def gray_profile(self, which: int):
        """``(ms, launches, bytes)`` of one gray-value kernel (L.GRAY_HIST, L.GRAY_THRESHOLD), collected under
        profile(True) and cleared by profile_reset (fpm_gray_profile)."""
        return self._profile(self._lib.fpm_gray_profile, int(which), fail=f"gray_profile({which!r}) failed")

    # -- sub-pattern locators: template regions found again on every hit (fpm_last_locate / fpm_locate_at) ------------
    @staticmethod
    def _locate_buffers(n, feats, raw, maps):
        K = len(feats)
        if n * K > L.LOCATE_MAX_JOBS:
            raise ValueError(f"{n} hits x {K} features above {L.LOCATE_MAX_JOBS}")
        res = np.zeros((n, K), LOCATE_DTYPE)
        rw = np.zeros((n, K), LOCATE_RAW_DTYPE) if raw else None
        stride = int(((2 * feats["rx"] + 1) * (2 * feats["ry"] + 1)).max())
        mp = np.zeros((n, K, 3, stride), np.int32) if maps else None
        return res, rw, mp, stride

    @staticmethod
    def _locate_result(res, rw, mp, raw, maps):
        out = (res,) + ((rw,) if raw else ()) + ((mp,) if maps else ())
        return out if len(out) > 1 else res

    def last_locate(self, features, source: int = 0, raw: bool = False, maps: bool = False):
        """The features ``features`` (records of feature()) found again on every result of the last search, where the
        pixels are: one launch of k_patch_locate, no image crosses the host (fpm_last_locate).  Each feature's template
        region is correlated (the search's own normalized correlation) with the hit's pixels at every offset of +-rx,
        +-ry around its nominal place.  Returns a LOCATE_DTYPE array (n_hits, K): the peak (dx, dy), score and
        score_nominal (the score at offset 0), the sub-pixel displacement (ox, oy) in template pixels, the found centre
        in template (tx, ty) and source (sx, sy) coordinates, and flags (L.LOCATE_EDGE_X / _EDGE_Y: the peak lies on
        the search range's border, no sub-pixel step on that axis; L.LOCATE_FLAT: no contrast, score 0 at nominal;
        L.LOCATE_OUTSIDE: the window leaves the source, border zeros are in it).  Hits come in result order of
        ``source`` (``source=-1``: all sources), at the raw poses, or the aligned ones after align_last(adopt=True).
        ``raw=True`` adds the LOCATE_RAW_DTYPE records, ``maps=True`` the int32 sums (n_hits, K, 3, the largest offset
        count), offsets row-major, zero behind a feature's own count.  A template mask is not honoured."""
        arr = _features(features)
        pf = arr.ctypes.data_as(C.POINTER(L.Feature))

        def call(o, cap, n):
            return self._lib.fpm_last_locate(self._ctx, int(source), pf, len(arr), *o, cap, n)

        def alloc(n):
            res, rw, mp, stride = self._locate_buffers(n, arr, raw, maps)
            return (res, rw, mp), (_ptr(res, L.LocateResult), _ptr(rw, L.LocateRaw), _ptr(mp, C.c_int32), stride)

        res, rw, mp = self._last("last_locate", call, (None, None, None, 0), alloc)
        return self._locate_result(res, rw, mp, raw, maps)

    def locate_at(self, src_index, lts, angles, features, raw: bool = False, maps: bool = False):
        """last_locate at poses the caller supplies, on the staged sources (fpm_locate_at); poses as patches_at.  Needs
        staged sources and a template, not a search; nothing in the matcher changes."""
        poses = _pose_args(src_index, lts, angles)
        arr = _features(features)
        res, rw, mp, stride = self._locate_buffers(poses[3], arr, raw, maps)
        rc = self._lib.fpm_locate_at(self._ctx, *poses, _ptr(arr, L.Feature), len(arr), _ptr(res, L.LocateResult),
                                     _ptr(rw, L.LocateRaw), _ptr(mp, C.c_int32), stride)
        if rc != L.FPM_OK:
            self._patch_fail(rc, "locate_at")
        return self._locate_result(res, rw, mp, raw, maps)

    def locate_profile(self):
        """``(ms, launches, bytes)`` of k_patch_locate, collected under profile(True) and cleared by profile_reset
        (fpm_locate_profile)."""
        return self._profile(self._lib.fpm_locate_profile, fail="fpm_locate_profile failed")

    # -- pixel operators (fpm_op_*) ---------------------------------------------------------------------------
    def pyr_down(self, img) -> np.ndarray:
        g = _gray(img)
        h, w = g.shape
        out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
        rc = self._check(self._lib.fpm_op_pyr_down(self._ctx, L.u8ptr(g), w, h, g.strides[0], L.u8ptr(out),
                                                   out.strides[0]), "pyr_down")
        if rc != L.FPM_OK:
            raise ValueError(self.last_error())
        return out

    def bitwise_not(self, img) -> np.ndarray:
        """255 - img by the kernel a bitwise-not search runs over its staged sources (fpm_op_bitwise_not)."""
        a = np.asarray(img)
        # a row-strided view (a column slice of a wider image) goes down as it is, with its row stride
        strided = a.ndim == 2 and a.dtype == np.uint8 and a.shape[1] > 0 and a.strides[1] == 1 and a.strides[0] >= a.shape[1]
        g = a if strided else _gray(a)
        h, w = g.shape
        out = np.zeros((h, w), np.uint8)
        rc = self._check(self._lib.fpm_op_bitwise_not(self._ctx, L.u8ptr(g), w, h, g.strides[0], L.u8ptr(out),
                                                      out.strides[0]), "bitwise_not")
        if rc != L.FPM_OK:
            raise ValueError(self.last_error())
        return out

    def to_gray(self, img, channel_order: str = "bgr", layout=None, invert: bool = False, dst=None) -> np.ndarray:
        """The gray plane match_device / stage_device search, for a host array (fpm_op_to_gray): the staging kernel over
        one image.  img is a uint8 numpy array laid out as device_layout accepts (views go down as they are, with their
        strides and their base address modulo 16, so the kernel takes the path it would take on the device); invert
        gives 255 - gray.  dst (optional): a 2-D uint8 array with unit pixel stride to write into; its bytes between
        the width and its row stride keep their values."""
        a = np.asarray(img)
        if a.dtype != np.uint8:
            raise TypeError(f"expected a uint8 array, got {a.dtype}")
        kind, h, w, ch, row, plane = device_layout(a.shape, a.strides, layout)
        fmt = device_format(kind, ch, channel_order)
        out = np.zeros((h, w), np.uint8) if dst is None else dst
        if out.dtype != np.uint8 or out.shape != (h, w) or (w > 1 and out.strides[1] != 1) or (h > 1 and out.strides[0] < w):
            raise ValueError(f"dst must be a ({h}, {w}) uint8 array with unit pixel stride")
        rc = self._check(self._lib.fpm_op_to_gray(self._ctx, a.ctypes.data, w, h, row, plane, fmt, 1 if invert else 0,
                                                  L.u8ptr(out), out.strides[0] if h > 1 else max(out.strides[0], w)),
                         "to_gray")
        if rc != L.FPM_OK:
            raise ValueError(self.last_error())
        return out

    def pyr_down2(self, img, seg_chunks: int = 0, chunk_rows: int = 0):
        """(pyrDown(img), pyrDown(pyrDown(img))) from the search's two-level pyramid kernel (chunk_rows 16 / 32 forces
        its level-1 chunk height; 0 chooses it as the search does)."""
        g = _gray(img)
        h, w = g.shape
        b = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
        c = np.zeros(((b.shape[0] + 1) // 2, (b.shape[1] + 1) // 2), np.uint8)
        rc = self._check(self._lib.fpm_op_pyr_down2(self._ctx, L.u8ptr(g), w, h, g.strides[0], L.u8ptr(b), b.strides[0],
                                                    L.u8ptr(c), c.strides[0], int(seg_chunks), int(chunk_rows)),
                         "pyr_down2")
        if rc != L.FPM_OK:
            raise ValueError(self.last_error())
        return b, c

    def warp_affine(self, img, m, dsize, border: int = 0) -> np.ndarray:
        g = _gray(img)
        h, w = g.shape
        dw, dh = dsize
        out = np.zeros((dh, dw), np.uint8)
        mm = (C.c_double * 6)(*np.asarray(m, np.float64).ravel().tolist())
        rc = self._check(self._lib.fpm_op_warp_affine(self._ctx, L.u8ptr(g), w, h, g.strides[0], mm, L.u8ptr(out),
                                                      dw, dh, out.strides[0], int(border)), "warp_affine")
        if rc != L.FPM_OK:
            raise ValueError(self.last_error())
        return out

    def ncc_map(self, img, layer: int, fold: bool) -> np.ndarray:
        g = _gray(img)
        h, w = g.shape
        tw, th = self.template_level(layer)[0].shape[::-1]
        out = np.zeros((h - th + 1, w - tw + 1), np.float32)
        rc = self._check(self._lib.fpm_op_ncc_map(self._ctx, L.u8ptr(g), w, h, g.strides[0], int(layer),
                                                  1 if fold else 0,
                                                  out.ctypes.data_as(C.POINTER(C.c_float))), "ncc_map")
        if rc != L.FPM_OK:
            raise ValueError(self.last_error())
        return out

    def refine_rois(self, levels, layer: int, lt, angles, fold, round_rois: int = 0, pixels: bool = True):
        """fpm_op_refine: one refinement layer of the search on caller-supplied ROIs.  levels: S same-size level
        images; lt: (S, n, 2) ptLT in the level's coordinates; angles: (S, n, n3) degrees, n3 in (1, 3).  Returns
        (records (S, n, n3) ROI_RECORD_DTYPE, ROI pixels (S, n, n3, th + 6, tw + 6) u8, or None where the form that
        ran keeps the ROI on the chip)."""
        gs = [_gray(g) for g in levels]
        h, w = gs[0].shape
        if any(g.shape != (h, w) or g.strides != gs[0].strides for g in gs):
            raise ValueError("all level images must have the same size")
        S = len(gs)
        p = np.ascontiguousarray(lt, np.float32).reshape(S, -1, 2)
        n = p.shape[1]
        a = np.ascontiguousarray(angles, np.float64).reshape(S, n, -1)
        n3 = a.shape[2]
        rec = np.zeros((S, n, n3), ROI_RECORD_DTYPE)
        px = None
        if pixels and self.isPatternLearned() and 0 <= layer < self.template_info()[0]:
            th, tw = self.template_level(layer)[0].shape
            px = np.zeros((S, n, n3, th + 6, tw + 6), np.uint8)
        wrote = C.c_int32()
        ptrs = (L._U8P * S)(*[L.u8ptr(g) for g in gs])
        rc = self._check(self._lib.fpm_op_refine(
            self._ctx, ptrs, S, w, h, gs[0].strides[0], int(layer), p.ctypes.data_as(C.POINTER(C.c_float)),
            a.ctypes.data_as(C.POINTER(C.c_double)), n, n3, 1 if fold else 0, int(round_rois),
            rec.ctypes.data_as(C.POINTER(L.RoiRecord)), L.u8ptr(px) if px is not None else None, C.byref(wrote)),
            "refine_rois")
        if rc != L.FPM_OK:
            raise ValueError(f"fpm_op_refine failed with {rc}: {self.last_error()}")
        return rec, (px if wrote.value else None)

    def peaks(self, maps, tw: int, th: int, cap: int, by_block: bool, mfc: bool, thr: float, overlap: float,
              form: int = 0, list_cap: int = 0, list_seed: int = 0):
        """fpm_op_peaks: the search's top-layer peak pass on caller-supplied f32 score maps (finite values), one job
        each; needs no learned template.  form 0: the split kernels, 1: the candidate-list path.  Returns (peaks: one
        PEAK_DTYPE array per map, stats: dict of the call-level entries, 'counts' and 'jobs', an (n, 4) int array, as
        include/fpm.h lists them)."""
        ms = [np.ascontiguousarray(m, np.float32) for m in maps]
        if any(m.ndim != 2 for m in ms):
            raise ValueError("maps must be 2-D")
        n = len(ms)
        mw = np.array([m.shape[1] for m in ms], np.int32)
        mh = np.array([m.shape[0] for m in ms], np.int32)
        cap = int(cap)
        pk = np.zeros((max(n, 1), max(cap, 1)), PEAK_DTYPE)
        cnt = np.full(max(n, 1), -7, np.int32)
        st = np.zeros(L.PEAKS_STATS_CALL + L.PEAKS_STATS_JOB * max(n, 1), np.int32)
        FP = C.POINTER(C.c_float)
        ptrs = (FP * max(n, 1))(*[m.ctypes.data_as(FP) for m in ms])
        IP = C.POINTER(C.c_int32)
        rc = self._lib.fpm_op_peaks(self._ctx, ptrs, mw.ctypes.data_as(IP), mh.ctypes.data_as(IP), n, int(tw), int(th),
                                    cap, 1 if by_block else 0, 1 if mfc else 0, float(thr), float(overlap), int(form),
                                    int(list_cap), int(list_seed) & 0xffffffff, pk.ctypes.data_as(C.POINTER(L.Peak)),
                                    cnt.ctypes.data_as(IP), st.ctypes.data_as(IP))
        if rc != L.FPM_OK:
            raise ValueError(f"fpm_op_peaks failed with {rc}: {self.last_error()}")
        bad = np.flatnonzero((cnt[:n] < 0) | (cnt[:n] > cap))   # (the operator pre-fills the device counts with -1)
        if len(bad):
            raise RuntimeError(f"fpm_op_peaks: no kernel wrote a valid count for jobs {bad.tolist()}")
        out = [pk[i, :int(cnt[i])].copy() for i in range(n)]
        stats = dict(kernels=int(st[0]), lds_blocks=int(st[1]), cand_lds=int(st[2]), greedy_cap=int(st[3]),
                     blk_lds=int(st[4]), list_cap=int(st[5]), max_blocks=int(st[6]), max_cells=int(st[7]),
                     counts=cnt[:n].copy(), jobs=st[L.PEAKS_STATS_CALL:].reshape(-1, L.PEAKS_STATS_JOB)[:n].copy())
        return out, stats

    def top_maps(self, form: int, thr: float = 0.0):
        """fpm_op_top_maps: the top-layer scoring of the staged batch by the search's own plan and launchers.  form 0:
        the split kernels' maps, 1: k_top_map's maps, 2: k_top_mma's candidate lists at `thr` (<= 0: the layer score).
        Returns a dict: 'geom' (n_angles, 4) int32 rows (bw, bh, mw, mh); 'stats' dict as include/fpm.h lists them;
        forms 0 and 1: 'maps'[source][angle] f32 (mh, mw) arrays; form 2: 'counts' (n_sources, n_angles) true counts,
        'index' and 'value' (n_sources, n_angles, list_cap), the first min(count, list_cap) of each job filled.  Raises
        ValueError carrying the status as `.rc` (FPM_E_SIZE: the plan does not take the matrix-core form)."""
        IP, FP = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        ns, na, lc, mf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        st = np.zeros(L.TOP_MAPS_STATS, np.int32)
        self._push()

        def call(geom, gcap, maps, mcap, cnt, idx, val, slots):
            rc = self._check(self._lib.fpm_op_top_maps(
                self._ctx, int(form), float(thr), C.byref(ns), C.byref(na), C.byref(mf), C.byref(lc), geom, gcap, maps,
                mcap, cnt, idx, val, slots, st.ctypes.data_as(IP)), "top_maps")
            if rc != L.FPM_OK:
                e = ValueError(f"fpm_op_top_maps failed with {rc}: {self.last_error()}")
                e.rc = rc
                raise e

        call(None, 0, None, 0, None, None, None, 0)
        S, nang, cap, dense = ns.value, na.value, lc.value, mf.value
        geom = np.zeros((max(nang, 1), 4), np.int32)
        out = {}
        if form in (0, 1):
            flat = np.zeros(max(S * dense, 1), np.float32)
            call(geom.ctypes.data_as(IP), nang, flat.ctypes.data_as(FP), S * dense, None, None, None, 0)
            offs = np.concatenate([[0], np.cumsum(geom[:nang, 2].astype(np.int64) * geom[:nang, 3])])
            out["maps"] = [[flat[s * dense + offs[a]:s * dense + offs[a + 1]].reshape(geom[a, 3], geom[a, 2])
                            for a in range(nang)] for s in range(S)]
        else:
            cnt = np.zeros(max(S * nang, 1), np.int32)
            idx = np.zeros(max(S * nang * cap, 1), np.int32)
            val = np.zeros(max(S * nang * cap, 1), np.float32)
            call(geom.ctypes.data_as(IP), nang, None, 0, cnt.ctypes.data_as(IP), idx.ctypes.data_as(IP),
                 val.ctypes.data_as(FP), S * nang * cap)
            out["counts"] = cnt[:S * nang].reshape(S, nang)
            out["index"] = idx[:S * nang * cap].reshape(S, nang, cap)
            out["value"] = val[:S * nang * cap].reshape(S, nang, cap)
        out["geom"] = geom[:nang]
        out["stats"] = dict(top_mma=int(st[0]), list_cap=int(st[1]), sw=int(st[2]), run=int(st[3]), nunits=int(st[4]),
                            form=int(st[5]), map_grid=int(st[6]), by_block=int(st[7]))
        return out

    TOP_FUSED_FILL = (-7, -7, -7.0)   # what top_fused leaves in a peak slot no kernel wrote (counts: -7)

    def top_fused(self):
        """fpm_op_top_fused: k_top_fused over the staged batch by the search's own plan, as the product kernel and as
        its map-writing instantiation.  Returns a dict: 'geom' (n_angles, 4) int32 rows (bw, bh, mw, mh); 'maps'
        [source][angle] f32 (mh, mw) arrays, unpainted; 'peaks' (n_sources, n_angles, cap) PEAK_DTYPE and 'counts'
        (n_sources, n_angles) of the product launch, 'dump_peaks' / 'dump_counts' of the map-writing one -- every slot
        from counts on holds TOP_FUSED_FILL; 'stats' dict as include/fpm.h lists them.  Raises ValueError carrying the
        status as `.rc` and, for FPM_E_SIZE (the fused form cannot run), the stats as `.stats`."""
        IP, FP, PP = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(L.Peak)
        ns, na, cp, mf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        st = np.zeros(L.TOP_FUSED_STATS, np.int32)
        self._push()

        def stats():
            return dict(lds=int(st[0]), static_lds=int(st[1]), lds_limit=int(st[2]), grid=int(st[3]), jobs=int(st[4]),
                        cap=int(st[5]), search_takes_it=int(st[6]), dump_static_lds=int(st[7]), copy_angles=int(st[8]),
                        bound=int(st[9]))

        def call(geom, gcap, maps, mcap, pk, cnt, dpk, dcnt, slots):
            rc = self._check(self._lib.fpm_op_top_fused(
                self._ctx, C.byref(ns), C.byref(na), C.byref(mf), C.byref(cp), geom, gcap, maps, mcap, pk, cnt, dpk, dcnt,
                slots, st.ctypes.data_as(IP)), "top_fused")
            if rc != L.FPM_OK:
                e = ValueError(f"fpm_op_top_fused failed with {rc}: {self.last_error()}")
                e.rc = rc
                e.stats = stats()
                raise e

        call(None, 0, None, 0, None, None, None, None, 0)
        S, nang, cap, dense = ns.value, na.value, cp.value, mf.value
        geom = np.zeros((max(nang, 1), 4), np.int32)
        flat = np.zeros(max(S * dense, 1), np.float32)
        pk = [np.zeros(max(S * nang * cap, 1), PEAK_DTYPE) for _ in range(2)]
        cnt = [np.full(max(S * nang, 1), self.TOP_FUSED_FILL[0], np.int32) for _ in range(2)]
        for p in pk:
            p["x"], p["y"], p["score"] = self.TOP_FUSED_FILL
        call(geom.ctypes.data_as(IP), nang, flat.ctypes.data_as(FP), S * dense, pk[0].ctypes.data_as(PP),
             cnt[0].ctypes.data_as(IP), pk[1].ctypes.data_as(PP), cnt[1].ctypes.data_as(IP), S * nang * cap)
        offs = np.concatenate([[0], np.cumsum(geom[:nang, 2].astype(np.int64) * geom[:nang, 3])])
        return dict(geom=geom[:nang], stats=stats(),
                    maps=[[flat[s * dense + offs[a]:s * dense + offs[a + 1]].reshape(geom[a, 3], geom[a, 2])
                           for a in range(nang)] for s in range(S)],
                    peaks=pk[0][:S * nang * cap].reshape(S, nang, cap), counts=cnt[0][:S * nang].reshape(S, nang),
                    dump_peaks=pk[1][:S * nang * cap].reshape(S, nang, cap),
                    dump_counts=cnt[1][:S * nang].reshape(S, nang))

    def overlap_filter(self, corners, scores, max_overlap: float, device: bool = True):
        """filterWithRotatedRect (TemplateMatcher.cpp:1133-1194) on rectangles given as rows (ltx, lty, rtx, rty, rbx,
        rby) with their scores, in the given order: (indices of the survivors, stats) -- stats as fpm_op_overlap_filter
        (path, host-decided pairs, device fallback flags, pair entries)."""
        c = np.ascontiguousarray(corners, np.float32).reshape(-1, 6)
        sc = np.ascontiguousarray(scores, np.float64).ravel()
        n = c.shape[0]
        assert sc.shape[0] == n
        keep = np.zeros(max(n, 1), np.int32)
        st = np.zeros(4, np.int32)
        nk = C.c_int32()
        rc = self._lib.fpm_op_overlap_filter(self._ctx, c.ctypes.data_as(C.POINTER(C.c_float)),
                                             sc.ctypes.data_as(C.POINTER(C.c_double)), n, float(max_overlap),
                                             1 if device else 0, keep.ctypes.data_as(C.POINTER(C.c_int32)),
                                             C.byref(nk), st.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != L.FPM_OK:
            raise ValueError(self.last_error())
        return keep[:nk.value].tolist(), st.tolist()

    def template_info(self):
        lv, border = C.c_int32(), C.c_int32()
        rc = self._lib.fpm_template_info(self._ctx, C.byref(lv), C.byref(border))
        if rc != L.FPM_OK:
            raise ValueError("template not learned")
        return lv.value, border.value

    def template_level(self, level: int):
        w, h, eq = C.c_int32(), C.c_int32(), C.c_int32()
        mean, norm, inv = C.c_double(), C.c_double(), C.c_double()
        rc = self._lib.fpm_template_level(self._ctx, level, C.byref(w), C.byref(h), C.byref(mean), C.byref(norm),
                                          C.byref(inv), C.byref(eq), None, 0)
        if rc != L.FPM_OK:
            raise ValueError("bad level")
        px = np.zeros((h.value, w.value), np.uint8)
        self._lib.fpm_template_level(self._ctx, level, C.byref(w), C.byref(h), C.byref(mean), C.byref(norm),
                                     C.byref(inv), C.byref(eq), L.u8ptr(px), px.strides[0])
        return px, mean.value, norm.value, inv.value, bool(eq.value)

    # -- kernel timing ------------------------------------------------------------------------------------------
    def profile(self, enable: bool):
        self._lib.fpm_profile_enable(self._ctx, 1 if enable else 0)

    def profile_reset(self):
        self._lib.fpm_profile_reset(self._ctx)

    def profile_last(self):
        """(device_ms, host_ms, call_ms) of the last search call (fpm_profile_last)."""
        d, h, c = C.c_double(), C.c_double(), C.c_double()
        self._lib.fpm_profile_last(self._ctx, C.byref(d), C.byref(h), C.byref(c))
        return d.value, h.value, c.value

    def profile_get(self, kernel: int):
        ms, n, b = C.c_double(), C.c_int64(), C.c_int64()
        self._lib.fpm_profile_get(self._ctx, kernel, C.byref(ms), C.byref(n), C.byref(b))
        return ms.value, n.value, b.value
