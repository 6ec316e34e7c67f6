"""The gray-value tools restated in numpy and Python (include/fpm.h, "gray-value tools"): the pixels are
oracle.warp_affine of matcher.patch_matrix's matrix (as caliper_ref takes them), a histogram is np.bincount over the used
pixels (mask_ref's crop of the mask), the statistics and Otsu's threshold are exact Python ints and Python floats (IEEE
f64) in the header's order, and the thresholded images go through blobs_ref.  Shared by tests/test_gray_host.py and
tests/test_gpu_gray.py."""
import math

import numpy as np

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import blobs_ref
from tests import mask_ref
from tests import oracle

STAT_FIELDS = ("n", "sum", "sum_sq", "min", "max", "median", "otsu", "mean", "stddev", "flags", "reserved")
INFO_FIELDS = ("n", "threshold", "flags")
MAX_N = 1 << 22


def patch(src, rect, lt, angle):
    """uint8 (h, w): the pixels I(u, v) of the rectangle (x, y, w, h) at the pose."""
    x, y, w, h = rect
    return oracle.warp_affine(src, M.patch_matrix(src.shape[1], src.shape[0], lt, angle, (x, y)), (w, h))


def used(mask, rect):
    """bool (h, w): the used pixels of the rectangle; ``mask``: the template mask (template size) or None."""
    x, y, w, h = rect
    return np.ones((h, w), bool) if mask is None else mask_ref.crop(mask, rect)


def histogram(I, m):
    """uint32 [256] of the patch I over the used pixels m."""
    return np.bincount(I[m].reshape(-1), minlength=256).astype(np.uint32)


def derive(H):
    """{field: value} of fpm_hist_stats for a histogram of 256 counts (Python ints and floats)."""
    H = [int(v) for v in H]
    assert len(H) == 256 and min(H) >= 0
    n = sum(H)
    assert n <= MAX_N
    out = dict.fromkeys(STAT_FIELDS, 0)
    out["mean"] = out["stddev"] = 0.0
    if n == 0:
        out["flags"] = L.HIST_EMPTY
        return out
    total = sum(b * H[b] for b in range(256))
    total_sq = sum(b * b * H[b] for b in range(256))
    occupied = [b for b in range(256) if H[b]]
    cum, median = 0, None
    for v in range(256):
        cum += H[v]
        if 2 * cum >= n:
            median = v
            break
    out.update(n=n, sum=total, sum_sq=total_sq, min=occupied[0], max=occupied[-1], median=median,
               mean=float(total) / float(n), stddev=math.sqrt(float(n * total_sq - total * total)) / float(n))
    if occupied[0] == occupied[-1]:
        out["otsu"], out["flags"] = occupied[0], L.HIST_FLAT
        return out
    n0 = s0 = 0
    best, otsu = None, None
    for t in range(255):
        n0 += H[t]
        s0 += t * H[t]
        if not 0 < n0 < n:
            continue
        N = n * s0 - n0 * total
        assert abs(N) < 1 << 53
        B = (float(N) * float(N)) / (float(n0) * float(n - n0))
        if best is None or B > best:
            best, otsu = B, t
    out["otsu"] = otsu
    return out


def inverted(sw, sh, rect, lt, angle):
    """The inverted patch matrix of the rectangle at the pose, as cv::warpAffine inverts it: six Python floats in
    fpm_geom.h's operation order (caliper_ref.inverted with the rectangle's origin)."""
    m = [float(v) for v in M.patch_matrix(sw, sh, lt, angle, (rect[0], rect[1])).reshape(-1)]
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0] = a11
    m[1] *= -d
    m[3] *= -d
    m[4] = a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def outside(sw, sh, rect, lt, angle):
    """The calipers' four-corner rule on the rectangle's corner pixels."""
    m = inverted(sw, sh, rect, lt, angle)
    for k in range(4):
        x = float(rect[2] - 1) if k & 1 else 0.0
        y = float(rect[3] - 1) if k & 2 else 0.0
        sx, sy = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
        if not (0.0 <= sx <= float(sw - 1) and 0.0 <= sy <= float(sh - 1)):
            return True
    return False


def threshold_image(I, m, t, polarity):
    """uint8 (h, w): e = I - t where I > t (polarity +1), t - I where I < t (-1), 0 elsewhere and at ignored pixels;
    polarity 0: no foreground."""
    d = (I.astype(np.int64) - t) * polarity
    return (np.clip(d, 0, 255) * m).astype(np.uint8)


def segment(src, rect, lt, angle, threshold, polarity, mask=None):
    """(info dict, e image) of one hit; ``threshold``: 0 .. 255 or "otsu"."""
    I, m = patch(src, rect, lt, angle), used(mask, rect)
    flags = L.GRAY_OUTSIDE if outside(src.shape[1], src.shape[0], rect, lt, angle) else 0
    t, pol = threshold, polarity
    if threshold == "otsu":
        s = derive(histogram(I, m))
        t = s["otsu"] if polarity > 0 else s["otsu"] + 1
        flags |= s["flags"]
        if s["flags"]:
            pol = 0
    return dict(n=int(m.sum()), threshold=int(t), flags=flags), threshold_image(I, m, int(t), pol)


# ---- the planted scene of the truth test: a bright part with dark discs of known radii ----------------------------------
DISCS = [(12.0, 12.0, 6.0), (30.5, 28.25, 8.25), (50.3, 12.7, 4.5), (62.0, 34.0, 3.0)]   # (cx, cy, r), template coordinates
BRIGHT, DARK = 200, 40


def planted_scene(tw, th, lt, angle, w=320, h=240, ss=8):
    """uint8 (h, w): a scene of gray BRIGHT in which the tw x th part at the pose (lt, angle) carries the DISCS at gray
    DARK, rendered by area coverage: every scene pixel is the mean of ss x ss samples of its unit square, each mapped
    into template coordinates by the pose's forward matrix and tested against the discs."""
    m = M.patch_matrix(w, h, lt, angle, (0, 0)).astype(np.float64)
    off = (np.arange(ss) + 0.5) / ss - 0.5
    ys = (np.arange(h)[:, None] + off[None, :]).reshape(-1)
    xs = (np.arange(w)[:, None] + off[None, :]).reshape(-1)
    X, Y = np.meshgrid(xs, ys)
    tx = m[0, 0] * X + m[0, 1] * Y + m[0, 2]
    ty = m[1, 0] * X + m[1, 1] * Y + m[1, 2]
    inside = np.zeros(X.shape, bool)
    for cx, cy, r in DISCS:
        inside |= (tx - cx) ** 2 + (ty - cy) ** 2 <= r * r
    cover = inside.reshape(h, ss, w, ss).mean(axis=(1, 3))
    return np.rint(BRIGHT + (DARK - BRIGHT) * cover).astype(np.uint8)


def assert_segment(got, srcs, idx, lts, angs, rect, threshold, polarity, connectivity, min_area, cap, mask, label):
    """Every field of a segmentation call (info, summary, blobs, images) against the restatement: == where the contract
    determines the output, blobs_ref.accept for a truncated hit.  Returns the e images of the reference."""
    info, summary, blobs, img = got
    assert info.dtype == M.SEGMENT_INFO_DTYPE and len(info) == len(summary) == len(blobs) == len(idx)
    x, y, w, h = rect
    assert img.shape == (len(idx), h, w) and img.dtype == np.uint8
    out = []
    for i in range(len(idx)):
        where = f"{label}: hit {i}"
        ri, e = segment(srcs[idx[i]], rect, lts[i], angs[i], threshold, polarity, mask)
        for f in INFO_FIELDS:
            assert info[i][f].item() == ri[f], f"{where}: info.{f}: {info[i][f].item()!r} != {ri[f]!r}"
        assert np.array_equal(img[i], e), f"{where}: e image differs at {np.argwhere(img[i] != e)[:4].tolist()}"
        _, recs, rs = blobs_ref.blobs(e, 0, connectivity, min_area, cap, hit=i)
        bad = blobs_ref.accept(summary[i], blobs[i], recs, rs, cap)
        assert bad is None, f"{where}: {bad}"
        out.append(e)
    return out
