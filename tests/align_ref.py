"""The pose alignment restated in numpy (include/fpm.h, "pose alignment"): exact integers for the eleven sums, np.float64
operations in the header's order for the solve, and the iteration around them.  The loop samples with
oracle.warp_affine of matcher.patch_matrix's matrix and takes its tail -- the solve and the pose update -- from the
library's own host entries (fpm_align_solve, fpm_align_update; tests/test_align_host.py pins those).  Shared by
tests/test_align_host.py and tests/test_gpu_align.py."""
import math

import numpy as np

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import compare_ref
from tests import oracle

SUM_FIELDS = ("n_used", "h_xx", "h_xy", "h_yy", "h_xt", "h_yt", "h_tt", "g_x", "g_y", "g_t", "ssd")
RESULT_FIELDS = ("lt_x", "lt_y", "angle", "ssd_start", "ssd", "n_used", "evals", "best_eval", "flags", "reserved")
MAX_AREA, MAX_SIDE = 1 << 20, 4096


def sums(I, T, rect, lut=None):
    """{field: Python int} of patch ``I`` (h, w) against the whole template ``T`` for the rectangle (x, y, w, h);
    ``lut``: the hit's uint8 [256] table or None."""
    x, y, w, h = rect
    th, tw = T.shape
    assert I.shape == (h, w) and I.dtype == T.dtype == np.uint8
    assert 0 <= x and 0 <= y and x + w <= tw and y + h <= th and 1 <= w * h <= MAX_AREA and max(w, h) <= MAX_SIDE
    t = T.astype(np.int64)
    gx, gy = np.zeros_like(t), np.zeros_like(t)
    used = np.zeros(t.shape, bool)
    if tw >= 3 and th >= 3:
        gx[:, 1:-1] = t[:, 2:] - t[:, :-2]        # twice the derivative, from the whole template
        gy[1:-1, :] = t[2:, :] - t[:-2, :]
        used[1:-1, 1:-1] = True                   # all four neighbours inside the template
    crop = (slice(y, y + h), slice(x, x + w))
    u = used[crop].astype(np.int64)
    tx, ty = gx[crop] * u, gy[crop] * u
    v = (lut[I] if lut is not None else I).astype(np.int64)
    r = (v - t[crop]) * u
    X = (2 * np.arange(w, dtype=np.int64) - (w - 1))[None, :]
    Y = (2 * np.arange(h, dtype=np.int64) - (h - 1))[:, None]
    jt = X * ty - Y * tx
    # every product is below 2^41 and, under the caps, every sum below 2^62: int64 sums are exact
    out = dict(n_used=u.sum(), h_xx=(tx * tx).sum(), h_xy=(tx * ty).sum(), h_yy=(ty * ty).sum(), h_xt=(tx * jt).sum(),
               h_yt=(ty * jt).sum(), h_tt=(jt * jt).sum(), g_x=(tx * r).sum(), g_y=(ty * r).sum(), g_t=(jt * r).sum(),
               ssd=(r * r).sum())
    return {k: int(val) for k, val in out.items()}


def solve(s):
    """(du, dv, dphi, singular) from the integer sums, np.float64 in the header's order."""
    zero = (0.0, 0.0, 0.0, True)
    if s["n_used"] < 3:
        return zero
    f = {k: np.float64(s[k]) for k in SUM_FIELDS}
    hxx, hxy, hyy, hxt, hyt, htt = f["h_xx"], f["h_xy"], f["h_yy"], f["h_xt"], f["h_yt"], f["h_tt"]
    gx, gy, gt = f["g_x"], f["g_y"], f["g_t"]
    with np.errstate(all="ignore"):
        c00, c01, c02 = hyy * htt - hyt * hyt, hxt * hyt - hxy * htt, hxy * hyt - hxt * hyy
        c11, c12, c22 = hxx * htt - hxt * hxt, hxy * hxt - hxx * hyt, hxx * hyy - hxy * hxy
        det = (hxx * c00 + hxy * c01) + hxt * c02
        if not (det > 0.0) or not np.isfinite(det):
            return zero
        q0 = -(((c00 * gx + c01 * gy) + c02 * gt) / det)
        q1 = -(((c01 * gx + c11 * gy) + c12 * gt) / det)
        q2 = -(((c02 * gx + c12 * gy) + c22 * gt) / det)
        du, dv, dphi = np.float64(2.0) * q0, np.float64(2.0) * q1, np.float64(4.0) * q2
    if not (np.isfinite(du) and np.isfinite(dv) and np.isfinite(dphi)):
        return zero
    return float(du), float(dv), float(dphi), False


def step_too_far(rect, du, dv, dphi, max_step):
    """Would the step move a corner of the rectangle by more than max_step?  Python floats are IEEE f64 and math.cos /
    math.sin are the C library's: the header's expressions, value for value."""
    _, _, w, h = rect
    c, s, hx, hy = math.cos(dphi), math.sin(dphi), (w - 1) / 2.0, (h - 1) / 2.0
    lim = max_step * max_step
    for k in range(4):
        ex, ey = (hx if k & 1 else -hx), (hy if k & 2 else -hy)
        mx, my = ((c * ex - s * ey) - ex) + du, ((s * ex + c * ey) - ey) + dv
        if mx * mx + my * my > lim:
            return True
    return False


def patch(src, rect, lt, angle):
    x, y, w, h = rect
    return oracle.warp_affine(src, M.patch_matrix(src.shape[1], src.shape[0], lt, angle, (x, y)), (w, h))


def table(src, T, rect, lt, angle):
    """The hit's normalising table, as fpm_last_compare builds it at that pose."""
    x, y, w, h = rect
    I = patch(src, rect, lt, angle)
    return compare_ref.derive(*compare_ref.sums(I, np.ascontiguousarray(T[y:y + h, x:x + w])), True)[3]


def loop(src, T, rect, lt, angle, iters, max_step=2.0, normalize=False):
    """{field: value} of fpm_align_result for one hit.  The freeze on leaving the samplers' 2^20-pixel range is not
    restated: no pose of the tests comes near it."""
    sh, sw = src.shape
    lt = (float(np.float32(lt[0])), float(np.float32(lt[1])))
    lut = table(src, T, rect, lt, angle) if normalize else None
    cur = best = (lt, float(angle))
    o = dict(flags=0, best_eval=0, evals=1, reserved=0)
    frozen = moved = False
    for k in range(iters + 1):
        s = sums(patch(src, rect, *cur), T, rect, lut)
        if k == 0:
            o.update(ssd_start=s["ssd"], ssd=s["ssd"], n_used=s["n_used"])
        elif moved:
            o["evals"] = k + 1
            if s["ssd"] < o["ssd"]:
                o.update(ssd=s["ssd"], n_used=s["n_used"], best_eval=k)
                best = cur
        moved = False
        if k == iters or frozen:
            continue
        du, dv, dphi, singular = M.align_solve(s)
        if singular:
            frozen, o["flags"] = True, o["flags"] | L.ALIGN_SINGULAR
        elif step_too_far(rect, du, dv, dphi, max_step):
            frozen, o["flags"] = True, o["flags"] | L.ALIGN_STEP_CLAMPED
        else:
            cur = M.align_update(sw, sh, rect, cur[0], cur[1], du, dv, dphi)
            moved = True
    if o["best_eval"] == 0:
        o["flags"] |= L.ALIGN_KEPT_START
    o.update(lt_x=best[0][0], lt_y=best[0][1], angle=best[1])
    return o


def centre(src_shape, rect, lt, angle):
    """Where the pose puts the rectangle's centre in the source: the inverted patch matrix at ((w - 1) / 2, (h - 1) / 2)."""
    x, y, w, h = rect
    m = np.vstack([M.patch_matrix(src_shape[1], src_shape[0], lt, angle, (x, y)), [0.0, 0.0, 1.0]])
    return (np.linalg.inv(m) @ np.array([(w - 1) / 2.0, (h - 1) / 2.0, 1.0]))[:2]


def assert_rows(got, exp, fields, label):
    """Every field of every row equal (==)."""
    assert len(got) == len(exp), f"{label}: {len(got)} rows vs {len(exp)}"
    for i, e in enumerate(exp):
        for f in fields:
            g = got[i][f].item()
            assert g == e[f], f"{label}: row {i} field {f}: {g!r} != {e[f]!r}"


# ---- the planted scenes of the convergence tests ------------------------------------------------------------------
TW, TH = 71, 45
PLANTED = [((120.3, 80.7), 17.0), ((150.6, 100.2), -123.5)]   # two non-trivial angles, sub-pixel ptLT
_planted = {}


def smooth_scene(w=320, h=240, seed=13, blobs=120, smin=3.0, smax=8.0):
    """A smooth synthetic scene: Gaussian blobs on gray, textured everywhere (a flat neighbourhood leaves the angle
    loose, and the loop then creeps along a valley instead of converging)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 128.0)
    for _ in range(blobs):
        cx, cy, s, a = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(smin, smax), rng.uniform(-70, 70)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def planted():
    """(scene, [(template, lt, angle)]): every template is the TW x TH patch cut from the scene at its pose, so at that
    pose the patch equals the template."""
    if not _planted:
        s = smooth_scene()
        _planted["v"] = (s, [(patch(s, (0, 0, TW, TH), lt, a), lt, a) for lt, a in PLANTED])
    return _planted["v"]


def starts(lt, angle):
    """The planted pose plus (+-0.45, -+0.3) px and +-0.25 degrees."""
    return [((lt[0] + sg * 0.45, lt[1] - sg * 0.3), angle + sg * 0.25) for sg in (1, -1)]
