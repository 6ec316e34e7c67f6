"""The template-mask contract restated on top of the references that exist (include/fpm.h, "template masks"): a masked
pixel is a pixel that adds nothing.  compare_ref, align_ref, model_ref and blobs_ref are imported and left as they are.
  comparison: compare_ref.derive of the sums of the used pixels taken as 1-D arrays; deviations, count and box on the 2-D
              image under the mask
  alignment:  align_ref.sums' expressions with used &= mask, inside align_ref.loop's iteration
  inspection: model_ref.inspect with the excess zeroed under the mask; blobs are blobs_ref on that excess image
Shared by tests/test_mask_host.py and tests/test_gpu_masks.py."""
import numpy as np

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import align_ref
from tests import compare_ref
from tests import model_ref
from tests import oracle

IDENTITY = np.arange(256, dtype=np.uint8)


def crop(mask, rect):
    """bool (h, w): the mask (template size, any integer or bool type; nonzero = used) under the rectangle."""
    x, y, w, h = rect
    return np.ascontiguousarray(np.asarray(mask)[y:y + h, x:x + w] != 0)


def _box(sel):
    h, w = sel.shape
    if not sel.any():
        return (w, h, -1, -1)
    ys, xs = np.nonzero(sel)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def derive(I, T, m, normalize):
    """(n, sums (5), zncc, gain, offset, lut) of patch I against template crop T over the used pixels m (bool)."""
    n = int(m.sum())
    if n == 0:
        return 0, (0, 0, 0, 0, 0), 0.0, 1.0, 0.0, IDENTITY
    s = compare_ref.sums(np.ascontiguousarray(I[m]), np.ascontiguousarray(T[m]))
    assert s[0] == n
    return (n, s[1:]) + compare_ref.derive(*s, normalize)


def table(I, T, m):
    """The normalising table of a masked call: from the sums of the used pixels."""
    return derive(I, T, m, True)[5]


def compare(I, T, m, threshold, normalize):
    """({field: value}, difference image) of patch I against template crop T under the crop m of the mask."""
    n, (si, sii, st, stt, sit), zncc, gain, offset, lut = derive(I, T, m, normalize)
    d = np.abs(lut[I].astype(np.int32) - T.astype(np.int32)) * m
    over = d > threshold
    box = _box(over)
    row = dict(n=n, sum_i=si, sum_ii=sii, sum_t=st, sum_tt=stt, sum_it=sit, sum_abs=int(d.sum()), n_over=int(over.sum()),
               max_abs=int(d.max()), x0=box[0], y0=box[1], x1=box[2], y1=box[3], zncc=zncc, gain=gain, offset=offset)
    return row, d.astype(np.uint8)


def align_sums(I, T, rect, mask, lut=None):
    """align_ref.sums with used &= mask: {field: Python int}.  ``mask``: the whole mask (template size), or None."""
    x, y, w, h = rect
    th, tw = T.shape
    assert I.shape == (h, w) and I.dtype == T.dtype == np.uint8
    t = T.astype(np.int64)
    gx, gy = np.zeros_like(t), np.zeros_like(t)
    used = np.zeros(t.shape, bool)
    if tw >= 3 and th >= 3:
        gx[:, 1:-1] = t[:, 2:] - t[:, :-2]        # from the whole template: the neighbours' mask bytes do not matter
        gy[1:-1, :] = t[2:, :] - t[:-2, :]
        used[1:-1, 1:-1] = True
    if mask is not None:
        used &= np.asarray(mask) != 0
    c = (slice(y, y + h), slice(x, x + w))
    u = used[c].astype(np.int64)
    tx, ty = gx[c] * u, gy[c] * u
    v = (lut[I] if lut is not None else I).astype(np.int64)
    r = (v - t[c]) * u
    X = (2 * np.arange(w, dtype=np.int64) - (w - 1))[None, :]
    Y = (2 * np.arange(h, dtype=np.int64) - (h - 1))[:, None]
    jt = X * ty - Y * tx
    out = dict(n_used=u.sum(), h_xx=(tx * tx).sum(), h_xy=(tx * ty).sum(), h_yy=(ty * ty).sum(), h_xt=(tx * jt).sum(),
               h_yt=(ty * jt).sum(), h_tt=(jt * jt).sum(), g_x=(tx * r).sum(), g_y=(ty * r).sum(), g_t=(jt * r).sum(),
               ssd=(r * r).sum())
    return {k: int(val) for k, val in out.items()}


def align_table(src, T, rect, mask, lt, angle):
    """The hit's normalising table as the masked fpm_last_compare builds it at that pose."""
    x, y, w, h = rect
    I = align_ref.patch(src, rect, lt, angle)
    return table(I, np.ascontiguousarray(T[y:y + h, x:x + w]), crop(mask, rect))


def align_loop(src, T, rect, mask, lt, angle, iters, max_step=2.0, normalize=False):
    """align_ref.loop's iteration around align_sums: {field: value} of fpm_align_result for one hit."""
    sh, sw = src.shape
    lt = (float(np.float32(lt[0])), float(np.float32(lt[1])))
    lut = None
    if normalize:
        lut = align_table(src, T, rect, mask, lt, angle) if mask is not None else align_ref.table(src, T, rect, lt, angle)
    cur = best = (lt, float(angle))
    o = dict(flags=0, best_eval=0, evals=1, reserved=0)
    frozen = moved = False
    for k in range(iters + 1):
        s = align_sums(align_ref.patch(src, rect, *cur), T, rect, mask, lut)
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
        elif align_ref.step_too_far(rect, du, dv, dphi, max_step):
            frozen, o["flags"] = True, o["flags"] | L.ALIGN_STEP_CLAMPED
        else:
            cur = M.align_update(sw, sh, rect, cur[0], cur[1], du, dv, dphi)
            moved = True
    if o["best_eval"] == 0:
        o["flags"] |= L.ALIGN_KEPT_START
    o.update(lt_x=best[0][0], lt_y=best[0][1], angle=best[1])
    return o


def sample(I, T, m, normalize):
    """(v, gain, offset): what the model sees of patch I under the mask crop m -- model_ref.sample with the masked table."""
    if not normalize:
        return I, 1.0, 0.0
    _, _, _, gain, offset, lut = derive(I, T, m, True)
    return lut[I], gain, offset


def inspect(v, lo, hi, m, gain=1.0, offset=0.0):
    """({field: value}, excess image): model_ref.inspect with the excess zeroed under the mask crop m."""
    _, e = model_ref.inspect(v, lo, hi, gain, offset)
    e = e * m.astype(np.uint8)
    u, l, h_ = v.astype(np.int32), lo.astype(np.int32), hi.astype(np.int32)
    low, high = (u < l) & m, (u >= l) & (u > h_) & m
    assert np.array_equal(e > 0, low | high)
    box = _box(e > 0)
    row = dict(n=int(m.sum()), sum_excess=int(e.astype(np.int64).sum()), n_low=int(low.sum()), n_high=int(high.sum()),
               max_excess=int(e.max()), x0=box[0], y0=box[1], x1=box[2], y1=box[3], gain=gain, offset=offset)
    return row, e


def ellipse(w, h, cx, cy, rx, ry, grow=0.0):
    """bool (h, w): ((u - cx) / rx)^2 + ((v - cy) / ry)^2 <= 1, the half-axes grown by ``grow`` pixels."""
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    return ((u - cx) / (rx + grow)) ** 2 + ((v - cy) / (ry + grow)) ** 2 <= 1.0


# ---- the planted scene of the masked convergence tests -----------------------------------------------------------------
_planted = {}


def planted():
    """(mask, [(scene, template, lt, angle)]): align_ref's 71 x 45 templates at their planted poses in smooth_scene(13);
    the mask is the ellipse ((u - 35) / 30)^2 + ((v - 22) / 17)^2 <= 1; each scene keeps the ellipse grown by 1.5 px at
    the planted pose from seed 13, everything else comes from smooth_scene(seed=29)."""
    if not _planted:
        tw, th = align_ref.TW, align_ref.TH
        part, others = align_ref.smooth_scene(seed=13), align_ref.smooth_scene(seed=29)
        mask = ellipse(tw, th, 35, 22, 30, 17)
        grown = ellipse(tw, th, 35, 22, 30, 17, 1.5).astype(np.uint8) * np.uint8(255)
        out = []
        for lt, a in align_ref.PLANTED:
            t = align_ref.patch(part, (0, 0, tw, th), lt, a)
            # the grown ellipse carried into the scene at the planted pose: the forward warp of its image
            fwd = np.vstack([M.patch_matrix(part.shape[1], part.shape[0], lt, a), [0.0, 0.0, 1.0]])
            keep = oracle.warp_affine(grown, np.linalg.inv(fwd)[:2], (part.shape[1], part.shape[0])) >= 128
            out.append((np.where(keep, part, others).astype(np.uint8), t, lt, a))
        _planted["v"] = (mask, out)
    return _planted["v"]


PLANT_RECT = (0, 0, align_ref.TW, align_ref.TH)


def centre_error(scene, lt, angle, truth):
    """Distance in source pixels of where the pose puts the template's centre from ``truth``."""
    return float(np.hypot(*(align_ref.centre(scene.shape, PLANT_RECT, lt, angle) - truth)))


def planted_alignments():
    """[(start error, unmasked end error, masked end error)] over the four starts of planted(), from the CPU reference
    (iters = 3); the unmasked loop is align_ref.loop's, and the restated loop without a mask must equal it."""
    mask, scenes = planted()
    out = []
    for scene, t, lt, a in scenes:
        truth = align_ref.centre(scene.shape, PLANT_RECT, lt, a)
        for slt, sa in align_ref.starts(lt, a):
            un = align_ref.loop(scene, t, PLANT_RECT, slt, sa, 3)
            mk = align_loop(scene, t, PLANT_RECT, mask, slt, sa, 3)
            assert un == align_loop(scene, t, PLANT_RECT, None, slt, sa, 3)
            out.append((centre_error(scene, slt, sa, truth), centre_error(scene, (un["lt_x"], un["lt_y"]), un["angle"], truth),
                        centre_error(scene, (mk["lt_x"], mk["lt_y"]), mk["angle"], truth)))
    return out


def box_reaches_a_corner(row, w, h):
    """Is a corner of the box of an inspection or comparison row a corner pixel of its w x h rectangle?"""
    box = {(row["x0"], row["y0"]), (row["x1"], row["y0"]), (row["x0"], row["y1"]), (row["x1"], row["y1"])}
    return any((x, y) in box for x in (0, w - 1) for y in (0, h - 1))
