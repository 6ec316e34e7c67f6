"""Inputs shared by the refinement-ROI tests (tests/test_oracle_refine.py on the CPU, tests/test_gpu_refine.py on the
device): textured images, synthetic templates of an exact size, the 49-offset position sweep and seeded random ROIs."""
import math

import numpy as np

from fastest_image_pattern_matching_amd import synth
from tests import oracle

# min_reduce_area large enough that getTopLayer stops at level 0 for every template here: the learned pyramid then is
# the template itself and `layer` 0 has exactly the size asked for
ONE_LEVEL = 1 << 30


def texture(w, h, seed):
    """Box-blurred noise with a standard deviation of about 25 grey levels (>= 20 asserted): no flat window."""
    a = synth.box_blur(synth.noise(w, h, 128, 75, seed), 3)
    assert a.std() >= 20
    return a


def layer_step(tw, th):
    """The refinement angle step of a layer with a tw x th template level, degrees (TemplateMatcher.cpp:283)."""
    return math.atan(2.0 / max(tw, th)) * 180.0 / math.pi


def learn_one_level(m, t):
    """Learn t so that its pyramid is level 0 alone (m: OracleMatcher or TemplateMatcher)."""
    if hasattr(m, "set"):
        m.set(min_reduce_area=ONE_LEVEL)
    else:
        m._params.min_reduce_area = ONE_LEVEL
    assert m.learnPattern(t)
    return m


def pasted_lt(cx, cy, tw, th, angle):
    """ptLT of a tw x th template pasted with its centre at (cx, cy) and matched at `angle` (the corner the search
    reports: rt = lt + w (cos a, sin a), lb = lt + h (-sin a, cos a), TemplateMatcher.cpp:380-390)."""
    a = math.radians(angle)
    hx, hy = (tw - 1) / 2.0, (th - 1) / 2.0
    return (cx - hx * math.cos(a) + hy * math.sin(a), cy - hx * math.sin(a) - hy * math.cos(a))


def sweep_case(tw, th, angle, seed, size=(260, 220)):
    """Scene with one copy of a textured tw x th template at `angle`, and the 49 ROI triples whose ptLT is the copy's
    shifted by every integer offset in [-3, 3]^2 with angles (angle - step, angle, angle + step).
    Returns (scene, template, lt (49, 2) f32, angles (49, 3) f64, offsets (49, 2))."""
    t = texture(tw, th, seed)
    s = texture(size[0], size[1], seed + 1)
    cx, cy = size[0] // 2, size[1] // 2
    if angle == 0.0:
        x0, y0 = cx - tw // 2, cy - th // 2
        synth.paste(s, t, x0, y0)
        lt0 = (float(x0), float(y0))
    else:
        synth.paste_rotated(s, t, cx, cy, angle)
        lt0 = pasted_lt(cx, cy, tw, th, angle)
    step = layer_step(tw, th)
    offs = [(dx, dy) for dy in range(-3, 4) for dx in range(-3, 4)]
    lt = np.array([(lt0[0] + dx, lt0[1] + dy) for dx, dy in offs], np.float32)
    ang = np.array([(angle - step, angle, angle + step)] * 49, np.float64)
    return s, t, lt, ang, offs


def random_rois(rng, w, h, tw, th, n, n3, wide=False):
    """n seeded ROIs: ptLT uniform over the image grown by the template diagonal on every side (partly and wholly
    off-image ROIs), the last one pushed wholly off the image; centre angles uniform in +-180 with the layer step, or
    (wide) triples (a, a + 20, a - 35) far apart.  Returns (lt (n, 2) f32, angles (n, n3) f64)."""
    d = math.hypot(tw + 6, th + 6)
    lt = np.stack([rng.uniform(-d, w + d, n), rng.uniform(-d, h + d, n)], 1).astype(np.float32)
    lt[-1] = (-(2 * d + 8), -(2 * d + 8))   # farther than the ROI's diagonal from the image at every angle
    a = rng.uniform(-180, 180, n)
    step = layer_step(tw, th)
    if n3 == 1:
        ang = a[:, None]
    elif wide:
        ang = np.stack([a, a + 20.0, a - 35.0], 1)
    else:
        ang = np.stack([a - step, a, a + step], 1)
    return lt, np.ascontiguousarray(ang, np.float64)


def oracle_refine(o, levels, layer, lt, angles, fold, pixels=True):
    """refine_roi over (S, n, 2) ptLT and (S, n, n3) angles: (records (S, n, n3), ROI pixels (S, n, n3, th+6, tw+6))."""
    lt = np.asarray(lt, np.float32).reshape(len(levels), -1, 2)
    S, n = lt.shape[:2]
    angles = np.asarray(angles, np.float64).reshape(S, n, -1)
    n3 = angles.shape[2]
    rec = np.zeros((S, n, n3), oracle.ROI_RECORD_DTYPE)
    px = None
    for s in range(S):
        for i in range(n):
            for j in range(n3):
                roi, _, r = o.refine_roi(levels[s], layer, lt[s, i], angles[s, i, j], fold)
                if px is None:
                    px = np.zeros((S, n, n3) + roi.shape, np.uint8)
                px[s, i, j] = roi
                rec[s, i, j] = r
    return rec, px


# ---- host mirrors of the kernels' integer layout rules (fpm_kernels.hip): which form and path a shape takes ---------
ROI_T, ROI_FT, FT_PITCH, MMA_ROWS, BAND_ROWS, SMALL_LDS_MAX = 32, 4096, 68, 16, 32, 72 * 1024


def roi_pitch(tw):   # roi_pitch_calc
    q = (max(tw + 6 + 16, 64 * ((tw + 63) // 64) + 22) + 15) // 16
    return (q + 1 if q % 2 == 0 else q) * 16


def tmpl_lds_pitch(tp8):
    q = tp8 // 16
    return (q + 1 if q % 2 == 0 else q) * 16


def small_footprint_bound(rw, rh):
    n = (rw - 1) ** 2 + (rh - 1) ** 2
    d = math.isqrt(n)
    d = (d if d * d == n else d + 1) + 2
    return ((d + 16) * (d + 6) + 15) & ~15


def small_layout(tw, th, nw=4):
    """(total LDS bytes, U bytes past the ROI rows, footprint bound) of k_roi_small's workgroup (small_layout)."""
    sbp, tbp, rh = roi_pitch(tw), tmpl_lds_pitch(64 * ((tw + 63) // 64)), th + 6
    th16 = (th + MMA_ROWS - 1) // MMA_ROWS * MMA_ROWS
    u = ((rh + 16) * sbp + 15) & ~15
    fb = small_footprint_bound(tw + 6, th + 6)
    ub = max(th16 * tbp, min(fb, nw * ROI_FT))
    tab = u + ub
    sums = tab + 4 * (2 * sbp + 2 * ((rh + 3) & ~3))
    rs_size = 4 * BAND_ROWS * 49
    after = sums + 4 * (2 * rh + 2 * 7 * rh) + 8 * 49 * 2
    if th16 * tbp + rs_size <= sums - u:
        sc = after
    else:
        sc = after + rs_size
    return sc + 4 * 64 + 4 * th16, ub, fb


def roi_small_fits(tw, th):
    return th <= 256 and small_layout(tw, th)[0] <= SMALL_LDS_MAX


def _rotate_pt(ix, iy, ox, oy, c, s):   # fpm_geom.h rotate_pt: float inputs, double arithmetic, float result
    f = np.float32
    h = float(f(oy * f(2)))
    y1, y2 = h - float(iy), h - float(oy)
    dx = float(f(ix - ox))
    x = dx * c - (y1 - float(oy)) * s + float(ox)
    y = -(dx * s + (y1 - float(oy)) * c + y2) + h
    return f(x), f(y)


def tile_boxes(W, H, tw, th, lt, angle):
    """The footprint boxes k_roi_tables gives the 32 x 32 tiles of one ROI (roi_tables_fill): per tile
    (bxa, by0, wpr, fth, any, in_lds)."""
    f = np.float32
    r = angle * (math.pi / 180.0)
    c, s = math.cos(r), math.sin(r)
    cx, cy = f(f(W - 1) / f(2)), f(f(H - 1) / f(2))
    lx, ly = _rotate_pt(f(lt[0]), f(lt[1]), cx, cy, c, s)
    M = [c, s, (1 - c) * float(cx) - s * float(cy), -s, c, s * float(cx) + (1 - c) * float(cy)]
    M[2] -= float(f(lx - f(3)))
    M[5] -= float(f(ly - f(3)))
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = M[4] * D, M[0] * D
    M[0], M[1], M[3], M[4] = a11, M[1] * -D, M[3] * -D, a22
    M[2], M[5] = -M[0] * M[2] - M[1] * M[5], -M[3] * M[2] - M[4] * M[5]
    RW, RH = tw + 6, th + 6
    out = []
    for ry0 in range(0, RH, ROI_T):
        for cx0 in range(0, RW, ROI_T):
            xs, ys = [], []
            for cc in (cx0, min(cx0 + ROI_T, RW) - 1):
                for rr in (ry0, min(ry0 + ROI_T, RH) - 1):
                    ad, bd = round(M[0] * cc * 1024), round(M[3] * cc * 1024)
                    x0 = round((M[1] * rr + M[2]) * 1024) + 16
                    y0 = round((M[4] * rr + M[5]) * 1024) + 16
                    xs.append(((x0 + ad) >> 5) >> 5)
                    ys.append(((y0 + bd) >> 5) >> 5)
            bx0, by0 = max(min(xs) - 1, 0), max(min(ys) - 1, 0)
            bx1, by1 = min(max(xs) + 2, W - 1), min(max(ys) + 2, H - 1)
            any_ = bx0 <= bx1 and by0 <= by1
            bxa = bx0 & ~3
            wpr = (bx1 - bxa + 4) >> 2 if any_ else 0
            fth = by1 - by0 + 1 if any_ else 0
            out.append((bxa, by0, wpr, fth, any_, wpr <= 16 and FT_PITCH * fth <= ROI_FT))
    return out


def warp3_fallback_tiles(W, H, tw, th, lt, angles3):
    """Tiles of a candidate's three ROIs for which k_roi_warp3 cannot stage one union footprint (the boxes that stage
    into LDS span more than 16 dwords = 64 px or more than ROI_FT / pitch = 60 rows) and samples each ROI from its own
    box instead."""
    boxes = [tile_boxes(W, H, tw, th, lt, a) for a in angles3]
    n = 0
    for t3 in zip(*boxes):
        lds = [b for b in t3 if b[4] and b[5]]
        if not lds:
            continue
        ux0, uy0 = min(b[0] for b in lds), min(b[1] for b in lds)
        ux1, uy1 = max(b[0] + 4 * b[2] for b in lds), max(b[1] + b[3] for b in lds)
        if (ux1 - ux0) >> 2 > 16 or FT_PITCH * (uy1 - uy0) > ROI_FT:
            n += 1
    return n
