"""The edge probes restated in numpy and math (include/fpm.h, "edge probes"): the probe's frame, the composition with the
hit's inverted matrix, the derivation, the summary and both fits in Python floats (IEEE f64; math.cos / math.sin /
math.atan2 / math.sqrt are the C library's) in the header's order; the sampler written out in integers (ad, X0, the four
taps with their weights, (.. + 2^14) >> 15, border 0); step, edge and select rules on int64.  Shared by
tests/test_probe_host.py, tests/test_gpu_probes.py and tests/test_gpu_probe_entries.py."""
import math

import numpy as np

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests.caliper_ref import inverted

D2R = math.pi / 180.0
R2D = 180.0 / math.pi
AB_BITS, INTER_BITS = 10, 5
AB_SCALE, INTER_TAB = 1 << AB_BITS, 1 << INTER_BITS
ROUND_DELTA = AB_SCALE // INTER_TAB // 2
RESULT_INTS = ("index", "n_edges", "d", "flags")
RESULT_FIELDS = RESULT_INTS + ("dev", "contrast", "tx", "ty", "sx", "sy")
SUMMARY_FIELDS = ("n_found", "n_missing", "n_ambiguous", "n_outside", "worst", "reserved", "sum_dev", "sum_dev_sq",
                  "max_abs_dev", "lt_x", "lt_y", "angle")
SELECT = {"nearest": L.PROBE_NEAREST, "strongest": L.PROBE_STRONGEST, "first": L.PROBE_FIRST, "last": L.PROBE_LAST}


def params(length, width, half=2, contrast=12, polarity=0, select="nearest"):
    """The call's parameters as a plain dict (the reference never goes through the library's record)."""
    return dict(length=int(length), width=int(width), half=int(half), contrast=int(contrast), polarity=int(polarity),
                select=SELECT.get(select, select))


def record(prm):
    return M.probe_params(**prm)


def probes_array(ps):
    """[(x, y, phi)] as the library's PROBE_DTYPE array."""
    out = np.zeros(len(ps), M.PROBE_DTYPE)
    for k, (x, y, phi) in enumerate(ps):
        out[k] = (x, y, phi)
    return out


def geom(p, prm):
    """(cp, sp, ox, oy, hl, hw) of probe p = (x, y, phi)."""
    x, y, phi = float(p[0]), float(p[1]), float(p[2])
    hl, hw = (prm["length"] - 1) / 2.0, (prm["width"] - 1) / 2.0
    rp = phi * D2R
    cp, sp = math.cos(rp), math.sin(rp)
    return cp, sp, x - (hl * cp - hw * sp), y - (hl * sp + hw * cp), hl, hw


def compose(m, g):
    """The composed matrix N, six Python floats, every product and sum rounded once in the header's order."""
    cp, sp, ox, oy = g[:4]
    return [m[0] * cp + m[1] * sp,
            m[1] * cp - m[0] * sp,
            (m[0] * ox + m[1] * oy) + m[2],
            m[3] * cp + m[4] * sp,
            m[4] * cp - m[3] * sp,
            (m[3] * ox + m[4] * oy) + m[5]]


def matrix(sw, sh, lt, angle, p, prm):
    return compose(inverted(sw, sh, lt, angle), geom(p, prm))


def sample(src, N, length, width):
    """(I, outside): the int64 pixels [K, width, length] of K composed matrices N [K, 6] on the u8 image src, and the
    bool [K] of FPM_PROBE_OUTSIDE.  Every step is the sampler's integer arithmetic."""
    src = np.asarray(src)
    sh, sw = src.shape
    N = np.asarray(N, np.float64).reshape(-1, 6)
    u = np.arange(length, dtype=np.float64)[None, :]
    v = np.arange(width, dtype=np.float64)[None, :]
    ad = np.rint(N[:, 0:1] * u * AB_SCALE).astype(np.int64)
    bd = np.rint(N[:, 3:4] * u * AB_SCALE).astype(np.int64)
    X0 = np.rint((N[:, 1:2] * v + N[:, 2:3]) * AB_SCALE).astype(np.int64) + ROUND_DELTA
    Y0 = np.rint((N[:, 4:5] * v + N[:, 5:6]) * AB_SCALE).astype(np.int64) + ROUND_DELTA
    X = (X0[:, :, None] + ad[:, None, :]) >> (AB_BITS - INTER_BITS)
    Y = (Y0[:, :, None] + bd[:, None, :]) >> (AB_BITS - INTER_BITS)
    ox, oy = X >> INTER_BITS, Y >> INTER_BITS
    sx, sy = np.clip(ox, -32768, 32767), np.clip(oy, -32768, 32767)
    fx, fy = X & (INTER_TAB - 1), Y & (INTER_TAB - 1)
    acc = np.zeros(X.shape, np.int64)
    for dy, dx, w in ((0, 0, (INTER_TAB - fy) * (INTER_TAB - fx) * 32), (0, 1, (INTER_TAB - fy) * fx * 32),
                      (1, 0, fy * (INTER_TAB - fx) * 32), (1, 1, fy * fx * 32)):
        x, y = sx + dx, sy + dy
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        val = np.where(inside, src[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int64), 0)   # border 0
        acc += val * w
    I = (acc + (1 << 14)) >> 15
    corner = (ox < 0) | (ox > sw - 2) | (oy < 0) | (oy > sh - 2)
    cu, cv = [0, length - 1], [0, width - 1]
    outside = corner[:, cv][:, :, cu].any(axis=(1, 2))
    return I, outside


def steps(P, prm):
    """int64 [length + 1]: D[0 .. L], 0 outside s .. L - s."""
    P = np.asarray(P, np.int64)
    n, s = prm["length"], prm["half"]
    assert P.shape == (n,)
    D = np.zeros(n + 1, np.int64)
    S = np.concatenate([[0], np.cumsum(P)])
    i = np.arange(s, n - s + 1)
    D[i] = (S[i + s] - S[i]) - (S[i] - S[i - s])
    return D


def edges_all(P, prm):
    """Every edge as (index, d_prev, d, d_next) Python ints, in ascending index."""
    D = steps(P, prm)
    n, s, thr = prm["length"], prm["half"], prm["contrast"] * prm["half"] * prm["width"]
    out = []
    for i in range(s, n - s + 1):
        for p in (1, -1):
            if prm["polarity"] not in (0, p):
                continue
            a, am, ap = p * D[i], p * D[i - 1], p * D[i + 1]
            if a >= thr and a > am and a >= ap:
                out.append((i, int(D[i - 1]), int(D[i]), int(D[i + 1])))
    return out


def select(edges, prm):
    """The raw record (index, n_edges, d_prev, d, d_next) of a probe with the edges ``edges``."""
    if not edges:
        return (0, 0, 0, 0, 0)
    n = prm["length"]
    sel = prm["select"]
    if sel == L.PROBE_NEAREST:
        e = min(edges, key=lambda r: (abs(2 * r[0] - n), r[0]))
    elif sel == L.PROBE_STRONGEST:
        e = min(edges, key=lambda r: (-abs(r[2]), r[0]))
    elif sel == L.PROBE_FIRST:
        e = edges[0]
    else:
        e = edges[-1]
    return (e[0], len(edges), e[1], e[2], e[3])


def edges_raw(P, prm):
    return select(edges_all(P, prm), prm)


def derive(p, prm, lt, angle, raw, flags=0):
    """{field: value} of fpm_probe_result for one raw record (index, n_edges, d_prev, d, d_next)."""
    i, n_edges, dp, d, dn = raw
    if i == 0:
        return dict(index=0, n_edges=0, d=0, flags=flags, dev=0.0, contrast=0.0, tx=0.0, ty=0.0, sx=0.0, sy=0.0, delta=0.0)
    g = 1 if d > 0 else -1
    am, a0, ap = g * dp, g * d, g * dn
    den = (am - a0) + (ap - a0)
    assert den < 0
    delta = 0.5 * float(am - ap) / float(den)
    t = (float(i) - 0.5) + delta
    cp, sp, ox, oy, hl, hw = geom(p, prm)
    ra = angle * D2R
    c, s = math.cos(ra), math.sin(ra)
    ltx, lty = float(np.float32(lt[0])), float(np.float32(lt[1]))
    tx, ty = ox + (t * cp - hw * sp), oy + (t * sp + hw * cp)
    return dict(index=i, n_edges=n_edges, d=d, flags=flags, dev=t - hl, contrast=float(a0) / float(prm["half"] * prm["width"]),
                tx=tx, ty=ty, sx=ltx + (tx * c - ty * s), sy=lty + (tx * s + ty * c), delta=delta)


def summarize(results, lt, angle):
    s = dict(n_found=0, n_missing=0, n_ambiguous=0, n_outside=0, worst=-1, reserved=0, sum_dev=0.0, sum_dev_sq=0.0,
             max_abs_dev=0.0, lt_x=float(np.float32(lt[0])), lt_y=float(np.float32(lt[1])), angle=float(angle))
    for k, r in enumerate(results):
        if r["flags"] & L.PROBE_OUTSIDE:
            s["n_outside"] += 1
        if r["index"] < 1:
            s["n_missing"] += 1
            continue
        s["n_found"] += 1
        if r["n_edges"] > 1:
            s["n_ambiguous"] += 1
        a = abs(r["dev"])
        if s["worst"] < 0 or a > s["max_abs_dev"]:
            s["worst"], s["max_abs_dev"] = k, a
        s["sum_dev"] += r["dev"]
        s["sum_dev_sq"] += r["dev"] * r["dev"]
    return s


def measure(src, lt, angle, ps, prm):
    """(summary dict, [result dicts], profiles int64 [K, length]) of the probes ps on a hit at (lt, angle) on src."""
    m = inverted(src.shape[1], src.shape[0], lt, angle)
    N = [compose(m, geom(p, prm)) for p in ps]
    I, out = sample(src, N, prm["length"], prm["width"])
    P = I.sum(axis=1)
    res = [derive(p, prm, lt, angle, edges_raw(P[k], prm), L.PROBE_OUTSIDE if out[k] else 0) for k, p in enumerate(ps)]
    return summarize(res, lt, angle), res, P


def assert_call(summary, results, prof, srcs, idx, lts, angs, ps, prm, label):
    """Every field of every summary and result of a call equal (==) to the reference, and the profiles.  srcs: the staged
    sources as sampled (255 - source under bitwise_not)."""
    assert summary.shape == (len(idx),) and results.shape == (len(idx), len(ps))
    for i in range(len(idx)):
        s, res, P = measure(srcs[idx[i]], lts[i], angs[i], ps, prm)
        for f in SUMMARY_FIELDS:
            assert summary[i][f].item() == s[f], f"{label}: pose {i}: summary {f}: {summary[i][f].item()!r} != {s[f]!r}"
        for f in RESULT_FIELDS:
            want = np.array([r[f] for r in res])
            bad = np.nonzero(results[i][f] != want)[0]
            assert bad.size == 0, (f"{label}: pose {i} probe {bad[0]} {tuple(ps[bad[0]])}: {f}: "
                                   f"{results[i][f][bad[0]]!r} != {want[bad[0]]!r}")
        if prof is not None:
            assert prof.shape[2] >= prm["length"]
            assert np.array_equal(prof[i, :, :prm["length"]], P), f"{label}: pose {i}: profile"
            assert not prof[i, :, prm["length"]:].any(), f"{label}: pose {i}: profile tail not zero"
    return None


# ---- fits -------------------------------------------------------------------------------------------------------------
def _stats(res):
    ss, mx = 0.0, 0.0
    for r in res:
        ss += r * r
        if abs(r) > mx:
            mx = abs(r)
    return math.sqrt(ss / float(len(res))), mx


def _line_once(pts, idx):
    m = float(len(idx))
    sx = sy = 0.0
    for i in idx:
        sx += pts[i][0]
        sy += pts[i][1]
    mx, my = sx / m, sy / m
    sxx = sxy = syy = 0.0
    for i in idx:
        dx, dy = pts[i][0] - mx, pts[i][1] - my
        sxx += dx * dx
        sxy += dx * dy
        syy += dy * dy
    theta = 0.5 * math.atan2(2.0 * sxy, sxx - syy)
    c, s = math.cos(theta), math.sin(theta)
    res = [(pts[i][1] - my) * c - (pts[i][0] - mx) * s for i in idx]
    along = mx * c + my * s
    rms, mr = _stats(res)
    return dict(angle=theta * R2D, px=mx - along * c, py=my - along * s, rms=rms, max_resid=mr, n_used=len(idx), flags=0), res


def _circle_once(pts, idx):
    m = float(len(idx))
    f = dict(cx=0.0, cy=0.0, r=0.0, rms=0.0, max_resid=0.0, n_used=len(idx), flags=0)
    sx = sy = 0.0
    for i in idx:
        sx += pts[i][0]
        sy += pts[i][1]
    mx, my = sx / m, sy / m
    suu = suv = svv = suuu = svvv = suvv = svuu = 0.0
    for i in idx:
        u, v = pts[i][0] - mx, pts[i][1] - my
        uu, vv = u * u, v * v
        suu += uu
        suv += u * v
        svv += vv
        suuu += uu * u
        svvv += vv * v
        suvv += u * vv
        svuu += v * uu
    det, tr = suu * svv - suv * suv, suu + svv
    if not det > 1e-12 * (tr * tr):
        f["flags"] = L.FIT_COLLINEAR
        return f, [0.0] * len(idx)
    bu, bv = 0.5 * (suuu + suvv), 0.5 * (svvv + svuu)
    a, b = (bu * svv - bv * suv) / det, (bv * suu - bu * suv) / det
    r = math.sqrt((a * a + b * b) + tr / m)
    converged = False
    for _ in range(8):
        jxx = jxy = jx1 = jyy = jy1 = gx = gy = g1 = 0.0
        for i in idx:
            du, dv = (pts[i][0] - mx) - a, (pts[i][1] - my) - b
            d = math.sqrt(du * du + dv * dv)
            ex, ey = (du / d, dv / d) if d > 0.0 else (0.0, 0.0)
            q = d - r
            jxx += ex * ex
            jxy += ex * ey
            jx1 += ex
            jyy += ey * ey
            jy1 += ey
            gx += ex * q
            gy += ey * q
            g1 += q
        c00, c01, c02 = jyy * m - jy1 * jy1, jxy * m - jy1 * jx1, jxy * jy1 - jyy * jx1
        dd = (jxx * c00 - jxy * c01) + jx1 * c02
        if not abs(dd) > 0.0 or not math.isfinite(dd):
            break
        da = ((gx * c00 - jxy * (gy * m - jy1 * g1)) + jx1 * (gy * jy1 - jyy * g1)) / dd
        db = ((jxx * (gy * m - jy1 * g1) - gx * c01) + jx1 * (jxy * g1 - gy * jx1)) / dd
        dr = ((jxx * (jyy * g1 - gy * jy1) - jxy * (jxy * g1 - gy * jx1)) + gx * c02) / dd
        a, b, r = a + da, b + db, r + dr
        converged = abs(da) <= 1e-10 and abs(db) <= 1e-10 and abs(dr) <= 1e-10
        if converged:
            break
    if not converged:
        f["flags"] |= L.FIT_NOT_CONVERGED
    res = []
    for i in idx:
        du, dv = (pts[i][0] - mx) - a, (pts[i][1] - my) - b
        res.append(math.sqrt(du * du + dv * dv) - r)
    f["cx"], f["cy"], f["r"] = mx + a, my + b, r
    f["rms"], f["max_resid"] = _stats(res)
    return f, res


def _trimmed(pts, trim, least, once):
    pts = [(float(p[0]), float(p[1])) for p in np.asarray(pts, np.float64).reshape(-1, 2)]
    idx = list(range(len(pts)))
    f, res = once(pts, idx)
    if not trim > 0.0:
        return f
    kept = [i for i, r in zip(idx, res) if not abs(r) > trim]
    if len(kept) == len(idx):
        return f
    if len(kept) < least:
        f["flags"] |= L.FIT_TRIM_STARVED
        return f
    return once(pts, kept)[0]


def fit_line(pts, trim=0.0):
    return _trimmed(pts, trim, 2, _line_once)


def fit_circle(pts, trim=0.0):
    return _trimmed(pts, trim, 3, _circle_once)
