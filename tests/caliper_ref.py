"""The edge calipers restated in numpy and math (include/fpm.h, "edge calipers"): the sampling pose and the derivation in
Python floats (IEEE f64, math.cos / math.sin are the C library's) in the header's order, the profile as column sums of
oracle.warp_affine of matcher.patch_matrix's matrix, the step filter and the edge rules on int64.  Shared by
tests/test_caliper_host.py and tests/test_gpu_calipers.py."""
import math

import numpy as np

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import oracle

D2R = math.pi / 180.0
RAW_FIELDS = ("index", "d_prev", "d", "d_next")
EDGE_FIELDS = RAW_FIELDS + ("t", "contrast", "tx", "ty", "sx", "sy")
SUMMARY_FIELDS = ("n_edges", "n_returned", "strongest", "flags", "lt_x", "lt_y", "angle")


def cal(cx, cy, phi, length, width, half=2, contrast=12, polarity=0):
    """A caliper as a plain dict (the reference never goes through the library's record)."""
    return dict(cx=float(cx), cy=float(cy), phi=float(phi), length=int(length), width=int(width), half=int(half),
                contrast=int(contrast), polarity=int(polarity))


def record(c):
    return M.caliper(**c)


def frame(c):
    """(ox, oy, cp, sp, hw): the template point of sample (0, 0), the scan direction, half the width."""
    hl, hw = (c["length"] - 1) / 2.0, (c["width"] - 1) / 2.0
    rp = c["phi"] * D2R
    cp, sp = math.cos(rp), math.sin(rp)
    return c["cx"] - (hl * cp - hw * sp), c["cy"] - (hl * sp + hw * cp), cp, sp, hw


def pose(lt, angle, c):
    """((lt_k as f32 values), angle_k)."""
    ox, oy, _, _, _ = frame(c)
    ra = angle * D2R
    cs, sn = math.cos(ra), math.sin(ra)
    x = float(np.float32(lt[0])) + (ox * cs - oy * sn)
    y = float(np.float32(lt[1])) + (ox * sn + oy * cs)
    return (float(np.float32(x)), float(np.float32(y))), angle + c["phi"]


def inverted(sw, sh, lt_k, angle_k):
    """The inverted patch matrix of the rectangle (0, 0, ..) at the sampling pose, as cv::warpAffine inverts it: six
    Python floats in fpm_geom.h's operation order."""
    m = [float(v) for v in M.patch_matrix(sw, sh, lt_k, angle_k, (0, 0)).reshape(-1)]
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


def outside(sw, sh, lt_k, angle_k, c):
    m = inverted(sw, sh, lt_k, angle_k)
    for k in range(4):
        x = float(c["length"] - 1) if k & 1 else 0.0
        y = float(c["width"] - 1) if k & 2 else 0.0
        sx, sy = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
        if not (0.0 <= sx <= float(sw - 1) and 0.0 <= sy <= float(sh - 1)):
            return True
    return False


def profile(src, lt_k, angle_k, c):
    """int64 [length]: the column sums of the caliper-sized patch."""
    m = M.patch_matrix(src.shape[1], src.shape[0], lt_k, angle_k, (0, 0))
    return oracle.warp_affine(src, m, (c["length"], c["width"])).astype(np.int64).sum(axis=0)


def steps(P, c):
    """int64 [length + 1]: D[0 .. L], 0 outside s .. L - s."""
    P = np.asarray(P, np.int64)
    n, s = c["length"], c["half"]
    assert P.shape == (n,)
    D = np.zeros(n + 1, np.int64)
    S = np.concatenate([[0], np.cumsum(P)])       # S[i] = P[0] + .. + P[i - 1]
    i = np.arange(s, n - s + 1)
    D[i] = (S[i + s] - S[i]) - (S[i] - S[i - s])
    return D


def edges_raw(P, c):
    """Every edge as (index, d_prev, d, d_next) Python ints, in ascending index (no capacity)."""
    D = steps(P, c)
    n, s, thr = c["length"], c["half"], c["contrast"] * c["half"] * c["width"]
    out = []
    for i in range(s, n - s + 1):
        for p in (1, -1):
            if c["polarity"] not in (0, p):
                continue
            a, am, ap = p * D[i], p * D[i - 1], p * D[i + 1]
            if a >= thr and a > am and a >= ap:
                out.append((i, int(D[i - 1]), int(D[i]), int(D[i + 1])))
    return out


def derive(c, lt_k, angle_k, raw):
    """{field: value} of fpm_edge for one raw record."""
    i, dp, d, dn = raw
    g = 1 if d > 0 else -1
    am, a0, ap = g * dp, g * d, g * dn
    den = (am - a0) + (ap - a0)
    assert den < 0
    delta = 0.5 * float(am - ap) / float(den)
    t = (float(i) - 0.5) + delta
    ox, oy, cp, sp, hw = frame(c)
    rk = angle_k * D2R
    ck, sk = math.cos(rk), math.sin(rk)
    ltx, lty = float(np.float32(lt_k[0])), float(np.float32(lt_k[1]))
    return dict(index=i, d_prev=dp, d=d, d_next=dn, t=t, contrast=float(abs(d)) / float(c["half"] * c["width"]),
                tx=ox + (t * cp - hw * sp), ty=oy + (t * sp + hw * cp),
                sx=ltx + (t * ck - hw * sk), sy=lty + (t * sk + hw * ck), delta=delta)


def summarize(raws, cap, flags0, lt_k, angle_k):
    """(summary dict, the returned raw records)."""
    ret = raws[:cap]
    strongest = -1
    for k, r in enumerate(ret):
        if strongest < 0 or abs(r[2]) > abs(ret[strongest][2]):
            strongest = k
    flags = flags0 | (L.CALIPER_TRUNCATED if len(raws) > cap else 0)
    return dict(n_edges=len(raws), n_returned=len(ret), strongest=strongest, flags=flags, lt_x=lt_k[0], lt_y=lt_k[1],
                angle=angle_k), ret


def measure(src, lt, angle, c, cap):
    """(summary dict, [edge dicts], profile) of caliper c on a hit at (lt, angle) on src."""
    lt_k, ak = pose(lt, angle, c)
    P = profile(src, lt_k, ak, c)
    fl = L.CALIPER_OUTSIDE if outside(src.shape[1], src.shape[0], lt_k, ak, c) else 0
    s, ret = summarize(edges_raw(P, c), cap, fl, lt_k, ak)
    return s, [derive(c, lt_k, ak, r) for r in ret], P


def assert_call(summary, edges, prof, srcs, idx, lts, angs, cals, cap, label):
    """Every field of every summary and edge of a call equal (==) to the reference; the records behind n_returned and the
    profile entries from length on zero.  srcs: the staged sources as sampled (255 - source under bitwise_not)."""
    assert summary.shape == (len(idx), len(cals)) and edges.shape == (len(idx), len(cals), cap)
    for i in range(len(idx)):
        for k, c in enumerate(cals):
            s, es, P = measure(srcs[idx[i]], lts[i], angs[i], c, cap)
            where = f"{label}: pose {i} caliper {k} {c}"
            for f in SUMMARY_FIELDS:
                assert summary[i, k][f].item() == s[f], f"{where}: summary {f}: {summary[i, k][f].item()!r} != {s[f]!r}"
            for j, e in enumerate(es):
                for f in EDGE_FIELDS:
                    assert edges[i, k, j][f].item() == e[f], f"{where}: edge {j} {f}: {edges[i, k, j][f].item()!r} != {e[f]!r}"
            assert edges[i, k, len(es):].tobytes() == bytes(edges.dtype.itemsize * (cap - len(es))), f"{where}: tail not zero"
            if prof is not None:
                assert np.array_equal(prof[i, k, :c["length"]], P), f"{where}: profile"
                assert not prof[i, k, c["length"]:].any(), f"{where}: profile tail not zero"
