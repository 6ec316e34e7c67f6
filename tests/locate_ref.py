"""The sub-pattern locators restated in numpy and Python (include/fpm.h, "sub-pattern locators"): the window is
gray_ref.patch (the oracle's warpAffine of fpm_patch_matrix's matrix) of the rectangle (x - rx, y - ry, w + 2 rx, h + 2
ry), the sums per offset are int64 numpy, and z, the tie rule and the derivation are Python ints and Python floats (IEEE
f64) in the header's order.  Shared by tests/test_locate_host.py and tests/test_gpu_locate.py."""
import math

import numpy as np

from fastest_image_pattern_matching_amd import _lib as L
from tests import gray_ref

RAW_FIELDS = ("dx", "dy", "flags", "reserved", "n", "sum_t", "sum_tt", "s_i", "s_ii", "s_it", "c_i", "c_ii", "c_it")
RESULT_FIELDS = ("dx", "dy", "flags", "reserved", "score", "score_nominal", "ox", "oy", "tx", "ty", "sx", "sy")


def window(src, feat, lt, angle):
    """uint8 (h + 2 ry, w + 2 rx): the window pixels I(u, v) of the feature (x, y, w, h, rx, ry) at the pose."""
    x, y, w, h, rx, ry = feat
    return gray_ref.patch(src, (x - rx, y - ry, w + 2 * rx, h + 2 * ry), lt, angle)


def sums(win, tmpl, rx, ry):
    """int64 (3, 2 ry + 1, 2 rx + 1): S_i, S_ii, S_it of every offset."""
    h, w = tmpl.shape
    assert win.shape == (h + 2 * ry, w + 2 * rx)
    I, T = win.astype(np.int64), tmpl.astype(np.int64)
    out = np.zeros((3, 2 * ry + 1, 2 * rx + 1), np.int64)
    for j in range(2 * ry + 1):
        for i in range(2 * rx + 1):
            c = I[j:j + h, i:i + w]
            out[0, j, i], out[1, j, i], out[2, j, i] = c.sum(), (c * c).sum(), (c * T).sum()
    return out


def zncc(n, si, sii, st, stt, sit):
    n, si, sii, st, stt, sit = (int(v) for v in (n, si, sii, st, stt, sit))
    Di, Dt, N = n * sii - si * si, n * stt - st * st, n * sit - si * st
    assert max(abs(Di), abs(Dt), abs(N)) < 1 << 62
    sdi, sdt = math.sqrt(float(Di)), math.sqrt(float(Dt))
    return 0.0 if Di == 0 or Dt == 0 else float(N) / (sdi * sdt)


def locate(win, tmpl, rx, ry):
    """(raw, maps): raw a {field: value} of fpm_locate_raw (the arrays as lists of 9), maps the int64 sums."""
    h, w = tmpl.shape
    S = sums(win, tmpl, rx, ry)
    assert S.max() < 1 << 31
    T = tmpl.astype(np.int64)
    n, st, stt = w * h, int(T.sum()), int((T * T).sum())
    best = None
    for j in range(2 * ry + 1):
        for i in range(2 * rx + 1):
            dx, dy = i - rx, j - ry
            key = (-zncc(n, S[0, j, i], S[1, j, i], st, stt, S[2, j, i]), dx * dx + dy * dy, dy, dx)
            if best is None or key < best:
                best = key
    dx, dy = best[3], best[2]
    raw = dict(dx=dx, dy=dy, flags=0, reserved=0, n=n, sum_t=st, sum_tt=stt, s_i=[0] * 9, s_ii=[0] * 9, s_it=[0] * 9,
               c_i=int(S[0, ry, rx]), c_ii=int(S[1, ry, rx]), c_it=int(S[2, ry, rx]))
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            qi, qj = dx + i + rx, dy + j + ry
            if 0 <= qi <= 2 * rx and 0 <= qj <= 2 * ry:
                e = (j + 1) * 3 + (i + 1)
                raw["s_i"][e], raw["s_ii"][e], raw["s_it"][e] = (int(S[k, qj, qi]) for k in range(3))
    return raw, S


def derive(feat, lt, angle, raw):
    """{field: value} of fpm_locate_result for a raw record (a dict as locate() gives, flags as the entry left them)."""
    x, y, w, h, rx, ry = feat
    z = [zncc(raw["n"], raw["s_i"][e], raw["s_ii"][e], raw["sum_t"], raw["sum_tt"], raw["s_it"][e]) for e in range(9)]
    out = dict.fromkeys(RESULT_FIELDS, 0)
    out["dx"], out["dy"] = raw["dx"], raw["dy"]
    flags = raw["flags"] & L.LOCATE_OUTSIDE
    out["score"] = z[4]
    out["score_nominal"] = zncc(raw["n"], raw["c_i"], raw["c_ii"], raw["sum_t"], raw["sum_tt"], raw["c_it"])
    Di = raw["n"] * raw["s_ii"][4] - raw["s_i"][4] ** 2
    Dt = raw["n"] * raw["sum_tt"] - raw["sum_t"] ** 2
    if Di == 0 or Dt == 0:
        flags |= L.LOCATE_FLAT

    def sub(zm, z0, zp):
        den = (zm - z0) + (zp - z0)
        return 0.5 * (zm - zp) / den if den < 0.0 else 0.0

    ddx = ddy = 0.0
    if abs(raw["dx"]) == rx:
        flags |= L.LOCATE_EDGE_X
    else:
        ddx = sub(z[3], z[4], z[5])
    if abs(raw["dy"]) == ry:
        flags |= L.LOCATE_EDGE_Y
    else:
        ddy = sub(z[1], z[4], z[7])
    out["flags"] = flags
    out["ox"], out["oy"] = float(raw["dx"]) + ddx, float(raw["dy"]) + ddy
    out["tx"] = (float(x) + float(w - 1) / 2.0) + out["ox"]
    out["ty"] = (float(y) + float(h - 1) / 2.0) + out["oy"]
    ra = float(angle) * (math.pi / 180.0)
    c, s = math.cos(ra), math.sin(ra)
    ltx, lty = float(np.float32(lt[0])), float(np.float32(lt[1]))
    out["sx"] = ltx + (out["tx"] * c - out["ty"] * s)
    out["sy"] = lty + (out["tx"] * s + out["ty"] * c)
    return out


def outside(sw, sh, feat, lt, angle):
    """FPM_LOCATE_OUTSIDE or 0: the calipers' four-corner rule on the window's corner pixels."""
    x, y, w, h, rx, ry = feat
    rect = (x - rx, y - ry, w + 2 * rx, h + 2 * ry)
    return L.LOCATE_OUTSIDE if gray_ref.outside(sw, sh, rect, lt, angle) else 0


def raw_equal(got, exp):
    """A LOCATE_RAW_DTYPE record against a dict of locate()."""
    return all((list(got[f]) if f in ("s_i", "s_ii", "s_it") else got[f]) == exp[f] for f in RAW_FIELDS)


def result_equal(got, exp):
    """A LOCATE_DTYPE record against a dict of derive(): ==, floats included."""
    return all(got[f] == exp[f] for f in RESULT_FIELDS)


def feat_tuple(f):
    return tuple(int(f[k]) for k in ("x", "y", "w", "h", "rx", "ry"))


def raw_dict(rec):
    """A LOCATE_RAW_DTYPE record as the dict derive() takes."""
    return {f: ([int(v) for v in rec[f]] if f in ("s_i", "s_ii", "s_it") else int(rec[f])) for f in RAW_FIELDS}
