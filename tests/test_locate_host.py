"""The host half of the sub-pattern locators (fpm_locate_host, fpm_locate_derive) against the restatement of
tests/locate_ref.py: every comparison is ==.  Then the planted accuracy test of a smooth scene shifted by known
sub-pixel amounts.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import locate_ref as ref


def _check(win, tmpl, rx, ry, feat_xy=(3, 5), lt=(12.25, -7.5), angle=33.0):
    raw, maps = M.locate_host(win, tmpl, rx, ry, maps=True)
    exp_raw, exp_maps = ref.locate(win, tmpl, rx, ry)
    assert maps.dtype == np.int32 and np.array_equal(maps, exp_maps)
    assert ref.raw_equal(raw, exp_raw), (ref.raw_dict(raw), exp_raw)
    assert ref.raw_equal(M.locate_host(win, tmpl, rx, ry), exp_raw)          # without maps: the same record
    h, w = tmpl.shape
    feat = M.feature(feat_xy[0], feat_xy[1], w, h, rx, ry)
    for flags in (0, L.LOCATE_OUTSIDE):                                       # the entries' flag passes through
        r = raw.copy()
        r["flags"] = flags
        got = M.locate_derive(feat, lt, angle, r)
        exp = ref.derive(ref.feat_tuple(feat), lt, angle, dict(exp_raw, flags=flags))
        assert ref.result_equal(got, exp), ({f: got[f] for f in ref.RESULT_FIELDS}, exp)
    return raw, M.locate_derive(feat, lt, angle, raw)


def test_struct_sizes():
    assert C.sizeof(L.Feature) == 32 and C.sizeof(L.LocateRaw) == 160 and C.sizeof(L.LocateResult) == 80
    assert M.FEATURE_DTYPE.itemsize == 32 and M.LOCATE_RAW_DTYPE.itemsize == 160 and M.LOCATE_DTYPE.itemsize == 80
    assert (L.LOCATE_EDGE_X, L.LOCATE_EDGE_Y, L.LOCATE_FLAT, L.LOCATE_OUTSIDE) == (1, 2, 4, 8)


@pytest.mark.parametrize("w,h,rx,ry", [(9, 7, 3, 2), (1, 1, 1, 1), (1, 17, 0, 3), (16, 1, 4, 0), (5, 5, 0, 0), (64, 33, 1, 3),
                                        (128, 128, 1, 0), (3, 4, 16, 16), (65, 16, 16, 1)])
def test_host_against_restatement(w, h, rx, ry):
    rng = np.random.default_rng(1000 * w + 10 * h + rx + ry)
    for k in range(3):
        tmpl = rng.integers(0, 256, (h, w), dtype=np.uint8)
        win = rng.integers(0, 256, (h + 2 * ry, w + 2 * rx), dtype=np.uint8)
        if k == 1:      # the template planted at a known offset: found there with score 1 (or flat when it has one value)
            px, py = int(rng.integers(0, 2 * rx + 1)), int(rng.integers(0, 2 * ry + 1))
            win[py:py + h, px:px + w] = tmpl
        raw, res = _check(win, tmpl, rx, ry)
        if k == 1 and tmpl.min() != tmpl.max():
            assert abs(res["score"] - 1.0) < 1e-12
        if k == 2:      # the extreme values: the largest sums
            _check(np.full_like(win, 255), np.full_like(tmpl, 255), rx, ry)


def test_flat_and_ties():
    rng = np.random.default_rng(5)
    h, w, rx, ry = 12, 10, 4, 3
    tmpl = rng.integers(0, 256, (h, w), dtype=np.uint8)
    win = rng.integers(0, 256, (h + 2 * ry, w + 2 * rx), dtype=np.uint8)
    flat_t, flat_w = np.full_like(tmpl, 77), np.full_like(win, 200)
    for a, b in ((win, flat_t), (flat_w, tmpl), (flat_w, flat_t), (np.zeros_like(win), tmpl)):
        raw, res = _check(a, b, rx, ry)
        assert (raw["dx"], raw["dy"]) == (0, 0) and res["score"] == 0.0 and res["score_nominal"] == 0.0
        assert res["flags"] == L.LOCATE_FLAT and (res["ox"], res["oy"]) == (0.0, 0.0)
    # all ties with contrast: a window of period 2 in x and y under a template of the same pattern -- every even offset
    # scores 1; the nearest to nominal wins, (0, 0) itself
    vv, uu = np.mgrid[0:h + 2 * ry, 0:w + 2 * rx]
    per = (((uu + rx) % 2) * 100 + ((vv + ry) % 2) * 50 + 10).astype(np.uint8)
    pt = per[ry:ry + h, rx:rx + w].copy()
    raw, res = _check(per, pt, rx, ry)
    assert (raw["dx"], raw["dy"]) == (0, 0) and abs(res["score"] - 1.0) < 1e-12
    # the same pattern one pixel off in x: (-1, 0) and (1, 0) tie at distance 1; the smaller dx wins
    raw, res = _check(per, per[ry:ry + h, rx + 1:rx + 1 + w].copy(), rx, ry)
    assert (raw["dx"], raw["dy"]) == (-1, 0)
    # one off in both: four offsets at distance 2; the smaller dy, then the smaller dx
    raw, res = _check(per, per[ry + 1:ry + 1 + h, rx + 1:rx + 1 + w].copy(), rx, ry)
    assert (raw["dx"], raw["dy"]) == (-1, -1)
    # a peak on the border: no sub-pixel step on that axis
    win2 = rng.integers(0, 256, (h + 2 * ry, w + 2 * rx), dtype=np.uint8)
    win2[0:h, 2 * rx:2 * rx + w] = tmpl
    raw, res = _check(win2, tmpl, rx, ry)
    assert (raw["dx"], raw["dy"]) == (rx, -ry) and res["flags"] == L.LOCATE_EDGE_X | L.LOCATE_EDGE_Y
    assert (res["ox"], res["oy"]) == (float(rx), float(-ry))
    assert raw["s_i"][0] == raw["s_i"][1] == raw["s_i"][2] == raw["s_i"][5] == raw["s_i"][8] == 0   # outside the range


def test_argument_rules():
    lib = L.load()
    t, w = np.zeros((8, 8), np.uint8), np.zeros((12, 12), np.uint8)
    raw = np.frombuffer(bytearray(b"\xa5" * 160), M.LOCATE_RAW_DTYPE)      # a sentinel: an error writes nothing
    sent = raw.tobytes()
    pw, pt, pr = L.u8ptr(w), L.u8ptr(t), raw.ctypes.data_as(C.POINTER(L.LocateRaw))
    ok = np.zeros(1, M.LOCATE_RAW_DTYPE)
    assert lib.fpm_locate_host(pw, 12, pt, 8, 8, 8, 2, 2, ok.ctypes.data_as(C.POINTER(L.LocateRaw)), None) == L.FPM_OK
    assert ok["n"][0] == 64
    for args in [(None, 12, pt, 8, 8, 8, 2, 2, pr), (pw, 12, None, 8, 8, 8, 2, 2, pr), (pw, 12, pt, 8, 8, 8, 2, 2, None),
                 (pw, 11, pt, 8, 8, 8, 2, 2, pr), (pw, 12, pt, 7, 8, 8, 2, 2, pr), (pw, 12, pt, 8, 0, 8, 2, 2, pr),
                 (pw, 12, pt, 8, 8, 0, 2, 2, pr), (pw, 200, pt, 200, 129, 8, 2, 2, pr), (pw, 12, pt, 8, 8, 129, 2, 2, pr),
                 (pw, 12, pt, 8, 8, 8, -1, 2, pr), (pw, 12, pt, 8, 8, 8, 2, -1, pr), (pw, 64, pt, 8, 8, 8, 17, 2, pr),
                 (pw, 12, pt, 8, 8, 8, 2, 17, pr)]:
        assert lib.fpm_locate_host(*args, None) == L.FPM_E_INVALID_ARG, args[1:8]
        assert raw.tobytes() == sent
    for bad in [dict(w=0), dict(w=129), dict(h=0), dict(h=129), dict(rx=-1), dict(rx=17), dict(ry=17), dict(x=-1), dict(w=2.5)]:
        kw = dict(x=0, y=0, w=8, h=8, rx=2, ry=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            M.feature(**kw)
    assert M.feature(1, 2, 3, 4)["ry"] == 8 and M.feature(1, 2, 3, 4, 5)["ry"] == 5 and M.feature(1, 2, 3, 4, 5, 0)["ry"] == 0
    # fpm_locate_derive: a record no search of the feature can have produced, a bad feature, null pointers, bad poses
    good, _ = ref.locate(np.arange(144, dtype=np.uint8).reshape(12, 12), np.arange(64, dtype=np.uint8).reshape(8, 8), 2, 2)
    rec = np.zeros(1, M.LOCATE_RAW_DTYPE)
    for f in ref.RAW_FIELDS:
        rec[f][0] = good[f]
    feat = np.zeros(1, M.FEATURE_DTYPE)
    feat[0] = M.feature(0, 0, 8, 8, 2, 2)
    out = np.zeros(1, M.LOCATE_DTYPE)
    pf, pr, po = (feat.ctypes.data_as(C.POINTER(L.Feature)), rec.ctypes.data_as(C.POINTER(L.LocateRaw)),
                  out.ctypes.data_as(C.POINTER(L.LocateResult)))
    assert lib.fpm_locate_derive(pf, 1.0, 2.0, 3.0, pr, po) == L.FPM_OK and out["score"][0] != 0
    out = np.frombuffer(bytearray(b"\xa5" * 80), M.LOCATE_DTYPE)
    po = out.ctypes.data_as(C.POINTER(L.LocateResult))
    clean = out.tobytes()
    for args in [(None, 1.0, 2.0, 3.0, pr, po), (pf, 1.0, 2.0, 3.0, None, po), (pf, 1.0, 2.0, 3.0, pr, None),
                 (pf, math.inf, 2.0, 3.0, pr, po), (pf, 1.0, math.nan, 3.0, pr, po), (pf, 1.0, 2.0, math.inf, pr, po)]:
        assert lib.fpm_locate_derive(*args) == L.FPM_E_INVALID_ARG
    for field, v in (("n", 63), ("dx", 3), ("dx", -3), ("dy", 3), ("dy", -3)):
        r2 = rec.copy()
        r2[field][0] = v
        assert lib.fpm_locate_derive(pf, 1.0, 2.0, 3.0, r2.ctypes.data_as(C.POINTER(L.LocateRaw)), po) == L.FPM_E_INVALID_ARG
    for field, v in (("w", 0), ("h", 129), ("rx", 17), ("ry", -1), ("reserved", (0, 1))):
        f2 = feat.copy()
        f2[field][0] = v
        assert lib.fpm_locate_derive(f2.ctypes.data_as(C.POINTER(L.Feature)), 1.0, 2.0, 3.0, pr, po) == L.FPM_E_INVALID_ARG
    assert out.tobytes() == clean


# ---- planted accuracy: a smooth scene shifted by known sub-pixel amounts ------------------------------------------------
SPOTS = [(30, 28, 3.0, 150), (44, 36, 2.2, -30), (36, 44, 4.0, 90)]
FEAT = (20, 18, 40, 36)
R = 4


def _scene(sx=0.0, sy=0.0):
    """The 80 x 80 scene evaluated at (u - sx, v - sy), rounded to u8."""
    v, u = np.mgrid[0:80, 0:80].astype(np.float64)
    u, v = u - sx, v - sy
    f = 40 + 0.3 * u + 0.2 * v + 60 / (1 + np.exp(-(u - 50) / 1.2))
    for c, d, s, a in SPOTS:
        f = f + a * np.exp(-((u - c) ** 2 + (v - d) ** 2) / (2 * s * s))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def test_planted_shifts_are_found_to_three_hundredths_of_a_pixel():
    """The restatement's own worst error on these 84 shifts is 0.0221 px; the bound is 0.03."""
    x, y, w, h = FEAT
    tmpl = _scene()[y:y + h, x:x + w]
    feat = M.feature(x, y, w, h, R, R)
    worst = 0.0
    for sy in (-1.6, 0.0, 0.4, 2.3):
        for q in range(-10, 11):
            sx = q / 4.0
            win = np.ascontiguousarray(_scene(sx, sy)[y - R:y + h + R, x - R:x + w + R])
            raw = M.locate_host(win, tmpl, R, R)
            res = M.locate_derive(feat, (0.0, 0.0), 0.0, raw)
            exp_raw, _ = ref.locate(win, tmpl, R, R)
            assert ref.raw_equal(raw, exp_raw) and ref.result_equal(res, ref.derive(FEAT + (R, R), (0.0, 0.0), 0.0, exp_raw))
            assert res["flags"] == 0, f"shift ({sx}, {sy}): the peak ({raw['dx']}, {raw['dy']}) is not interior"
            err = math.hypot(res["ox"] - sx, res["oy"] - sy)
            worst = max(worst, err)
            assert err <= 0.03, f"shift ({sx}, {sy}): found ({res['ox']}, {res['oy']}), {err:.4f} px off"
            assert res["tx"] == (x + (w - 1) / 2) + res["ox"] and res["sx"] == res["tx"] and res["sy"] == res["ty"]
    print(f"worst error {worst:.4f} px")
