"""Edge calipers, host side (no GPU): the struct layouts, fpm_caliper_pose, fpm_caliper_edges_host and
fpm_caliper_derive against the restatement of tests/caliper_ref.py (every comparison ==), the argument errors, and on
the CPU reference alone what a caliper is for: planted straight edges found to a fraction of a sample, and the edge's
source point agreeing with the sampler's own matrix."""
import ctypes as C
import math

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import align_ref
from tests import caliper_ref as ref

PHIS = [0.0, 90.0, 37.5, -137.5, 180.0]


def test_struct_layouts(fpm_lib):
    assert C.sizeof(L.Caliper) == M.CALIPER_DTYPE.itemsize == 48
    assert C.sizeof(L.CaliperSummary) == M.CALIPER_SUMMARY_DTYPE.itemsize == 32
    assert C.sizeof(L.Edge) == M.EDGE_DTYPE.itemsize == 64 and C.sizeof(L.EdgeRaw) == M.EDGE_RAW_DTYPE.itemsize == 16
    off = lambda dt: [dt.fields[n][1] for n in dt.names]   # noqa: E731
    assert off(M.CALIPER_DTYPE) == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    assert M.CALIPER_DTYPE.names == ("cx", "cy", "phi", "length", "width", "half", "contrast", "polarity", "reserved")
    assert off(M.CALIPER_SUMMARY_DTYPE) == [0, 4, 8, 12, 16, 20, 24]
    assert M.CALIPER_SUMMARY_DTYPE.names == ("n_edges", "n_returned", "strongest", "flags", "lt_x", "lt_y", "angle")
    assert off(M.EDGE_DTYPE) == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56]
    assert M.EDGE_DTYPE.names == ("index", "d_prev", "d", "d_next", "t", "contrast", "tx", "ty", "sx", "sy")
    for dt, ct in [(M.CALIPER_DTYPE, L.Caliper), (M.CALIPER_SUMMARY_DTYPE, L.CaliperSummary), (M.EDGE_DTYPE, L.Edge)]:
        assert off(dt) == [getattr(ct, n).offset for n in dt.names]
    assert (L.CALIPER_TRUNCATED, L.CALIPER_OUTSIDE) == (1, 2)


def _grid_cals():
    cals = []
    for k, phi in enumerate(PHIS):
        cals.append(ref.cal(20.5 + k, 11.25, phi, 2 + 7 * k, 1 + 5 * k, half=1))
        cals.append(ref.cal(-13.0 - k, -4.5, phi, 64, 24))            # a negative centre
        cals.append(ref.cal(500.25, 300.0 + k, phi, 1024, 256))       # far beyond any template
    return cals


def test_pose_equals_the_restatement(fpm_lib):
    poses = [((40.0, 30.0), 0.0), ((52.25, 41.5), 30.0), ((70.5, 66.125), -137.5), ((-7.375, 40.5), 90.0),
             ((120.3, 80.7), 17.0), ((0.0, 0.0), 180.0), ((1e5 + 0.3, -2e4), 359.999)]
    for lt, a in poses:
        for c in _grid_cals():
            got = M.caliper_pose(lt, a, ref.record(c))
            assert got == ref.pose(lt, a, c), (lt, a, c, got, ref.pose(lt, a, c))
    # the centre sample lands where the pose puts the caliper's centre: lt + L (cx, cy)
    c = ref.cal(30.0, 12.0, 37.5, 65, 17)
    (x, y), ak = M.caliper_pose((50.0, 60.0), 20.0, ref.record(c))
    ck, sk = math.cos(ak * ref.D2R), math.sin(ak * ref.D2R)
    ca, sa = math.cos(20.0 * ref.D2R), math.sin(20.0 * ref.D2R)
    assert abs(x + (32.0 * ck - 8.0 * sk) - (50.0 + (30.0 * ca - 12.0 * sa))) < 1e-4
    assert abs(y + (32.0 * sk + 8.0 * ck) - (60.0 + (30.0 * sa + 12.0 * ca))) < 1e-4


def _check_edges(P, c, cap, label):
    """fpm_caliper_edges_host and fpm_caliper_derive on profile P against the restatement; returns the reference's list."""
    exp = ref.edges_raw(P, c)
    raw, n, flags = M.caliper_edges_host(P, ref.record(c), cap)
    assert n == len(exp), f"{label}: {n} edges vs {len(exp)}"
    assert flags == (L.CALIPER_TRUNCATED if len(exp) > cap else 0), label
    assert [tuple(int(r[f]) for f in ref.RAW_FIELDS) for r in raw] == exp[:cap], label
    lt_k, ak = (33.25, -7.5), 61.0 + c["phi"]
    got = M.caliper_derive(ref.record(c), lt_k, ak, raw)
    for g, r in zip(got, exp[:cap]):
        e = ref.derive(c, lt_k, ak, r)
        for f in ref.EDGE_FIELDS:
            assert g[f].item() == e[f], f"{label}: edge {r} field {f}: {g[f].item()!r} != {e[f]!r}"
        assert -0.5 < e["delta"] <= 0.5
    return exp


@pytest.mark.parametrize("polarity", [1, -1, 0])
def test_edges_host_random_profiles(fpm_lib, polarity):
    rng = np.random.default_rng(100 + polarity)
    total = 0
    for k in range(200):
        L_ = int(rng.integers(2, 200))
        W = int(rng.integers(1, 257))
        s = int(rng.integers(1, min(16, L_ // 2) + 1))
        c = ref.cal(0, 0, 0, L_, W, s, int(rng.choice([1, 12, 60, 255])), polarity)
        if k % 3 == 0:      # smooth: few edges, plateaus from the rounding
            P = np.rint(255 * W * (0.5 + 0.5 * np.sin(np.arange(L_) * rng.uniform(0.05, 0.6) + rng.uniform(0, 6))))
        elif k % 3 == 1:    # rough
            P = rng.integers(0, 255 * W + 1, L_)
        else:               # a few levels: equal neighbours
            P = rng.integers(0, 4, L_) * (255 * W // 3)
        total += len(_check_edges(P.astype(np.int64), c, int(rng.choice([1, 8, 64])), f"random {k}"))
    assert total > 200


def test_edges_host_hand_made_profiles(fpm_lib):
    # a sharp step: one edge, a symmetric triple, delta exactly 0
    e = _check_edges([0] * 8 + [100] * 8, ref.cal(0, 0, 0, 16, 1, 1, 10, 0), 8, "step")
    assert e == [(8, 0, 100, 0)] and ref.derive(ref.cal(0, 0, 0, 16, 1, 1, 10, 0), (0, 0), 0, e[0])["t"] == 7.5
    e = _check_edges([100] * 8 + [0] * 8, ref.cal(0, 0, 0, 16, 1, 1, 10, -1), 8, "falling step")
    assert e == [(8, 0, -100, 0)]
    assert _check_edges([100] * 8 + [0] * 8, ref.cal(0, 0, 0, 16, 1, 1, 10, 1), 8, "falling step, rising asked") == []
    # a two-sample ramp makes a plateau of D: the first sample is taken, delta = 0.5
    c = ref.cal(0, 0, 0, 10, 1, 1, 10, 1)
    e = _check_edges([0, 0, 0, 50, 100, 100, 100, 100, 100, 100], c, 8, "plateau")
    assert e == [(3, 0, 50, 50)] and ref.derive(c, (0, 0), 0, e[0])["delta"] == 0.5
    # an edge at i = s and at i = L - s
    c = ref.cal(0, 0, 0, 8, 1, 2, 10, 0)
    assert _check_edges([0, 0, 100, 100, 100, 100, 100, 100], c, 8, "i = s") == [(2, 0, 200, 100)]
    assert _check_edges([0, 0, 0, 0, 0, 0, 100, 100], c, 8, "i = L - s") == [(6, 100, 200, 0)]
    # A == c s W is kept, one below is dropped
    c = ref.cal(0, 0, 0, 12, 3, 1, 10, 0)
    assert _check_edges([0] * 6 + [30] * 6, c, 8, "at the threshold") == [(6, 0, 30, 0)]
    assert _check_edges([0] * 6 + [29] * 6, c, 8, "below the threshold") == []
    # L = 2 s: one index
    assert _check_edges([0, 0, 9, 9], ref.cal(0, 0, 0, 4, 1, 2, 1, 0), 8, "L = 2 s") == [(2, 0, 18, 0)]
    # all-equal profiles: none
    for v in (0, 77, 255 * 5):
        assert _check_edges([v] * 40, ref.cal(0, 0, 0, 40, 5, 3, 1, 0), 8, "flat") == []


@pytest.mark.parametrize("cap", [1, 8, 64])
def test_edges_host_capacity(fpm_lib, cap):
    for extra in (0, 1):
        n = cap + extra
        P = ([0, 0, 10, 10] * (n + 1))[:4 * n + 2]
        e = _check_edges(P, ref.cal(0, 0, 0, len(P), 1, 1, 1, 1), cap, f"{n} edges, cap {cap}")
        assert len(e) == n and [r[0] for r in e] == [2 + 4 * k for k in range(n)]
        raw, cnt, flags = M.caliper_edges_host(P, M.caliper(0, 0, 0, len(P), 1, 1, 1, 1), cap)
        assert cnt == n and len(raw) == cap and flags == (L.CALIPER_TRUNCATED if extra else 0)


def test_edges_host_extremes(fpm_lib):
    P = ([0] * 16 + [65280] * 16) * 4
    c = ref.cal(0, 0, 0, len(P), 256, 16, 255, 0)
    e = _check_edges(P, c, 64, "extremes")
    assert [r[0] for r in e] == [16, 32, 48, 64, 80, 96, 112] and {abs(r[2]) for r in e} == {1044480}
    assert ref.derive(c, (0, 0), 0, e[0])["contrast"] == 255.0


def test_derive_symmetric_triple(fpm_lib):
    c = ref.cal(12.5, 3.0, 37.5, 64, 24, 2, 12, 0)
    for raw in [(10, 700, 900, 700), (31, -5000, -8000, -5000), (2, 0, 576, 0)]:
        got = M.caliper_derive(ref.record(c), (10.0, 20.0), 5.0, [raw])[0]
        e = ref.derive(c, (10.0, 20.0), 5.0, raw)
        assert e["delta"] == 0.0 and got["t"] == raw[0] - 0.5
        for f in ref.EDGE_FIELDS:
            assert got[f].item() == e[f]


def _c_cal(**kw):
    d = dict(cx=1.0, cy=2.0, phi=3.0, length=16, width=4, half=2, contrast=12, polarity=0, reserved=0)
    d.update(kw)
    return L.Caliper(**d)


BAD_CALS = [dict(length=1), dict(length=1025), dict(width=0), dict(width=257), dict(half=0), dict(half=17),
            dict(length=6, half=4), dict(contrast=0), dict(contrast=256), dict(polarity=2), dict(polarity=-2),
            dict(reserved=1), dict(cx=float("nan")), dict(cy=float("inf")), dict(phi=float("-inf"))]


def test_argument_errors_leave_outputs_untouched(fpm_lib):
    x, y, a = C.c_float(-1.5), C.c_float(-2.5), C.c_double(-3.5)
    raw = (L.EdgeRaw * 4)(*[L.EdgeRaw(9, 9, 9, 9)] * 4)
    n, fl = C.c_int32(-7), C.c_int32(-8)
    out = (L.Edge * 2)()
    C.memset(out, 0x5a, C.sizeof(out))
    prof = (C.c_int32 * 16)(*([0] * 8 + [100] * 8))
    good = (L.EdgeRaw * 2)(L.EdgeRaw(8, 0, 400, 0), L.EdgeRaw(8, 10, 400, 20))

    def untouched():
        return ((x.value, y.value, a.value, n.value, fl.value) == (-1.5, -2.5, -3.5, -7, -8) and
                all((r.index, r.d_prev, r.d, r.d_next) == (9, 9, 9, 9) for r in raw) and bytes(out) == b"\x5a" * C.sizeof(out))

    def pose(cal, ltx=1.0, lty=2.0, ang=3.0, px=x, py=y, pa=a):
        return fpm_lib.fpm_caliper_pose(ltx, lty, ang, cal, px, py, pa)

    def edges(cal, p=prof, cap=4, r=raw, pn=n, pf=fl):
        return fpm_lib.fpm_caliper_edges_host(p, cal, cap, r, pn, pf)

    def derive(cal, r, cnt, ltx=1.0, lty=2.0, ang=3.0, o=out):
        return fpm_lib.fpm_caliper_derive(cal, ltx, lty, ang, r, cnt, o)

    ok = C.byref(_c_cal())
    for bad in BAD_CALS:
        cal = C.byref(_c_cal(**bad))
        assert pose(cal) == L.FPM_E_INVALID_ARG, bad
        assert edges(cal) == L.FPM_E_INVALID_ARG, bad
        assert derive(cal, good, 2) == L.FPM_E_INVALID_ARG, bad
    assert pose(None) == pose(ok, px=None) == pose(ok, py=None) == pose(ok, pa=None) == L.FPM_E_INVALID_ARG
    assert pose(ok, ltx=float("nan")) == pose(ok, lty=float("inf")) == pose(ok, ang=float("nan")) == L.FPM_E_INVALID_ARG
    assert edges(None) == edges(ok, p=None) == edges(ok, r=None) == edges(ok, pn=None) == edges(ok, pf=None) == L.FPM_E_INVALID_ARG
    assert edges(ok, cap=0) == edges(ok, cap=65) == L.FPM_E_INVALID_ARG
    for v in (-1, 255 * 4 + 1):      # of no 4 pixels
        p = (C.c_int32 * 16)(*([0] * 15 + [v]))
        assert edges(ok, p=p) == L.FPM_E_INVALID_ARG
    assert derive(None, good, 2) == derive(ok, None, 2) == derive(ok, good, 2, o=None) == derive(ok, good, -1) == L.FPM_E_INVALID_ARG
    assert derive(ok, good, 2, ltx=float("nan")) == derive(ok, good, 2, ang=float("inf")) == L.FPM_E_INVALID_ARG
    # records that are no edge, behind a good one: nothing is written
    for r in [L.EdgeRaw(8, 0, 0, 0), L.EdgeRaw(8, 500, 400, 0), L.EdgeRaw(8, 0, 400, 401), L.EdgeRaw(8, 400, 400, 400),
              L.EdgeRaw(1, 0, 400, 0), L.EdgeRaw(15, 0, 400, 0), L.EdgeRaw(8, 0, -400, -401)]:
        assert derive(ok, (L.EdgeRaw * 2)(good[0], r), 2) == L.FPM_E_INVALID_ARG
    assert untouched()
    # and the same calls with good arguments succeed
    assert pose(ok) == L.FPM_OK and edges(ok) == L.FPM_OK and (n.value, fl.value) == (1, 0)
    assert derive(ok, good, 2) == L.FPM_OK and out[1].index == 8
    assert derive(ok, None, 0, o=None) == L.FPM_OK
    for bad in [dict(length=1), dict(half=9, length=16), dict(polarity=3), dict(contrast=0), dict(cx=float("nan"))]:
        with pytest.raises(ValueError):
            M.caliper(**{**dict(cx=0, cy=0, phi=0, length=16, width=4), **bad})


# ---- planted truth, on the CPU reference ------------------------------------------------------------------------------
BAR_DIR, BAR_CENTRE, BAR_HALF = 12.0, (160.3, 120.6), 9.35      # direction in degrees, a point of the centre line, half width
BAR_LOW, BAR_HIGH = 40, 200
PLANTED_MAX = 0.0296   # measured: see the test's docstring


def _clip(poly, nx, ny, d):
    """Sutherland-Hodgman: the part of a convex polygon with nx x + ny y <= d."""
    out = []
    for k in range(len(poly)):
        (x0, y0), (x1, y1) = poly[k], poly[(k + 1) % len(poly)]
        f0, f1 = nx * x0 + ny * y0 - d, nx * x1 + ny * y1 - d
        if f0 <= 0:
            out.append((x0, y0))
        if (f0 < 0 < f1) or (f1 < 0 < f0):
            t = f0 / (f0 - f1)
            out.append((x0 + t * (x1 - x0), y0 + t * (y1 - y0)))
    return out


def _area(poly):
    return 0.5 * abs(sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1]
                         for k in range(len(poly)))) if len(poly) >= 3 else 0.0


def bar_scene(w=320, h=240):
    """A bright bar on a dark ground rendered by exact area coverage (pixel (x, y) is the square x +- 0.5, y +- 0.5), so
    its two long edges are the lines n . p = d0 -+ BAR_HALF exactly.  Returns (scene, (nx, ny), (d_lo, d_hi))."""
    th = math.radians(BAR_DIR)
    nx, ny = -math.sin(th), math.cos(th)
    d0 = nx * BAR_CENTRE[0] + ny * BAR_CENTRE[1]
    d_lo, d_hi = d0 - BAR_HALF, d0 + BAR_HALF
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    dist = nx * xx + ny * yy
    cov = ((dist > d_lo) & (dist < d_hi)).astype(np.float64)
    for y, x in zip(*np.nonzero((np.abs(dist - d_lo) < 0.75) | (np.abs(dist - d_hi) < 0.75))):
        sq = [(x - 0.5, y - 0.5), (x + 0.5, y - 0.5), (x + 0.5, y + 0.5), (x - 0.5, y + 0.5)]
        cov[y, x] = _area(_clip(_clip(sq, nx, ny, d_hi), -nx, -ny, -d_lo))
    return np.rint(BAR_LOW + (BAR_HIGH - BAR_LOW) * cov).astype(np.uint8), (nx, ny), (d_lo, d_hi)


def planted_calipers(lt, angle, n, d_edge, sign):
    """Calipers of a template frame at (lt, angle) across the edge n . p = d_edge, centred on three points of it, scanning
    perpendicular to the bar and 20 degrees off; sign +1 scans along +n.  Template coordinates by the header's rule:
    (x, y) = L^-1 (p - lt)."""
    nx, ny = n
    ra = angle * ref.D2R
    ca, sa = math.cos(ra), math.sin(ra)
    out = []
    for along in (-30.0, 0.0, 25.5):
        px = BAR_CENTRE[0] + along * ny + (d_edge - (nx * BAR_CENTRE[0] + ny * BAR_CENTRE[1])) * nx
        py = BAR_CENTRE[1] - along * nx + (d_edge - (nx * BAR_CENTRE[0] + ny * BAR_CENTRE[1])) * ny
        dx, dy = px - float(np.float32(lt[0])), py - float(np.float32(lt[1]))
        cx, cy = ca * dx + sa * dy, -sa * dx + ca * dy
        scan = math.degrees(math.atan2(sign * ny, sign * nx))
        for off in (0.0, 20.0):
            out.append(ref.cal(cx, cy, scan + off - angle, 16, 9, 2, 20, 0))
    return out


def test_planted_edges_on_the_reference(fpm_lib, oracle_lib):
    """A 320 x 240 scene with a bar of exact area coverage (edges known analytically), a template frame at
    tests/align_ref.py's two PLANTED poses, calipers of 16 x 9 samples (s = 2) across both edges at three places, scanning
    perpendicular to the bar and 20 degrees off it, in both directions: 48 calipers.  Every caliper finds exactly one
    edge, of the polarity its direction implies.  Measured on the CPU reference: the largest distance of an edge's
    source point from the true line is 0.0296 source pixels (samples are source pixels: scale 1), the mean 0.0083
    (profiles/calipers/README.txt).  The test asserts at most twice the measured maximum, and in any case below 0.5
    sample, beyond which a sub-sample estimate means nothing."""
    scene, n, (d_lo, d_hi) = bar_scene()
    assert scene.min() == BAR_LOW and scene.max() == BAR_HIGH and len(np.unique(scene)) > 20
    worst, dists = 0.0, []
    for lt, angle in align_ref.PLANTED:
        for d_edge, rising_along_n in ((d_lo, True), (d_hi, False)):
            for sign in (1, -1):
                for c in planted_calipers(lt, angle, n, d_edge, sign):
                    s, es, P = ref.measure(scene, lt, angle, c, 8)
                    assert s["n_edges"] == 1 and s["flags"] == 0, (c, s)
                    assert (es[0]["d"] > 0) == (rising_along_n == (sign > 0))
                    dist = abs(n[0] * es[0]["sx"] + n[1] * es[0]["sy"] - d_edge)
                    dists.append(dist)
                    worst = max(worst, dist)
                    # the library's host entries give the same edge from the same profile
                    raw, cnt, _ = M.caliper_edges_host(P, ref.record(c), 8)
                    lt_k, ak = M.caliper_pose(lt, angle, ref.record(c))
                    got = M.caliper_derive(ref.record(c), lt_k, ak, raw)
                    assert cnt == 1 and all(got[0][f].item() == es[0][f] for f in ref.EDGE_FIELDS)
    print(f"planted edges: {len(dists)} calipers, max {worst:.4f} px, mean {sum(dists) / len(dists):.4f} px")
    assert len(dists) == 48
    assert worst < 0.5
    assert worst <= 2 * PLANTED_MAX


def test_edge_source_point_agrees_with_the_patch_matrix(fpm_lib, oracle_lib):
    """The source point of an edge against the inverted patch matrix of (lt_k, angle_k) applied to (t, hw): the pose rule
    and the sampler's f32-rounded matrix agree to within 1/64 px on these small sources (the sampler's quantum is 1/32);
    a sign or convention error in the pose rule is pixels off."""
    scene, n, (d_lo, d_hi) = bar_scene()
    worst = 0.0
    for lt, angle in align_ref.PLANTED + [((40.0, 30.0), 0.0), ((70.5, 66.125), -137.5)]:
        for c in planted_calipers(lt, angle, n, d_lo, 1) + [ref.cal(10.0, 5.0, phi, 33, 17, 2, 1, 0) for phi in PHIS]:
            lt_k, ak = ref.pose(lt, angle, c)
            m = ref.inverted(scene.shape[1], scene.shape[0], lt_k, ak)
            hw = (c["width"] - 1) / 2.0
            for i in (c["half"], 8, c["length"] - c["half"]):
                e = ref.derive(c, lt_k, ak, (i, 30, 100, 70))   # any record: only t matters
                t = e["t"]
                mx, my = m[0] * t + m[1] * hw + m[2], m[3] * t + m[4] * hw + m[5]
                worst = max(worst, abs(mx - e["sx"]), abs(my - e["sy"]))
            # and the template point goes to the source point through the hit's own pose
            ra = angle * ref.D2R
            sx = float(np.float32(lt[0])) + (e["tx"] * math.cos(ra) - e["ty"] * math.sin(ra))
            sy = float(np.float32(lt[1])) + (e["tx"] * math.sin(ra) + e["ty"] * math.cos(ra))
            assert abs(sx - e["sx"]) < 1e-4 and abs(sy - e["sy"]) < 1e-4
    print(f"source point vs patch matrix: max {worst:.6f} px")
    assert worst <= 1.0 / 64.0
