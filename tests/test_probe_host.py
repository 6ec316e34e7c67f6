"""Edge probes, host half (no GPU): struct layouts, fpm_probe_matrix, the restated integer sampler against the oracle,
fpm_probe_edges_host / fpm_probe_derive, the fits, every argument error, the builders and planted truth on the CPU
restatement (tests/probe_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import align_ref, oracle
from tests import probe_ref as ref
from tests.test_caliper_host import BAR_CENTRE, BAR_DIR, bar_scene

PHIS = [0.0, 90.0, 37.5, -137.5, 180.0]
SELECTS = ["nearest", "strongest", "first", "last"]


def test_struct_layouts(fpm_lib):
    assert C.sizeof(L.Probe) == M.PROBE_DTYPE.itemsize == 24
    assert C.sizeof(L.ProbeParams) == M.PROBE_PARAMS_DTYPE.itemsize == 32
    assert C.sizeof(L.ProbeRaw) == M.PROBE_RAW_DTYPE.itemsize == 24
    assert C.sizeof(L.ProbeResult) == M.PROBE_RESULT_DTYPE.itemsize == 64
    assert C.sizeof(L.ProbeSummary) == M.PROBE_SUMMARY_DTYPE.itemsize == 64
    off = lambda dt: [dt.fields[n][1] for n in dt.names]   # noqa: E731
    assert M.PROBE_DTYPE.names == ("x", "y", "phi") and off(M.PROBE_DTYPE) == [0, 8, 16]
    assert M.PROBE_PARAMS_DTYPE.names == ("length", "width", "half", "contrast", "polarity", "select", "reserved")
    assert off(M.PROBE_PARAMS_DTYPE) == [0, 4, 8, 12, 16, 20, 24]
    assert M.PROBE_RAW_DTYPE.names == ("index", "n_edges", "d_prev", "d", "d_next", "flags")
    assert off(M.PROBE_RAW_DTYPE) == [0, 4, 8, 12, 16, 20]
    assert M.PROBE_RESULT_DTYPE.names == ("index", "n_edges", "d", "flags", "dev", "contrast", "tx", "ty", "sx", "sy")
    assert off(M.PROBE_RESULT_DTYPE) == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56]
    assert M.PROBE_SUMMARY_DTYPE.names == ("n_found", "n_missing", "n_ambiguous", "n_outside", "worst", "reserved",
                                           "sum_dev", "sum_dev_sq", "max_abs_dev", "lt_x", "lt_y", "angle")
    assert off(M.PROBE_SUMMARY_DTYPE) == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 52, 56]
    for dt, ct in [(M.PROBE_DTYPE, L.Probe), (M.PROBE_PARAMS_DTYPE, L.ProbeParams), (M.PROBE_RAW_DTYPE, L.ProbeRaw),
                   (M.PROBE_RESULT_DTYPE, L.ProbeResult), (M.PROBE_SUMMARY_DTYPE, L.ProbeSummary)]:
        assert off(dt) == [getattr(ct, n).offset for n in dt.names]
    assert (L.PROBE_NEAREST, L.PROBE_STRONGEST, L.PROBE_FIRST, L.PROBE_LAST, L.PROBE_OUTSIDE) == (0, 1, 2, 3, 1)
    assert C.sizeof(L.LineFit) == C.sizeof(L.CircleFit) == 48


POSES = [((40.0, 30.0), 0.0), ((52.25, 41.5), 30.0), ((70.5, 66.125), -137.5), ((-7.375, 40.5), 90.0),
         ((120.3, 80.7), 17.0), ((0.0, 0.0), 180.0), ((1e5 + 0.3, -2e4), 359.999)]


def _grid_probes():
    ps = []
    for k, phi in enumerate(PHIS):
        ps.append((20.5 + k, 11.25, phi))
        ps.append((-13.0 - k, -4.5, phi + 0.125))       # a negative point
        ps.append((500.25, 300.0 + k, phi - 71.0))      # far beyond any template
    return ps


def test_matrix_equals_the_restatement(fpm_lib):
    grids = [ref.params(4, 1, 1), ref.params(24, 5), ref.params(64, 16, 8)]
    assert len(POSES) == 7 and len(_grid_probes()) == 15
    for lt, a in POSES:
        for k, p in enumerate(_grid_probes()):
            prm = grids[k % 3]
            got = M.probe_matrix(161, 97, lt, a, M.probe(*p), ref.record(prm)).reshape(-1).tolist()
            assert got == ref.matrix(161, 97, lt, a, p, prm), (lt, a, p, prm)
    # phi = 0 and ox = oy = 0: the composed matrix is the hit's inverted patch matrix itself
    prm = ref.params(24, 5)
    for lt, a in POSES:
        got = M.probe_matrix(161, 97, lt, a, M.probe(11.5, 2.0, 0.0), ref.record(prm)).reshape(-1).tolist()
        assert got == ref.inverted(161, 97, lt, a)
    # the centre sample lands where the pose puts the probe's point: lt + R (x, y)
    n = M.probe_matrix(161, 97, (50.0, 60.0), 20.0, M.probe(30.0, 12.0, 37.5), ref.record(ref.params(33, 9)))
    ca, sa = math.cos(20.0 * ref.D2R), math.sin(20.0 * ref.D2R)
    assert abs(n[0, 0] * 16 + n[0, 1] * 4 + n[0, 2] - (50.0 + (30.0 * ca - 12.0 * sa))) < 1e-4
    assert abs(n[1, 0] * 16 + n[1, 1] * 4 + n[1, 2] - (60.0 + (30.0 * sa + 12.0 * ca))) < 1e-4


@pytest.mark.parametrize("size", [(161, 97), (164, 100)])
def test_restated_sampler_equals_the_oracle(fpm_lib, oracle_lib, size):
    """With phi = 0 and ox = oy = 0 a probe's pixels are the patch (0, 0, L, W) of the pose: the integer sampler of
    tests/probe_ref.py against oracle.warp_affine of matcher.patch_matrix, inside the source and across each border."""
    sw, sh = size
    src = np.random.default_rng(sw).integers(0, 256, (sh, sw), dtype=np.uint8)
    poses = [((40.0, 30.0), 0.0), ((52.25, 41.5), 30.0), ((70.5, 66.125), -137.5),     # inside
             ((-7.375, 40.5), 10.0), ((sw - 9.5, 40.0), -20.0), ((60.0, -5.25), 33.0), ((60.0, sh - 3.5), -70.0),
             ((-3.0, -2.0), 0.0), ((sw - 2.0, sh - 2.0), 0.0), ((-300.0, 50.0), 45.0), ((sw + 40.0, sh + 40.0), 0.0)]
    for L_, W in [(4, 1), (24, 5), (33, 16), (64, 16), (63, 15)]:
        prm = ref.params(L_, W, 1)
        p = ((L_ - 1) / 2.0, (W - 1) / 2.0, 0.0)
        assert ref.geom(p, prm)[2:4] == (0.0, 0.0)
        for lt, a in poses:
            N = ref.matrix(sw, sh, lt, a, p, prm)
            I, out = ref.sample(src, [N], L_, W)
            want = oracle.warp_affine(src, M.patch_matrix(sw, sh, lt, a, (0, 0)), (L_, W))
            assert np.array_equal(I[0], want.astype(np.int64)), (L_, W, lt, a)
    # the OUTSIDE rule on a plain pose: tap origins 0 .. sw - 2 are inside, sw - 1 is the border path
    prm = ref.params(4, 1, 1)
    for x0, exp in [(0.0, False), (sw - 5.0, False), (sw - 4.0, True), (-0.25, True)]:
        N = [1.0, 0.0, x0, 0.0, 1.0, 3.0]
        assert bool(ref.sample(src, [N], 4, 1)[1][0]) == exp, x0


def _check(P, prm, label):
    """fpm_probe_edges_host and fpm_probe_derive on profile P against the restatement; returns the reference's record."""
    exp = ref.edges_raw(P, prm)
    raw = M.probe_edges_host(P, ref.record(prm))
    got = tuple(int(raw[f]) for f in ("index", "n_edges", "d_prev", "d", "d_next"))
    assert got == exp and int(raw["flags"]) == 0, f"{label}: {got} != {exp}"
    p, lt, a = (12.5, 3.0, 37.5), (33.25, -7.5), 61.0
    res = M.probe_derive([M.probe(*p)], ref.record(prm), lt, a, raw)[0]
    e = ref.derive(p, prm, lt, a, exp)
    for f in ref.RESULT_FIELDS:
        assert res[f].item() == e[f], f"{label}: record {exp} field {f}: {res[f].item()!r} != {e[f]!r}"
    assert -0.5 < e["delta"] <= 0.5
    return exp


@pytest.mark.parametrize("polarity", [1, -1, 0])
def test_edges_host_random_profiles(fpm_lib, polarity):
    rng = np.random.default_rng(300 + polarity)
    found = 0
    for k in range(200):
        L_ = int(rng.integers(4, 65))
        W = int(rng.integers(1, 17))
        s = int(rng.integers(1, min(8, L_ // 2) + 1))
        prm = ref.params(L_, W, s, int(rng.choice([1, 12, 60, 255])), polarity, SELECTS[k % 4])
        if k % 3 == 0:      # smooth: few edges, plateaus from the rounding
            P = np.rint(255 * W * (0.5 + 0.5 * np.sin(np.arange(L_) * rng.uniform(0.05, 0.6) + rng.uniform(0, 6))))
        elif k % 3 == 1:    # rough
            P = rng.integers(0, 255 * W + 1, L_)
        else:               # a few levels: equal neighbours, equal |D|
            P = rng.integers(0, 4, L_) * (255 * W // 3)
        found += _check(P.astype(np.int64), prm, f"random {k}")[0] > 0
    assert found > 100


def test_edges_host_hand_made_profiles(fpm_lib):
    # a sharp step: one edge, a symmetric triple, delta exactly 0
    prm = ref.params(16, 1, 1, 10, 0)
    e = _check([0] * 8 + [100] * 8, prm, "step")
    assert e == (8, 1, 0, 100, 0)
    d = ref.derive((5.0, 5.0, 0.0), prm, (0, 0), 0, e)
    assert d["delta"] == 0.0 and d["dev"] == 0.0 and d["tx"] == 5.0     # boundary 8 lies at 7.5 = hl: on the nominal point
    assert _check([100] * 8 + [0] * 8, ref.params(16, 1, 1, 10, -1), "falling step") == (8, 1, 0, -100, 0)
    assert _check([100] * 8 + [0] * 8, ref.params(16, 1, 1, 10, 1), "falling step, rising asked") == (0, 0, 0, 0, 0)
    # a two-sample ramp makes a plateau of D: the first sample is taken, delta = 0.5
    prm = ref.params(10, 1, 1, 10, 1)
    e = _check([0, 0, 0, 50, 100, 100, 100, 100, 100, 100], prm, "plateau")
    assert e == (3, 1, 0, 50, 50) and ref.derive((0, 0, 0), prm, (0, 0), 0, e)["delta"] == 0.5
    # an edge at i = s and at i = L - s
    prm = ref.params(8, 1, 2, 10, 0)
    assert _check([0, 0, 100, 100, 100, 100, 100, 100], prm, "i = s") == (2, 1, 0, 200, 100)
    assert _check([0, 0, 0, 0, 0, 0, 100, 100], prm, "i = L - s") == (6, 1, 100, 200, 0)
    # A == c s W is kept, one below is dropped
    prm = ref.params(12, 3, 1, 10, 0)
    assert _check([0] * 6 + [30] * 6, prm, "at the threshold") == (6, 1, 0, 30, 0)
    assert _check([0] * 6 + [29] * 6, prm, "below the threshold") == (0, 0, 0, 0, 0)
    # L = 2 s: one index
    assert _check([0, 0, 9, 9], ref.params(4, 1, 2, 1, 0), "L = 2 s") == (2, 1, 0, 18, 0)
    # all-equal profiles: none
    for v in (0, 77, 255 * 5):
        assert _check([v] * 40, ref.params(40, 5, 3, 1, 0), "flat") == (0, 0, 0, 0, 0)
    # two edges equidistant from the centre (|2 i - L| = 4 at i = 6 and 10 of 16), the second the stronger
    P = [0] * 6 + [50] * 4 + [200] * 6
    want = {"nearest": (6, 2, 0, 50, 0), "strongest": (10, 2, 0, 150, 0), "first": (6, 2, 0, 50, 0), "last": (10, 2, 0, 150, 0)}
    for sel in SELECTS:
        assert _check(P, ref.params(16, 1, 1, 10, 0, sel), f"equidistant, {sel}") == want[sel]
    # two of equal |D|, opposite polarity, not equidistant: strongest takes the lower index, nearest the nearer
    P = [0] * 3 + [90] * 8 + [0] * 5
    want = {"nearest": (11, 2, 0, -90, 0), "strongest": (3, 2, 0, 90, 0), "first": (3, 2, 0, 90, 0), "last": (11, 2, 0, -90, 0)}
    for sel in SELECTS:
        assert _check(P, ref.params(16, 1, 1, 10, 0, sel), f"equal |D|, {sel}") == want[sel]
    # the extreme: s W 255 = 32 640
    P = [0] * 8 + [4080] * 8 + [0] * 8
    for sel in SELECTS:
        e = _check(P, ref.params(24, 16, 8, 255, 0, sel), f"extreme, {sel}")
        assert abs(e[3]) == 32640 and e[1] == 2
    assert ref.derive((0, 0, 0), ref.params(24, 16, 8, 255, 0), (0, 0), 0, (8, 2, 28560, 32640, 28560))["contrast"] == 255.0


def _c_params(**kw):
    d = dict(length=16, width=4, half=2, contrast=12, polarity=0, select=0)
    d.update(kw)
    r = d.pop("reserved", (0, 0))
    p = L.ProbeParams(**d)
    p.reserved[0], p.reserved[1] = r
    return p


BAD_PARAMS = [dict(length=3), dict(length=65), dict(width=0), dict(width=17), dict(half=0), dict(half=9),
              dict(length=6, half=4), dict(contrast=0), dict(contrast=256), dict(polarity=2), dict(polarity=-2),
              dict(select=-1), dict(select=4), dict(reserved=(1, 0)), dict(reserved=(0, 1))]
BAD_PROBES = [dict(x=float("nan")), dict(y=float("inf")), dict(phi=float("-inf"))]


def test_argument_errors_leave_outputs_untouched(fpm_lib):
    n6 = (C.c_double * 6)(*[-1.5] * 6)
    raw = L.ProbeRaw(9, 9, 9, 9, 9, 9)
    out = (L.ProbeResult * 2)()
    C.memset(out, 0x5a, C.sizeof(out))
    lf, cf = L.LineFit(), L.CircleFit()
    C.memset(C.byref(lf), 0x5a, C.sizeof(lf))
    C.memset(C.byref(cf), 0x5a, C.sizeof(cf))
    prof = (C.c_int32 * 16)(*([0] * 8 + [100] * 8))
    good = (L.ProbeRaw * 2)(L.ProbeRaw(8, 1, 0, 400, 0, 0), L.ProbeRaw(8, 2, 10, 400, 20, 1))
    two = (L.Probe * 2)(L.Probe(1.0, 2.0, 3.0), L.Probe(4.0, 5.0, 6.0))

    def untouched():
        return (list(n6) == [-1.5] * 6 and tuple(getattr(raw, f) for f, _ in L.ProbeRaw._fields_) == (9,) * 6 and
                bytes(out) == b"\x5a" * C.sizeof(out) and bytes(lf) == b"\x5a" * 48 and bytes(cf) == b"\x5a" * 48)

    def matrix(prb, prm, sw=161, sh=97, ltx=1.0, lty=2.0, ang=3.0, o=n6):
        return fpm_lib.fpm_probe_matrix(sw, sh, ltx, lty, ang, prb, prm, o)

    def edges(prm, p=prof, r=C.byref(raw)):
        return fpm_lib.fpm_probe_edges_host(p, prm, r)

    def derive(prm, r, cnt, prbs=two, ltx=1.0, lty=2.0, ang=3.0, o=out):
        return fpm_lib.fpm_probe_derive(prbs, prm, ltx, lty, ang, r, cnt, o)

    ok, okp = C.byref(_c_params()), C.byref(two[0])
    INV = L.FPM_E_INVALID_ARG
    for bad in BAD_PARAMS:
        prm = C.byref(_c_params(**bad))
        assert matrix(okp, prm) == INV and edges(prm) == INV and derive(prm, good, 2) == INV, bad
    for bad in BAD_PROBES:
        prb = L.Probe(**{**dict(x=1.0, y=2.0, phi=3.0), **bad})
        assert matrix(C.byref(prb), ok) == INV, bad
        assert derive(ok, good, 2, prbs=(L.Probe * 2)(two[0], prb)) == INV, bad
    assert matrix(None, ok) == matrix(okp, None) == matrix(okp, ok, o=None) == INV
    assert matrix(okp, ok, sw=0) == matrix(okp, ok, sh=-1) == INV
    assert matrix(okp, ok, ltx=float("nan")) == matrix(okp, ok, lty=float("inf")) == matrix(okp, ok, ang=float("nan")) == INV
    assert edges(None) == edges(ok, p=None) == edges(ok, r=None) == INV
    for v in (-1, 255 * 4 + 1):      # of no 4 pixels
        assert edges(ok, p=(C.c_int32 * 16)(*([0] * 15 + [v]))) == INV
    assert derive(None, good, 2) == derive(ok, None, 2) == derive(ok, good, 2, o=None) == derive(ok, good, -1) == INV
    assert derive(ok, good, 2, prbs=None) == INV
    assert derive(ok, good, 2, ltx=float("nan")) == derive(ok, good, 2, ang=float("inf")) == INV
    # records that are no edge, behind a good one: nothing is written
    for r in [L.ProbeRaw(8, 1, 0, 0, 0, 0), L.ProbeRaw(8, 1, 500, 400, 0, 0), L.ProbeRaw(8, 1, 0, 400, 401, 0),
              L.ProbeRaw(8, 1, 400, 400, 400, 0), L.ProbeRaw(1, 1, 0, 400, 0, 0), L.ProbeRaw(15, 1, 0, 400, 0, 0),
              L.ProbeRaw(8, 1, 0, -400, -401, 0), L.ProbeRaw(8, 0, 0, 400, 0, 0), L.ProbeRaw(8, 17, 0, 400, 0, 0),
              L.ProbeRaw(0, 1, 0, 0, 0, 0), L.ProbeRaw(0, 0, 0, 5, 0, 0)]:
        assert derive(ok, (L.ProbeRaw * 2)(good[0], r), 2) == INV
    # fits
    pts = (C.c_double * 8)(0, 0, 1, 1, 2, 0, 3, 5)
    bad_pts = (C.c_double * 8)(0, 0, 1, float("nan"), 2, 0, 3, 5)
    fl, fc = fpm_lib.fpm_fit_line, fpm_lib.fpm_fit_circle
    assert fl(None, 4, 0.0, C.byref(lf)) == fl(pts, 1, 0.0, C.byref(lf)) == fl(pts, 4, 0.0, None) == INV
    assert fl(bad_pts, 4, 0.0, C.byref(lf)) == fl(pts, 4, -1.0, C.byref(lf)) == fl(pts, 4, float("nan"), C.byref(lf)) == INV
    assert fc(None, 4, 0.0, C.byref(cf)) == fc(pts, 2, 0.0, C.byref(cf)) == fc(pts, 4, 0.0, None) == INV
    assert fc(bad_pts, 4, 0.0, C.byref(cf)) == fc(pts, 4, -1.0, C.byref(cf)) == fc(pts, 4, float("inf"), C.byref(cf)) == INV
    assert untouched()
    # and the same calls with good arguments succeed
    assert matrix(okp, ok) == L.FPM_OK and edges(ok) == L.FPM_OK and (raw.index, raw.n_edges, raw.d, raw.flags) == (8, 1, 200, 0)
    assert derive(ok, good, 2) == L.FPM_OK and (out[1].index, out[1].n_edges, out[1].flags) == (8, 2, 1)
    assert derive(ok, (L.ProbeRaw * 2)(good[0], L.ProbeRaw(0, 0, 0, 0, 0, 1)), 2) == L.FPM_OK
    assert (out[1].index, out[1].flags, out[1].dev, out[1].sx) == (0, 1, 0.0, 0.0)
    assert derive(ok, None, 0, prbs=None, o=None) == L.FPM_OK
    assert fl(pts, 2, 0.0, C.byref(lf)) == L.FPM_OK and fc(pts, 3, 0.0, C.byref(cf)) == L.FPM_OK
    for bad in [dict(length=3), dict(half=9, length=32), dict(polarity=3), dict(contrast=0), dict(select="middle")]:
        with pytest.raises(ValueError):
            M.probe_params(**{**dict(length=16, width=4), **bad})
    with pytest.raises(ValueError):
        M.probe(float("nan"), 0.0, 0.0)


# ---- fits -------------------------------------------------------------------------------------------------------------
def _same(got, want, label):
    for k, v in want.items():
        assert got[k] == v, f"{label}: {k}: {got[k]!r} != {v!r}"


def test_fit_line(fpm_lib):
    rng = np.random.default_rng(5)
    for ang, (x0, y0) in [(0.0, (3.0, 4.0)), (90.0, (-2.5, 7.0)), (33.0, (100.25, -40.5)), (-71.5, (0.0, 0.0)), (-89.0, (5.0, 5.0))]:
        t = np.linspace(-30.0, 45.0, 25)
        c, s = math.cos(math.radians(ang)), math.sin(math.radians(ang))
        pts = np.stack([x0 + t * c, y0 + t * s], axis=1)
        got = M.fit_line(pts)
        _same(got, ref.fit_line(pts), f"line {ang}")
        assert abs(got["angle"] - ang) < 1e-9 and -90.0 < got["angle"] <= 90.0 and got["n_used"] == 25 and got["flags"] == 0
        assert got["rms"] < 1e-9 and got["max_resid"] < 1e-9
        # the point nearest the origin lies on the line and is perpendicular to the direction
        assert abs((got["px"] - x0) * -s + (got["py"] - y0) * c) < 1e-9 and abs(got["px"] * c + got["py"] * s) < 1e-9
        # one gross outlier: removed by trim, not without it
        bad = pts.copy()
        bad[7] += (-s * 25.0, c * 25.0)
        plain, trimmed = M.fit_line(bad), M.fit_line(bad, trim=5.0)
        _same(plain, ref.fit_line(bad), "outlier")
        _same(trimmed, ref.fit_line(bad, 5.0), "outlier trimmed")
        assert plain["n_used"] == 25 and plain["max_resid"] > 20.0
        assert trimmed["n_used"] == 24 and abs(trimmed["angle"] - ang) < 1e-9 and trimmed["max_resid"] < 1e-9
        noisy = pts + rng.normal(0, 0.3, pts.shape)
        _same(M.fit_line(noisy, 0.5), ref.fit_line(noisy, 0.5), "noisy")
    assert M.fit_line([(0, 0), (0, 1)])["angle"] == 90.0
    starved = M.fit_line([(0, 0), (1, 0), (2, 0.9)], trim=0.05)      # every point is farther than trim
    assert starved["flags"] == L.FIT_TRIM_STARVED and starved["n_used"] == 3


def test_fit_circle(fpm_lib):
    rng = np.random.default_rng(6)
    for (cx, cy, r), arc in [((171.4, 118.7, 41.3), 360.0), ((-20.0, 5.5, 3.25), 360.0), ((1000.5, -300.25, 250.0), 90.0)]:
        a = np.radians(np.linspace(10.0, 10.0 + arc, 40, endpoint=False))
        pts = np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], axis=1)
        got = M.fit_circle(pts)
        _same(got, ref.fit_circle(pts), f"circle {cx}")
        assert max(abs(got["cx"] - cx), abs(got["cy"] - cy), abs(got["r"] - r)) < 1e-9 and got["flags"] == 0
        assert got["n_used"] == 40 and got["rms"] < 1e-9 and got["max_resid"] < 1e-9
        bad = pts.copy()
        bad[11] += (0.6 * r, -0.4 * r)
        plain, trimmed = M.fit_circle(bad), M.fit_circle(bad, trim=0.2 * r)
        _same(plain, ref.fit_circle(bad), "outlier")
        _same(trimmed, ref.fit_circle(bad, 0.2 * r), "outlier trimmed")
        assert plain["n_used"] == 40 and max(abs(plain["cx"] - cx), abs(plain["cy"] - cy), abs(plain["r"] - r)) > 1e-3 * r
        assert trimmed["n_used"] == 39 and trimmed["flags"] == 0
        assert max(abs(trimmed["cx"] - cx), abs(trimmed["cy"] - cy), abs(trimmed["r"] - r)) < 1e-9
        noisy = pts + rng.normal(0, 0.2, pts.shape)
        _same(M.fit_circle(noisy, 0.4), ref.fit_circle(noisy, 0.4), "noisy")
    col = M.fit_circle([(0.0, 0.0), (1.0, 2.0), (2.0, 4.0), (5.0, 10.0)])
    _same(col, ref.fit_circle([(0.0, 0.0), (1.0, 2.0), (2.0, 4.0), (5.0, 10.0)]), "collinear")
    assert col["flags"] == L.FIT_COLLINEAR and (col["cx"], col["cy"], col["r"]) == (0.0, 0.0, 0.0)


# ---- builders ---------------------------------------------------------------------------------------------------------
def test_builders(fpm_lib):
    c = M.circle_probes(10.0, 20.0, 5.0, 4)
    assert np.allclose(c["x"], [15, 10, 5, 10]) and np.allclose(c["y"], [20, 25, 20, 15]) and c["phi"].tolist() == [0, 90, 180, 270]
    assert M.circle_probes(10.0, 20.0, 5.0, 4, outward=False)["phi"].tolist() == [180, 270, 360, 450]
    ln = M.line_probes((0.0, 0.0), (10.0, 0.0), 5)
    assert np.allclose(ln["x"], [1, 3, 5, 7, 9]) and not ln["y"].any() and np.allclose(ln["phi"], 90.0)
    assert np.allclose(M.line_probes((0.0, 0.0), (0.0, 4.0), 2, normal_side=-1)["phi"], 0.0)
    for bad in [lambda: M.circle_probes(0, 0, 0.0, 4), lambda: M.circle_probes(0, 0, 1.0, 0),
                lambda: M.line_probes((1, 1), (1, 1), 3), lambda: M.line_probes((0, 0), (1, 1), 3, normal_side=0),
                lambda: M.contour_probes(np.zeros((8, 8), np.float32), 2, 10), lambda: M.contour_probes(np.zeros((8, 8), np.uint8), 0, 10)]:
        with pytest.raises(ValueError):
            bad()
    assert len(M.contour_probes(np.full((20, 20), 9, np.uint8), 2.0, 5.0)) == 0


# ---- planted truth, on the CPU restatement ----------------------------------------------------------------------------
DISC_CENTRE, DISC_R, DISC_LOW, DISC_HIGH = (171.4, 118.7), 41.3, 40, 200
# measured on the restatement: see the tests' docstrings and DESIGN.md section 25
DISC_CENTRE_MAX, DISC_RADIUS_MAX = 0.0026, 0.0202      # px
BAR_LINE_MAX, BAR_ANGLE_MAX = 0.0017, 0.0021           # px, degrees
CONTOUR_PHI_MAX = 3.1969                               # degrees


def disc_scene(w=320, h=240, centre=DISC_CENTRE, r=DISC_R):
    """A bright disc on a dark ground rendered by area coverage: 16 x 16 sub-samples per pixel (pixel (x, y) is the
    square x +- 0.5, y +- 0.5) where the rim passes, 0 or 1 elsewhere."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    dist = np.hypot(xx - centre[0], yy - centre[1])
    cov = (dist < r).astype(np.float64)
    sub = (np.arange(16) + 0.5) / 16.0 - 0.5
    for y, x in zip(*np.nonzero(np.abs(dist - r) < 0.75)):
        cov[y, x] = (np.hypot(x + sub[None, :] - centre[0], y + sub[:, None] - centre[1]) < r).mean()
    return np.rint(DISC_LOW + (DISC_HIGH - DISC_LOW) * cov).astype(np.uint8)


def to_template(lt, angle, p):
    """The template point of the source point p for a frame at (lt, angle), by the header's rule: R^-1 (p - lt)."""
    ra = angle * ref.D2R
    ca, sa = math.cos(ra), math.sin(ra)
    dx, dy = p[0] - float(np.float32(lt[0])), p[1] - float(np.float32(lt[1]))
    return ca * dx + sa * dy, -sa * dx + ca * dy


def planted_disc_errors():
    scene = disc_scene()
    prm = ref.params(16, 5, 2, 20, 0)
    worst_c = worst_r = 0.0
    for lt, angle in align_ref.PLANTED:
        cx, cy = to_template(lt, angle, DISC_CENTRE)
        for outward in (True, False):
            ps = [tuple(p) for p in M.circle_probes(cx, cy, DISC_R, 64, outward=outward)]
            s, res, P = ref.measure(scene, lt, angle, ps, prm)
            assert s["n_found"] == 64 and s["n_ambiguous"] == 0 and s["n_outside"] == 0, s
            assert all(r["n_edges"] == 1 and (r["d"] < 0) == outward for r in res)
            # the library's host entries give the same records from the same profiles
            for k in (0, 17, 63):
                raw = M.probe_edges_host(P[k], ref.record(prm))
                got = M.probe_derive([M.probe(*ps[k])], ref.record(prm), lt, angle, raw)[0]
                assert all(got[f].item() == res[k][f] for f in ref.RESULT_FIELDS)
            fit = M.fit_circle([(r["sx"], r["sy"]) for r in res])
            assert fit["flags"] == 0 and fit["n_used"] == 64
            worst_c = max(worst_c, math.hypot(fit["cx"] - DISC_CENTRE[0], fit["cy"] - DISC_CENTRE[1]))
            worst_r = max(worst_r, abs(fit["r"] - DISC_R))
            tfit = M.fit_circle([(r["tx"], r["ty"]) for r in res])      # and in the template frame
            worst_c = max(worst_c, math.hypot(tfit["cx"] - cx, tfit["cy"] - cy))
            worst_r = max(worst_r, abs(tfit["r"] - DISC_R))
    return worst_c, worst_r


def test_planted_disc_on_the_restatement(fpm_lib):
    """A 320 x 240 scene with a disc of centre (171.4, 118.7) and radius 41.3 rendered by area coverage, a template frame
    at tests/align_ref.py's two PLANTED poses, 64 circle_probes of 16 x 5 samples (s = 2), outward and inward.  Every
    probe finds exactly one edge of the polarity its direction implies.  The fitted circle, from the source points and
    from the template points, against the planted one -- measured on the restatement: see
    DISC_CENTRE_MAX and DISC_RADIUS_MAX.  The test asserts at most twice the measured maxima, and in any case below half
    a sample."""
    worst_c, worst_r = planted_disc_errors()
    print(f"planted disc: centre error max {worst_c:.4f} px, radius error max {worst_r:.4f} px")
    assert worst_c < 0.5 and worst_r < 0.5
    assert worst_c <= 2 * DISC_CENTRE_MAX and worst_r <= 2 * DISC_RADIUS_MAX


def planted_bar_errors():
    scene, n, (d_lo, d_hi) = bar_scene()
    prm = ref.params(16, 5, 2, 20, 0)
    d0 = n[0] * BAR_CENTRE[0] + n[1] * BAR_CENTRE[1]
    worst_d = worst_a = 0.0
    for lt, angle in align_ref.PLANTED:
        for d_edge in (d_lo, d_hi):
            ends = []
            for along in (-40.0, 40.0):      # two points of the edge, in source coordinates (n = (-sin, cos) of BAR_DIR)
                ends.append((BAR_CENTRE[0] + along * n[1] + (d_edge - d0) * n[0], BAR_CENTRE[1] - along * n[0] + (d_edge - d0) * n[1]))
            for side in (1, -1):
                ps = [tuple(p) for p in M.line_probes(to_template(lt, angle, ends[0]), to_template(lt, angle, ends[1]), 32, side)]
                s, res, P = ref.measure(scene, lt, angle, ps, prm)
                assert s["n_found"] == 32 and s["n_ambiguous"] == 0 and s["n_outside"] == 0, s
                fit = M.fit_line([(r["sx"], r["sy"]) for r in res])
                c, sn = math.cos(math.radians(fit["angle"])), math.sin(math.radians(fit["angle"]))
                for ex, ey in ends:      # the distance of the planted edge's end points from the fitted line
                    worst_d = max(worst_d, abs((ex - fit["px"]) * -sn + (ey - fit["py"]) * c))
                da = (fit["angle"] - BAR_DIR + 90.0) % 180.0 - 90.0
                worst_a = max(worst_a, abs(da))
    return worst_d, worst_a


def test_planted_bar_on_the_restatement(fpm_lib):
    """The caliper test's planted bar (exact area coverage, edges known analytically): 32 line_probes of 16 x 5 samples
    (s = 2) along 80 px of each edge, on either side, at the two PLANTED poses.  Every probe finds exactly one edge.
    The fitted line against the planted edge: the distance of the edge's end points from it and the angle -- measured on
    the restatement: see BAR_LINE_MAX and BAR_ANGLE_MAX.  At most twice the measured maxima, and
    in any case below half a sample (over the 80 px: 0.5 / 40 rad)."""
    worst_d, worst_a = planted_bar_errors()
    print(f"planted bar: line distance max {worst_d:.4f} px, angle error max {worst_a:.4f} deg")
    assert worst_d < 0.5 and worst_a < math.degrees(0.5 / 40.0)
    assert worst_d <= 2 * BAR_LINE_MAX and worst_a <= 2 * BAR_ANGLE_MAX


def contour_errors():
    centre, r = (63.6, 64.2), DISC_R
    tmpl = disc_scene(128, 128, centre, r)
    out = []
    for step in (1.0, 3.0):
        ps = M.contour_probes(tmpl, step, 20.0)
        again = M.contour_probes(tmpl, step, 20.0)
        assert ps.tobytes() == again.tobytes()                             # deterministic
        assert len(ps) > 2 * math.pi * r / (3.0 * step)
        xy = np.stack([ps["x"], ps["y"]], axis=1)
        d = np.hypot(xy[:, None, 0] - xy[None, :, 0], xy[:, None, 1] - xy[None, :, 1])
        assert d[np.triu_indices(len(ps), 1)].min() >= step
        assert np.all(np.lexsort((ps["x"], ps["y"])) == np.arange(len(ps)))   # row-major order
        rad = np.hypot(ps["x"] - centre[0], ps["y"] - centre[1])
        inward = np.degrees(np.arctan2(centre[1] - ps["y"], centre[0] - ps["x"]))   # dark to bright: towards the centre
        dphi = (ps["phi"] - inward + 180.0) % 360.0 - 180.0
        out.append((float(np.abs(rad - r).max()), float(np.abs(dphi).max())))
    half = np.zeros((128, 128), np.uint8)
    half[:, :64] = 1
    masked = M.contour_probes(tmpl, 3.0, 20.0, mask=half)
    assert 0 < len(masked) < len(M.contour_probes(tmpl, 3.0, 20.0)) and masked["x"].max() < 64
    return max(o[0] for o in out), max(o[1] for o in out)


def test_contour_probes_on_the_disc(fpm_lib):
    """contour_probes on a taught 128 x 128 image of the disc (the same rendering), step 1 and 3, min_contrast 20: the
    result is deterministic, in row-major order and thinned to the step; every probe point lies within one pixel of the
    true circle, and every phi within a bound of the radial direction towards the centre (dark to bright) -- measured
    (DESIGN.md section 25): see CONTOUR_PHI_MAX; the test asserts at most twice that and in any case below 45 degrees,
    the width of a Sobel direction bin."""
    worst_d, worst_phi = contour_errors()
    print(f"contour probes: radial distance max {worst_d:.4f} px, phi error max {worst_phi:.4f} deg")
    assert worst_d <= 1.0
    assert worst_phi < 45.0 and worst_phi <= 2 * CONTOUR_PHI_MAX
