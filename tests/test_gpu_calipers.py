"""Edge calipers on the HIP path (fpm_calipers_at / fpm_last_calipers): k_caliper's profiles, raw records, counts and the
derived doubles against the restatement of tests/caliper_ref.py (the oracle's warpAffine of fpm_patch_matrix's matrix on
caliper-sized patches, then exact integers and Python floats in the header's order).  Every comparison is ==."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import caliper_ref as ref
from tests.cases import CASES
from tests.test_gpu_align import EDGE_POSES

pytestmark = pytest.mark.gpu

LENGTHS = [2, 3, 4, 5, 63, 64, 65, 129, 1024]
WIDTHS = [1, 15, 16, 17, 33, 256]
PHIS = [0.0, 90.0, 37.5, -137.5]
# the source's four sides crossed by a 64-sample caliper about (35.5, 11), and one pose wholly outside for every caliper
SIDE_POSES = [((-40.0, 50.0), 0.0), ((150.0, 50.25), 0.0), ((60.5, -20.0), 0.0), ((60.0, 112.0), 0.0)]
FAR_POSE = ((5000.0, 5000.0), 0.0)


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


def paired_calipers():
    """Every length and every width with every phi at least once (9 >= 6: the width index runs with the length's,
    shifted per phi), and over them every half in {1, 2, 16} (as far as the length admits it) with every polarity,
    and every contrast in {1, 12, 255}."""
    cals = []
    for p, phi in enumerate(PHIS):
        for i, n in enumerate(LENGTHS):
            half = min((1, 2, 16)[(i + p) % 3], n // 2)
            cals.append(ref.cal(35.5 + 0.25 * i, 11.0 - 0.5 * p, phi, n, WIDTHS[(i + p) % len(WIDTHS)], half,
                                (1, 12, 255)[(len(cals) // 4) % 3], (1, -1, 0)[(i + 2 * p) % 3]))
    assert {(c["length"], c["phi"]) for c in cals} == {(n, phi) for n in LENGTHS for phi in PHIS}
    assert {(c["width"], c["phi"]) for c in cals} == {(w, phi) for w in WIDTHS for phi in PHIS}
    big = [c for c in cals if c["length"] >= 63]
    assert {(c["half"], c["polarity"]) for c in big} == {(s, p) for s in (1, 2, 16) for p in (1, -1, 0)}
    assert {c["contrast"] for c in big} == {1, 12, 255}
    return cals


def _run(hip, srcs, idx, poses, cals, cap, label, profiles=True):
    lts, angs = [p[0] for p in poses], [p[1] for p in poses]
    out = hip.calipers_at(idx, lts, angs, [ref.record(c) for c in cals], cap=cap, profiles=profiles)
    summary, edges = out[0], out[1]
    assert summary.dtype == M.CALIPER_SUMMARY_DTYPE and edges.dtype == M.EDGE_DTYPE
    ref.assert_call(summary, edges, out[2] if profiles else None, srcs, idx, lts, angs, cals, cap, label)
    return out


@pytest.mark.parametrize("sw", [161, 164])
def test_profiles_edges_and_summaries(hip, sw):
    sh = 119
    rng = np.random.default_rng(sw)
    src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    # smooth the left half: fewer, wider edges there; the right half stays rough (more edges than capacity at contrast 1)
    src[:, :sw // 2] = (src[:, :sw // 2].astype(np.int32) // 64 * 64 + 31).astype(np.uint8)
    hip.resetParams()
    assert hip.learnPattern(rng.integers(0, 256, (23, 71), dtype=np.uint8))
    hip.stage([src])
    cals = paired_calipers()
    poses = EDGE_POSES + SIDE_POSES + [FAR_POSE]
    summary, edges, prof = _run(hip, [src], [0] * len(poses), poses, cals, 8, f"sw {sw}")
    assert prof.shape == (len(poses), len(cals), 1024)
    # the pose wholly outside: zeros, no edge, flagged
    assert not prof[-1].any() and not summary[-1]["n_edges"].any() and (summary[-1]["flags"] == L.CALIPER_OUTSIDE).all()
    # a caliper inside the source is not flagged; the rough half overflows the capacity somewhere
    inside = [k for k, c in enumerate(cals) if c["length"] <= 5 and c["width"] <= 17]
    assert inside and not (summary[0, inside]["flags"] & L.CALIPER_OUTSIDE).any()
    assert (summary["flags"] & L.CALIPER_TRUNCATED).any() and (summary["n_edges"] > 0).sum() > 50
    assert ((summary["n_edges"] > 0) & (summary["n_edges"] <= 8)).any()
    # without the profiles the records are the same bytes
    s2, e2 = hip.calipers_at([0] * len(poses), [p[0] for p in poses], [p[1] for p in poses],
                             [ref.record(c) for c in cals], cap=8)
    assert s2.tobytes() == summary.tobytes() and e2.tobytes() == edges.tobytes()


def test_saturated_checker(hip):
    """A 0 / 255 checker whose cells are 16 samples along the scan and 256 across it, the caliper's 256 rows on one row
    of cells: P alternates between 0 and 65280 and |d| reaches 1,044,480 (W = 256, s = 16).  Half a cell lower every
    column holds 128 bright pixels and nothing steps; a square 16 x 16 checker does the same at any offset."""
    yy, xx = np.mgrid[0:560, 0:200]
    tall = np.where((xx // 16 + yy // 256) % 2 == 1, 255, 0).astype(np.uint8)
    square = np.where((xx // 16 + yy // 16) % 2 == 1, 255, 0).astype(np.uint8)
    hip.resetParams()
    assert hip.learnPattern(np.random.default_rng(1).integers(0, 256, (23, 71), dtype=np.uint8))
    hip.stage([tall, square])
    c = ref.cal(16 + 63.5, 127.5, 0.0, 128, 256, 16, 255, 0)
    poses = [((0.0, 0.0), 0.0), ((0.0, 128.0), 0.0), ((3.0, 256.0), 0.0), ((0.0, 7.0), 0.0)]
    idx = [0, 0, 0, 1]
    summary, edges, prof = _run(hip, [tall, square], idx, poses, [c], 8, "checker")
    assert set(np.unique(prof[0, 0, :128])) == {0, 65280} and prof.max() == 65280
    assert summary[0, 0]["n_edges"] == 7 and set(np.abs(edges[0, 0, :7]["d"])) == {1044480}
    assert (edges[0, 0, :7]["contrast"] == 255.0).all() and edges[0, 0, :7]["index"].tolist() == list(range(16, 128, 16))
    assert (edges[0, 0, 1:6]["t"] == edges[0, 0, 1:6]["index"] - 0.5).all()     # symmetric triples off the range's ends
    assert summary[1, 0]["n_edges"] == 0 and set(np.unique(prof[1, 0, :128])) == {32640}
    assert summary[2, 0]["n_edges"] >= 6 and summary[3, 0]["n_edges"] == 0


@pytest.mark.parametrize("cap", [1, 8, 64])
def test_more_edges_than_capacity(hip, cap):
    yy, xx = np.mgrid[0:40, 0:1100]
    src = np.where(xx % 4 < 2, 255, 0).astype(np.uint8)
    hip.resetParams()
    assert hip.learnPattern(np.random.default_rng(2).integers(0, 256, (23, 71), dtype=np.uint8))
    hip.stage([src])
    cals = [ref.cal(20 + 511.5, 15.5, 0.0, 1024, 8, 1, 50, pol) for pol in (0, 1, -1)]
    summary, edges, _ = _run(hip, [src], [0], [((0.0, 0.0), 0.0)], cals, cap, f"stripes cap {cap}")
    assert summary[0]["n_edges"].tolist() == [511, 256, 255] or summary[0]["n_edges"].tolist() == [511, 255, 256]
    assert (summary[0]["flags"] == L.CALIPER_TRUNCATED).all() and (summary[0]["n_returned"] == cap).all()
    assert (np.diff(edges[0, 0]["index"]) == 2).all() if cap > 1 else True     # the first cap by index, none skipped


def test_mixed_calipers_and_permutation(hip):
    rng = np.random.default_rng(77)
    srcs = [rng.integers(0, 256, (119, 164), dtype=np.uint8) // 32 * 32 for _ in range(2)]
    srcs = [np.ascontiguousarray(s.astype(np.uint8)) for s in srcs]
    hip.resetParams()
    assert hip.learnPattern(rng.integers(0, 256, (23, 71), dtype=np.uint8))
    hip.stage(srcs)
    cals = [ref.cal(35.5, 11.0, 0.0, 64, 24, 2, 12, 1), ref.cal(10.0, 5.5, 90.0, 129, 3, 1, 30, -1),
            ref.cal(60.25, 20.0, 37.5, 5, 17, 2, 1, 0), ref.cal(-8.0, 30.0, -137.5, 200, 33, 16, 5, 0),
            ref.cal(35.5, 11.0, 180.0, 2, 1, 1, 1, 0), ref.cal(20.0, 0.0, 12.25, 65, 16, 3, 20, 1),
            ref.cal(50.0, 12.0, -90.0, 100, 40, 7, 8, -1)]
    poses = EDGE_POSES + [SIDE_POSES[0], ((90.5, 60.0), 77.0)]
    idx = [0, 1, 0, 1, 1]
    summary, edges, prof = _run(hip, srcs, idx, poses, cals, 8, "mixed")
    perm = [3, 6, 0, 5, 2, 1, 4]
    s2, e2, p2 = _run(hip, srcs, idx, poses, [cals[k] for k in perm], 8, "mixed, permuted")
    assert s2.tobytes() == np.ascontiguousarray(summary[:, perm]).tobytes()
    assert e2.tobytes() == np.ascontiguousarray(edges[:, perm]).tobytes()
    assert np.array_equal(p2, prof[:, perm])
    again = hip.calipers_at(idx, [p[0] for p in poses], [p[1] for p in poses], [ref.record(c) for c in cals], cap=8,
                            profiles=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (summary, edges, prof)))


# ---- over the hits of a search ----------------------------------------------------------------------------------------
def _search(m, templates, bitwise_not=False):
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    m.resetParams()
    for k, v in prm.items():
        setattr(m._params, k, v)
    m.setBitwiseNot(bitwise_not)
    assert m.learnPattern(t)
    m.stage([np.ascontiguousarray(255 - s) if bitwise_not else s])
    res = m.match_staged()
    assert len(res[0]) == 3
    ps = [(r.ptLT, r.dMatchedAngle) for r in res[0]]     # Qt semantics: the raw pose
    return s, t, [p[0] for p in ps], [p[1] for p in ps]


def _hit_calipers(t):
    th, tw = t.shape
    return [ref.cal(tw / 2.0, th / 2.0, 0.0, min(tw, 64), 9, 2, 12, 0), ref.cal(tw / 2.0, 2.0, 90.0, 24, 15, 2, 12, 1),
            ref.cal(3.0, th / 2.0, 0.0, 20, 11, 1, 20, 0), ref.cal(tw / 3.0, th / 3.0, 37.5, 33, 5, 3, 8, -1)]


def test_last_calipers_after_a_search(hip, templates):
    s, t, lts, angs = _search(hip, templates)
    cals = _hit_calipers(t)
    recs = [ref.record(c) for c in cals]
    got = hip.last_calipers(recs, source=0, cap=8, profiles=True)
    ref.assert_call(*got, [s], [0, 0, 0], lts, angs, cals, 8, "last_calipers")
    assert (got[0]["n_edges"] > 0).any()
    at = hip.calipers_at(0, lts, angs, recs, cap=8, profiles=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, at))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hip.last_calipers(recs, source=-1, cap=8), got[:2]))
    # after adoption the calipers sample at the aligned poses
    al = hip.align_last(0, adopt=True)
    assert (al["best_eval"] > 0).any(), "no hit moved: the test shows nothing"
    alt, aang = np.stack([al["lt_x"], al["lt_y"]], 1), al["angle"]
    got2 = hip.last_calipers(recs, source=0, cap=8, profiles=True)
    at2 = hip.calipers_at(0, alt, aang, recs, cap=8, profiles=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got2, at2))
    assert got2[0].tobytes() != got[0].tobytes()
    ref.assert_call(*got2, [s], [0, 0, 0], [tuple(p) for p in alt.tolist()], aang.tolist(), cals, 8, "adopted")


def test_last_calipers_under_bitwise_not(hip, templates):
    s, t, lts, angs = _search(hip, templates, bitwise_not=True)     # staged: 255 - s; sampled: the inverted plane, s
    try:
        cals = _hit_calipers(t)
        got = hip.last_calipers([ref.record(c) for c in cals], source=0, cap=8, profiles=True)
        ref.assert_call(*got, [s], [0, 0, 0], lts, angs, cals, 8, "bitwise_not")
        assert (got[0]["n_edges"] > 0).any()
    finally:
        hip.setBitwiseNot(False)


# ---- state ----------------------------------------------------------------------------------------------------------
def _results(m, n_src):
    n = (C.c_int32 * n_src)()
    m._lib.fpm_last_results(m._ctx, None, 0, n)
    out = (L.Result * max(sum(n), 1))()
    assert m._lib.fpm_last_results(m._ctx, out, sum(n), n) == L.FPM_OK
    return bytes(out), list(n)


def test_state_rules(gpu_matcher_factory, templates):
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    m = gpu_matcher_factory(**prm)
    cals = [ref.record(c) for c in _hit_calipers(t)]
    arr = M._calipers(cals)
    pc = arr.ctypes.data_as(C.POINTER(L.Caliper))
    n = C.c_int32(-1)
    with pytest.raises(ValueError):
        m.last_calipers(cals)                                   # no template, nothing staged
    with pytest.raises(ValueError, match="no staged sources"):
        m.calipers_at(0, [(10.0, 10.0)], [0.0], cals)
    assert m.learnPattern(t)
    with pytest.raises(ValueError, match="no staged sources"):
        m.last_calipers(cals)
    m.stage([s])
    with pytest.raises(ValueError, match="no search has run"):
        m.last_calipers(cals)
    assert m.calipers_at(0, [(10.0, 10.0)], [5.0], cals)[0].shape == (1, 4)      # poses of the caller's need no search
    m.match_staged_launch()
    for call in (lambda: m.last_calipers(cals), lambda: m.calipers_at(0, [(10.0, 10.0)], [0.0], cals)):
        with pytest.raises(ValueError, match="in flight"):
            call()
    counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [3]
    results, cands = _results(m, 1), m.last_candidates(0).tobytes()
    patches = m.last_patches(0).tobytes()
    # the count-only call, then a capacity below the count: FPM_E_CAPACITY, nothing written
    rc = m._lib.fpm_last_calipers(m._ctx, 0, pc, 4, 8, None, None, None, 0, 0, C.byref(n))
    assert rc == L.FPM_E_CAPACITY and n.value == 3
    summary, edges = np.zeros((3, 4), M.CALIPER_SUMMARY_DTYPE), np.zeros((3, 4, 8), M.EDGE_DTYPE)
    stride = int(arr["length"].max())
    prof = np.zeros((3, 4, stride), np.int32)
    ps, pe, pp = (summary.ctypes.data_as(C.POINTER(L.CaliperSummary)), edges.ctypes.data_as(C.POINTER(L.Edge)),
                  prof.ctypes.data_as(C.POINTER(C.c_int32)))

    def untouched():
        return not summary.tobytes().strip(b"\0") and not edges.tobytes().strip(b"\0") and not prof.any()

    rc = m._lib.fpm_last_calipers(m._ctx, 0, pc, 4, 8, ps, pe, pp, stride, 2, C.byref(n))
    assert rc == L.FPM_E_CAPACITY and n.value == 3 and untouched()
    m.profile(True)
    try:
        m.profile_reset()
        # arguments out of range: FPM_E_INVALID_ARG, nothing launched, nothing written
        for ncal, cap_per, st, pcal in [(0, 8, stride, pc), (65, 8, stride, pc), (4, 0, stride, pc), (4, 65, stride, pc),
                                        (4, 8, stride - 1, pc), (4, 8, stride, None)]:
            rc = m._lib.fpm_last_calipers(m._ctx, 0, pcal, ncal, cap_per, ps, pe, pp, st, 3, C.byref(n))
            assert rc == L.FPM_E_INVALID_ARG and untouched(), (ncal, cap_per, st)
        assert m._lib.fpm_last_calipers(m._ctx, 0, pc, 4, 8, None, pe, pp, stride, 3, C.byref(n)) == L.FPM_E_INVALID_ARG
        assert m._lib.fpm_last_calipers(m._ctx, 0, pc, 4, 8, ps, None, pp, stride, 3, C.byref(n)) == L.FPM_E_INVALID_ARG
        assert m._lib.fpm_last_calipers(m._ctx, 1, pc, 4, 8, ps, pe, pp, stride, 3, C.byref(n)) == L.FPM_E_INVALID_ARG
        for field, v in [("length", 1), ("width", 257), ("half", 17), ("contrast", 0), ("polarity", 2), ("reserved", 1),
                         ("cx", float("nan")), ("phi", float("inf"))]:
            bad = arr.copy()
            bad[2][field] = v
            rc = m._lib.fpm_last_calipers(m._ctx, 0, bad.ctypes.data_as(C.POINTER(L.Caliper)), 4, 8, ps, pe, pp, stride, 3,
                                          C.byref(n))
            assert rc == L.FPM_E_INVALID_ARG and untouched(), field
        far = arr.copy()
        far[1]["cx"] = 3e6                                       # a sampling pose beyond the samplers' 2^20 range
        rc = m._lib.fpm_last_calipers(m._ctx, 0, far.ctypes.data_as(C.POINTER(L.Caliper)), 4, 8, ps, pe, pp, stride, 3, C.byref(n))
        assert rc == L.FPM_E_INVALID_ARG and untouched()
        with pytest.raises(ValueError):
            m.calipers_at(1, [(10.0, 10.0)], [5.0], cals)       # source index past the batch
        with pytest.raises(ValueError):
            m.calipers_at(0, [(2e6, 10.0)], [5.0], cals)
        with pytest.raises(ValueError):
            m.last_calipers(cals, cap=65)
        with pytest.raises(ValueError):
            m.last_calipers([cals[0]] * 65)
        assert m.caliper_profile() == (0.0, 0, 0)
        # one launch per call, bytes = L W per job + the records, counts and profiles written
        m.last_calipers(cals, source=0, cap=8)
        area = sum(int(c["length"]) * int(c["width"]) for c in arr)
        ms, launches, nbytes = m.caliper_profile()
        assert launches == 1 and ms > 0 and nbytes == 3 * area + 12 * (8 * 16 + 4)
        m.last_calipers(cals, source=-1, cap=4, profiles=True)
        m.calipers_at(0, [(10.0, 10.0)] * 5, [5.0] * 5, cals[:2], cap=1)
        ms, launches, nbytes = m.caliper_profile()
        assert launches == 3 and m.profile_get(L.K_PATCH)[1] == 0 and m.profile_get(L.K_COMPARE)[1] == 0
        assert len(L.KERNEL_NAMES) == 15 and len(L.PROFILE_NAMES) == 16     # no FPM_K_* index was added
        m.profile_reset()
        assert m.caliper_profile() == (0.0, 0, 0)
    finally:
        m.profile(False)
    rc = m._lib.fpm_last_calipers(m._ctx, 0, pc, 4, 8, ps, pe, pp, stride, 3, C.byref(n))
    assert rc == L.FPM_OK and n.value == 3 and summary["n_edges"].sum() > 0 and not untouched()
    # the search's records and the poses are what they were, and a following search returns what it returned
    assert _results(m, 1) == results and m.last_candidates(0).tobytes() == cands and m.last_patches(0).tobytes() == patches
    assert len(m.match_staged()[0]) == 3 and _results(m, 1) == results and m.last_candidates(0).tobytes() == cands
    m.stage([s])                                                # staged again, not searched
    with pytest.raises(ValueError, match="no search has run"):
        m.last_calipers(cals)
    m.match_staged_candidates()                                 # a search without results
    none = m.last_calipers(cals, source=-1)
    assert none[0].shape == (0, 4) and none[1].shape == (0, 4, 8)
