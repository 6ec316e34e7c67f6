"""The top-layer scores of the matrix-core form (top_mma_body: k_top_mma's candidate lists, k_top_map's full maps) and
of the split chain, map by map against the oracle's kept maps (gfx950 required).  fpm_op_top_maps runs the search's own
plan, job tables, work units and launchers and hands back what they computed; every f32 score must equal the oracle's
bit for bit (compared as uint32, so -0.0 and +0.0 differ).  No tolerance anywhere.

Each test asserts from the operator's stats that it reached the path it was written for: two or more strips, more
than one row run per strip, and the kernel instantiation the shape is meant to exercise.

List thresholds, picked on the CPU with the oracle (tests/top_map_cases.py scenes, 470 x 310, +-180 deg): per map
(min, max) and total count of pixels with (double)v >= thr.  "in": every job within the list capacity (512; 8192 in
block mode) and at least 500 entries in all; "over": at least one job overflows.

  scene      top      angles  in: thr  (min, max, total)     over: thr  (min, max, total)
  noise      16 x 16    53     0.32    (15, 293, 3364)         0.25     (195, 1022, 24698)
  noise      14 x 14    47     0.35    (40, 137, 5163)         0.30     (189, 584, 18023)
  noise      12 x 9     41     0.42    (77, 466, 9124)         0.35     (387, 1058, 30966)
  noise      17 x 15    55     0.32    (32, 337, 8602)         0.25     (275, 1131, 44337)
  noise      43 x 6    137     0.30    (11, 255, 5646)         0.25     (101, 617, 30441)
  noise      49 x 16   157     0.15    (118, 291, 28360)       0.12     (497, 1074, 115310)
  noise      17 x 32   103     0.20    (57, 262, 15134)        0.15     (504, 1339, 91103)
  saturated  16 x 16    53     0.25    (9, 193, 3406)          0.20     (154, 1235, 29130)
  saturated  12 x 9     41     0.32    (71, 495, 11345)        0.25     (301, 1436, 42347)
  saturated  43 x 6    137     0.25    (10, 151, 9862)         0.20     (110, 890, 80467)
  batch      16 x 16    53     0.32    source seeds 0, 1, 2: max 293, 308, 324; totals 3364, 3366, 3503    0.25: max 1022, 1053, 1071
  block      12 x 9     41     0.30    (3930, 6429, 236628)    0.25     (8026, 11484, 440055)   940 x 620, MaxPos 11
Exact zeros (flat windows, never listed) among the saturated maps' pixels: 0.9, 0.92 and 2.0 million.

Faults planted one at a time in top_mma_body on a scratch build (arithmetic only), and what this file reported:
  prefilter slack E negated            17 of 33 fail: every list test of the shapes with the prefilter (area <= 258),
                                       the threshold-on-a-score tests, the batch and block-mode lists; maps unaffected
  `ro >= th` mask of the last slot off  16 fail: maps and lists of 12 x 9, 17 x 15 and 43 x 6 (a row or slots past the height)
  band of ones one column short        29 fail: every map and list test
"""
import ctypes as C

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from tests.top_map_cases import case

pytestmark = pytest.mark.gpu

FORM = {(16, 16): L.TOP_FORM_EXACT16, (14, 14): L.TOP_FORM_EXACT14, (12, 9): L.TOP_FORM_SMALL,
        (17, 15): L.TOP_FORM_SMALL, (43, 6): L.TOP_FORM_LARGE, (49, 16): L.TOP_FORM_LARGE, (17, 32): L.TOP_FORM_LARGE}
# (thr within capacity, thr with overflow), see the table above
THR = {("noise", (16, 16)): (0.32, 0.25), ("noise", (14, 14)): (0.35, 0.30), ("noise", (12, 9)): (0.42, 0.35),
       ("noise", (17, 15)): (0.32, 0.25), ("noise", (43, 6)): (0.30, 0.25), ("noise", (49, 16)): (0.15, 0.12),
       ("noise", (17, 32)): (0.20, 0.15), ("saturated", (16, 16)): (0.25, 0.20), ("saturated", (12, 9)): (0.32, 0.25),
       ("saturated", (43, 6)): (0.25, 0.20)}
EDGE_SHAPES = [(16, 16), (12, 9), (43, 6)]
ALL_CASES = [("noise", top) for top in FORM] + [("saturated", top) for top in EDGE_SHAPES]
IDS = [f"{k}-{t[0]}x{t[1]}" for k, t in ALL_CASES]


@pytest.fixture(autouse=True)
def _forced(monkeypatch):
    """The matrix-core form also for lone small searches (read when a context's plan is built)."""
    monkeypatch.delenv("FPM_TOP_LIST_CAP", raising=False)
    monkeypatch.setenv("FPM_TOP_MMA", "1")


def _staged(factory, cases):
    """A matcher with the cases' (shared) template learned and their sources staged."""
    _, t, prm, _, _, _ = cases[0]
    m = factory(**prm)
    assert m.learnPattern(t)
    m.stage([c[0] for c in cases])
    return m


def _check_path(st, geom, top, by_block=0):
    """The stats say the call ran what the test is about."""
    assert st["top_mma"] == 1 and st["by_block"] == by_block, st
    assert st["form"] == FORM[top], st
    max_mw, max_mh = int(geom[:, 2].max()), int(geom[:, 3].max())
    assert st["sw"] % 16 == 0 and 16 <= st["sw"] <= 192, st
    assert -(-max_mw // st["sw"]) >= 2, (st, max_mw)            # nstrip
    assert 1 <= st["run"] and -(-max_mh // st["run"]) > 1, (st, max_mh)   # row runs per strip
    assert st["nunits"] >= 2 * len(geom) and 1 <= st["map_grid"] <= st["nunits"], st


def _check_geom(geom, cases, top):
    tw, th = top
    _, _, _, omaps, nang, _ = cases[0]
    assert len(geom) == nang
    kept = {k: (bw, bh, m.shape) for k, bw, bh, m in omaps}
    for a in range(nang):
        if a in kept:
            bw, bh, shp = kept[a]
            assert tuple(geom[a]) == (bw, bh, shp[1], shp[0]), (a, geom[a])
        else:   # an angle the search skips: no map
            assert tuple(geom[a, 2:]) == (0, 0) and (geom[a, 0] < tw or geom[a, 1] < th), (a, geom[a])


def _check_maps(res, cases, what):
    for s, c in enumerate(cases):
        for k, _, _, exp in c[3]:
            got = res["maps"][s][k]
            assert got.shape == exp.shape, (what, s, k)
            if not np.array_equal(got.view(np.uint32), exp.view(np.uint32)):
                bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
                y, x = bad[0]
                pytest.fail(f"{what}: source {s} angle {k} map {exp.shape[1]} x {exp.shape[0]}: {len(bad)} pixels differ, "
                            f"columns {bad[:, 1].min()}..{bad[:, 1].max()} rows {bad[:, 0].min()}..{bad[:, 0].max()}, "
                            f"first (x {x}, y {y}): got {got[y, x]!r} expected {exp[y, x]!r}")


def _check_lists(res, cases, thr, what):
    """Per job: the true count is the oracle's; the stored pairs are distinct members of the oracle's set with its
    value bits, all of the set where it fits the capacity.  Returns (entries listed within capacity, jobs that overflow)."""
    cap = res["stats"]["list_cap"]
    assert res["index"].shape[2] == cap and cap >= 1
    listed = over = 0
    for s, c in enumerate(cases):
        kept = {k: m for k, _, _, m in c[3]}
        for a in range(c[4]):
            n = int(res["counts"][s, a])
            if a not in kept:
                assert n == 0, (what, s, a)
                continue
            flat = kept[a].ravel()
            sel = np.flatnonzero(flat.astype(np.float64) >= thr)
            assert n == len(sel), f"{what}: source {s} angle {a}: count {n}, oracle {len(sel)}"
            stored = min(n, cap)
            idx, val = res["index"][s, a, :stored], res["value"][s, a, :stored]
            assert len(np.unique(idx)) == stored, (what, s, a)
            assert stored == 0 or (idx.min() >= 0 and idx.max() < flat.size), (what, s, a)
            assert np.array_equal(val.view(np.uint32), flat[idx].view(np.uint32)), (what, s, a)
            assert np.all(flat[idx].astype(np.float64) >= thr), (what, s, a)
            if n <= cap:
                assert np.array_equal(np.sort(idx), sel), (what, s, a)
                listed += n
            else:
                over += 1
    return listed, over


@pytest.mark.parametrize("kind,top", ALL_CASES, ids=IDS)
def test_full_maps(gpu_matcher_factory, kind, top):
    """k_top_map (form 1) and the split chain (form 0): every pixel of every angle's map, and the geometry."""
    cases = [case(kind, top)]
    m = _staged(gpu_matcher_factory, cases)
    for form in (1, 0):
        res = m.top_maps(form)
        _check_path(res["stats"], res["geom"], top)
        _check_geom(res["geom"], cases, top)
        _check_maps(res, cases, f"{kind} {top} form {form}")
    if kind == "saturated":
        assert sum(int((mm == 0).sum()) for _, _, _, mm in cases[0][3]) >= 500000


@pytest.mark.parametrize("kind,top", ALL_CASES, ids=IDS)
def test_lists(gpu_matcher_factory, kind, top):
    """k_top_mma's lists (form 2) at a threshold every job holds, and at one where jobs overflow."""
    cases = [case(kind, top)]
    m = _staged(gpu_matcher_factory, cases)
    thr_in, thr_over = THR[(kind, top)]
    res = m.top_maps(2, thr_in)
    _check_path(res["stats"], res["geom"], top)
    _check_geom(res["geom"], cases, top)
    assert res["stats"]["list_cap"] == 512
    listed, over = _check_lists(res, cases, thr_in, f"{kind} {top} thr {thr_in}")
    assert over == 0 and listed >= 500, (listed, over)
    res = m.top_maps(2, thr_over)
    _, over = _check_lists(res, cases, thr_over, f"{kind} {top} thr {thr_over}")
    assert over >= 1


def test_lists_at_the_layer_score(gpu_matcher_factory):
    """thr <= 0 takes the plan's layer score (0.6 * 0.9)."""
    cases = [case("noise", (12, 9))]
    m = _staged(gpu_matcher_factory, cases)
    res = m.top_maps(2)
    listed, over = _check_lists(res, cases, cases[0][2]["score"] * 0.9, "layer score")
    assert listed >= 3 and over == 0


@pytest.mark.parametrize("kind,top", [(k, t) for k, t in ALL_CASES if t in EDGE_SHAPES],
                         ids=[i for i, (k, t) in zip(IDS, ALL_CASES) if t in EDGE_SHAPES])
def test_threshold_on_a_score(gpu_matcher_factory, kind, top):
    """thr = (double)v of a score v that occurs in the maps lists every pixel equal to v; the next double lists none of
    them: the prefilter rejects no output with (double)score >= thr, where that is tightest."""
    cases = [case(kind, top)]
    m = _staged(gpu_matcher_factory, cases)
    allv = np.concatenate([mm.ravel() for _, _, _, mm in cases[0][3]])
    listed = np.sort(allv[allv.astype(np.float64) >= THR[(kind, top)][0]])
    v = listed[len(listed) // 2]   # the median of the within-capacity test's listed values
    thr = float(np.float64(v))
    n_eq = int((allv == v).sum())
    assert n_eq >= 1
    res = m.top_maps(2, thr)
    _check_path(res["stats"], res["geom"], top)
    _, over = _check_lists(res, cases, thr, f"{kind} {top} thr = v")
    assert over == 0
    got_eq = sum(int((res["value"][0, a, :res["counts"][0, a]] == v).sum()) for a in range(cases[0][4]))
    assert got_eq == n_eq
    up = float(np.nextafter(thr, 1.0))
    assert up > thr
    res = m.top_maps(2, up)
    _, over = _check_lists(res, cases, up, f"{kind} {top} thr = next(v)")
    assert over == 0
    assert sum(int((res["value"][0, a, :res["counts"][0, a]] == v).sum()) for a in range(cases[0][4])) == 0
    assert int(res["counts"].sum()) == int((allv.astype(np.float64) > thr).sum())


def test_batch(gpu_matcher_factory):
    """Different sources staged together: every source's maps and lists are its own (the s * nang + a job indexing,
    mode 0's XCD unit order), with more work units than the mode-1 grid so that form 1 walks its unit list."""
    top = (16, 16)
    n = 3
    cases = _batch_cases(top, n)
    m = _staged(gpu_matcher_factory, cases)
    res = m.top_maps(1)
    while res["stats"]["nunits"] <= res["stats"]["map_grid"] and n < 12:   # a device with more CUs: more sources
        n += 2
        cases = _batch_cases(top, n)
        m = _staged(gpu_matcher_factory, cases)
        res = m.top_maps(1)
    assert res["stats"]["nunits"] > res["stats"]["map_grid"], res["stats"]
    _check_path(res["stats"], res["geom"], top)
    _check_geom(res["geom"], cases, top)
    _check_maps(res, cases, "batch form 1")
    _check_maps(m.top_maps(0), cases, "batch form 0")
    for thr in (0.32, 0.25):
        listed, over = _check_lists(m.top_maps(2, thr), cases, thr, f"batch thr {thr}")
        assert (over == 0 and listed >= 500 * n) if thr == 0.32 else over >= 1, (thr, listed, over)
    assert not np.array_equal(cases[0][3][0][3], cases[1][3][0][3])   # (the sources do differ)


def _batch_cases(top, n):
    return [case("noise", top, seed) for seed in range(n)]   # (one template, the sources differ by seed)


def test_block_mode_capacity(gpu_matcher_factory):
    """s_BlockMax peaks (MaxPos 11 on a 940 x 620 source, top level 470 x 310): lists of 8192 entries."""
    top = (12, 9)
    cases = [case("noise", top, 0, 940, 620, 11)]
    m = _staged(gpu_matcher_factory, cases)
    res = m.top_maps(2, 0.3)
    _check_path(res["stats"], res["geom"], top, by_block=1)
    _check_geom(res["geom"], cases, top)
    assert res["stats"]["list_cap"] == 8192
    listed, over = _check_lists(res, cases, 0.3, "block thr 0.3")
    assert over == 0 and listed >= 100000
    _, over = _check_lists(m.top_maps(2, 0.25), cases, 0.25, "block thr 0.25")
    assert over >= 1


def _search(m):
    res = [[r.as_tuple() for r in rr] for rr in m.match_staged()]
    return res, [m.last_candidates(s).tobytes() for s in range(len(res))]


def test_state_is_kept(gpu_matcher_factory):
    """The operator between two searches: the last candidates, the profile counters and the next search's results and
    candidates are those of a context that never called it."""
    cases = _batch_cases((16, 16), 2)
    ref = _staged(gpu_matcher_factory, cases)
    exp = _search(ref)
    assert any(len(r) for r in exp[0])
    m = _staged(gpu_matcher_factory, cases)
    m.profile(True)
    m.profile_reset()
    assert _search(m) == exp
    prof = [m.profile_get(k) for k in range(len(L.KERNEL_NAMES))]
    for form, thr in ((0, 0.0), (1, 0.0), (2, 0.0), (2, 0.3)):
        m.top_maps(form, thr)
        assert [m.last_candidates(s).tobytes() for s in range(2)] == exp[1]
        assert [m.profile_get(k) for k in range(len(L.KERNEL_NAMES))] == prof
    assert m.isPatternLearned()
    assert _search(m) == exp
    m.profile(False)
    m.top_maps(2, 0.2)
    assert _search(m) == exp   # (the replayed graph after the operator's eager launches)


@pytest.mark.parametrize("why", ["env", "shape"])
def test_not_the_matrix_core_form(gpu_matcher_factory, monkeypatch, why):
    """A plan without the matrix-core form: forms 1 and 2 return FPM_E_SIZE; form 0 still gives the oracle's maps."""
    if why == "env":
        monkeypatch.setenv("FPM_TOP_MMA", "0")
        cases = [case("noise", (12, 9))]
    else:
        cases = [case("big", (60, 60))]   # beyond both MFMA layouts
    m = _staged(gpu_matcher_factory, cases)
    for form in (1, 2):
        with pytest.raises(ValueError) as e:
            m.top_maps(form)
        assert e.value.rc == L.FPM_E_SIZE
    res = m.top_maps(0)
    assert res["stats"]["top_mma"] == 0 and res["stats"]["form"] == -1 and res["stats"]["nunits"] == 0
    _check_maps(res, cases, f"split only ({why})")


def test_bad_arguments(gpu_matcher_factory):
    cases = [case("noise", (12, 9))]
    _, t, prm, _, _, _ = cases[0]
    m = gpu_matcher_factory(**prm)
    IP, FP = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ns, na, lc, mf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()

    def raw(form, thr, geom=None, gcap=0, maps=None, mcap=0, cnt=None, idx=None, val=None, slots=0):
        return m._lib.fpm_op_top_maps(m._ctx, form, thr, C.byref(ns), C.byref(na), C.byref(mf), C.byref(lc), geom, gcap,
                                      maps, mcap, cnt, idx, val, slots, None)

    assert raw(1, 0.0) == L.FPM_E_NOT_LEARNED
    assert m.learnPattern(t)
    assert raw(1, 0.0) == L.FPM_E_INVALID_ARG   # nothing staged
    m.stage([cases[0][0]])
    assert raw(1, 0.0) == L.FPM_OK
    S, nang, dense, cap = ns.value, na.value, mf.value, lc.value
    assert (S, nang, cap) == (1, cases[0][4], 512) and dense == sum(mm.size for _, _, _, mm in cases[0][3])
    for form, thr in ((3, 0.0), (-1, 0.0), (2, 0.005), (2, 0.01), (1, float("nan")), (2, float("inf"))):
        assert raw(form, thr) == L.FPM_E_INVALID_ARG, (form, thr)
    geom = np.zeros((nang, 4), np.int32)
    flat = np.full(dense, 7.0, np.float32)
    cnt = np.full(nang, -5, np.int32)
    idx = np.zeros(nang * cap, np.int32)
    val = np.zeros(nang * cap, np.float32)
    g, f = geom.ctypes.data_as(IP), flat.ctypes.data_as(FP)
    c, i, v = cnt.ctypes.data_as(IP), idx.ctypes.data_as(IP), val.ctypes.data_as(FP)
    assert raw(1, 0.0, g, nang) == L.FPM_E_INVALID_ARG                      # form 1 without maps
    assert raw(2, 0.0, g, nang, f, dense) == L.FPM_E_INVALID_ARG            # form 2 without lists
    assert raw(2, 0.0, g, nang, None, 0, c, i, None, nang * cap) == L.FPM_E_INVALID_ARG
    assert raw(1, 0.0, None, 0, f, dense) == L.FPM_E_INVALID_ARG            # no geometry
    assert raw(1, 0.0, g, nang, f, -1) == L.FPM_E_INVALID_ARG
    assert raw(1, 0.0, g, nang - 1, f, dense) == L.FPM_E_CAPACITY
    assert raw(1, 0.0, g, nang, f, dense - 1) == L.FPM_E_CAPACITY
    assert raw(2, 0.0, g, nang, None, 0, c, i, v, nang * cap - 1) == L.FPM_E_CAPACITY
    assert np.all(flat == 7.0) and np.all(cnt == -5) and not geom.any()    # nothing written by the rejected calls
    assert raw(1, 0.0, g, nang, f, dense) == L.FPM_OK and geom.any() and not np.any(flat == 7.0)
