"""The fused top-layer kernel (k_top_fused: canvas warp, NCC by v_dot4 on funnel-shifted words, plain getNextMaxLoc, all
in one workgroup's LDS) stage by stage against the oracle (gfx950 required).  fpm_op_top_fused runs the search's own
plan, job tables, job order and peak arguments through launch_top_fused twice: the product instantiation gives the
peaks, the map-writing one (template parameter DUMP, otherwise the same source) also the maps before any peak is painted.

Expected values are the oracle's alone: the maps are OracleMatcher.set_keep_maps() / top_maps() (tests/top_map_cases.case),
the peaks oracle.peak_sequence(map, tw, th, False, False, overlap, cap - 1, thr) on each oracle map.  Maps are compared
as uint32 (-0.0 != +0.0), peaks by count, every (x, y) and the score's bits; the two instantiations' peak and count
arrays are byte-equal, and every slot past a job's count still holds what the caller put there.  No tolerance anywhere.
Every test asserts from the operator's stats that the fused kernel ran, with which LDS and which grid.

Cases (tests/top_fused_cases.py; the facts in this table are asserted on the CPU by tests/test_oracle_top_fused.py):

  top template   source       angles  largest job's LDS  what it cuts
  16 x 16        180 x 120      53       32.1 KB         tw % 4 = 0, map widths % 4 = 1, 3
  14 x 14        180 x 120      47       34.8 KB         tw % 4 = 2, map widths % 4 = 1, 3
  12 x 9         180 x 120      41       39.3 KB         tw % 4 = 0, odd height, map widths % 4 = 1, 3
  17 x 15        180 x 120      55       32.1 KB         tw % 4 = 1, map widths % 4 = 0, 2
  43 x 6         180 x 120     137       21.6 KB         tw % 4 = 3, 11 words per row, map widths % 4 = 0, 2
  (each on the noise scene and the saturated one: >= 500 exact ties and >= 1000 flat-window zeros per case)
  3 x 30         150 x 130      97       25.6 KB         narrower than one word (ntw 1, mask 0x00ffffff); % 4 = 0, 1, 2
  60 x 60        176 x 150     191       30.5 KB         15 words per row; maps from 55 x 55 down to 1 x 7, all residues
  12 x 9         200 x 140      41       52.7 KB         near the LDS limit; 220 x 150 (64.2 KB) must be FPM_E_SIZE
  43 x 6         200 x 40      137       10.0 KB         top level 100 x 20: 22 angles around +-90 degrees have no map
  14 x 5         301 x 235       5        5.2 KB         test_gpu_fuzz._case(24), three pyramid layers, rectangle 5 x 1
The issue's narrow source (a top level 20 wide and 100 tall under 43 x 6) is refused by the search's own size guard
(template wider than the source and lower: FPM_E_SIZE in the oracle and the engine alike), so its transpose is used.

Dense peaks: MaxPos 130 (cap 135 > kNmsInitCap 128), score -1 (layer score -0.9: below every map value, above the
painted -1), MaxOverlap 0.8 (rectangles 6 x 6, 4 x 3, 6 x 5, 23 x 23: each covers its own peak, no position twice).
Over saturated 16 x 16 and 12 x 9, noise 12 x 9, 17 x 15 and 60 x 60: 190 jobs end at cap, 191 (the small maps of
60 x 60) at the threshold, 51 saturated jobs take two or more equal values in a row.

Faults planted one at a time in top_fused_job on a scratch build (arithmetic only, every index stays inside the launched
LDS), and what this file's 42 tests reported:
  `Mw` built with `4k + b <= tw`          16 fail: every map test of the widths with tw % 4 != 0 (14, 17, 3, 43, and 14 of
                                          fuzz 24), their dense, skipped-angle and grid-cap tests and the 17 x 15 whole
                                          searches; the widths 16 and 12 are untouched (the extra byte lies past the word)
  argmax scans take `x >= v`              5 fail: the tie order in dense saturated 16 x 16, both clipped-rectangle
                                          tests, the constant template (row-major order) and the constant source (zeros)
  `x2 = min(sx + rw, ow - 1)`             16 fail: every dense and clipped-rectangle test, the constant inputs, all four
                                          grid-cap tests, both cap-135 whole searches and the 3 x 30 maps' peaks
  funnel word zero at `k + 1 == ntw`      32 fail: maps of every width but 17 (tw % 4 = 1 never needs the word past the
                                          template's last one), and all that follows from the maps
  funnel word zero at the row's pad word  none, and none can: `w1 = q + k + 1 < cpw - 1 ? ir[k + 1] : 0` is the same
  (`cpw` without its `+ 1`)               program.  Word cpw - 1 of a canvas row holds only pixels >= dw, which K2 writes
                                          as zero, so the `+ 1` buys an in-row address for that read, not a value.  What
                                          the pad protects against -- reading the next row's first word there -- changes
                                          an address range and was left out.
"""
import ctypes as C

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import TemplateMatcher, synth, _lib as L
from fastest_image_pattern_matching_amd.matcher import PEAK_DTYPE
from tests import oracle
from tests import top_fused_cases as F
from tests.top_map_cases import case, noise_scene

pytestmark = pytest.mark.gpu

FILL = TemplateMatcher.TOP_FUSED_FILL


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("FPM_TOP_FUSED", "FPM_TOP_MMA", "FPM_GRID_TOP", "FPM_TOP_LIST_CAP"):
        monkeypatch.delenv(k, raising=False)


def _staged(factory, cases, **over):
    """A matcher with the cases' (shared) template learned and their sources staged; `over` replaces parameters the
    maps do not depend on (max_pos, score, max_overlap)."""
    _, t, prm, _, _, _ = cases[0]
    prm = dict(prm, **over)
    m = factory(**prm)
    assert m.learnPattern(t)
    m.stage([c[0] for c in cases])
    return m, prm


def _check_ran(st, geom, top, n_src, prm, grid=None):
    """The stats say the fused kernel ran: over every job, with the LDS of the largest canvas and the expected grid."""
    jobs = n_src * len(geom)
    need = max(F.top_fused_lds(int(bw), int(bh), *top) for bw, bh, _, _ in geom)
    assert st["jobs"] == jobs and st["cap"] == prm["max_pos"] + F.MATCH_CANDIDATE_NUM, st
    assert st["lds"] == need and 0 < st["lds"] <= st["lds_limit"], (st, need)
    assert 0 < st["static_lds"] == st["dump_static_lds"] <= F.STATIC_LDS_MAX, st
    assert st["lds_limit"] == 65536 - st["static_lds"], st
    assert st["grid"] == (jobs if grid is None else min(grid, jobs)), st


def _check(res, cases, top, prm, what, levels=2, peaks=None):
    """Geometry, every map pixel, every peak of both instantiations and every untouched slot, against the oracle."""
    tw, th = top
    cap = prm["max_pos"] + F.MATCH_CANDIDATE_NUM
    nang = cases[0][4]
    geom = res["geom"]
    assert len(geom) == nang and res["peaks"].shape == (len(cases), nang, cap)
    assert res["peaks"].tobytes() == res["dump_peaks"].tobytes(), f"{what}: the two instantiations' peaks differ"
    assert res["counts"].tobytes() == res["dump_counts"].tobytes(), f"{what}: the two instantiations' counts differ"
    fill = np.zeros((), res["peaks"].dtype)
    fill["x"], fill["y"], fill["score"] = FILL
    totals = dict(peaks=0, at_cap=0, at_thr=0, skipped=0)
    for s, c in enumerate(cases):
        kept = {k: (bw, bh, m) for k, bw, bh, m in c[3]}
        seqs = dict(zip([k for k, _, _, _ in c[3]], peaks[s] if peaks is not None else F.peak_lists(c, top, prm, levels)))
        for a in range(nang):
            n = int(res["counts"][s, a])
            got = res["maps"][s][a]
            if a not in kept:   # an angle the search skips: no map, no peak
                assert tuple(geom[a, 2:]) == (0, 0) and (geom[a, 0] < tw or geom[a, 1] < th), (what, a, geom[a])
                assert got.size == 0 and n == 0, (what, s, a, n)
                assert np.all(res["peaks"][s, a] == fill), (what, s, a)
                totals["skipped"] += 1
                continue
            bw, bh, exp = kept[a]
            assert tuple(geom[a]) == (bw, bh, exp.shape[1], exp.shape[0]), (what, a, geom[a])
            assert got.shape == exp.shape, (what, s, a)
            if not np.array_equal(got.view(np.uint32), exp.view(np.uint32)):
                bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
                y, x = bad[0]
                pytest.fail(f"{what}: source {s} angle {a} map {exp.shape[1]} x {exp.shape[0]}: {len(bad)} pixels differ, "
                            f"columns {bad[:, 1].min()}..{bad[:, 1].max()} rows {bad[:, 0].min()}..{bad[:, 0].max()}, "
                            f"first (x {x}, y {y}): got {got[y, x]!r} expected {exp[y, x]!r}")
            seq = seqs[a]
            assert n == len(seq), f"{what}: source {s} angle {a}: {n} peaks, oracle {len(seq)}"
            pk = res["peaks"][s, a]
            gxy = list(zip(pk["x"][:n].tolist(), pk["y"][:n].tolist()))
            exy = [(x, y) for _, x, y in seq]
            assert gxy == exy, f"{what}: source {s} angle {a}: peak {next(i for i in range(n) if gxy[i] != exy[i])} differs"
            ev = np.array([v for v, _, _ in seq], np.float64).astype(np.float32)
            assert np.array_equal(pk["score"][:n].view(np.uint32), ev.view(np.uint32)), (what, s, a)
            assert np.all(pk[n:] == fill), f"{what}: source {s} angle {a}: a slot past the count was written"
            totals["peaks"] += n
            totals["at_cap"] += n == cap
            totals["at_thr"] += n < cap
    return totals


def _run(factory, cases, top, what, grid=None, levels=2, **over):
    m, prm = _staged(factory, cases, **over)
    res = m.top_fused()
    _check_ran(res["stats"], res["geom"], top, len(cases), prm, grid)
    return res, _check(res, cases, top, prm, what, levels), m


@pytest.mark.parametrize("cid", sorted(F.MAP_CASES))
def test_maps_and_peaks(gpu_matcher_factory, cid):
    """Every pixel of every angle's map and the peaks at the cases' own parameters (MaxPos 3, score 0.6, MaxOverlap 0)."""
    kind, top, w, h = F.MAP_CASES[cid]
    res, tot, _ = _run(gpu_matcher_factory, [F.get(cid)], top, cid)
    assert res["stats"]["search_takes_it"] == 0          # fewer than kTopFusedMinJobs jobs: the operator runs it all the same
    lo, hi = F.MAP_FACTS[cid.split("-", 1)[1]][1]
    assert lo * 1024 <= res["stats"]["lds"] < hi * 1024
    assert tot["skipped"] == 0


def test_lds_limit(gpu_matcher_factory):
    """One size above the near-limit case the largest job needs more than the limit the stats report: FPM_E_SIZE."""
    near, _ = _staged(gpu_matcher_factory, [F.get("noise-12x9-near-limit")])
    limit = near.top_fused()["stats"]["lds_limit"]
    kind, top, w, h = F.OVER_LIMIT
    m, _ = _staged(gpu_matcher_factory, [case(kind, top, 0, w, h)])
    with pytest.raises(ValueError) as e:
        m.top_fused()
    assert e.value.rc == L.FPM_E_SIZE
    assert e.value.stats["lds_limit"] == limit and e.value.stats["lds"] > limit, e.value.stats
    assert e.value.stats["lds"] == F.case_lds(case(kind, top, 0, w, h), top)


@pytest.mark.parametrize("cid", F.DENSE_CASES)
def test_dense_peaks(gpu_matcher_factory, cid):
    """cap 135 (beyond the LDS peak list of the fused candidate init), a layer score below every map value: peak
    lists up to cap and lists that end when the whole map is painted, first-maximum order among exact ties."""
    kind, top, w, h = F.MAP_CASES[cid]
    c = F.get(cid)
    m, prm = _staged(gpu_matcher_factory, [c], **F.DENSE)
    res = m.top_fused()
    _check_ran(res["stats"], res["geom"], top, 1, prm)
    assert res["stats"]["cap"] == 135 > F.K_NMS_INIT_CAP
    tot = _check(res, [c], top, prm, f"dense {cid}", peaks=[F.expected_peaks(kind, top, 0, w, h, prm)])
    assert tot["at_cap"] + tot["at_thr"] == c[4] and tot["peaks"] >= 135
    assert (tot["at_thr"] >= 50) if top == (60, 60) else (tot["at_cap"] == c[4])


def test_overlap_rectangle_misses_its_peak(gpu_matcher_factory):
    """The 14 x 5 top of fuzz case 24 (MaxOverlap 0.8: a 5 x 1 rectangle above the peak): the same peak up to cap."""
    c = F.fuzz24()
    res, tot, _ = _run(gpu_matcher_factory, [c], (14, 5), "fuzz24", levels=4)
    assert tot["at_cap"] == 5 and all(len(set(zip(res["peaks"][0, a]["x"].tolist(), res["peaks"][0, a]["y"].tolist()))) == 1
                                      for a in range(5))


@pytest.mark.parametrize("ov", [0.0, -0.5])
def test_overlap_clipped_rectangles(gpu_matcher_factory, ov):
    """MaxOverlap 0 (rectangles of twice the template) and -0.5 (three times), clipped on all four map edges."""
    kind, top, w, h = F.MAP_CASES["noise-12x9"]
    over = dict(max_pos=30, score=-1.0, max_overlap=ov)
    c = F.get("noise-12x9")
    m, prm = _staged(gpu_matcher_factory, [c], **over)
    res = m.top_fused()
    _check_ran(res["stats"], res["geom"], top, 1, prm)
    tot = _check(res, [c], top, prm, f"overlap {ov}", peaks=[F.expected_peaks(kind, top, 0, w, h, prm)])
    assert tot["peaks"] >= 2 * c[4]


def test_empty_maps(gpu_matcher_factory):
    """A layer score above every value: no peak anywhere, nothing written but the counts."""
    res, tot, _ = _run(gpu_matcher_factory, [F.get("noise-12x9")], (12, 9), "empty", score=1.2)
    assert tot["peaks"] == 0 and not res["counts"].any()


def test_constant_template(gpu_matcher_factory):
    """ResultEqual1: every map pixel is 1.0f and the peaks run in row-major order."""
    kind, top, w, h = F.MAP_CASES["noise-12x9"]
    c = case("constant_template", top, 0, w, h)
    res, tot, _ = _run(gpu_matcher_factory, [c], top, "constant template")
    assert tot["at_cap"] == c[4]
    assert all(np.all(mm.view(np.uint32) == 0x3f800000) for mm in res["maps"][0])
    for a in range(c[4]):
        idx = res["peaks"][0, a]["y"].astype(np.int64) * res["geom"][a, 2] + res["peaks"][0, a]["x"]
        assert idx[0] == 0 and np.all(np.diff(idx) > 0)


def test_constant_source(gpu_matcher_factory):
    """Flat windows: exact zeros over most of every map (a lower score lets the loop walk them: ties at 0)."""
    kind, top, w, h = F.MAP_CASES["noise-12x9"]
    c = case("constant_source", top, 0, w, h)
    res, tot, _ = _run(gpu_matcher_factory, [c], top, "constant source", score=-0.01, max_pos=20)
    assert sum(int((mm == 0).sum()) for mm in res["maps"][0]) >= 10000 and tot["peaks"] >= 5 * c[4]


def test_skipped_angles(gpu_matcher_factory):
    """A top level lower than the top template is wide: the jobs around +-90 degrees have no map, write a count of 0
    and leave their neighbours' outputs alone."""
    kind, top, w, h = F.NARROW
    c = case(kind, top, 0, w, h)
    res, tot, _ = _run(gpu_matcher_factory, [c], top, "narrow", score=0.3)
    assert tot["skipped"] == c[4] - len(c[3]) == 22 and tot["peaks"] >= 50


def _batch(top, n=3):
    kind, _, w, h = F.MAP_CASES[f"noise-{top[0]}x{top[1]}"]
    return [case(kind, top, seed, w, h) for seed in range(n)]


def test_batch_equals_single_calls(gpu_matcher_factory):
    """Three sources in one batch: the oracle's, and byte for byte what three single calls give."""
    top = (12, 9)
    cases = _batch(top)
    res, tot, _ = _run(gpu_matcher_factory, cases, top, "batch")
    assert tot["peaks"] >= 9
    assert not np.array_equal(cases[0][3][0][3], cases[1][3][0][3])   # (the sources do differ)
    for s, c in enumerate(cases):
        one, _, _ = _run(gpu_matcher_factory, [c], top, f"single {s}")
        assert one["peaks"].tobytes() == res["peaks"][s:s + 1].tobytes()
        assert one["counts"].tobytes() == res["counts"][s:s + 1].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one["maps"][0], res["maps"][s]))


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("which", ["12x9", "narrow-43x6"])
def test_grid_caps(gpu_matcher_factory, monkeypatch, grid, which):
    """FPM_GRID_TOP=1 and =3: one workgroup walks jobs of different canvas sizes (and, on the narrow source, jobs
    without a map) through the same LDS; a dense peak pass so that painted maps precede fresh ones."""
    monkeypatch.setenv("FPM_GRID_TOP", str(grid))
    if which == "12x9":
        top, cases = (12, 9), _batch((12, 9))
    else:
        kind, top, w, h = F.NARROW
        cases = [case(kind, top, seed, w, h) for seed in range(3)]
    res, tot, _ = _run(gpu_matcher_factory, cases, top, f"grid {grid} {which}", grid=grid, score=-1.0, max_pos=10,
                       max_overlap=0.5)
    assert res["stats"]["grid"] == grid < res["stats"]["jobs"] and tot["peaks"] >= 10 * len(cases[0][3])


def _search(m):
    res = [[r.as_tuple() for r in rr] for rr in m.match_staged()]
    return res, [m.last_candidates(s).tobytes() for s in range(len(res))]


@pytest.mark.parametrize("forced", ["1", None])
def test_state_is_kept(gpu_matcher_factory, monkeypatch, forced):
    """The operator between two searches (the fused form forced, and the search's own choice): the last candidates, the
    profile counters and the next search's results and candidates are those of a context that never called it."""
    if forced:
        monkeypatch.setenv("FPM_TOP_FUSED", forced)
    top = (12, 9)
    cases = _batch(top, 2)
    ref, _ = _staged(gpu_matcher_factory, cases)
    exp = _search(ref)
    assert any(len(r) for r in exp[0])
    m, prm = _staged(gpu_matcher_factory, cases)
    m.profile(True)
    m.profile_reset()
    assert _search(m) == exp
    prof = [m.profile_get(k) for k in range(len(L.KERNEL_NAMES))]
    for _ in range(2):
        res = m.top_fused()
        assert res["stats"]["search_takes_it"] == (1 if forced else 0)
        _check_ran(res["stats"], res["geom"], top, 2, prm)
        _check(res, cases, top, prm, "state")
        assert [m.last_candidates(s).tobytes() for s in range(2)] == exp[1]
        assert [m.profile_get(k) for k in range(len(L.KERNEL_NAMES))] == prof
    assert m.isPatternLearned()
    assert _search(m) == exp
    m.profile(False)
    m.top_fused()
    assert _search(m) == exp   # (the replayed graph after the operator's eager launches)


def test_refusals_and_bad_arguments(gpu_matcher_factory):
    """FPM_E_SIZE with nothing launched in block mode and for a template level beyond k_ncc_tile's form; the state
    rules and capacities of fpm_op_top_maps."""
    c = F.get("noise-12x9")
    _, t, prm, _, nang, _ = c
    m = gpu_matcher_factory(**prm)
    IP, FP, PP = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(L.Peak)
    ns, na, cp, mf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()

    def raw(geom=None, gcap=0, maps=None, mcap=0, pk=None, cnt=None, dpk=None, dcnt=None, slots=0, mm=None):
        mm = mm or m
        return mm._lib.fpm_op_top_fused(mm._ctx, C.byref(ns), C.byref(na), C.byref(mf), C.byref(cp), geom, gcap, maps,
                                        mcap, pk, cnt, dpk, dcnt, slots, None)

    assert raw() == L.FPM_E_NOT_LEARNED
    assert m.learnPattern(t)
    assert raw() == L.FPM_E_INVALID_ARG   # nothing staged
    m.stage([c[0]])
    assert raw() == L.FPM_OK
    cap, dense = cp.value, mf.value
    assert (ns.value, na.value, cap) == (1, nang, 8) and dense == sum(mm.size for _, _, _, mm in c[3])
    geom = np.zeros((nang, 4), np.int32)
    flat = np.full(dense, 7.0, np.float32)
    pk = [np.zeros(nang * cap, PEAK_DTYPE) for _ in range(2)]
    cnt = [np.full(nang, -5, np.int32) for _ in range(2)]
    g, f = geom.ctypes.data_as(IP), flat.ctypes.data_as(FP)
    p0, p1 = (p.ctypes.data_as(PP) for p in pk)
    c0, c1 = (x.ctypes.data_as(IP) for x in cnt)
    assert raw(g, nang, f, dense, p0, c0, p1, None, nang * cap) == L.FPM_E_INVALID_ARG     # a missing output
    assert raw(None, 0, f, dense, p0, c0, p1, c1, nang * cap) == L.FPM_E_INVALID_ARG
    assert raw(g, nang, f, -1, p0, c0, p1, c1, nang * cap) == L.FPM_E_INVALID_ARG
    assert raw(g, nang - 1, f, dense, p0, c0, p1, c1, nang * cap) == L.FPM_E_CAPACITY
    assert raw(g, nang, f, dense - 1, p0, c0, p1, c1, nang * cap) == L.FPM_E_CAPACITY
    assert raw(g, nang, f, dense, p0, c0, p1, c1, nang * cap - 1) == L.FPM_E_CAPACITY
    assert np.all(flat == 7.0) and all(np.all(x == -5) for x in cnt) and not geom.any()   # nothing written
    assert raw(g, nang, f, dense, p0, c0, p1, c1, nang * cap) == L.FPM_OK
    assert geom.any() and not np.any(flat == 7.0) and np.all(cnt[0] >= 0) and np.array_equal(cnt[0], cnt[1])
    # block mode (s_BlockMax peaks): MaxPos 11 on a top level 500 times the template's area
    s, tt = noise_scene((12, 9), 0, 940, 620)
    mb = gpu_matcher_factory(**dict(prm, max_pos=11))
    assert mb.learnPattern(tt)
    mb.stage([s])
    with pytest.raises(ValueError) as e:
        mb.top_fused()
    assert e.value.rc == L.FPM_E_SIZE and e.value.stats["lds"] == 0
    # a top template level 70 x 70: beyond k_ncc_tile's 128 x 64
    big = synth.box_blur(synth.noise(140, 140, 128, 60, 5), 3)
    src = synth.box_blur(synth.noise(300, 300, 128, 60, 6), 3)
    mt = gpu_matcher_factory(max_pos=3, tolerance_angle=180.0, score=0.6, min_reduce_area=4900)
    assert mt.learnPattern(big)
    assert mt.template_level(1)[0].shape == (70, 70) and mt.template_info()[0] == 2
    mt.stage([src])
    with pytest.raises(ValueError) as e:
        mt.top_fused()
    assert e.value.rc == L.FPM_E_SIZE and e.value.stats["lds"] == 0
    o = oracle.OracleMatcher().set(max_pos=3, tolerance_angle=180.0, score=0.6, min_reduce_area=4900)
    assert o.learnPattern(big)
    assert [r.as_tuple() for r in mt.match_staged()[0]] == o.match(src)   # the refused call left the search alone


# ---- the fused candidate init, through whole searches ------------------------------------------------------------
def _whole_search(factory, monkeypatch, s, t, prm, init_kernel):
    """A search with the fused top layer forced on a fresh context against the oracle's: results, per-layer counts and
    every candidate record; the profile counters say which kernels ran."""
    monkeypatch.setenv("FPM_TOP_FUSED", "1")
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    exp = o.match(s)
    m = factory(**prm)
    assert m.learnPattern(t)
    m.profile(True)
    m.profile_reset()
    got = [r.as_tuple() for r in m.match(s)]
    launches = {k: m.profile_get(i)[1] for i, k in enumerate(L.KERNEL_NAMES)}
    m.profile(False)
    assert launches["top_warp"] == 0 and launches["top_map"] == 0 and launches["top_nms"] == 0, launches
    assert launches["top_ncc"] == 1 and launches["cand_init"] == (1 if init_kernel else 0), launches
    assert m.search_stats() == o.stats()
    assert got == exp
    assert m.last_candidates(0).tobytes() == o.candidates().tobytes()
    assert [r.as_tuple() for r in m.match(s)] == exp   # (and as the replayed graph)
    assert m.last_candidates(0).tobytes() == o.candidates().tobytes()
    return o.stats()


@pytest.mark.parametrize("top", [(12, 9), (17, 15)])
@pytest.mark.parametrize("layers", [0, 1, 2])
def test_fused_candidate_init(gpu_matcher_factory, monkeypatch, top, layers):
    """cand_init_job in k_top_fused: no pyramid (L = 0: mode 1, block 0 zeroes the counters), L = 1 (mode 3: the first
    refined layer is layer 0) and L = 2 (mode 2)."""
    s, t, prm = F.search_scene(top, layers)
    st = _whole_search(gpu_matcher_factory, monkeypatch, s, t, prm, init_kernel=False)
    assert len(st) == 2 + layers and st[1] >= 1


@pytest.mark.parametrize("top", [(12, 9), (17, 15)])
def test_separate_candidate_init_beyond_the_lds_list(gpu_matcher_factory, monkeypatch, top):
    """cap 135 > kNmsInitCap: the fused kernel leaves the candidates to k_cand_init."""
    s, t, prm = F.search_scene(top, 1)
    st = _whole_search(gpu_matcher_factory, monkeypatch, s, t, dict(prm, max_pos=130, max_overlap=0.8, score=0.3),
                       init_kernel=True)
    assert st[1] >= 500
