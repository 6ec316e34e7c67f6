"""Edge probes on the HIP path (fpm_probes_at / fpm_last_probes): k_probe's records, flags and profiles, the summaries
and the derived doubles against the restatement of tests/probe_ref.py (the composition in Python floats, the sampler in
integers, anchored to the oracle by tests/test_probe_host.py).  Every comparison is ==."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import probe_ref as ref
from tests.cases import CASES
from tests.test_gpu_align import EDGE_POSES

pytestmark = pytest.mark.gpu

LENGTHS = [4, 5, 31, 32, 33, 63, 64]
WIDTHS = [1, 2, 15, 16]
SELECTS = ["nearest", "strongest", "first", "last"]
COUNTS = [1, 3, 4, 5]
SIZES = [(161, 97), (164, 100)]
FAR_POSE = ((5000.0, 5000.0), 0.0)


def side_poses(sw, sh):
    """The source's four sides crossed by probes about (35.5, 11)."""
    return [((-40.0, 50.0), 0.0), ((sw - 11.0, 50.25), 0.0), ((60.5, -14.0), 0.0), ((60.0, sh - 9.0), 0.0)]


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


def paired_params():
    """Every length with every width, and over them every half in {1, 2, 8} (as far as the length admits it) with every
    polarity, every select rule and every contrast in {1, 12, 255}: [(params, n_probes)]."""
    out = []
    for i, n in enumerate(LENGTHS):
        for j, w in enumerate(WIDTHS):
            k = len(out)
            half = min((1, 2, 8)[(i + j) % 3], n // 2)
            out.append((ref.params(n, w, half, (1, 12, 255)[(k // 2) % 3], (1, -1, 0)[(i + 2 * j) % 3], SELECTS[(i + j + k // 7) % 4]),
                        COUNTS[k % 4]))
    prms = [p for p, _ in out]
    assert {(p["length"], p["width"]) for p in prms} == {(n, w) for n in LENGTHS for w in WIDTHS}
    big = [p for p in prms if p["length"] >= 31]
    assert {(p["half"], p["polarity"]) for p in big} == {(s, p) for s in (1, 2, 8) for p in (1, -1, 0)}
    assert {p["contrast"] for p in prms} == {1, 12, 255} and {p["select"] for p in prms} == {0, 1, 2, 3}
    assert {c for _, c in out} == set(COUNTS)
    return out


def some_probes(n, seed):
    """n probes about (35.5, 11) in the four directions of the caliper tests and in between."""
    rng = np.random.default_rng(seed)
    phis = [0.0, 90.0, 37.5, -137.5, 180.0]
    return [(35.5 + float(rng.integers(-40, 41)) * 0.25, 11.0 + float(rng.integers(-20, 21)) * 0.25,
             phis[(k + seed) % 5] + (0.0 if k % 2 == 0 else float(rng.integers(-300, 300)) * 0.125)) for k in range(n)]


def _source(sw, sh):
    rng = np.random.default_rng(sw)
    src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    # smooth the left half: fewer, wider edges there; the right half stays rough
    src[:, :sw // 2] = (src[:, :sw // 2].astype(np.int32) // 64 * 64 + 31).astype(np.uint8)
    return src


def _stage(hip, srcs, seed=1):
    """Staging lays the sources out for a template's pyramid: any template will do, the probes never read it."""
    hip.resetParams()
    assert hip.learnPattern(np.random.default_rng(seed).integers(0, 256, (23, 71), dtype=np.uint8))
    hip.stage(srcs)


def _run(hip, srcs, idx, poses, ps, prm, label, profiles=True):
    lts, angs = [p[0] for p in poses], [p[1] for p in poses]
    out = hip.probes_at(idx, lts, angs, ref.probes_array(ps), ref.record(prm), profiles=profiles)
    assert out[0].dtype == M.PROBE_SUMMARY_DTYPE and out[1].dtype == M.PROBE_RESULT_DTYPE
    ref.assert_call(out[0], out[1], out[2] if profiles else None, srcs, idx, lts, angs, ps, prm, label)
    return out


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("length", LENGTHS)
def test_records_flags_profiles_and_summaries(hip, size, length):
    sw, sh = size
    src = _source(sw, sh)
    _stage(hip, [src])
    poses = EDGE_POSES + side_poses(sw, sh) + [FAR_POSE]
    calls = [(p, c) for p, c in paired_params() if p["length"] == length]
    assert len(calls) == len(WIDTHS)
    found = outside = 0
    for prm, count in calls:
        ps = some_probes(count, length * 17 + prm["width"])
        summary, results, prof = _run(hip, [src], [0] * len(poses), poses, ps, prm, f"{size} {prm} x {count}")
        assert prof.shape == (len(poses), count, length)
        # the pose wholly outside: zeros, no edge, every probe flagged
        assert not prof[-1].any() and summary[-1]["n_found"] == 0 and summary[-1]["n_missing"] == count
        assert summary[-1]["n_outside"] == count and (results[-1]["flags"] == L.PROBE_OUTSIDE).all()
        found += int(summary["n_found"].sum())
        outside += int(summary[:-1]["n_outside"].sum())
        # without the profiles the records are the same bytes
        s2, r2 = hip.probes_at([0] * len(poses), [p[0] for p in poses], [p[1] for p in poses], ref.probes_array(ps), ref.record(prm))
        assert s2.tobytes() == summary.tobytes() and r2.tobytes() == results.tobytes()
    assert found > 0 and outside > 0


@pytest.mark.parametrize("shape", [(5, 2, 1), (64, 16, 8), (24, 5, 2)])
def test_a_full_probe_list(hip, shape):
    """4096 probes, the most a call takes: 1024 full workgroups per hit."""
    sw, sh = SIZES[1]
    src = _source(sw, sh)
    _stage(hip, [src])
    k = np.arange(4096)
    ps = list(zip((5.0 + (k % 64) * 1.25).tolist(), (3.0 + (k // 64) * 0.5).tolist(), (k * 7.375).tolist()))
    prm = ref.params(shape[0], shape[1], shape[2], 12, 0, "nearest")
    poses = [EDGE_POSES[1], side_poses(sw, sh)[1]] if shape[0] < 64 else [EDGE_POSES[1]]
    summary, results, prof = _run(hip, [src], [0] * len(poses), poses, ps, prm, f"4096 probes {shape}")
    assert summary[0]["n_found"] + summary[0]["n_missing"] == 4096 and summary[0]["n_found"] > 100


def test_saturated_checker(hip):
    """0 / 255 stripes 8 samples wide under a probe of 16 rows with s = 8: P alternates between 0 and 4080 and |d|
    reaches 32 640 = s W 255, the contract's extreme, at every stripe boundary."""
    yy, xx = np.mgrid[0:40, 0:120]
    src = np.where((xx // 8) % 2 == 1, 255, 0).astype(np.uint8)
    _stage(hip, [src])
    ps = [(8 + 15.5, 12.0 + 7.5, 0.0), (16 + 15.5, 12.0 + 7.5, 0.0), (8 + 15.5, 12.0 + 7.5, 180.0)]
    for sel, want in [("nearest", (16, 16, 16)), ("first", (8, 8, 8)), ("last", (24, 24, 24)), ("strongest", (8, 8, 8))]:
        prm = ref.params(32, 16, 8, 255, 0, sel)
        summary, results, prof = _run(hip, [src], [0], [((0.0, 0.0), 0.0)], ps, prm, f"checker {sel}")
        assert set(np.unique(prof[0, 0])) == {0, 4080} and prof.max() == 4080
        assert (np.abs(results[0]["d"]) == 32640).all() and (results[0]["contrast"] == 255.0).all()
        assert (results[0]["n_edges"] == 3).all() and tuple(results[0]["index"]) == want, (sel, results[0]["index"])
        assert summary[0]["n_found"] == 3 and summary[0]["n_ambiguous"] == 3 and summary[0]["n_outside"] == 0


def test_five_poses_two_sources_permuted(hip):
    rng = np.random.default_rng(77)
    srcs = [np.ascontiguousarray((rng.integers(0, 256, (100, 164), dtype=np.uint8) // 32 * 32).astype(np.uint8)) for _ in range(2)]
    _stage(hip, srcs)
    ps = some_probes(11, 5)
    prm = ref.params(33, 5, 2, 12, 0, "strongest")
    poses = EDGE_POSES + [side_poses(164, 100)[0], ((90.5, 60.0), 77.0)]
    idx = [0, 1, 0, 1, 1]
    summary, results, prof = _run(hip, srcs, idx, poses, ps, prm, "two sources")
    perm = [3, 6, 0, 5, 2, 1, 4, 10, 8, 9, 7]
    s2, r2, p2 = _run(hip, srcs, idx, poses, [ps[k] for k in perm], prm, "two sources, permuted")
    assert r2.tobytes() == np.ascontiguousarray(results[:, perm]).tobytes() and np.array_equal(p2, prof[:, perm])
    for f in ("n_found", "n_missing", "n_ambiguous", "n_outside", "max_abs_dev"):
        assert np.array_equal(s2[f], summary[f]), f
    again = hip.probes_at(idx, [p[0] for p in poses], [p[1] for p in poses], ref.probes_array(ps), ref.record(prm), profiles=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (summary, results, prof)))


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


def _hit_probes(t):
    th, tw = t.shape
    ring = [tuple(p) for p in M.circle_probes(tw / 2.0, th / 2.0, min(tw, th) / 3.0, 9)]
    row = [tuple(p) for p in M.line_probes((2.0, 1.5), (tw - 2.0, 2.5), 6)]
    return ring + row + [(tw / 2.0, th / 2.0, 37.5)], ref.params(24, 5, 2, 12, 0, "nearest")


def test_last_probes_after_a_search(hip, templates):
    s, t, lts, angs = _search(hip, templates)
    ps, prm = _hit_probes(t)
    arr, rec = ref.probes_array(ps), ref.record(prm)
    got = hip.last_probes(arr, rec, source=0, profiles=True)
    ref.assert_call(*got, [s], [0, 0, 0], lts, angs, ps, prm, "last_probes")
    assert got[0]["n_found"].sum() > 0
    at = hip.probes_at(0, lts, angs, arr, rec, profiles=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, at))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hip.last_probes(arr, rec), got[:2]))      # source = -1: all
    # after adoption the probes sample at the aligned poses
    al = hip.align_last(0, adopt=True)
    assert (al["best_eval"] > 0).any(), "no hit moved: the test shows nothing"
    alt, aang = np.stack([al["lt_x"], al["lt_y"]], 1), al["angle"]
    got2 = hip.last_probes(arr, rec, source=0, profiles=True)
    at2 = hip.probes_at(0, alt, aang, arr, rec, profiles=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got2, at2))
    assert got2[0].tobytes() != got[0].tobytes()
    ref.assert_call(*got2, [s], [0, 0, 0], [tuple(p) for p in alt.tolist()], aang.tolist(), ps, prm, "adopted")


def test_last_probes_under_bitwise_not(hip, templates):
    s, t, lts, angs = _search(hip, templates, bitwise_not=True)     # staged: 255 - s; sampled: the inverted plane, s
    try:
        ps, prm = _hit_probes(t)
        got = hip.last_probes(ref.probes_array(ps), ref.record(prm), source=0, profiles=True)
        ref.assert_call(*got, [s], [0, 0, 0], lts, angs, ps, prm, "bitwise_not")
        assert got[0]["n_found"].sum() > 0
    finally:
        hip.setBitwiseNot(False)


# ---- state ------------------------------------------------------------------------------------------------------------
def _results(m, n_src):
    n = (C.c_int32 * n_src)()
    m._lib.fpm_last_results(m._ctx, None, 0, n)
    out = (L.Result * max(sum(n), 1))()
    assert m._lib.fpm_last_results(m._ctx, out, sum(n), n) == L.FPM_OK
    return bytes(out), list(n)


def test_state_profile_and_nothing_else_changes(gpu_matcher_factory, templates):
    make, cprm = CASES["dst10_multi"]
    s, t = make(templates)
    m = gpu_matcher_factory(**cprm)
    ps, prm = _hit_probes(t)
    arr, rec = ref.probes_array(ps), ref.record(prm)
    K = len(arr)
    with pytest.raises(ValueError):
        m.last_probes(arr, rec)                                 # no template, nothing staged
    with pytest.raises(ValueError, match="no staged sources"):
        m.probes_at(0, [(10.0, 10.0)], [0.0], arr, rec)
    assert m.learnPattern(t)
    with pytest.raises(ValueError, match="no staged sources"):
        m.last_probes(arr, rec)
    m.stage([s])
    with pytest.raises(ValueError, match="no search has run"):
        m.last_probes(arr, rec)
    assert m.probes_at(0, [(10.0, 10.0)], [5.0], arr, rec)[1].shape == (1, K)      # poses of the caller's need no search
    m.match_staged_launch()
    for call in (lambda: m.last_probes(arr, rec), lambda: m.probes_at(0, [(10.0, 10.0)], [0.0], arr, rec)):
        with pytest.raises(ValueError, match="in flight"):
            call()
    counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [3]
    results, cands = _results(m, 1), m.last_candidates(0).tobytes()
    patches = m.last_patches(0).tobytes()
    m.profile(True)
    try:
        m.profile_reset()
        with pytest.raises(ValueError):
            m.probes_at(1, [(10.0, 10.0)], [5.0], arr, rec)     # source index past the batch
        with pytest.raises(ValueError, match="2\\^20"):
            m.probes_at(0, [(2e6, 10.0)], [5.0], arr, rec)
        far = arr.copy()
        far[3]["x"] = 3e6                                        # one probe's grid beyond the samplers' range
        with pytest.raises(ValueError, match="2\\^20"):
            m.last_probes(far, rec)
        assert m.probe_profile() == (0.0, 0, 0)                  # nothing was launched
        # one launch per call; bytes = L W per (hit, probe) + the job table + the records and profiles written
        got = m.last_probes(arr, rec, source=0)
        tab = -(-(64 * 3 + 32 * K) // 256) * 256
        recs = -(-(24 * 3 * K) // 16) * 16
        ms, launches, nbytes = m.probe_profile()
        assert launches == 1 and ms > 0 and nbytes == 3 * K * 24 * 5 + tab + recs
        m.last_probes(arr, rec, source=-1, profiles=True)
        m.probes_at(0, [(10.0, 10.0)] * 5, [5.0] * 5, arr[:2], rec)
        ms, launches, nbytes = m.probe_profile()
        assert launches == 3 and m.profile_get(L.K_PATCH)[1] == 0 and m.caliper_profile()[1] == 0
        assert len(L.KERNEL_NAMES) == 15 and len(L.PROFILE_NAMES) == 16     # no FPM_K_* index was added
        m.profile_reset()
        assert m.probe_profile() == (0.0, 0, 0)
    finally:
        m.profile(False)
    assert got[0]["n_found"].sum() > 0
    # the search's records and the poses are what they were, and a following search returns what it returned
    assert _results(m, 1) == results and m.last_candidates(0).tobytes() == cands and m.last_patches(0).tobytes() == patches
    assert len(m.match_staged()[0]) == 3 and _results(m, 1) == results and m.last_candidates(0).tobytes() == cands
    m.stage([s])                                                # staged again, not searched
    with pytest.raises(ValueError, match="no search has run"):
        m.last_probes(arr, rec)
    m.match_staged_candidates()                                 # a search without results
    none = m.last_probes(arr, rec, source=-1)
    assert none[0].shape == (0,) and none[1].shape == (0, K)
