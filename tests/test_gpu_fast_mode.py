"""Fast mode on the HIP path (fpm_params.stop_layer: the MFC tool's m_bStopLayer1, MatchToolDlg.cpp:936-1054), through
the C ABI, against the records tests/fast_mode_ref.py derives from the oracle's trace.  Every comparison is exact."""
import numpy as np
import pytest

from fastest_image_pattern_matching_amd.matcher import merge_candidates
from tests.cases import CASES, _scene_rotated
from tests.fast_mode_ref import fast_reference
from tests.test_gpu_parity import assert_same_results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


_refs = {}


def _ref(templates, case):
    """(scene, template, params, fast records, oracle, normal results, L) of a shared case, computed once."""
    if case not in _refs:
        make, prm = CASES[case]
        s, t = make(templates)
        _refs[case] = (s, t, prm) + fast_reference(t, s, prm)
    return _refs[case]


def _setup(hip, t, prm, **extra):
    hip.resetParams()
    for k, v in {**prm, **extra}.items():
        setattr(hip._params, k, v)
    assert hip.learnPattern(t)


def _assert_records(got, exp, label):
    assert len(got) == len(exp), f"{label}: {len(got)} records vs {len(exp)}"
    for f in exp.dtype.names:
        bad = np.nonzero(got[f] != exp[f])[0]
        assert bad.size == 0, f"{label}: field {f} differs at {bad[:5]}: {got[f][bad[:5]]} vs {exp[f][bad[:5]]}"
    assert got.tobytes() == exp.tobytes(), label


def _tuples(res):
    return [r.as_tuple() for r in res]


@pytest.mark.parametrize("case", sorted(CASES))
def test_fast_mode_records_and_stats(hip, templates, case):
    s, t, prm, rec, o, _, L = _ref(templates, case)
    _setup(hip, t, prm, stop_layer=1)
    hip.match(s)
    _assert_records(hip.last_candidates(0), rec, case)
    assert hip.search_stats() == o.stats()[:2 + L - min(1, L)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_fast_mode_results(hip, templates, case):
    s, t, prm, rec, _, normal, L = _ref(templates, case)
    _setup(hip, t, prm, stop_layer=1)
    got = hip.match(s)
    th, tw = t.shape
    exp = merge_candidates(hip._params, tw, th, rec)
    assert _tuples(got) == _tuples(exp)
    assert len(got) >= 1
    if (th, tw) == (54, 54):   # even sizes: the overlap rectangle is the level-0 one
        hip._params.stop_layer = 0
        assert _tuples(got) == _tuples(merge_candidates(hip._params, tw, th, rec))
    if L == 0:
        assert_same_results(got, normal, case)


@pytest.mark.parametrize("env", ["FPM_STEP_PROLOGUE", "FPM_STEP_TABLES"])
@pytest.mark.parametrize("value", ["0", "1"])
@pytest.mark.parametrize("case", ["dst1_rot30", "dst3_range"])
def test_fast_mode_schedule_switches(gpu_matcher_factory, templates, monkeypatch, case, env, value):
    s, t, prm, rec, _, _, _ = _ref(templates, case)
    monkeypatch.setenv(env, value)
    m = gpu_matcher_factory()
    _setup(m, t, prm, stop_layer=1)
    m.match(s)
    _assert_records(m.last_candidates(0), rec, f"{case} {env}={value}")


def test_fast_mode_batch_and_toggle(gpu_matcher_factory, templates):
    """Three staged scenes; fast, normal and fast again over the same staged batch (the plan is re-recorded)."""
    prm = CASES["dst3_range"][1]
    scenes = [_scene_rotated(templates, "Dst3", [(150, 150, 12.0), (400, 260, -33.0)], (560, 420), seed)
              for seed in (7, 17, 27)]
    t = scenes[0][1]
    th, tw = t.shape
    refs = [fast_reference(t, s, prm) for s, _ in scenes]
    m = gpu_matcher_factory()
    _setup(m, t, prm, stop_layer=1)
    m.stage([s for s, _ in scenes])
    first = m.match_staged()
    for i, (rec, _, _, _) in enumerate(refs):
        assert _tuples(first[i]) == _tuples(merge_candidates(m._params, tw, th, rec)), i
        assert len(first[i]) >= 1
    for i, c in enumerate(m.match_staged_candidates()):
        exp = refs[i][0].copy()
        exp["source"] = i
        _assert_records(c, exp, f"staged {i}")
    m._params.stop_layer = 0
    for i, got in enumerate(m.match_staged()):
        assert_same_results(got, refs[i][2], f"normal {i}")
        exp = refs[i][1].candidates().copy()
        exp["source"] = i
        _assert_records(m.last_candidates(i), exp, f"normal staged {i}")
    m._params.stop_layer = 1
    again = m.match_staged()
    assert [_tuples(r) for r in again] == [_tuples(r) for r in first]


def test_fast_mode_angle_shards(gpu_matcher_factory, templates):
    s, t, prm, rec, _, _, _ = _ref(templates, "dst10_multi")
    whole = gpu_matcher_factory()
    _setup(whole, t, prm, stop_layer=1)
    full = whole.match(s)
    _assert_records(whole.last_candidates(0), rec, "unsharded")
    parts = []
    for k in range(2):
        m = gpu_matcher_factory()
        _setup(m, t, prm, stop_layer=1)
        m.setAngleShard(k, 2)
        m.match(s)
        parts.append(m.last_candidates(0))
    assert len(parts[0]) and len(parts[1])
    _assert_records(np.concatenate(parts), rec, "shards concatenated")
    merged = merge_candidates(whole._params, t.shape[1], t.shape[0], np.concatenate(parts))
    assert _tuples(merged) == _tuples(full) and len(full) >= 1
