"""Bitwise-not search on the HIP path (fpm_params.bitwise_not: the MFC tool's m_ckBitwiseNot, MatchToolDlg.cpp:788-796),
through the C ABI: the k_bitwise_not operator byte for byte, searches of 255 - source against the oracle on the inverted
image, and the context's tracking of its staged slab's polarity.  Every comparison is exact."""
import numpy as np
import pytest

from tests import oracle
from tests.cases import CASES
from tests.fast_mode_ref import fast_reference
from tests.test_gpu_parity import assert_same_results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


def _setup(hip, t, prm, **extra):
    hip.resetParams()
    for k, v in {**prm, **extra}.items():
        setattr(hip._params, k, v)
    assert hip.learnPattern(t)


def _oracle(t, prm):
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    return o


def _inv(s):
    return np.ascontiguousarray(255 - s)


def _tuples(res):
    return [r.as_tuple() for r in res]


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (9, 17), (33, 67), (64, 64), (5, 4099)])
def test_bitwise_not_operator(hip, shape):
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    out = hip.bitwise_not(img)
    assert out.dtype == np.uint8 and np.array_equal(out, 255 - img)


def test_bitwise_not_operator_strided(hip):
    wide = np.random.default_rng(5).integers(0, 256, (33, 200), dtype=np.uint8)
    view = wide[:, 11:78]   # 33 x 67, row stride 200
    assert view.strides == (200, 1)
    assert np.array_equal(hip.bitwise_not(view), 255 - view)


def _check_search(hip, o, s_hip, s_orc, label):
    """hip (bitwise_not on) over s_hip == the oracle over s_orc: results, records, stats."""
    exp = o.match(s_orc)
    got = hip.match(s_hip)
    assert_same_results(got, exp, label)
    assert hip.last_candidates(0).tobytes() == o.candidates().tobytes(), f"{label}: records differ"
    assert hip.search_stats() == o.stats(), label
    return exp


@pytest.mark.parametrize("case", sorted(CASES))
def test_bitwise_not_search(hip, templates, case):
    make, prm = CASES[case]
    s, t = make(templates)
    o = _oracle(t, prm)
    _setup(hip, t, prm, bitwise_not=1)
    assert len(_check_search(hip, o, _inv(s), s, f"{case} inverted source")) >= 1
    _check_search(hip, o, s, _inv(s), f"{case} plain source")
    if case in ("dst1_rot30", "dst5_subpixel"):   # the inverted scene still has top-layer candidates to descend
        assert len(o.candidates()) >= 10


@pytest.mark.parametrize("width", [557, 558, 559])
def test_bitwise_not_search_ragged_width(hip, templates, width):
    """Row lengths that end in the kernel's dword and byte tails."""
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    s = np.ascontiguousarray(s[:, :width])
    o = _oracle(t, prm)
    assert len(o.match(s)) >= 1
    _setup(hip, t, prm, bitwise_not=1)
    _check_search(hip, o, _inv(s), s, f"width {width}")
    _check_search(hip, o, s, _inv(s), f"width {width} plain source")


def test_polarity_tracking(gpu_matcher_factory, templates):
    make, prm = CASES["dst1_rot30"]
    s, t = make(templates)
    srcs = [s, _inv(s)]
    o = _oracle(t, prm)
    plain = [o.match(x) for x in srcs]
    inverted = [o.match(_inv(x)) for x in srcs]
    assert len(plain[0]) >= 1 and len(inverted[1]) >= 1
    m = gpu_matcher_factory()
    _setup(m, t, prm, bitwise_not=1)
    m.stage(srcs)
    first = m.match_staged()
    m._params.bitwise_not = 0
    second = m.match_staged()
    m._params.bitwise_not = 1
    third = m.match_staged()
    for i in range(2):
        assert_same_results(first[i], inverted[i], f"pass 1 source {i}")
        assert_same_results(second[i], plain[i], f"pass 2 source {i}")
        assert _tuples(third[i]) == _tuples(first[i])
    m.stage(srcs)   # a fresh upload is plain again, whatever the slab held
    again = m.match_staged()
    assert [_tuples(r) for r in again] == [_tuples(r) for r in first]
    # lone searches: on, then off
    assert_same_results(m.match(s), inverted[0], "lone, on")
    m._params.bitwise_not = 0
    assert_same_results(m.match(s), plain[0], "lone, off")


def test_bitwise_not_with_fast_mode(hip, templates):
    make, prm = CASES["dst3_range"]
    s, t = make(templates)
    rec, _, _, _ = fast_reference(t, s, prm)
    _setup(hip, t, prm, bitwise_not=1, stop_layer=1)
    hip.match(_inv(s))
    got = hip.last_candidates(0)
    for f in rec.dtype.names:
        assert np.array_equal(got[f], rec[f]), f
    assert got.tobytes() == rec.tobytes() and rec["kept"].sum() >= 1
