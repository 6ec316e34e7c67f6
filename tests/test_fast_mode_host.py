"""Fast mode (fpm_params.stop_layer, MatchToolDlg.cpp:936-1054) and bitwise-not (fpm_params.bitwise_not, :788-796): the
parts that need no device -- the ABI defaults, the overlap filter's rectangle in fpm_merge_candidates (:1053-1054) and
the trace-derived reference of tests/fast_mode_ref.py."""
import ctypes as C

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib
from fastest_image_pattern_matching_amd.matcher import CANDIDATE_DTYPE, merge_candidates
from tests import oracle
from tests.cases import CASES
from tests.fast_mode_ref import fast_reference


def test_defaults_and_abi(fpm_lib):
    names = [f[0] for f in _lib.Params._fields_]
    assert names[-2:] == ["stop_layer", "bitwise_not"]   # appended: the oracle's memset default leaves them 0
    p = _lib.Params()
    p.stop_layer = p.bitwise_not = 7
    fpm_lib.fpm_params_default(C.byref(p))
    assert (p.stop_layer, p.bitwise_not) == (0, 0)
    assert fpm_lib.fpm_abi_version() == 11


def _params(fpm_lib, **kw):
    p = _lib.Params()
    fpm_lib.fpm_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _two_records(dx, y=40.0, x=30.0):
    """Two kept records at angle 0 on one row, `dx` apart, scores 0.9 and 0.8 (push order: one angle, ranks 0, 1)."""
    c = np.zeros(2, CANDIDATE_DTYPE)
    c["top_score"] = [0.9, 0.8]
    c["score"] = [0.9, 0.8]
    c["x"] = [x, x + dx]
    c["y"] = y
    c["peak_rank"] = [0, 1]
    c["kept"] = 1
    return c


def _top_layer(w, h, min_reduce_area):
    """The search's own rule, through the oracle: levels of a learned w x h template minus one."""
    o = oracle.OracleMatcher().set(min_reduce_area=min_reduce_area)
    assert o.learnPattern(np.random.default_rng(w * 100 + h).integers(0, 256, (h, w), dtype=np.uint8))
    return len(o.template_levels()[0]) - 1


def _spans(res, w, h):
    for r in res:
        assert (r.ptRT[0] - r.ptLT[0], r.ptRT[1] - r.ptLT[1]) == (w, 0.0)
        assert (r.ptLB[0] - r.ptLT[0], r.ptLB[1] - r.ptLT[1]) == (0.0, h)


def test_overlap_rectangle_is_the_doubled_layer1_size(fpm_lib):
    w = h = 9
    assert _top_layer(w, h, 16) >= 1
    c = _two_records(w - 0.5)
    kw = dict(min_reduce_area=16, max_overlap=0.1, score=0.5)
    normal = merge_candidates(_params(fpm_lib, stop_layer=0, **kw), w, h, c)
    fast = merge_candidates(_params(fpm_lib, stop_layer=1, **kw), w, h, c)
    # 9 wide: the rectangles share 0.5 / 9 of their area; 10 wide (layer 1's 5 x 5 times two): 1.5 / 10
    assert [r.dMatchScore for r in normal] == [0.9, 0.8]
    assert [r.dMatchScore for r in fast] == [0.9]
    assert fast[0] == normal[0]
    _spans(normal, 9.0, 9.0)   # the corners keep the level-0 size (MatchToolDlg.cpp:1080)
    _spans(fast, 9.0, 9.0)


def test_overlap_rectangle_unchanged_for_even_sizes(fpm_lib):
    w, h = 10, 8
    assert _top_layer(w, h, 16) >= 1
    kw = dict(min_reduce_area=16, max_overlap=0.1, score=0.5)
    for dx in (w - 0.5, w - 1.5):   # either side of the 0.1 overlap
        c = _two_records(dx)
        normal = merge_candidates(_params(fpm_lib, stop_layer=0, **kw), w, h, c)
        fast = merge_candidates(_params(fpm_lib, stop_layer=1, **kw), w, h, c)
        assert fast == normal and len(normal) == (2 if dx == w - 0.5 else 1)


def test_stop_layer_clamps_to_a_top_layer_of_zero(fpm_lib):
    w = h = 9
    assert _top_layer(w, h, 1024) == 0
    c = _two_records(w - 0.5)
    kw = dict(min_reduce_area=1024, max_overlap=0.1, score=0.5)
    normal = merge_candidates(_params(fpm_lib, stop_layer=0, **kw), w, h, c)
    fast = merge_candidates(_params(fpm_lib, stop_layer=1, **kw), w, h, c)
    assert fast == normal and len(normal) == 2


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_helper_is_not_vacuous(templates, case):
    make, prm = CASES[case]
    s, t = make(templates)
    rec, o, _, L = fast_reference(t, s, prm)
    normal = o.candidates()
    assert len(rec) == len(normal) >= 1
    if L == 0:
        assert rec.tobytes() == normal.tobytes()
        return
    assert rec["kept"].sum() >= 1
    assert np.all(rec["kept"] >= normal["kept"])   # whatever reaches layer 0's decision passed layer 1
    for f in ("top_score", "angle_index", "peak_rank", "source"):
        assert np.array_equal(rec[f], normal[f])
    dead = rec[rec["kept"] == 0]
    assert not dead["x"].any() and not dead["y"].any() and not dead["score"].any() and not dead["angle"].any()
    if case in ("dst1_rot30", "dst3_range", "score_low_many"):
        assert not np.array_equal(rec["kept"], normal["kept"])
