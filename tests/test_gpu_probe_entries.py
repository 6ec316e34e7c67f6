"""fpm_last_probes / fpm_probes_at held to the step order of DESIGN.md section 14.1, row by row, in the manner of
tests/test_gpu_hit_entries.py (whose Tool, rows and check this file reuses): for every row the return code, the text left
in the context's error string, ``*n`` and whether the marker-filled output buffers are still all marker.  The expected
codes and texts are literals, read off csrc/fpm_engine.hip: they pin the order of the checks, which decides a call with
two faults.  One source and three hits (CASES["dst10_multi"]), one search."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests.cases import CASES
from tests.test_gpu_hit_entries import (CAPACITY, HITS, IN_FLIGHT, INV, MARK, NO_SEARCH, NO_SOURCES, NO_SOURCES_CALIPER,
                                        NO_TEMPLATE, NULLS, OK, ONE, Poses, Tool, call_last, check, marked, ptr)

pytestmark = pytest.mark.gpu

EARLY, LATE, CAP_MSG = "1 .. 4096 probes expected", "null summary or result buffer", "probe buffers too small"
K, STRIDE = 7, 30


def make_tool(tw, th):
    probes = np.zeros(K, M.PROBE_DTYPE)
    probes["x"] = tw / 2.0 + np.arange(K) - 3.0
    probes["y"] = th / 2.0
    probes["phi"] = 37.5 * np.arange(K)
    probes[K - 1] = (-40.0, 3.0 * th, 10.0)             # far off the template: a probe needs no rectangle inside it
    prm = M.probe_params(24, 5, 2, 12, 0, "nearest")
    b = dict(summary=marked((HITS,), M.PROBE_SUMMARY_DTYPE), results=marked((HITS, K), M.PROBE_RESULT_DTYPE),
             prof=marked((HITS, K, STRIDE), np.int32))

    def args(b, bad, probes=probes, prm=prm, stride=STRIDE, n_probes=K):
        none = bad in ("late", "count")
        return (ptr(probes, L.Probe), 0 if bad == "early" else n_probes, ptr(np.atleast_1d(prm), L.ProbeParams),
                None if none else ptr(b["summary"], L.ProbeSummary), None if bad == "count" else ptr(b["results"], L.ProbeResult),
                None if bad == "count" else ptr(b["prof"], C.c_int32), stride)

    def last(m, source, cap, n, bad, b=b, **kw):
        return m._lib.fpm_last_probes(m._ctx, source, *args(b, bad, **kw), cap, C.byref(n))

    def at(m, p, bad, b=b, **kw):
        return m._lib.fpm_probes_at(m._ctx, p[0], p[1], p[2], p[3], *args(b, bad, **kw))

    tool = Tool("probes", b, last, at, EARLY, LATE, cap_msg=CAP_MSG, no_template_at=NO_SOURCES_CALIPER,
                no_sources_at=NO_SOURCES_CALIPER)
    tool.probes, tool.prm = probes, prm
    return tool


@pytest.fixture(scope="module")
def scene(templates):
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    return s, t, prm


@pytest.fixture(scope="module")
def tool(scene):
    th, tw = scene[1].shape
    return make_tool(tw, th)


@pytest.fixture(scope="module")
def searched(gpu_matcher_factory, scene):
    s, t, prm = scene
    m = gpu_matcher_factory(**prm)
    assert m.learnPattern(t)
    m.stage([s])
    counts, res = m.match_staged_array()
    assert counts.tolist() == [HITS]
    rows = res[0, :HITS]
    return m, Poses([0] * HITS, rows[:, 0:2], rows[:, 10])


def test_states(gpu_matcher_factory, scene, tool):
    """Step 3.  Not learned, nothing staged, staged but not searched, search in flight: both entries.  The _at entry needs
    staged sources only (as fpm_calipers_at), the last entry a template and a search."""
    s, t, prm = scene
    m = gpu_matcher_factory(**prm)
    tool.reset()

    def both(last_expect, at_expect, at_written=False, what=""):
        rc, n = call_last(m, tool)
        check(m, tool, rc, last_expect, n, 0, what=what + " last")
        check(m, tool, tool.at(m, ONE.p, None), at_expect, written=at_written, what=what + " at")

    both(NO_TEMPLATE, NO_SOURCES_CALIPER, what="no template")
    assert m.learnPattern(t)
    both(NO_SOURCES, NO_SOURCES_CALIPER, what="nothing staged")
    m.stage([s])
    both(NO_SEARCH, (OK, None), at_written=True, what="not searched")
    rc, n = call_last(m, tool, bad="early")                     # step 2 before step 3: the argument before the state
    check(m, tool, rc, (INV, EARLY), n, 0, what="early + not searched")
    m.match_staged_launch()
    try:
        both(IN_FLIGHT, IN_FLIGHT, what="in flight")
    finally:
        counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [HITS]


def test_rows(searched, tool):
    """Steps 1, 2, 5, 6 and 7 and the order between them, the rows of tests/test_gpu_hit_entries.py::test_rows."""
    m, _ = searched
    tool.reset()
    rows = [(dict(source=1), (INV, "bad source index"), 0),
            (dict(source=-2), (INV, "bad source index"), 0),
            (dict(bad="early", cap=HITS - 1), (INV, EARLY), 0),            # two faults: the argument before the capacity
            (dict(bad="count", cap=0), (CAPACITY, CAP_MSG), HITS),
            (dict(cap=HITS - 1), (CAPACITY, CAP_MSG), HITS),
            (dict(bad="late", cap=HITS - 1), (CAPACITY, CAP_MSG), HITS),   # two faults: the capacity first
            (dict(bad="late"), (INV, LATE), HITS)]
    for kw, expect, n_expect in rows:
        rc, n = call_last(m, tool, **kw)
        check(m, tool, rc, expect, n, n_expect, what=f"last {kw}")
    rows = [(NULLS, None, (OK, None)),
            (NULLS, "early", (INV, EARLY)),
            ((None, None, None, -1), None, (INV, "bad poses")),
            (ONE.p, "early", (INV, EARLY))]
    rows += [(ONE.without(k), None, (INV, "bad poses")) for k in range(3)]
    rows += [(ONE.without(k), "early", (INV, "bad poses")) for k in range(3)]       # two faults: the poses first
    rows += [(NULLS, "late", (OK, None)), (ONE.p, "late", (INV, LATE)), (ONE.without(1), "late", (INV, "bad poses"))]
    for p, bad, expect in rows:
        if expect[1] is None:
            before = m.last_error()
        check(m, tool, tool.at(m, p, bad), expect, what=f"at {p[3]} {[v is None for v in p[:3]]} {bad}")
        if expect[1] is None:
            assert m.last_error() == before


def test_arguments_and_outputs(searched, tool):
    """Step 2 in full (the probes, the parameters), step 4 (none: a probe may lie off the template), step 5's pose checks
    and step 6 (null outputs, the stride, hits x probes), each with nothing launched and nothing written."""
    m, poses = searched
    tool.reset()
    m.profile(True)
    try:
        m.profile_reset()

        def last(expect, n_expect, **kw):
            n = C.c_int32(-7)
            check(m, tool, tool.last(m, 0, HITS, n, None, **kw), expect, n, n_expect, what=f"last {sorted(kw)}")

        # step 2: the argument rules, before the hits are counted (*n stays 0)
        last((INV, EARLY), 0, n_probes=4097)
        for field, v, msg in [("length", 3, "length must be 4 .. 64"), ("length", 65, "length must be 4 .. 64"),
                              ("width", 0, "width must be 1 .. 16"), ("width", 17, "width must be 1 .. 16"),
                              ("half", 0, "half must be"), ("half", 9, "half must be"), ("half", 13, "half must be"),
                              ("contrast", 0, "contrast must be"), ("contrast", 256, "contrast must be"),
                              ("polarity", 2, "polarity must be"), ("select", 4, "unknown select rule"),
                              ("select", -1, "unknown select rule"), ("reserved", 1, "reserved must be 0")]:
            bad = tool.prm.copy()
            bad[field] = v
            last((INV, "probe: " + msg), 0, prm=bad)
        for field, v in [("x", float("nan")), ("y", float("inf")), ("phi", float("-inf"))]:
            bad = tool.probes.copy()
            bad[2][field] = v
            last((INV, "probe: x, y and phi must be finite"), 0, probes=bad)
        n = C.c_int32(-7)
        rc = m._lib.fpm_last_probes(m._ctx, 0, ptr(tool.probes, L.Probe), K, None, None, None, None, 0, HITS, C.byref(n))
        check(m, tool, rc, (INV, "null probe parameters"), n, 0, what="null params")
        # step 5: a pose of the caller's that is no pose, and a probe or a pose beyond the samplers' 2^20 range
        far = tool.probes.copy()
        far[4]["x"] = 3e6
        last((INV, "farther than 2^20 pixels from the source"), HITS, probes=far)
        check(m, tool, tool.at(m, Poses([1], [(10.0, 10.0)], [0.0]).p, None), (INV, "pose 0: bad source index"), what="source 1")
        check(m, tool, tool.at(m, Poses([0], [(float("nan"), 10.0)], [0.0]).p, None), (INV, "pose 0: not finite"), what="nan")
        check(m, tool, tool.at(m, Poses([0, 0], [(10.0, 10.0), (2e6, 10.0)], [0.0, 0.0]).p, None),
              (INV, "pose 1: farther than 2^20 pixels from the source"), what="far pose")
        # step 6: the outputs, after the capacity
        last((INV, "profile_stride below the length"), HITS, stride=23)
        n = C.c_int32(-7)
        rc = m._lib.fpm_last_probes(m._ctx, 0, ptr(tool.probes, L.Probe), K, ptr(np.atleast_1d(tool.prm), L.ProbeParams),
                                    ptr(tool.bufs["summary"], L.ProbeSummary), None, None, 0, HITS, C.byref(n))
        check(m, tool, rc, (INV, LATE), n, HITS, what="null results")
        many = Poses([0] * 1025, [(10.0, 10.0)] * 1025, [0.0] * 1025)      # 1025 x 4096 > 2^22: checked before any buffer is touched
        big = np.zeros(4096, M.PROBE_DTYPE)
        check(m, tool, tool.at(m, many.p, None, probes=big, n_probes=4096), (INV, "hits x probes above 2^22"), what="slots")
        assert m.probe_profile() == (0.0, 0, 0)                  # nothing was launched by any row above
    finally:
        m.profile(False)


def test_pair_agrees(searched, tool):
    """Step 7.  The last entry and the _at entry fed the poses of fpm_last_results return the same bytes; a profile
    stride above the length is zero-filled; without profiles the records are the same."""
    m, poses = searched
    tool.reset()
    rc, n = call_last(m, tool)
    assert rc == OK and n.value == HITS, (rc, m.last_error())
    a = tool.snapshot()
    assert not any(set(s) <= {MARK} for s in a)
    prof = tool.bufs["prof"]
    assert not prof[:, :, 24:].any() and prof[:, :, :24].any()
    found = int(tool.bufs["summary"]["n_found"].sum())
    assert found > 0 and (tool.bufs["summary"]["n_found"] + tool.bufs["summary"]["n_missing"] == K).all()
    tool.reset()
    assert tool.at(m, poses.p, None) == OK
    assert tool.snapshot() == a
    tool.reset()
    n = C.c_int32()
    rc = m._lib.fpm_last_probes(m._ctx, -1, ptr(tool.probes, L.Probe), K, ptr(np.atleast_1d(tool.prm), L.ProbeParams),
                                ptr(tool.bufs["summary"], L.ProbeSummary), ptr(tool.bufs["results"], L.ProbeResult), None, 0,
                                HITS, C.byref(n))
    assert rc == OK and n.value == HITS
    assert tool.snapshot()[:2] == a[:2] and set(tool.snapshot()[2]) <= {MARK}
    tool.reset()
