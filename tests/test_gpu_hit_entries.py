"""The entry pairs of the per-hit tools (fpm_last_X / fpm_X_at) as one table: for every pair the same rows of calls
through the C ABI, with the output buffers pre-filled with a marker byte, and for every row the return code, the text
left in the context's error string, ``*n`` and whether the buffers are still all marker.  The expected codes and texts
are literals, read off csrc/fpm_engine.hip: they pin the order of the checks, which decides a call with two faults.
One source and three hits (CASES["dst10_multi"]), one search."""
import ctypes as C

import numpy as np
import pytest
import torch

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests.cases import CASES

pytestmark = pytest.mark.gpu

OK, INV, NOT_LEARNED, CAPACITY = L.FPM_OK, L.FPM_E_INVALID_ARG, L.FPM_E_NOT_LEARNED, L.FPM_E_CAPACITY
MARK = 0xA5
HITS = 3
RECT = (3, 2, 21, 17)                    # inside every template of the cases
RW, RH = RECT[2], RECT[3]
ROW, PATCH = RW, RW * RH
CAP_PER = 64                             # blob records per hit: no hit of the scene is truncated

NO_TEMPLATE = (NOT_LEARNED, "template not learned")
NO_SOURCES = (INV, "no staged sources to take patches from")
NO_SOURCES_CALIPER = (INV, "no staged sources to measure on")
NO_SEARCH = (INV, "no search has run since the sources were staged")
IN_FLIGHT = (INV, "a search is in flight")
NO_MODEL = (INV, "no variation model")
PATCH_CAP = "patch buffer too small"


def marked(shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(bytearray([MARK]) * n, dtype).reshape(shape)


def ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def rect_ptr(r=RECT):
    return C.byref(L.PatchRect(*r))


class Tool:
    """One entry pair.  ``last(m, source, cap, n, bad)`` and ``at(m, pose, bad)`` make the C calls (None: the pair has
    no such entry); ``bad`` is None, "early" (the tool argument that is checked before the poses are looked at), "late"
    (the one checked after the capacity) or "count" (every output NULL: the count-only call).  ``early`` and ``late``
    are the texts of those two faults, ``cap_msg`` the tool's own capacity text."""

    def __init__(self, name, bufs, last, at, early, late, cap_msg=PATCH_CAP, early_beats_state=True,
                 no_template_at=NO_TEMPLATE, no_sources_at=NO_SOURCES, unsearched_at=(OK, None)):
        self.name, self.bufs, self.last, self.at = name, bufs, last, at
        self.early, self.late, self.cap_msg = early, late, cap_msg
        self.early_beats_state = early_beats_state
        self.no_template_at, self.no_sources_at, self.unsearched_at = no_template_at, no_sources_at, unsearched_at

    def snapshot(self):
        return [b.cpu().numpy().tobytes() if isinstance(b, torch.Tensor) else b.tobytes() for b in self.bufs.values()]

    def reset(self):
        for b in self.bufs.values():
            if isinstance(b, torch.Tensor):
                b.fill_(MARK)
            else:
                b.view(np.uint8)[...] = MARK

    def untouched(self):
        return all(set(s) <= {MARK} for s in self.snapshot())


def make_tools(tw, th):
    """The pairs, each with buffers for HITS hits."""
    tools = []

    # patches: host, device, _at
    b = dict(out=marked((HITS, RH, RW), np.uint8), mats=marked((HITS, 6), np.float64))

    def patch_args(b, bad):
        r = rect_ptr((3, 2, 0, 17) if bad == "early" else RECT)
        none = bad in ("late", "count")
        return r, (None if none else L.u8ptr(b["out"])), (None if bad == "count" else ptr(b["mats"], C.c_double))

    def patches_last(m, source, cap, n, bad, b=b):
        r, out, mats = patch_args(b, bad)
        return m._lib.fpm_last_patches(m._ctx, r, source, out, ROW, PATCH, cap, C.byref(n), mats)

    def patches_at(m, p, bad, b=b):
        r, out, mats = patch_args(b, bad)
        return m._lib.fpm_patches_at(m._ctx, r, p[0], p[1], p[2], p[3], out, ROW, PATCH, mats)

    tools.append(Tool("patches", b, patches_last, patches_at, "bad patch rectangle", "null patch buffer",
                      early_beats_state=False))

    b = dict(out=torch.full((HITS, RH, RW), MARK, dtype=torch.uint8, device="cuda:0"))

    def patches_device(m, source, cap, n, bad, b=b):
        r = rect_ptr((3, 2, 0, 17) if bad == "early" else RECT)
        out = None if bad in ("late", "count") else b["out"].data_ptr()
        return m._lib.fpm_last_patches_device(m._ctx, r, source, out, ROW, PATCH, cap, C.byref(n), m._producer_stream(None))

    tools.append(Tool("patches_device", b, patches_device, None, "bad patch rectangle", "null patch buffer",
                      early_beats_state=False))

    # compare
    b = dict(stats=marked((HITS,), M.COMPARE_DTYPE), diff=marked((HITS, RH, RW), np.uint8))

    def compare_args(b, bad):
        none = bad in ("late", "count")
        return (256 if bad == "early" else 16), (None if none else ptr(b["stats"], L.CompareStats)), \
            (None if bad == "count" else L.u8ptr(b["diff"]))

    def compare_last(m, source, cap, n, bad, b=b):
        t, stats, diff = compare_args(b, bad)
        return m._lib.fpm_last_compare(m._ctx, rect_ptr(), source, t, 0, stats, cap, C.byref(n), diff, ROW, PATCH)

    def compare_at(m, p, bad, b=b):
        t, stats, diff = compare_args(b, bad)
        return m._lib.fpm_compare_at(m._ctx, rect_ptr(), p[0], p[1], p[2], p[3], t, 0, stats, diff, ROW, PATCH)

    tools.append(Tool("compare", b, compare_last, compare_at, "threshold must be 0 .. 255", "null statistics buffer"))

    # model_train: no output buffer and no capacity; *n is the count added
    def train_last(m, source, cap, n, bad):
        return m._lib.fpm_model_train_last(m._ctx, rect_ptr(), source, 2 if bad == "early" else 0, C.byref(n))

    def train_at(m, p, bad):
        return m._lib.fpm_model_train_at(m._ctx, rect_ptr(), p[0], p[1], p[2], p[3], 2 if bad == "early" else 0)

    tools.append(Tool("model_train", {}, train_last, train_at, "unknown training flags", None, cap_msg=None))

    # inspect
    b = dict(stats=marked((HITS,), M.INSPECT_DTYPE), img=marked((HITS, RH, RW), np.uint8))

    def inspect_args(b, bad):
        none = bad in ("late", "count")
        return (-1 if bad == "early" else 8), (None if none else ptr(b["stats"], L.InspectStats)), \
            (None if bad == "count" else L.u8ptr(b["img"]))

    def inspect_last(m, source, cap, n, bad, b=b):
        a, stats, img = inspect_args(b, bad)
        return m._lib.fpm_last_inspect(m._ctx, source, a, 48, 0, stats, cap, C.byref(n), img, ROW, PATCH)

    def inspect_at(m, p, bad, b=b):
        a, stats, img = inspect_args(b, bad)
        return m._lib.fpm_inspect_at(m._ctx, p[0], p[1], p[2], p[3], a, 48, 0, stats, img, ROW, PATCH)

    tools.append(Tool("inspect", b, inspect_last, inspect_at, "abs threshold must be 0 .. 255", "null statistics buffer",
                      unsearched_at=NO_MODEL))

    # blobs
    b = dict(rows=marked((HITS,), M.INSPECT_DTYPE), summary=marked((HITS,), M.BLOB_SUMMARY_DTYPE),
             recs=marked((HITS * CAP_PER,), M.BLOB_DTYPE))

    def blob_args(b, bad):
        none = bad == "count"
        return (-1 if bad == "early" else 8, 48, 0, -1 if bad == "late" else 0, 8, 4,
                None if none else ptr(b["rows"], L.InspectStats), None if none else ptr(b["summary"], L.BlobSummary),
                None if none else ptr(b["recs"], L.Blob), CAP_PER)

    def blobs_last(m, source, cap, n, bad, b=b):
        return m._lib.fpm_last_blobs(m._ctx, source, *blob_args(b, bad), cap, C.byref(n))

    def blobs_at(m, p, bad, b=b):
        return m._lib.fpm_blobs_at(m._ctx, p[0], p[1], p[2], p[3], *blob_args(b, bad))

    tools.append(Tool("blobs", b, blobs_last, blobs_at, "abs threshold must be 0 .. 255", "level must be 0 .. 254",
                      unsearched_at=NO_MODEL))

    # align: sums_at alone, then at and last
    b = dict(sums=marked((HITS,), M.ALIGN_SUMS_DTYPE))

    def sums_at(m, p, bad, b=b):
        out = None if bad in ("late", "count") else ptr(b["sums"], L.AlignSums)
        return m._lib.fpm_align_sums_at(m._ctx, rect_ptr(), p[0], p[1], p[2], p[3], 2 if bad == "early" else 0, out)

    tools.append(Tool("align_sums", b, None, sums_at, "unknown alignment flags", "null sums buffer"))

    b = dict(out=marked((HITS,), M.ALIGN_DTYPE))

    def align_args(b, bad):
        return (0 if bad == "early" else 2), 2.0, 0, (None if bad in ("late", "count") else ptr(b["out"], L.AlignResult))

    def align_last(m, source, cap, n, bad, b=b):
        return m._lib.fpm_align_last(m._ctx, rect_ptr(), source, *align_args(b, bad), cap, C.byref(n))

    def align_at(m, p, bad, b=b):
        return m._lib.fpm_align_at(m._ctx, rect_ptr(), p[0], p[1], p[2], p[3], *align_args(b, bad))

    tools.append(Tool("align", b, align_last, align_at, "iters must be 1 .. 8", "null result buffer"))

    # calipers: the _at entry needs no template
    cals = np.array([M.caliper(tw / 2, th / 2, 0.0, 24, 5), M.caliper(10.0, 8.0, 90.0, 12, 3)], M.CALIPER_DTYPE)
    stride = 30
    b = dict(summary=marked((HITS, 2), M.CALIPER_SUMMARY_DTYPE), edges=marked((HITS, 2, 4), M.EDGE_DTYPE),
             prof=marked((HITS, 2, stride), np.int32))

    def caliper_args(b, bad, cals=cals):
        none = bad in ("late", "count")
        return (ptr(cals, L.Caliper), 0 if bad == "early" else 2, 4, None if none else ptr(b["summary"], L.CaliperSummary),
                None if bad == "count" else ptr(b["edges"], L.Edge), None if bad == "count" else ptr(b["prof"], C.c_int32),
                stride)

    def calipers_last(m, source, cap, n, bad, b=b):
        return m._lib.fpm_last_calipers(m._ctx, source, *caliper_args(b, bad), cap, C.byref(n))

    def calipers_at(m, p, bad, b=b):
        return m._lib.fpm_calipers_at(m._ctx, p[0], p[1], p[2], p[3], *caliper_args(b, bad))

    tools.append(Tool("calipers", b, calipers_last, calipers_at, "1 .. 64 calipers expected", "null summary or edge buffer",
                      cap_msg="caliper buffers too small", no_template_at=NO_SOURCES_CALIPER,
                      no_sources_at=NO_SOURCES_CALIPER))

    # histogram
    rects = (L.PatchRect * 2)(L.PatchRect(*RECT), L.PatchRect(0, 0, 9, 7))
    b = dict(hist=marked((HITS, 2, 256), np.uint32))

    def hist_args(b, bad, rects=rects):
        return rects, (0 if bad == "early" else 2), (None if bad in ("late", "count") else ptr(b["hist"], C.c_uint32))

    def hist_last(m, source, cap, n, bad, b=b):
        r, k, h = hist_args(b, bad)
        return m._lib.fpm_last_histogram(m._ctx, r, k, source, h, cap, C.byref(n))

    def hist_at(m, p, bad, b=b):
        r, k, h = hist_args(b, bad)
        return m._lib.fpm_histogram_at(m._ctx, r, k, p[0], p[1], p[2], p[3], h)

    tools.append(Tool("histogram", b, hist_last, hist_at, "1 .. 64 rectangles expected", "null histogram buffer",
                      cap_msg="histogram buffer too small", early_beats_state=False))

    # segment
    b = dict(info=marked((HITS,), M.SEGMENT_INFO_DTYPE), summary=marked((HITS,), M.BLOB_SUMMARY_DTYPE),
             recs=marked((HITS * CAP_PER,), M.BLOB_DTYPE), img=marked((HITS, RH, RW), np.uint8))

    def seg_args(b, bad):
        none = bad == "count"
        return (128, 0 if bad == "early" else -1, 5 if bad == "late" else 8, 4,
                None if none else ptr(b["info"], L.SegmentInfo), None if none else ptr(b["summary"], L.BlobSummary),
                None if none else ptr(b["recs"], L.Blob), CAP_PER), (None if none else L.u8ptr(b["img"]))

    def seg_last(m, source, cap, n, bad, b=b):
        a, img = seg_args(b, bad)
        return m._lib.fpm_last_segment(m._ctx, source, rect_ptr(), *a, cap, C.byref(n), img, ROW, PATCH)

    def seg_at(m, p, bad, b=b):
        a, img = seg_args(b, bad)
        return m._lib.fpm_segment_at(m._ctx, p[0], p[1], p[2], p[3], rect_ptr(), *a, img, ROW, PATCH)

    tools.append(Tool("segment", b, seg_last, seg_at, "polarity must be +1 or -1", "connectivity must be 4 or 8"))

    # locate
    feats = np.array([M.feature(3, 2, 21, 17, 3, 5), M.feature(0, 0, 9, 7, 1, 0)], M.FEATURE_DTYPE)
    lstride = 77
    b = dict(res=marked((HITS, 2), M.LOCATE_DTYPE), raw=marked((HITS, 2), M.LOCATE_RAW_DTYPE),
             maps=marked((HITS, 2, 3, lstride), np.int32))

    def locate_args(b, bad, feats=feats):
        none = bad in ("late", "count")
        return (ptr(feats, L.Feature), 0 if bad == "early" else 2, None if none else ptr(b["res"], L.LocateResult),
                None if bad == "count" else ptr(b["raw"], L.LocateRaw), None if bad == "count" else ptr(b["maps"], C.c_int32),
                lstride)

    def locate_last(m, source, cap, n, bad, b=b):
        return m._lib.fpm_last_locate(m._ctx, source, *locate_args(b, bad), cap, C.byref(n))

    def locate_at(m, p, bad, b=b):
        return m._lib.fpm_locate_at(m._ctx, p[0], p[1], p[2], p[3], *locate_args(b, bad))

    tools.append(Tool("locate", b, locate_last, locate_at, "1 .. 64 features expected", "null result buffer",
                      cap_msg="locate buffers too small", early_beats_state=False))
    return tools


NAMES = ["patches", "patches_device", "compare", "model_train", "inspect", "blobs", "align_sums", "align", "calipers",
         "histogram", "segment", "locate"]


class Poses:
    """The three ctypes pointers and the count of an _at call; the arrays live as long as the object."""

    def __init__(self, idx, lts, angs):
        self.i, self.l, self.a = np.array(idx, np.int32), np.array(lts, np.float32).reshape(-1, 2), np.array(angs, np.float64)
        self.p = (ptr(self.i, C.c_int32), ptr(self.l, C.c_float), ptr(self.a, C.c_double), len(self.i))

    def without(self, k):
        return tuple(None if j == k else v for j, v in enumerate(self.p))


ONE = Poses([0], [(10.0, 10.0)], [0.0])
NULLS = (None, None, None, 0)


def check(m, tool, rc, expect, n=None, n_expect=None, written=False, what=""):
    """One row: the code, the text (None: the error string is what it was before the call), *n, the buffers."""
    code, msg = expect
    label = f"{tool.name} {what}"
    assert rc == code, (label, rc, m.last_error())
    if msg is not None:
        assert msg in m.last_error(), (label, m.last_error())
    if n is not None:
        assert n.value == n_expect, (label, n.value)
    if written:
        tool.reset()
    else:
        assert tool.untouched(), label


def call_last(m, tool, source=0, cap=HITS, bad=None):
    n = C.c_int32(-7)
    return tool.last(m, source, cap, n, bad), n


@pytest.fixture(scope="module")
def scene(templates):
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    return s, t, prm


@pytest.fixture(scope="module")
def tools(scene):
    th, tw = scene[1].shape
    return {t.name: t for t in make_tools(tw, th)}


@pytest.fixture(scope="module")
def searched(gpu_matcher_factory, scene):
    """The matcher after the one search, a model trained on RECT; the hits' poses as fpm_last_results gives them."""
    s, t, prm = scene
    m = gpu_matcher_factory(**prm)
    assert m.learnPattern(t)
    m.stage([s])
    counts, res = m.match_staged_array()
    assert counts.tolist() == [HITS]
    n = C.c_int32()
    assert m._lib.fpm_model_train_last(m._ctx, rect_ptr(), 0, 0, C.byref(n)) == OK and n.value == HITS
    rows = res[0, :HITS]
    return m, Poses([0] * HITS, rows[:, 0:2], rows[:, 10])


def test_tools_cover_every_pair(tools):
    assert list(tools) == NAMES


def test_states(gpu_matcher_factory, scene, tools):
    """Not learned, nothing staged, staged but not searched, search in flight: once per pair, both entries."""
    s, t, prm = scene
    m = gpu_matcher_factory(**prm)

    def both(tool, last_expect, at_expect, at_written=False, what=""):
        if tool.last:
            rc, n = call_last(m, tool)
            check(m, tool, rc, last_expect, n, 0, what=what + " last")
        if tool.at:
            check(m, tool, tool.at(m, ONE.p, None), at_expect, written=at_written, what=what + " at")

    for tool in tools.values():
        both(tool, NO_TEMPLATE, tool.no_template_at, what="no template")
    assert m.learnPattern(t)
    for tool in tools.values():
        both(tool, NO_SOURCES, tool.no_sources_at, what="nothing staged")
    m.stage([s])
    for tool in tools.values():
        both(tool, NO_SEARCH, tool.unsearched_at, at_written=tool.unsearched_at[0] == OK, what="not searched")
        m.model_clear()                                         # what model_train's _at entry has just trained
        if tool.last:                                           # a bad tool argument and no search: which is seen first
            rc, n = call_last(m, tool, bad="early")
            check(m, tool, rc, (INV, tool.early) if tool.early_beats_state else NO_SEARCH, n, 0, what="early + not searched")
    m.match_staged_launch()
    try:
        for tool in tools.values():
            both(tool, IN_FLIGHT, IN_FLIGHT, what="in flight")
    finally:
        counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [HITS]


@pytest.mark.parametrize("name", NAMES)
def test_rows(searched, tools, name):
    m, _ = searched
    tool = tools[name]
    tool.reset()
    if tool.last:
        has_cap = tool.cap_msg is not None
        rows = [(dict(source=1), (INV, "bad source index"), 0),
                (dict(source=-2), (INV, "bad source index"), 0),
                (dict(bad="early", cap=HITS - 1), (INV, tool.early), 0)]    # two faults: the argument before the capacity
        if has_cap:
            rows += [(dict(bad="count", cap=0), (CAPACITY, tool.cap_msg), HITS),
                     (dict(cap=HITS - 1), (CAPACITY, tool.cap_msg), HITS),
                     (dict(bad="late", cap=HITS - 1), (CAPACITY, tool.cap_msg), HITS),   # two faults: the capacity first
                     (dict(bad="late"), (INV, tool.late), HITS)]
        for kw, expect, n_expect in rows:
            rc, n = call_last(m, tool, **kw)
            check(m, tool, rc, expect, n, n_expect, what=f"last {kw}")
    if tool.at:
        rows = [(NULLS, None, (OK, None)),
                (NULLS, "early", (INV, tool.early)),
                ((None, None, None, -1), None, (INV, "bad poses")),
                (ONE.p, "early", (INV, tool.early))]
        rows += [(ONE.without(k), None, (INV, "bad poses")) for k in range(3)]
        rows += [(ONE.without(k), "early", (INV, "bad poses")) for k in range(3)]       # two faults: the poses first
        if tool.late:
            rows += [(NULLS, "late", (OK, None)), (ONE.p, "late", (INV, tool.late)),
                     (ONE.without(1), "late", (INV, "bad poses"))]
        for p, bad, expect in rows:
            if expect[1] is None:
                before = m.last_error()
            check(m, tool, tool.at(m, p, bad), expect, what=f"at {p[3]} {[v is None for v in p[:3]]} {bad}")
            if expect[1] is None:
                assert m.last_error() == before, name
    assert m.model_info() == (HITS, RECT)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "align_sums"])
def test_pair_agrees(searched, tools, name):
    """The last entry and the _at entry fed the poses of fpm_last_results return the same bytes."""
    m, poses = searched
    tool = tools[name]
    tool.reset()
    if name == "model_train":
        m.model_clear()
        rc, n = call_last(m, tool)
        assert rc == OK and n.value == HITS
        a = [x.tobytes() for x in m.model_sums()]
        m.model_clear()
        assert tool.at(m, poses.p, None) == OK and m.model_info() == (HITS, RECT)
        assert [x.tobytes() for x in m.model_sums()] == a
        return
    rc, n = call_last(m, tool)
    assert rc == OK and n.value == HITS, (rc, m.last_error())
    a = tool.snapshot()
    assert not all(set(s) <= {MARK} for s in a)
    if name == "patches_device":
        host = tools["patches"]
        host.reset()
        assert host.at(m, poses.p, None) == OK
        assert a[0] == host.snapshot()[0]
        host.reset()
        return
    tool.reset()
    assert tool.at(m, poses.p, None) == OK, m.last_error()
    assert tool.snapshot() == a
    tool.reset()
