"""The top-layer peak kernels (k_nms_blocks, k_nms, k_nms_fast, k_nms_greedy and the form selection of launch_nms /
launch_top_greedy) on hand-made maps, through the operator fpm_op_peaks, against the oracle's orc_peak_sequence
(gfx950 required for the tests marked gpu; the properties of the oracle's own output run without a device).

Every comparison is exact: the count, every (x, y) and the score, np.float32(oracle value) == kernel score.  Entries
past the count are not compared.  Where a group is meant to reach one path the test asserts it from the operator's
stats (what the launchers decided, the lists' counts) and from the oracle's sequence, never from the kernel's result.
The operator needs no learned template: every test but the isolation test runs on a context without one.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from tests import oracle
from tests.test_oracle_blockmax import SHAPES, _map

QT, MFC, PLAIN = (1, 0), (1, 1), (0, 0)   # (by_block, mfc)
RULES = {"qt": QT, "mfc": MFC, "plain": PLAIN}
BLOCKS, NMS, FAST, GREEDY = L.PEAKS_RAN_BLOCKS, L.PEAKS_RAN_NMS, L.PEAKS_RAN_FAST, L.PEAKS_RAN_GREEDY
# the launchers' thresholds (fpm_kernels.hip), restated for the choice of inputs
GREEDY_MAX, CAND_CAP, LDS_BLOCKS_MAX, PLAIN_LIST = 4096, 8192, 12288, 512


def expect(m, tw, th, rule, overlap, cap, thr):
    return oracle.peak_sequence(m, tw, th, rule[0], rule[1], overlap, cap - 1, thr)


def same(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for k, (v, x, y) in enumerate(exp):
        assert (int(got["x"][k]), int(got["y"][k])) == (x, y), (what, k, got[k], exp[k])
        assert np.float32(v) == got["score"][k], (what, k, got[k], exp[k])


def run(mt, maps, tw, th, cap, rule, thr, overlap, form, list_cap=0, seed=1, what=""):
    """One call of the operator on `maps`; every job is compared with the oracle.  Returns (peaks, stats)."""
    got, st = mt.peaks(maps, tw, th, cap, rule[0], rule[1], thr, overlap, form, list_cap, seed)
    assert len(got) == len(maps) and (st["counts"] >= 0).all()   # (a count of -1: no kernel took the job)
    for i, m in enumerate(maps):
        exp = expect(m, tw, th, rule, overlap, cap, thr)
        same(got[i], exp, (what, "job", i, m.shape, tw, th, cap, rule, thr, overlap, form, list_cap))
        assert st["jobs"][i, 0] == int(np.count_nonzero(m.astype(np.float64) >= thr))
    return got, st


def forms_for(thr, cap=1):
    """form 1 (the list path) takes what the search's plan admits to it: thr > 0.01 and cap <= 256"""
    return (0, 1) if thr > 0.01 and cap <= 256 else (0,)


def greedy_admits(m, tw, th, rule):
    """k_nms_greedy's shape rule: the plain key, or a block grid with at least one whole block"""
    f = 2 if rule == MFC else 1
    return rule == PLAIN or (m.shape[1] >= f * tw and m.shape[0] >= f * th)


@pytest.fixture(scope="module")
def mt():
    from fastest_image_pattern_matching_amd import TemplateMatcher

    return TemplateMatcher(0)   # no template learned


# ---------------------------------------------------------------------------------------------------- group 1
def empty_strip_map():
    """test_mfc_empty_bottom_strip_is_reported_as_reference's map (24 x 12, tw = th = 3)"""
    m = np.full((12, 24), -0.5, np.float32)
    m[3, 4] = 0.9
    return m


@functools.lru_cache(maxsize=None)
def group1_maps(tw, th):
    """every SHAPES map of this template size: 3 seeds x levels (7, 1000), sizes differ within a call"""
    out = []
    for (w, h, tw_, th_) in SHAPES:
        if (tw_, th_) == (tw, th):
            out += [_map(w, h, seed * 31 + w * 7 + h, lv) for seed in range(3) for lv in (7, 1000)]
    if (tw, th) == (3, 3):
        out.append(empty_strip_map())
    return out


TEMPLATES = sorted({(tw, th) for (_, _, tw, th) in SHAPES})


def _cell_of(w, h, tw, th):
    """Qt s_BlockMax block of every pixel (grid, right strip, bottom strip; the corner counts as the right strip)"""
    ncol, nrow = w // tw, h // th
    ys, xs = np.mgrid[0:h, 0:w]
    b = (ys // th) * ncol + xs // tw
    b = np.where(xs >= ncol * tw, ncol * nrow, b)
    return np.where((ys >= nrow * th) & (xs < ncol * tw), ncol * nrow + 1, b)


def test_group1_maps_hold_cross_block_ties_and_rules_differ():
    """CPU: on the levels-7 maps the maximum is tied across s_BlockMax blocks, and for every shape some map's Qt and MFC
    sequences differ (first block against last block on ties)."""
    for (w, h, tw, th) in SHAPES:
        differ = False
        for seed in range(3):
            m = _map(w, h, seed * 31 + w * 7 + h, 7)
            cells = _cell_of(w, h, tw, th)[m == m.max()]
            assert len(set(cells.tolist())) >= 2, (w, h, tw, th, seed)
            for overlap, thr in itertools.product((0.0, 0.3), (0.25, -2.0)):
                differ |= expect(m, tw, th, QT, overlap, 13, thr) != expect(m, tw, th, MFC, overlap, 13, thr)
        assert differ, (w, h, tw, th)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
@pytest.mark.parametrize("tw,th", TEMPLATES)
def test_residue_layouts_ties_all_rules(mt, tw, th, rule):
    maps = group1_maps(tw, th)
    r = RULES[rule]
    for overlap, thr in itertools.product((0.0, 0.3), (0.25, -2.0)):
        for form in forms_for(thr):
            _, st = run(mt, maps, tw, th, 13, r, thr, overlap, form, what="group1")
            k = st["kernels"]
            if form == 1:   # short lists: the list form takes every map that holds a whole block of the rule's size
                assert k & GREEDY
                assert [bool(t) for t in st["jobs"][:, 2]] == [greedy_admits(m, tw, th, r) for m in maps]
            elif r == QT:
                # thr > 0: greedy takes every map (< 4096 pixels each) where the map holds a whole block; thr <= 0: k_nms
                assert k == (BLOCKS | GREEDY | FAST if thr > 0 else BLOCKS | NMS), (k, thr)
            elif r == MFC:
                whole = any(m.shape[1] >= 2 * tw and m.shape[0] >= 2 * th for m in maps)
                assert k == ((BLOCKS if whole else 0) | (GREEDY if thr > 0 and whole else 0) | NMS), (k, thr)
            else:
                assert k == NMS


# ---------------------------------------------------------------------------------------------------- group 2
def dense_map(w, h, k, seed, levels=50, lo=0.3):
    """w x h map with exactly k pixels >= 0.25 (coarse values in [lo, lo + 0.5): ties in the sort), the rest at -0.5"""
    rng = np.random.default_rng(seed)
    m = (lo + rng.integers(0, levels, size=w * h) / (2.0 * levels)).astype(np.float32)
    low = rng.permutation(w * h)[:w * h - k]
    m[low] = -0.5
    return m.reshape(h, w)


GREEDY_K = {0: (20, 17), 1: (20, 17), 63: (20, 17), 64: (20, 17), 65: (20, 17), 4095: (64, 64), 4096: (64, 64),
            4097: (65, 64)}


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(GREEDY_K))
def test_greedy_sort_capacity(mt, k):
    w, h = GREEDY_K[k]
    m = dense_map(w, h, k, 100 + k)
    assert int(np.count_nonzero(m >= 0.25)) == k
    for form in (0, 1):
        _, st = run(mt, [m], 8, 8, 30, QT, 0.25, 0.0, form, what="greedy capacity")
        assert st["jobs"][0, 0] == k
        assert st["kernels"] == BLOCKS | GREEDY | FAST and st["greedy_cap"] == GREEDY_MAX
        assert bool(st["jobs"][0, 2]) == (k <= GREEDY_MAX)
        if k > GREEDY_MAX:
            assert st["jobs"][0, 1] == k   # k_nms_blocks' own count of the pixels >= thr, left to k_nms_fast


@pytest.mark.gpu
@pytest.mark.parametrize("k", [64, 65])
def test_greedy_list_cap_64(mt, k):
    m = dense_map(20, 17, k, 200 + k)
    _, st = run(mt, [m], 8, 8, 30, QT, 0.25, 0.0, 1, list_cap=64, what="list cap 64")
    assert st["list_cap"] == 64 and st["greedy_cap"] == 64
    # (the fallback launch_nms has the full-size greedy form again, but its lists hold 64 entries too)
    assert bool(st["jobs"][0, 2]) == (k <= 64)
    assert st["kernels"] == BLOCKS | GREEDY | FAST


# ---------------------------------------------------------------------------------------------------- group 3
@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_list_overflow(mt, form):
    m = dense_map(96, 96, 96 * 96, 300)
    _, st = run(mt, [m], 8, 8, 30, QT, 0.25, 0.0, form, what="list overflow")
    assert st["jobs"][0, 0] == 96 * 96 > CAND_CAP == st["list_cap"]
    assert st["kernels"] == BLOCKS | GREEDY | FAST and not st["jobs"][0, 2]
    assert st["jobs"][0, 1] == 96 * 96   # the count runs past the capacity; k_nms_fast then reads the map


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_list_beyond_fast_lds_room(mt, form):
    """12100 blocks leave k_nms_fast's LDS room for ~1.6 K candidates: a list of 5000 (greedy declines above 4096) is
    within cand_cap but beyond cand_lds"""
    k = 5000
    m = dense_map(220, 220, k, 301)
    _, st = run(mt, [m], 2, 2, 30, QT, 0.25, 0.0, form, what="cand_lds")
    assert st["max_blocks"] == 12100 == st["lds_blocks"]
    assert 0 < st["cand_lds"] < GREEDY_MAX < k <= CAND_CAP
    assert st["kernels"] == BLOCKS | GREEDY | FAST and not st["jobs"][0, 2] and st["jobs"][0, 1] == k


@pytest.mark.gpu
@pytest.mark.parametrize("corner", [0, 1])
def test_list_fills_fast_lds_exactly_or_by_corner_repeats(mt, corner):
    """100 x 100 with 8 x 8 blocks: right strip, bottom strip and a 4 x 4 corner whose pixels k_nms_fast files twice.
    corner 0: exactly 8192 candidates, none in the corner (the list fits the LDS to the last entry); corner 1: 8185 with
    the corner's 16, so the list fits cand_cap but its 8201 LDS entries do not (the kernel reads the map instead)."""
    rng = np.random.default_rng(302 + corner)
    m = (0.3 + rng.integers(0, 50, size=(100, 100)) / 100.0).astype(np.float32)
    in_corner = np.zeros((100, 100), bool)
    in_corner[96:, 96:] = True
    k = 8185 if corner else 8192
    free = np.flatnonzero(~in_corner.ravel())
    n_low = 100 * 100 - k - (0 if corner else 16)
    m.ravel()[rng.permutation(free)[:n_low]] = -0.5
    if not corner:
        m[in_corner] = -0.5
    assert int(np.count_nonzero(m >= 0.25)) == k
    _, st = run(mt, [m], 8, 8, 30, QT, 0.25, 0.0, 0, what="fast lds exact")
    assert st["cand_lds"] == CAND_CAP and st["kernels"] == BLOCKS | GREEDY | FAST
    assert not st["jobs"][0, 2] and st["jobs"][0, 1] == k   # every pixel listed once: the corner block emits none


# ---------------------------------------------------------------------------------------------------- group 4
def sparse_map(w, h, npeaks, seed, levels=12):
    """background below 0.2, npeaks pixels on a coarse grid of values in [0.3, 1): ties among the peaks"""
    rng = np.random.default_rng(seed)
    m = (rng.random((h, w)) * 0.5 - 0.3).astype(np.float32)
    at = rng.permutation(w * h)[:npeaks]
    m.ravel()[at] = (0.3 + rng.integers(0, levels, size=npeaks) * 0.7 / levels).astype(np.float32)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("npeaks", [60, 4500])
@pytest.mark.parametrize("side,blocks", [(220, 12100), (224, 12544)])
def test_block_count_across_lds_limit(mt, side, blocks, npeaks):
    """60 peaks: a list the greedy form takes where it is launched; 4500: beyond its sort, left to k_nms_fast / k_nms"""
    m = sparse_map(side, side, npeaks, 400 + side)
    assert (blocks <= LDS_BLOCKS_MAX) == (side == 220)
    # (224: 12544 coverage cells, more than the list form's plan admits)
    for form in ((0, 1) if side == 220 else (0,)):
        _, st = run(mt, [m], 2, 2, 20, QT, 0.25, 0.0, form, what="block count")
        assert st["max_blocks"] == blocks and st["jobs"][0, 0] == npeaks
        if side == 220:
            assert st["kernels"] == BLOCKS | GREEDY | FAST and st["lds_blocks"] == blocks
            assert bool(st["jobs"][0, 2]) == (npeaks <= GREEDY_MAX)
        else:
            assert st["kernels"] == BLOCKS | NMS and st["lds_blocks"] == 0   # k_nms, block maxima in global scratch


# ---------------------------------------------------------------------------------------------------- group 5
def cell_map(rule):
    rng = np.random.default_rng(500)
    w, h = (32, 32) if rule != "plain" else (32, 16)   # (the plain lists hold 512 entries)
    return (0.3 + rng.permutation(w * h) * (0.69 / (w * h))).astype(np.float32).reshape(h, w)


@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
def test_cell_map_fills_a_cell_beyond_its_id_list(rule):
    """CPU: with overlap 0.75 the painted rectangle is 4 x 4, and some 8 x 8 cell holds at least 7 of the oracle's peaks
    (k_nms_greedy lists 6 rectangles per cell before it scans all taken ones)"""
    m = cell_map(rule)
    assert len(np.unique(m)) == m.size and m.min() >= 0.25
    seq = expect(m, 8, 8, RULES[rule], 0.75, 200, 0.25)
    per_cell = np.zeros((m.shape[0] // 8, m.shape[1] // 8), int)
    for _, x, y in seq:
        per_cell[y // 8, x // 8] += 1
    assert per_cell.max() >= 7, per_cell


@pytest.mark.gpu
@pytest.mark.parametrize("rule,form", [("qt", 0), ("qt", 1), ("mfc", 0), ("mfc", 1), ("plain", 1)])
def test_more_rectangles_in_a_cell_than_its_id_list(mt, rule, form):
    _, st = run(mt, [cell_map(rule)], 8, 8, 200, RULES[rule], 0.25, 0.75, form, what="cell ids")
    assert st["kernels"] & GREEDY and st["jobs"][0, 2]


# ---------------------------------------------------------------------------------------------------- group 6
PEAK_CAP_MAPS = {"dense": lambda: dense_map(80, 80, 80 * 80, 600, levels=400),   # 6400 > 4096: greedy declines
                 "listed": lambda: dense_map(80, 80, 4000, 601, levels=400)}     # greedy takes it


@pytest.mark.parametrize("kind", sorted(PEAK_CAP_MAPS))
def test_peak_capacity_maps_fill_the_capacity(kind):
    """CPU: the oracle finds at least 257 peaks on the capacity maps"""
    m = PEAK_CAP_MAPS[kind]()
    for cap in (256, 257):
        assert len(expect(m, 2, 2, QT, 0.0, cap, 0.25)) == cap


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(PEAK_CAP_MAPS))
@pytest.mark.parametrize("cap", [256, 257])
def test_peak_capacity(mt, kind, cap):
    m = PEAK_CAP_MAPS[kind]()
    for form in forms_for(0.25, cap):
        _, st = run(mt, [m], 2, 2, cap, QT, 0.25, 0.0, form, what="peak capacity")
        if cap == 256:
            assert st["kernels"] == BLOCKS | GREEDY | FAST
            assert bool(st["jobs"][0, 2]) == (kind == "listed")
        else:
            assert st["kernels"] == BLOCKS | NMS and not st["jobs"][0, 2]   # cap > 256: k_nms


# ---------------------------------------------------------------------------------------------------- group 7
@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
def test_empty_painted_rectangle(mt, rule):
    """overlap 1.0 (and 0.999 on a 3 x 3 template: int(6 * 0.001) = 0): nothing is painted, the reference finds the same
    peak with every call"""
    r = RULES[rule]
    m = _map(25, 19, 71, 7)
    for tw, th, overlap in ((4, 3, 1.0), (3, 3, 0.999)):
        exp = expect(m, tw, th, r, overlap, 9, 0.25)
        assert len(exp) == 9 and len(set(exp)) == 1
        for form in (0, 1):
            _, st = run(mt, [m], tw, th, 9, r, 0.25, overlap, form, what="empty rectangle")
            assert not st["jobs"][0, 2]   # the greedy forms leave such a map to k_nms_fast / k_nms
            assert st["kernels"] & (NMS if r != QT else FAST)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
@pytest.mark.parametrize("thr", [0.0, -1.0, -2.0])
def test_thresholds_at_and_below_zero(mt, rule, thr):
    r = RULES[rule]
    maps = [_map(25, 19, 72, 7), _map(24, 12, 73, 1000), empty_strip_map()]
    for overlap in (0.0, 0.3):
        _, st = run(mt, maps, 4, 3, 13, r, thr, overlap, 0, what="thr <= 0")
        assert st["kernels"] == (NMS if r == PLAIN else BLOCKS | NMS)   # thr <= 0: no greedy form, no k_nms_fast


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
def test_maps_without_a_whole_block(mt, rule):
    """a map narrower than the template, one lower than it, and 1 x 1: Qt keeps strips (one of them empty, 0 at
    (-1, -1) of its origin), MFC has no blocks at all and scans the map"""
    r = RULES[rule]
    for shape in ((10, 3), (2, 10), (1, 1)):   # (h, w) against tw = 4, th = 3
        m = _map(shape[1], shape[0], 74 + shape[0], 7)
        m.ravel()[0] = 0.5
        for thr in (0.25, -2.0):
            for form in forms_for(thr):
                _, st = run(mt, [m], 4, 3, 6, r, thr, 0.0, form, what="no whole block")
                if r == MFC:
                    assert st["max_blocks"] == 0 and not st["kernels"] & BLOCKS


# regression: MaxOverlap < 0.  The painted rectangle, int(2 tw (1 - overlap)), is then wider than two templates and
# covers more than the 3 x 3 cells k_nms_greedy files a taken rectangle in: a later candidate in a covered cell beyond
# them was never tested against it and became an extra peak.  launch_nms launched the greedy form for MFC maps
# whatever the overlap, and plan_top_mma sent such searches to the list path; both now keep them on k_nms.
def negative_overlap_map():
    rng = np.random.default_rng(700)
    return (0.3 + rng.integers(0, 60, size=(32, 40)) / 100.0).astype(np.float32)   # every pixel >= thr, many ties


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
@pytest.mark.parametrize("overlap", [-0.5, -1.0])
def test_negative_overlap_runs_k_nms(mt, rule, overlap):
    r = RULES[rule]
    m = negative_overlap_map()
    assert int(2 * 4 * (1 - overlap)) > 2 * 4 and len(expect(m, 4, 3, r, overlap, 30, 0.25)) >= 4
    _, st = run(mt, [m, _map(25, 19, 701, 7)], 4, 3, 30, r, 0.25, overlap, 0, what="negative overlap")
    assert st["kernels"] == (NMS if r == PLAIN else BLOCKS | NMS) and not st["jobs"][:, 2].any()


@pytest.mark.gpu
@pytest.mark.parametrize("rule,t,overlap", [("qt", 2, -8.0), ("mfc", 1, -16.0)])
def test_negative_overlap_rectangle_over_more_than_256_blocks(mt, rule, t, overlap):
    """2 x 2 blocks in both layouts; Qt: a 36 x 36 rectangle meets 18 x 18 blocks, MFC: 34 x 34 meets 17 x 17 -- beyond
    k_nms's list of 256 affected blocks (its one-block-per-thread re-scan)"""
    m = sparse_map(80, 80, 300, 702)
    assert (int(2 * t * (1 - overlap)) // 2) ** 2 > 256
    assert len(expect(m, t, t, RULES[rule], overlap, 12, 0.25)) >= 4
    _, st = run(mt, [m], t, t, 12, RULES[rule], 0.25, overlap, 0, what="rectangle over > 256 blocks")
    assert st["kernels"] == BLOCKS | NMS


@pytest.mark.gpu
@pytest.mark.parametrize("semantics", [0, 1])
@pytest.mark.parametrize("case,overlap", [("dst4_overlap", -0.5), ("dst4_block", -0.3)])
def test_search_with_negative_overlap(gpu_matcher_factory, templates, case, overlap, semantics):
    """whole searches with MaxOverlap < 0, Qt and MFC semantics (thr > 0: the list path and the MFC greedy form would
    have taken them): results, live counts and candidate records equal the oracle's"""
    from tests import cases

    build, prm = cases.CASES[case]
    s, t = build(templates)
    prm = dict(prm, max_overlap=overlap, semantics=semantics)
    o = oracle.OracleMatcher()
    hip = gpu_matcher_factory()
    gpu, orc, ostats, gstats = cases._run_both(hip, s, t, oracle_matcher=o, **prm)
    assert gstats == ostats and [r.as_tuple() for r in gpu] == orc
    assert hip.last_candidates(0).tobytes() == o.candidates().tobytes()
    assert len(orc) >= 1


# ---------------------------------------------------------------------------------------------------- group 8
@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
def test_threshold_equal_as_float_not_as_double(mt, rule):
    """thr = 0.7 (double): float32(0.7) = 0.699999988 is below it, the next float above is not"""
    lo = np.float32(0.7)
    hi = np.nextafter(lo, np.float32(1))
    assert float(lo) < 0.7 <= float(hi)
    rng = np.random.default_rng(800)
    m = np.full((20, 20), 0.1, np.float32)
    at = rng.permutation(400)[:24]
    m.ravel()[at[:12]] = lo
    m.ravel()[at[12:]] = hi
    exp = expect(m, 4, 4, RULES[rule], 0.5, 30, 0.7)
    assert 1 <= len(exp) <= 12 and all(np.float32(v) == hi for v, _, _ in exp)
    for form in (0, 1):
        _, st = run(mt, [m], 4, 4, 30, RULES[rule], 0.7, 0.5, form, what="thr 0.7")
        assert st["jobs"][0, 0] == 12   # the lists hold the upper neighbours only


def zero_tie_map():
    """13 x 50 against 4 x 4 blocks: a 1 x 50 right strip in 4 chunks, a 12 x 2 bottom strip in 2.  -0.0 and +0.0 (equal
    as floats) tied inside a block, across two blocks and across the first and the last chunk of the right strip"""
    m = np.full((50, 13), -0.9, np.float32)
    m[1, 1], m[2, 2] = -0.0, 0.0        # one block
    m[9, 5], m[9, 9] = 0.0, -0.0        # two blocks of one row
    m[2, 12], m[47, 12] = -0.0, 0.0     # the right strip's first and last chunk
    m[49, 3] = -0.0                     # the bottom strip
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
def test_signed_zero_ties(mt, rule):
    m = zero_tie_map()
    tw = 4 if rule != "mfc" else 2   # MFC blocks are twice the template
    exp = expect(m, tw, tw, RULES[rule], 0.5, 12, -0.5)
    assert len(exp) >= 4 and all(v == 0.0 for v, _, _ in exp)
    run(mt, [m], tw, tw, 12, RULES[rule], -0.5, 0.5, 0, what="signed zeros")


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
def test_values_above_one(mt, rule):
    rng = np.random.default_rng(801)
    m = (rng.integers(0, 9, size=(19, 25)) * 0.5 - 0.5).astype(np.float32)   # -0.5 .. 3.5 in steps of 0.5
    for form in (0, 1):
        run(mt, [m], 4, 3, 13, RULES[rule], 0.25, 0.3, form, what="values above 1")


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
def test_native_minus_one_against_painted(mt, rule):
    """thr -2.0: pixels that are -1.0 from the start tie with painted ones"""
    rng = np.random.default_rng(802)
    m = np.where(rng.random((13, 17)) < 0.6, -1.0, rng.integers(0, 4, size=(13, 17)) * 0.25).astype(np.float32)
    exp = expect(m, 4, 3, RULES[rule], 0.0, 40, -2.0)
    assert any(v == -1.0 for v, _, _ in exp)
    run(mt, [m], 4, 3, 40, RULES[rule], -2.0, 0.0, 0, what="native -1")


# ---------------------------------------------------------------------------------------------------- group 9
def strip_chunks(w, h, bw, bh):
    """BlockGeom::chunks of the right and the bottom strip (block size bw x bh): ceil(strip area / block area)"""
    ncol, nrow = w // bw, h // bh
    right, bottom = (w - ncol * bw) * h, ncol * bw * (h - nrow * bh)
    return -(-right // (bw * bh)), -(-bottom // (bw * bh))


def strip_map(top):
    """50 x 51 against 4 x 4 blocks: a 2 x 51 right strip (7 chunks) and a 48 x 3 bottom strip (9 chunks), each strip's
    maximum present twice, in its first and in its last chunk.  top: the strips' maximum is the map's"""
    rng = np.random.default_rng(900)
    m = (rng.integers(0, 20, size=(51, 50)) * 0.02 + 0.3).astype(np.float32)   # 0.30 .. 0.68
    m[:, 48:] = np.minimum(m[:, 48:], np.float32(0.5))
    m[48:, :] = np.minimum(m[48:, :], np.float32(0.5))
    v = np.float32(0.9 if top else 0.6)
    m[3, 49], m[50, 48] = v, v           # right strip: elements 7 and 100 of 102 (chunks of 16: the first and the last)
    m[48, 5], m[50, 40] = v, v           # bottom strip: elements 5 and 136 of 144
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc"])
@pytest.mark.parametrize("top", [0, 1])
def test_strips_scanned_in_chunks(mt, rule, top):
    t = 4 if rule == "qt" else 2   # 4 x 4 blocks in both layouts
    assert min(strip_chunks(50, 51, 4, 4)) >= 3
    m = strip_map(top)
    r = RULES[rule]
    # the block maxima reach the result in k_nms (thr <= 0, or more than 256 peak slots) and in k_nms_fast (here: an empty
    # painted rectangle, which the greedy form declines); the greedy form orders the same pixels from its list
    for cap, thr, overlap in ((12, 0.25, 0.0), (12, -2.0, 0.0), (257, 0.25, 0.0), (5, 0.25, 1.0)):
        for form in forms_for(thr, cap):
            _, st = run(mt, [m], t, t, cap, r, thr, overlap, form, what="strip chunks")
            if form == 0 and (thr <= 0 or cap > 256):
                assert st["kernels"] == BLOCKS | NMS
            if form == 0 and overlap == 1.0 and r == QT:
                assert st["kernels"] & FAST and not st["jobs"][0, 2]
    if top:
        v, x, y = expect(m, t, t, r, 1.0, 5, 0.25)[0]
        assert np.float32(v) == np.float32(0.9) and (x >= 48 or y >= 48)   # the map's maximum lies in a strip


# --------------------------------------------------------------------------------------------------- group 10
PLAIN_SHAPES = [(60, 50, 0), (131, 77, 1), (512, 512, 1), (513, 512, 2)]   # (w, h, k_nms's plain form at cap 15)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,plain_form", PLAIN_SHAPES)
def test_plain_path_forms(mt, w, h, plain_form):
    """cap x pixels below 65536: full scans; from there on 64-pixel block maxima in LDS (131 x 77 ends in a partial
    block; 512 x 512 fills the 4096 blocks); 513 x 512 is beyond them: full scans.  Coarse levels: first in row-major"""
    px = w * h
    assert plain_form == (0 if 15 * px < 65536 else 1 if (px + 63) // 64 <= 4096 else 2)
    m = _map(w, h, 1000 + w, 9)
    m[-1, -1] = 0.95   # the map's only maximum is its last pixel (131 x 77: the last of the partial block's 39)
    assert expect(m, 12, 9, PLAIN, 0.0, 15, 0.25)[0][1:] == (w - 1, h - 1)
    for overlap in (0.0, 0.6):
        _, st = run(mt, [m], 12, 9, 15, PLAIN, 0.25, overlap, 0, what="plain forms")
        assert st["kernels"] == NMS and st["jobs"][0, 3] == plain_form
        assert st["blk_lds"] == (1 if 15 * px >= 65536 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [PLAIN_LIST, PLAIN_LIST + 1])
def test_plain_lists_at_capacity(mt, k):
    m = dense_map(60, 50, k, 1100 + k, levels=9)
    for overlap in (0.0, 0.6):
        _, st = run(mt, [m], 12, 9, 15, PLAIN, 0.25, overlap, 1, what="plain list capacity")
        assert st["list_cap"] == PLAIN_LIST and st["jobs"][0, 0] == k
        assert bool(st["jobs"][0, 2]) == (k <= PLAIN_LIST)
        assert st["kernels"] == GREEDY | NMS   # the fallback k_nms skips a taken map


# --------------------------------------------------------------------------------------------------- group 11
@functools.lru_cache(maxsize=None)
def many_maps():
    """300 jobs: group 1's maps of every template size (73 maps of 13 sizes), repeated; returns (maps, source index)"""
    src = [m for (tw, th) in TEMPLATES for m in group1_maps(tw, th)]
    idx = [i % len(src) for i in range(300)]
    return [src[i] for i in idx], idx, len(src)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["qt", "mfc", "plain"])
@pytest.mark.parametrize("form", [0, 1])
def test_many_jobs(mt, rule, form):
    """more workgroups than CUs in one call (against a 4 x 3 template); every one of the 300 jobs equals the oracle and
    the single-job call on its map"""
    maps, idx, nsrc = many_maps()
    r = RULES[rule]
    got, _ = run(mt, maps, 4, 3, 13, r, 0.25, 0.3, form, seed=7, what="many jobs")
    single = [mt.peaks([maps[i]], 4, 3, 13, r[0], r[1], 0.25, 0.3, form, 0, 7)[0][0] for i in range(nsrc)]
    for i in range(300):
        assert single[idx[i]].tobytes() == got[i].tobytes(), i


@pytest.mark.gpu
def test_list_order_does_not_matter(mt):
    maps = group1_maps(4, 3)
    a, _ = mt.peaks(maps, 4, 3, 13, 1, 0, 0.25, 0.3, 1, 0, 1)
    b, _ = mt.peaks(maps, 4, 3, 13, 1, 0, 0.25, 0.3, 1, 0, 99)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# --------------------------------------------------------------------------------------------------- group 12
@pytest.mark.gpu
def test_isolation_between_staged_searches(gpu_matcher_factory, templates):
    from tests import cases

    build, prm = cases.CASES["dst10_multi"]
    s, t = build(templates)
    m = gpu_matcher_factory(**prm)
    o = oracle.OracleMatcher().set(**prm)
    assert m.learnPattern(t) and o.learnPattern(t)
    exp = o.match(s)
    m.stage([s, s])
    first = m.match_staged()
    cand = [m.last_candidates(k).tobytes() for k in range(2)]
    for rule, form in (("qt", 0), ("mfc", 0), ("plain", 0), ("qt", 1), ("plain", 1)):
        run(m, group1_maps(4, 3), 4, 3, 13, RULES[rule], 0.25, 0.3, form, what="between searches")
    assert [m.last_candidates(k).tobytes() for k in range(2)] == cand
    second = m.match_staged()
    for res in (first, second):
        for k in range(2):
            assert [r.as_tuple() for r in res[k]] == exp
    assert [m.last_candidates(k).tobytes() for k in range(2)] == cand


def _raw(mt, maps, mw=None, mh=None, n=None, tw=4, th=3, cap=13, by_block=1, mfc=0, thr=0.25, overlap=0.0, form=0,
         list_cap=0, null=()):
    FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    ptrs = (FP * len(maps))(*[m.ctypes.data_as(FP) for m in maps])
    w = np.array([m.shape[1] for m in maps] if mw is None else mw, np.int32)
    h = np.array([m.shape[0] for m in maps] if mh is None else mh, np.int32)
    pk = np.zeros((len(maps), max(cap, 1)), [("x", "<i4"), ("y", "<i4"), ("score", "<f4")])
    cnt = np.full(len(maps), -7, np.int32)
    a = dict(maps=ptrs, mw=w.ctypes.data_as(IP), mh=h.ctypes.data_as(IP), peaks=pk.ctypes.data_as(C.POINTER(L.Peak)),
             counts=cnt.ctypes.data_as(IP))
    for k in null:
        a[k] = None
    rc = mt._lib.fpm_op_peaks(mt._ctx, a["maps"], a["mw"], a["mh"], len(maps) if n is None else n, tw, th, cap, by_block,
                              mfc, thr, overlap, form, list_cap, 0, a["peaks"], a["counts"], None)
    return rc, cnt


@pytest.mark.gpu
def test_argument_checks(mt):
    maps = [_map(24, 18, 1, 7), _map(25, 19, 2, 7)]
    rc, cnt = _raw(mt, maps)
    assert rc == L.FPM_OK and (cnt >= 0).all()
    bad = [dict(n=0), dict(n=-1), dict(mw=[0, 25]), dict(mw=[24, 65536]), dict(mh=[18, 0]), dict(mh=[65536, 19]),
           dict(tw=0), dict(th=0), dict(cap=0), dict(form=2), dict(form=-1), dict(null=("maps",)), dict(null=("mw",)),
           dict(null=("mh",)), dict(null=("peaks",)), dict(null=("counts",)), dict(list_cap=-1), dict(overlap=17.0),
           dict(overlap=float("inf")), dict(overlap=float("nan")), dict(thr=float("nan")),
           dict(mw=[40000, 25], mh=[40000, 19]),                  # beyond FPM_PEAKS_MAX_PIXELS, before any map is read
           dict(form=1, thr=0.0), dict(form=1, cap=257), dict(form=1, overlap=-0.5)]          # what the list form does not take
    for kw in bad:
        rc, cnt = _raw(mt, maps, **kw)
        assert rc == L.FPM_E_INVALID_ARG, kw
        assert (cnt == -7).all(), kw
    assert mt._lib.fpm_op_peaks(None, None, None, None, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 0, None, None, None) == \
        L.FPM_E_INVALID_ARG
    rc, cnt = _raw(mt, maps)   # the context still works
    assert rc == L.FPM_OK and (cnt >= 0).all()
