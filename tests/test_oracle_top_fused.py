"""What tests/test_gpu_top_fused.py relies on, checked on the CPU with the oracle alone: the cases cut the paths they are
chosen for (template and map widths modulo the kernel's 4-pixel words, LDS sizes either side of the limit, skipped
angles, exact ties, peak lists that end at cap and at the threshold, rectangles clipped at every map edge, the rectangle
that misses its own peak), and peak_sequence on the oracle's kept maps gives the top-layer candidates of the oracle's
own search.  CPU only.
"""
import numpy as np
import pytest

from tests import oracle
from tests import top_fused_cases as F
from tests.top_map_cases import case


@pytest.mark.parametrize("cid", sorted(F.MAP_CASES))
def test_map_case_facts(cid):
    """Angles, the largest job's LDS (top_fused_lds restated) and the map widths' residues modulo 4, per case."""
    kind, top, w, h = F.MAP_CASES[cid]
    nang, (lo, hi), residues = F.MAP_FACTS[cid.split("-", 1)[1]]
    c = F.get(cid)
    assert c[4] == nang and len(c[3]) == nang          # every angle scored
    assert lo * 1024 <= F.case_lds(c, top) < hi * 1024, F.case_lds(c, top)
    assert F.case_lds(c, top) <= 65536 - F.STATIC_LDS_MAX
    assert {m.shape[1] % 4 for _, _, _, m in c[3]} == residues
    for _, bw, bh, m in c[3]:
        assert m.shape == (bh - top[1] + 1, bw - top[0] + 1)
    if kind == "saturated":   # exact ties and flat-window zeros
        ties = sum(m.size - len(np.unique(m)) for _, _, _, m in c[3])
        zeros = sum(int((m == 0).sum()) for _, _, _, m in c[3])
        assert ties >= 500 and zeros >= 1000, (ties, zeros)


def test_template_widths_cover_the_word_residues():
    """tw % 4 = 0, 2, 0, 1, 3 for the five small shapes, a template narrower than one word, and 15 whole words."""
    tops = sorted({v[1] for v in F.MAP_CASES.values()})
    assert {tw % 4 for tw, _ in tops} == {0, 1, 2, 3}
    assert (3, 30) in tops and (60, 60) in tops
    assert min(m.shape for _, _, _, m in F.get("noise-60x60")[3]) <= (7, 7)   # maps down to a few pixels


def test_limit_cases():
    """200 x 140 lies below any plausible LDS limit of the kernel, 220 x 150 above 64 KB less any static LDS at all."""
    kind, top, w, h = F.OVER_LIMIT
    assert F.case_lds(case(kind, top, 0, w, h), top) > 65536 - 256
    assert F.case_lds(F.get("noise-12x9-near-limit"), top) < 65536 - F.STATIC_LDS_MAX


def test_narrow_source_skips_angles():
    kind, top, w, h = F.NARROW
    c = case(kind, top, 0, w, h)
    kept = {k for k, _, _, _ in c[3]}
    assert c[4] == 137 and 0 < len(kept) < c[4]
    assert 0 in kept and min(set(range(c[4])) - kept) > 0       # skipped jobs lie between scored ones
    assert any(k - 1 in kept and k + 1 not in kept for k in kept) and any(k + 1 in kept and k - 1 not in kept for k in kept)


def test_dense_cases():
    """cap 135 > kNmsInitCap, a rectangle of at least 3 x 3 that covers its peak, no position twice; over the cases
    jobs that end at cap and jobs that end at the threshold, and saturated jobs that take equal values in a row."""
    prm = F.DENSE
    cap = prm["max_pos"] + F.MATCH_CANDIDATE_NUM
    assert cap > F.K_NMS_INIT_CAP
    at_cap = at_thr = tie_jobs = 0
    for cid in F.DENSE_CASES:
        kind, top, w, h = F.MAP_CASES[cid]
        x0, y0, rw, rh = F.rect(50, 40, top, prm["max_overlap"])
        assert rw >= 3 and rh >= 3 and x0 <= 50 < x0 + rw and y0 <= 40 < y0 + rh
        for (_, _, _, m), seq in zip(F.get(cid)[3], F.expected_peaks(kind, top, 0, w, h, prm)):
            assert 1 <= len(seq) <= cap
            assert len({(x, y) for _, x, y in seq}) == len(seq), cid
            assert float(m.min()) > F.layer_score(prm) > -1.0
            at_cap += len(seq) == cap
            at_thr += len(seq) < cap
            if kind == "saturated":
                tie_jobs += any(a[0] == b[0] for a, b in zip(seq, seq[1:]))
    assert at_cap >= 50 and at_thr >= 50 and tie_jobs >= 10, (at_cap, at_thr, tie_jobs)


@pytest.mark.parametrize("ov", [0.0, -0.5])
def test_overlap_rectangles_are_clipped_at_every_edge(ov):
    """MaxOverlap 0 (twice the template) and -0.5 (three times): over the case's jobs a rectangle leaves the map on
    each of the four sides."""
    kind, top, w, h = F.MAP_CASES["noise-12x9"]
    prm = dict(max_pos=30, score=-1.0, max_overlap=ov)
    sides = set()
    for (_, _, _, m), seq in zip(F.get("noise-12x9")[3], F.expected_peaks(kind, top, 0, w, h, prm)):
        assert len(seq) >= 2
        for _, x, y in seq:
            x0, y0, rw, rh = F.rect(x, y, top, ov)
            assert (rw, rh) == (int(2 * top[0] * (1 - ov)), int(2 * top[1] * (1 - ov)))
            sides |= {s for s, out in (("l", x0 < 0), ("t", y0 < 0), ("r", x0 + rw > m.shape[1]),
                                       ("b", y0 + rh > m.shape[0])) if out}
    assert sides == {"l", "t", "r", "b"}


def test_fuzz24_rectangle_misses_its_peak():
    s, t, prm, maps, nang, o = F.fuzz24()
    top = (14, 5)
    x0, y0, rw, rh = F.rect(20, 10, top, prm["max_overlap"])
    assert (rw, rh) == (5, 1) and y0 == 9                       # one row, above the peak
    cap = prm["max_pos"] + F.MATCH_CANDIDATE_NUM
    seqs = F.peak_lists((s, t, prm, maps, nang, o), top, prm, levels=4)
    assert len(maps) == nang == 5
    assert all(len(q) == cap and len({(x, y) for _, x, y in q}) == 1 for q in seqs)   # the same peak up to cap


def test_constant_inputs():
    kind, top, w, h = F.MAP_CASES["noise-12x9"]
    c = case("constant_template", top, 0, w, h)
    assert all(np.all(m == np.float32(1.0)) for _, _, _, m in c[3])
    for (_, _, _, m), seq in zip(c[3], F.peak_lists(c, top, c[2])):
        idx = [y * m.shape[1] + x for _, x, y in seq]
        assert len(seq) == c[2]["max_pos"] + F.MATCH_CANDIDATE_NUM and idx[0] == 0 and idx == sorted(set(idx))
    c = case("constant_source", top, 0, w, h)
    assert sum(int((m == 0).sum()) for _, _, _, m in c[3]) >= 10000       # flat windows score exactly 0


@pytest.mark.parametrize("cid", ["noise-12x9", "noise-3x30", "noise-17x15"])
def test_peak_sequences_are_the_search_candidates(cid):
    """The top-layer candidates of the oracle's own search, angle by angle, are peak_sequence on the kept maps."""
    kind, top, w, h = F.MAP_CASES[cid]
    s, t, prm, maps, nang, o = F.get(cid)
    lvl = oracle.pyr_down(s)
    cx, cy = np.float32((lvl.shape[1] - 1) / 2.0), np.float32((lvl.shape[0] - 1) / 2.0)
    exp = []
    for (k, bw, bh, m), seq in zip(maps, F.peak_lists((s, t, prm, maps, nang, o), top, prm)):
        tx, ty = np.float32((bw - 1) / 2.0) - cx, np.float32((bh - 1) / 2.0) - cy   # the canvas translation
        exp += [(float(np.float32(x) - tx), float(np.float32(y) - ty), v) for v, x, y in seq]
    got = [(x, y, sc) for x, y, sc, _ in o.top_candidates()]
    assert got == exp and len(exp) == o.stats()[1] == len(o.candidates()) and len(exp) >= 1
    ranks = [(k, r, v) for (k, _, _, _), seq in zip(maps, F.peak_lists((s, t, prm, maps, nang, o), top, prm))
             for r, (v, _, _) in enumerate(seq)]
    assert [(int(c["angle_index"]), int(c["peak_rank"]), float(c["top_score"])) for c in o.candidates()] == ranks


def test_search_scenes_have_the_layers_they_are_for():
    for top in ((12, 9), (17, 15)):
        for layers in (0, 1, 2):
            s, t, prm = F.search_scene(top, layers)
            o = oracle.OracleMatcher().set(**prm)
            assert o.learnPattern(t)
            lv, _ = o.template_levels()
            assert len(lv) == layers + 1 and lv[layers][0].shape == (top[1], top[0]), (top, layers)
            o.match(s)
            st = o.stats()
            assert st[1] >= 1 and len(st) == 2 + layers, (top, layers, st)
