"""Cases and oracle expectations shared by tests/test_oracle_top_fused.py (CPU: the properties the cases are chosen for)
and tests/test_gpu_top_fused.py (k_top_fused against them).  Everything expected comes from the oracle: the kept
top-layer maps (tests/top_map_cases.case) and oracle.peak_sequence on each of them.
"""
import functools

import numpy as np

from fastest_image_pattern_matching_amd import synth
from tests import oracle
from tests.top_map_cases import case

MATCH_CANDIDATE_NUM = 5
K_NMS_INIT_CAP = 128          # kNmsInitCap: the peak list k_top_fused keeps in LDS for the fused candidate init
STATIC_LDS_MAX = 8192         # the kernel's static LDS lies well below this; the exact value comes from the stats

# id -> (kind, top, w, h): the smallest sources that still cut every path of the kernel (see test_gpu_top_fused.py)
SMALL = (180, 120)
MAP_CASES = {f"{kind}-{top[0]}x{top[1]}": (kind, top) + SMALL
             for top in [(16, 16), (14, 14), (12, 9), (17, 15), (43, 6)] for kind in ("noise", "saturated")}
MAP_CASES["noise-3x30"] = ("noise", (3, 30), 150, 130)
MAP_CASES["noise-60x60"] = ("noise", (60, 60), 176, 150)
MAP_CASES["noise-12x9-near-limit"] = ("noise", (12, 9), 200, 140)
# id -> (angles, (least, most) KB of the largest job's LDS, the map widths' residues mod 4)
MAP_FACTS = {"16x16": (53, (32, 33), {1, 3}), "14x14": (47, (34, 35), {1, 3}), "12x9": (41, (39, 40), {1, 3}),
             "17x15": (55, (32, 33), {0, 2}), "43x6": (137, (21, 22), {0, 2}), "3x30": (97, (25, 26), {0, 1, 2}),
             "60x60": (191, (30, 31), {0, 1, 2, 3}), "12x9-near-limit": (41, (52, 53), {1, 3})}
OVER_LIMIT = ("noise", (12, 9), 220, 150)      # one size on: 64.2 KB, above 64 KB - static LDS
NARROW = ("noise", (43, 6), 200, 40)           # top level 100 x 20: the angles around +-90 degrees have no map
# the dense-peak cases: MaxPos 130 (cap 135 > kNmsInitCap), score -1 (layer score -0.9, below every map value and
# above the painted -1), MaxOverlap 0.8
DENSE = dict(max_pos=130, score=-1.0, max_overlap=0.8)
DENSE_CASES = ["saturated-16x16", "saturated-12x9", "noise-12x9", "noise-17x15", "noise-60x60"]


def get(cid):
    kind, top, w, h = MAP_CASES[cid]
    return case(kind, top, 0, w, h)


def top_fused_lds(bw, bh, tw, th):
    """top_fused_lds (fpm_kernels.hip) restated: canvas words (+1 per row for the funnel read), map, template words,
    masks and the four warp tables, in bytes."""
    cpw, ntw = ((bw + 3) >> 2) + 1, (tw + 3) >> 2
    return 4 * (bh * cpw + max(bw - tw + 1, 0) * max(bh - th + 1, 0) + th * ntw + ntw + 2 * (bw + bh))


def case_lds(c, top):
    """The largest job's LDS over every angle of a case, scored or skipped (geometry from the oracle's kept maps)."""
    return max(top_fused_lds(bw, bh, *top) for _, bw, bh, _ in c[3])


def layer_score(prm, levels=2):
    v = prm["score"]
    for _ in range(levels - 1):
        v = v * 0.9
    return v


def peak_lists(c, top, prm, levels=2):
    """Per kept map of the case, the oracle's peak sequence [(value, x, y)] at the parameters' cap, overlap and layer score."""
    cap = prm["max_pos"] + MATCH_CANDIDATE_NUM
    thr = layer_score(prm, levels)
    return [oracle.peak_sequence(m, top[0], top[1], False, False, prm["max_overlap"], cap - 1, thr)
            for _, _, _, m in c[3]]


@functools.lru_cache(maxsize=None)
def _cached_peaks(key, top, max_pos, score, max_overlap):
    kind, seed, w, h = key
    return peak_lists(case(kind, top, seed, w, h), top, dict(max_pos=max_pos, score=score, max_overlap=max_overlap))


def expected_peaks(kind, top, seed, w, h, prm):
    return _cached_peaks((kind, seed, w, h), top, prm["max_pos"], prm["score"], prm["max_overlap"])


def rect(px, py, top, ov):
    """getNextMaxLoc's painted rectangle around a peak, unclipped: (x0, y0, w, h)."""
    tw, th = top
    return int(px - tw * (1 - ov)), int(py - th * (1 - ov)), int(2 * tw * (1 - ov)), int(2 * th * (1 - ov))


@functools.lru_cache(maxsize=None)
def fuzz24():
    """The 14 x 5 top level (three pyramid layers) of tests/test_gpu_fuzz._case(24): MaxOverlap 0.8 gives a 5 x 1
    rectangle one row above its peak, so the loop returns the same peak until cap.  A case tuple as top_map_cases.case."""
    from tests.test_gpu_fuzz import _case

    s, t, prm = _case(24)
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    o.set_keep_maps()
    o.match(s)
    maps = o.top_maps()
    levels, _ = o.template_levels()
    assert len(levels) == 4 and levels[3][0].shape == (5, 14)
    for _, _, _, m in maps:
        m.setflags(write=False)
    return s, t, prm, maps, o.stats()[0], o


@functools.lru_cache(maxsize=None)
def search_scene(top, layers):
    """(source, template, params) of a whole search whose top template level is `top` after `layers` pyramid steps
    (0: MinReduceArea above the template's area), the top source level 90 x 60."""
    kind, _, w, h = MAP_CASES[f"noise-{top[0]}x{top[1]}"]
    s, t, prm, _, _, o = case(kind, top, 0, w, h)
    if layers == 1:
        return s, t, dict(prm)
    if layers == 0:
        s0, t0 = oracle.pyr_down(s), o.template_levels()[0][1][0].copy()
        assert t0.shape == (top[1], top[0]) and t0.size < prm["min_reduce_area"]
        return s0, t0, dict(prm)
    assert layers == 2
    tw, th = 4 * top[0], 4 * top[1]
    t2 = synth.box_blur(synth.noise(tw, th, 128, 60, 190 + tw), 5)
    s2 = synth.box_blur(synth.noise(4 * 90, 4 * 60, 128, 60, 191 + tw), 5)
    for k, a in enumerate([23.0, -61.0, 148.0]):
        synth.paste_rotated(s2, t2, s2.shape[1] * (0.28 + 0.42 * (k % 2)), s2.shape[0] * (0.3 + 0.4 * (k // 2)), a)
    return s2, t2, dict(prm)
