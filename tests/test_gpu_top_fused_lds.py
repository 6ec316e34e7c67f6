"""k_top_fused's LDS level copy and its f32 bound ahead of the exact score, against the oracle (gfx950 required).

Level copy (fpm_op_top_fused: maps of the map-writing instantiation, peaks of both; tests/test_gpu_top_fused.py's checks:
every map pixel as uint32, every peak's position and score bits, every untouched slot).  A job samples from the copy
where the level's copy (u16 pixel pairs, the border colour around it) fits the job's map region, which the operator's
stats report per plan (copy_angles); the cases:

  top level   source     what it cuts
  49 x 38     98 x 76    sw % 4 = 1: the last staged source word of a row holds one pixel and three border bytes
  50 x 38     100 x 76   sw % 4 = 2
  51 x 38     102 x 76   sw % 4 = 3: entry sw (pixel sw - 1 with the border) is the last of its item
  52 x 38     104 x 76   sw % 4 = 0: entry sw opens an item of its own, whose word lies wholly past the row
  63 x 48     126 x 96   the Src7 bench's top level
(12 x 9 top template, 41 angles over +-180 degrees; the smallest levels of each residue whose every angle's map holds
the copy; every level's row pitch is 64 or 128 bytes, above its width.)
Each source is the noise scene clipped to 1..254, so no level pixel equals the border colour (0 or 255, asserted): a tap
that reads a pixel where the border belongs, or the border where a pixel belongs, changes a canvas byte.  The canvases
are the level rotated about its centre, so at the oblique angles canvas corners lie outside the level, opposite corners
past opposite sides (not asserted here: the maps would differ from the oracle's if such a tap went wrong).
Global path: under the 43 x 6 template the 90 x 60 level fits the maps of 104 of the 137 angles and not the other 33,
so one launch mixes jobs that hold the copy with jobs that cannot; no map
of the 60 x 60 template holds its 88 x 75 level (copy_angles 0: every tap of the launch reads global memory).

Bound (whole searches with the fused form forced; results, per-layer counts and every candidate record byte for byte
against OracleMatcher).  The top-layer threshold is placed at a peak value v of the oracle's own maps: the largest layer
score <= v (v is kept: the bound must pass an output whose exact score equals the threshold) and the smallest > v (v is
dropped); the oracle's own candidate counts differ between the two, which shows the threshold does straddle v.  Also: a
source with a flat block (df = 0 windows), a 43 x 6 top template (area 258: bound on) against 37 x 7 (259: off), and a
search whose layer score is 0.009 (bound off, every map full of peaks).
"""
import functools

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import synth
from tests import oracle
from tests import top_fused_cases as F
from tests.test_gpu_top_fused import _check, _check_ran, _staged, _whole_search
from tests.top_map_cases import noise_scene, params

pytestmark = pytest.mark.gpu

TOP = (12, 9)
LEVELS = {"49x38": (98, 76), "50x38": (100, 76), "51x38": (102, 76), "52x38": (104, 76), "63x48": (126, 96)}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("FPM_TOP_FUSED", "FPM_TOP_MMA", "FPM_GRID_TOP", "FPM_TOP_LIST_CAP"):
        monkeypatch.delenv(k, raising=False)


def _oracle_case(s, t, prm):
    """A case tuple as top_map_cases.case for any scene: (source, template, params, kept maps, angles, oracle)."""
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    o.set_keep_maps()
    o.match(s)
    maps = o.top_maps()
    for _, _, _, m in maps:
        m.setflags(write=False)
    return s, t, prm, maps, o.stats()[0], o


@functools.lru_cache(maxsize=None)
def _level_case(lid):
    w, h = LEVELS[lid]
    s, t = noise_scene(TOP, 0, w, h)
    s = np.clip(s, 1, 254).astype(np.uint8)
    c = _oracle_case(s, t, params(TOP))
    levels, border = c[5].template_levels()
    assert len(levels) == 2 and levels[1][0].shape == (TOP[1], TOP[0])
    top = oracle.pyr_down(s)
    assert top.shape == (h // 2, w // 2) and border in (0, 255) and not np.any(top == border)
    return c


def _level_fits(sw, sh, mw, mh):
    """top_fused_level_fits (fpm_kernels.h) restated: u16 pixel pairs, sh + 2 rows of (sw + 1 rounded up to 4) entries."""
    return mw > 0 and mh > 0 and 2 * ((sw + 1 + 3) & ~3) * (sh + 2) <= 4 * mw * mh


@pytest.mark.parametrize("lid", sorted(LEVELS))
def test_level_copy_widths(gpu_matcher_factory, lid):
    """Every residue of the level width modulo 4 and the bench's 63 x 48: every job samples from the copy."""
    c = _level_case(lid)
    w, h = LEVELS[lid]
    m, prm = _staged(gpu_matcher_factory, [c])
    res = m.top_fused()
    _check_ran(res["stats"], res["geom"], TOP, 1, prm)
    fits = sum(_level_fits(w // 2, h // 2, int(g[2]), int(g[3])) for g in res["geom"])
    assert res["stats"]["copy_angles"] == fits == c[4] == 41, (res["stats"], fits)
    assert res["stats"]["bound"] == 1
    tot = _check(res, [c], TOP, prm, f"level {lid}")
    assert tot["skipped"] == 0 and tot["peaks"] >= 1


@pytest.mark.parametrize("cid,level,copies", [("noise-43x6", (90, 60), 104), ("noise-60x60", (88, 75), 0)])
def test_level_copy_mixed_with_global_taps(gpu_matcher_factory, cid, level, copies):
    """43 x 6: the larger maps hold the level's copy, the others cannot and tap global memory; 60 x 60: none can."""
    c = F.get(cid)
    top = F.MAP_CASES[cid][1]
    m, prm = _staged(gpu_matcher_factory, [c])
    res = m.top_fused()
    _check_ran(res["stats"], res["geom"], top, 1, prm)
    fits = sum(_level_fits(*level, int(g[2]), int(g[3])) for g in res["geom"])
    assert res["stats"]["copy_angles"] == fits == copies < c[4], (res["stats"], fits)
    assert res["stats"]["bound"] == (1 if top[0] * top[1] <= 258 else 0)
    _check(res, [c], top, prm, f"mixed {cid}")


# ---- the bound, through whole searches --------------------------------------------------------------------------
def _scores_around(v):
    """(score whose layer score is the largest <= v, score whose layer score is the smallest > v), one pyramid layer."""
    v = float(v)
    lo = v / 0.9
    while F.layer_score(dict(score=lo)) > v:
        lo = np.nextafter(lo, -np.inf)
    while F.layer_score(dict(score=np.nextafter(lo, np.inf))) <= v:
        lo = np.nextafter(lo, np.inf)
    hi = np.nextafter(lo, np.inf)
    assert F.layer_score(dict(score=lo)) <= v < F.layer_score(dict(score=hi))
    return float(lo), float(hi)


def _cutoff_peak(c, top, near=0.54):
    """The peak value of the oracle's maps closest to `near` (peaks listed down to 0.3), and the two distinct map values
    next to it."""
    vals = [v for _, _, _, mm in c[3] for v, _, _ in oracle.peak_sequence(mm, top[0], top[1], False, False, 0.0, 7, 0.3)]
    v = np.float32(min(vals, key=lambda x: abs(x - near)))
    allv = np.unique(np.concatenate([mm.ravel() for _, _, _, mm in c[3]]))
    k = int(np.searchsorted(allv, v))
    assert allv[k] == v and 0 < k < len(allv) - 1
    return float(v), float(allv[k - 1]), float(allv[k + 1])   # (f64: a comparison with an f32 scalar rounds the other side)


def _bound_state(factory, s, t, prm):
    m = factory(**prm)
    assert m.learnPattern(t)
    m.stage([s])
    return m.top_fused()["stats"]["bound"]


@pytest.mark.parametrize("kind", ["noise", "flat-block"])
def test_bound_at_the_threshold(gpu_matcher_factory, monkeypatch, kind):
    """The layer score just at and just above a peak value of the oracle's maps; `flat-block` adds a constant block to
    the source (windows with df = 0 next to scored ones)."""
    s, t = noise_scene(TOP, 0, 180, 120)
    if kind == "flat-block":
        s = s.copy()
        s[62:118, 100:175] = 141   # clear of the three pasted templates
    c = _oracle_case(s, t, params(TOP))
    if kind == "flat-block":
        assert sum(int((mm == 0).sum()) for _, _, _, mm in c[3]) >= 30000   # (21610 without the block)
    v, below, above = _cutoff_peak(c, TOP)
    keep, drop = _scores_around(v)
    assert below < F.layer_score(dict(score=keep)) <= v < F.layer_score(dict(score=drop)) < above
    counts = []
    for score in (keep, drop):
        prm = dict(params(TOP), score=score)
        assert _bound_state(gpu_matcher_factory, s, t, prm) == 1
        st = _whole_search(gpu_matcher_factory, monkeypatch, s, t, prm, init_kernel=False)
        counts.append(st[1])
    assert counts[0] > counts[1] >= 1, counts   # the threshold does straddle v


def _scene(tw, th, mra, w=180, h=120):
    t = synth.box_blur(synth.noise(tw, th, 128, 60, 90 + tw), 3)
    s = synth.box_blur(synth.noise(w, h, 128, 60, 91 + tw), 3)
    for k, a in enumerate([23.0, -61.0, 148.0]):
        synth.paste_rotated(s, t, w * (0.28 + 0.42 * (k % 2)), h * (0.3 + 0.4 * (k // 2)), a)
    return s, t, dict(max_pos=3, tolerance_angle=180.0, score=0.6, max_overlap=0.0, min_reduce_area=mra)


@pytest.mark.parametrize("top,bound", [((43, 6), 1), ((37, 7), 0)])
def test_bound_area_limit(gpu_matcher_factory, monkeypatch, top, bound):
    """Top template area 258 (the last with the bound) and 259 (exact scores everywhere)."""
    s, t, prm = _scene(2 * top[0], 2 * top[1], 289)
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    levels, _ = o.template_levels()
    assert len(levels) == 2 and levels[1][0].shape == (top[1], top[0]) and top[0] * top[1] == (258 if bound else 259)
    assert _bound_state(gpu_matcher_factory, s, t, prm) == bound
    st = _whole_search(gpu_matcher_factory, monkeypatch, s, t, prm, init_kernel=False)
    assert st[1] >= 1


def test_bound_off_at_a_low_threshold(gpu_matcher_factory, monkeypatch):
    """Layer score 0.009 <= 0.01: no bound (its -2.f would not lie below such a threshold's neighbourhood of small
    scores by any argument the kernel makes); every map yields several peaks."""
    s, t = noise_scene(TOP, 0, 180, 120)
    prm = dict(params(TOP), score=0.01)
    assert F.layer_score(prm) <= 0.01
    assert _bound_state(gpu_matcher_factory, s, t, prm) == 0
    st = _whole_search(gpu_matcher_factory, monkeypatch, s, t, prm, init_kernel=False)
    assert st[1] >= 41 * 2
