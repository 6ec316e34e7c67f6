"""Scenes, shapes and oracle maps shared by tests/test_oracle_top_maps.py, tests/test_gpu_top_maps.py,
tests/test_oracle_top_fused.py and tests/test_gpu_top_fused.py.

A case is a (scene, top template shape) pair; its oracle run (OracleMatcher.set_keep_maps: the top-layer score map of
every scored angle, unpainted) is computed once per process and handed out read-only.
"""
import functools

import numpy as np

from fastest_image_pattern_matching_amd import synth
from tests import oracle

# top template (w, h) -> level-0 template (tw, th) and MinReduceArea; each gives a top layer of 1 and a template level
# that is not ResultEqual1
SHAPES = {
    (16, 16): (32, 32, 256),    # TH = 16 exact form; prefilter on
    (14, 14): (28, 28, 256),    # TH = 14 exact form
    (12, 9): (24, 18, 256),     # masked small form, odd height
    (17, 15): (34, 30, 256),    # widest two-row layout with the prefilter on
    (43, 6): (86, 12, 289),     # area 258: the last with the prefilter on; one-row layout
    (49, 16): (98, 32, 1024),   # widest one-row layout; no prefilter; <16, 64>
    (17, 32): (34, 64, 1024),   # tallest two-row layout; 47 ring rows in <16, 64>
    (60, 60): (120, 120, 4096),   # beyond both layouts: the split kernels only
    (3, 30): (6, 60, 256),      # narrower than one 4-pixel word (k_top_fused's template masks)
}
SCORE = 0.6   # layer score of the top layer: 0.54


def params(top, max_pos=3, score=SCORE, max_overlap=0.0):
    return dict(max_pos=max_pos, tolerance_angle=180.0, score=score, max_overlap=max_overlap,
                min_reduce_area=SHAPES[top][2])


def noise_scene(top, seed=0, w=470, h=310):
    """Blurred noise with three pasted rotated copies of the (blurred noise) template; `seed` varies the source only."""
    tw, th, _ = SHAPES[top]
    t = synth.box_blur(synth.noise(tw, th, 128, 60, 90 + tw), 3)
    s = synth.box_blur(synth.noise(w, h, 128, 60, 91 + tw + 7 * seed), 3)
    for k, a in enumerate([23.0, -61.0, 148.0]):
        synth.paste_rotated(s, t, w * (0.28 + 0.42 * (k % 2)), h * (0.3 + 0.4 * (k // 2)), a)
    return s, t


def saturated_scene(top, w=470, h=310):
    """Hard 0 / 255 regions: an all-255 third, a 3-pixel checker and random 0 / 255; the template random 0 / 255.  Large
    flat windows (score 0) next to windows at the extreme sums."""
    tw, th, _ = SHAPES[top]
    rng = np.random.default_rng(500 + tw)
    t = (rng.integers(0, 2, (th, tw)) * 255).astype(np.uint8)
    s = np.zeros((h, w), np.uint8)
    a, b = w // 3, 2 * w // 3
    s[:, :a] = 255
    yy, xx = np.mgrid[0:h, a:b]
    s[:, a:b] = ((((yy // 3) + (xx // 3)) & 1) * 255).astype(np.uint8)
    s[:, b:] = (rng.integers(0, 2, (h, w - b)) * 255).astype(np.uint8)
    return s, t


def constant_template_scene(top, seed=0, w=470, h=310):
    """The noise scene's source under a template of one value: every level is ResultEqual1."""
    s, t = noise_scene(top, seed, w, h)
    return s, np.full_like(t, 93)


def constant_source_scene(top, w=470, h=310):
    """A source of one value under the noise template: every window is flat."""
    _, t = noise_scene(top, 0, w, h)
    return np.full((h, w), 141, np.uint8), t


@functools.lru_cache(maxsize=None)
def case(kind, top, seed=0, w=470, h=310, max_pos=3, score=SCORE, max_overlap=0.0):
    """(source, template, params, oracle maps [(angle_index, bw, bh, map)], n_angles, OracleMatcher after its search);
    everything read-only.  kind: "saturated", "constant_template", "constant_source", anything else the noise scene; a
    narrow source (a top level narrower than the top template for some angles) is a matter of w and h."""
    if kind == "saturated":
        s, t = saturated_scene(top, w, h)
    elif kind == "constant_template":
        s, t = constant_template_scene(top, seed, w, h)
    elif kind == "constant_source":
        s, t = constant_source_scene(top, w, h)
    else:
        s, t = noise_scene(top, seed, w, h)
    prm = params(top, max_pos, score, max_overlap)
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    o.set_keep_maps()
    o.match(s)
    maps = o.top_maps()
    levels, _ = o.template_levels()
    assert len(levels) == 2 and levels[1][0].shape == (top[1], top[0]), (top, len(levels))
    assert levels[1][4] == (kind == "constant_template"), (kind, top)
    for _, _, _, m in maps:
        m.setflags(write=False)
    s.setflags(write=False)
    t.setflags(write=False)
    return s, t, prm, maps, o.stats()[0], o
