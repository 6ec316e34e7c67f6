"""The oracle's kept top-layer maps (OracleMatcher.set_keep_maps / top_maps) tied to its pieces that are pinned
elsewhere: each kept map is ncc_map(warp_affine(top level, M)) with M restated here from rotation_matrix and the
canvas translation (fpm_oracle.cpp, Matcher::match), and the peak sequence on it gives that angle's top candidates.
CPU only.
"""
import math

import numpy as np
import pytest

from tests import oracle
from tests.top_map_cases import case

MATCH_CANDIDATE_NUM = 5


def _angles(tw, th, tol):
    step = math.atan(2.0 / max(tw, th)) * (180.0 / math.pi)
    out, a = [], 0.0
    while a < tol + step:
        out.append(a)
        a += step
    a = -step
    while a > -tol - step:
        out.append(a)
        a -= step
    return out


@pytest.mark.parametrize("top", [(16, 16), (12, 9)])
def test_kept_maps_are_warp_then_ncc_and_give_the_candidates(top):
    s, t, prm, maps, nang, o = case("noise", top)
    tw, th = top
    angles = _angles(tw, th, prm["tolerance_angle"])
    assert nang == len(angles) and len(maps) >= 41
    assert [k for k, _, _, _ in maps] == sorted({k for k, _, _, _ in maps})   # angle order, one map per angle
    lvl = oracle.pyr_down(s)
    _, border = o.template_levels()
    cx, cy = np.float32((lvl.shape[1] - 1) / 2.0), np.float32((lvl.shape[0] - 1) / 2.0)
    thr = prm["score"] * 0.9
    cands = o.top_candidates()
    by_angle = {}
    for x, y, sc, ang in cands:
        by_angle.setdefault(ang, []).append((sc, x, y))
    seen = 0
    for k, bw, bh, m in maps:
        assert m.shape == (bh - th + 1, bw - tw + 1)
        tx = np.float32((bw - 1) / 2.0) - cx
        ty = np.float32((bh - 1) / 2.0) - cy
        M = oracle.rotation_matrix(float(cx), float(cy), angles[k])
        M[0, 2] += float(tx)
        M[1, 2] += float(ty)
        ref = o.ncc_map(oracle.warp_affine(lvl, M, (bw, bh), border), 1, False)
        assert np.array_equal(m.view(np.uint32), ref.view(np.uint32)), f"angle {k}"
        peaks = oracle.peak_sequence(m, tw, th, False, False, o.params.max_overlap, prm["max_pos"] + MATCH_CANDIDATE_NUM - 1, thr)
        exp = [(v, float(np.float32(x) - tx), float(np.float32(y) - ty)) for v, x, y in peaks]
        assert exp == by_angle.get(angles[k], []), f"angle {k}"
        seen += len(exp)
    assert seen == len(cands) and seen >= 3
