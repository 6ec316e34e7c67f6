"""The oracle's one-ROI refinement entry (OracleMatcher.refine_roi = orc_rotated_roi + ncc_map + the search's record
rules), pinned on the CPU: against the oracle's own search through its refinement trace, against a plain float64
normalised correlation with a derived bound, and the coverage the device tests' position sweep relies on."""
import ctypes as C

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib
from tests import cases, oracle, refine_cases as rc


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(levels):
        out.append(oracle.pyr_down(out[-1]))
    return out


def test_refine_roi_reproduces_the_search_trace(templates):
    """Every (candidate, layer, angle) of a small search: refine_roi at the trace's ptLT and angle on the oracle's own
    pyramid level gives the score and location the search took, exactly."""
    build, prm = cases.CASES["dst10_multi"]
    s, t = build(templates)
    o = oracle.OracleMatcher().set(**prm).set_trace(True)
    assert o.learnPattern(t)
    assert o.match(s)
    tr = o.trace()
    assert len(tr) > 0 and set(tr["layer"]) == set(range(len(o.template_levels()[0]) - 1))
    spyr = pyramid(s, int(tr["layer"].max()))
    rows = 0
    for row in tr:
        for j in range(row["n3"]):
            _, m, r = o.refine_roi(spyr[row["layer"]], int(row["layer"]), row["lt"], row["angle"][j], True)
            assert (np.float64(r["score"]), r["mx"], r["my"]) == (row["score"][j], row["x"][j], row["y"][j]), (row, j)
            second = np.delete(m.ravel(), r["my"] * 7 + r["mx"]).max()
            assert np.float64(second) == row["second"][j]
            rows += 1
    assert rows == 3 * len(tr)   # tolerance_angle 180: three angles per candidate and layer


def test_roi_record_rules():
    """First maximum in row-major order; a zeroed 3x3 on the border; vec[(x+1)*3 + (y+1)] off it."""
    m = np.zeros((7, 7), np.float32)
    m[2, 5] = m[4, 1] = 0.5   # equal maxima: row 2 comes first
    r = oracle.roi_record(m)
    assert (r["mx"], r["my"], r["on_border"]) == (5, 2, 0)
    m2 = np.arange(49, dtype=np.float32).reshape(7, 7)
    m2[3, 2] = 100
    r = oracle.roi_record(m2)
    assert (r["mx"], r["my"], r["on_border"]) == (2, 3, 0)
    assert r["vec"].tolist() == [m2[3 + y, 2 + x] for x in (-1, 0, 1) for y in (-1, 0, 1)]
    for mx, my in ((0, 3), (6, 3), (3, 0), (3, 6), (6, 6)):
        m3 = np.zeros((7, 7), np.float32)
        m3[my, mx] = 1
        r = oracle.roi_record(m3)
        assert (r["mx"], r["my"], r["on_border"]) == (mx, my, 1) and not r["vec"].any()


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("tw,th", [(37, 29), (90, 41)])
def test_refine_roi_against_float64(tw, th, fold):
    """The 7x7 map against numpy float64 from the ROI pixels and the template level.  The numerator C = sum I T is an
    exact integer, rounded once to f32 (fold 0) or accumulated in f32 over th rows (fold 1: th roundings of partial sums
    <= C), then the score is rounded to f32: |score - score64| <= (th_eff + 1) 2^-24 C / t + 2^-23."""
    t = rc.texture(tw, th, 11)
    s = rc.texture(200, 160, 12)
    o = rc.learn_one_level(oracle.OracleMatcher(), t)
    (px, mean, norm, inv_area, eq1), = o.template_levels()[0]
    assert not eq1 and px.shape == (th, tw)
    T = px.astype(np.float64)
    rng = np.random.default_rng(5)
    for _ in range(6):
        lt = (rng.uniform(10, 200 - tw - 10), rng.uniform(10, 160 - th - 10))
        roi, m, _ = o.refine_roi(s, 0, lt, rng.uniform(-180, 180), bool(fold))
        I = roi.astype(np.float64)
        for y in range(7):
            for x in range(7):
                w = I[y:y + th, x:x + tw]
                Cn, S, Q = (w * T).sum(), w.sum(), (w * w).sum()
                tt = np.sqrt(Q - S * S * inv_area) * norm
                num = Cn - S * mean
                assert tt > 0 and abs(num) < tt   # no clamp branch of CCOEFF_Denominator in play
                bound = ((th if fold else 1) + 1) * 2.0 ** -24 * Cn / tt + 2.0 ** -23
                assert abs(float(m[y, x]) - num / tt) <= bound, (x, y, m[y, x], num / tt, bound)


def test_position_sweep_covers_the_map():
    """The unrotated sweep of the device tests (tests/test_gpu_refine.py): the centre angle's maxima land on all 49 map
    positions, and on_border is set on exactly the 24 ring positions."""
    s, t, lt, ang, offs = rc.sweep_case(40, 30, 0.0, 21)
    o = rc.learn_one_level(oracle.OracleMatcher(), t)
    rec, _ = rc.oracle_refine(o, [s], 0, lt, ang, True)
    centre = rec[0, :, 1]
    pos = {(int(r["mx"]), int(r["my"])) for r in centre}
    assert pos == {(x, y) for x in range(7) for y in range(7)}
    for r, (dx, dy) in zip(centre, offs):
        assert (r["mx"], r["my"]) == (3 - dx, 3 - dy)
        assert r["on_border"] == int(r["mx"] in (0, 6) or r["my"] in (0, 6))
    assert int(centre["on_border"].sum()) == 24


def test_rotated_tile_boxes_fit_the_wave_buffer():
    """Why no device test reaches a kTileLds-clear tile: the ROI matrix is a pure rotation, so a 32 x 32 tile's source box
    (corners +- the tap margins, 4-byte aligned) spans at most 32 sqrt(2) + 8 px either way, inside the 64 px x 60 row
    wave buffer at every angle -- by the descriptors' own rule (refine_cases.tile_boxes), over a dense angle sweep."""
    n = 0
    for lt in ((37.0, 21.0), (101.5, 60.25), (-20.0, 150.0)):
        for a in np.arange(-180.0, 180.0, 0.75):
            for b in rc.tile_boxes(400, 300, 90, 70, lt, float(a)):
                if b[4]:
                    assert b[5] and b[2] <= 16 and b[3] <= 60, (lt, a, b)
                    n += 1
    assert n > 8000   # of 3 x 480 x 12 tiles, those that touch the image


def test_op_refine_rejects_a_null_context(fpm_lib):
    wrote = C.c_int32(7)
    assert fpm_lib.fpm_op_refine(None, None, 0, 0, 0, 0, 0, None, None, 0, 0, 0, 0, None, None,
                                 C.byref(wrote)) == _lib.FPM_E_INVALID_ARG
    assert C.sizeof(_lib.RoiRecord) == oracle.ROI_RECORD_DTYPE.itemsize == 52
