"""The host half of the gray-value tools (include/fpm.h, "gray-value tools"), no GPU: fpm_hist_derive against the
restatement of tests/gray_ref.py (== on every field, doubles included), its argument rules, and the restatement itself
against a planted truth: a bright part with dark discs of known radii, segmented with Otsu's threshold."""
import ctypes as C
import math

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import align_ref
from tests import blobs_ref
from tests import gray_ref as ref

# Twice the restatement's own largest |area - pi r^2| over the discs and poses of test_planted_discs, measured by that
# test (it prints every figure): 1.274 pixels, 27 against 28.27 at the disc of radius 3 at both poses (DESIGN.md section
# 23).
AREA_TOLERANCE = 2 * 1.274


def _check(hist, label):
    got = M.hist_derive(np.asarray(hist, np.uint32))
    exp = ref.derive(hist)
    assert got.dtype == M.HIST_STATS_DTYPE and got.shape == ()
    for f in ref.STAT_FIELDS:
        assert got[f].item() == exp[f], f"{label}: {f}: {got[f].item()!r} != {exp[f]!r}"
    return exp


def test_struct_sizes():
    assert C.sizeof(L.HistStats) == M.HIST_STATS_DTYPE.itemsize == 64
    assert C.sizeof(L.SegmentInfo) == M.SEGMENT_INFO_DTYPE.itemsize == 16
    assert [M.HIST_STATS_DTYPE.fields[n][1] for n, _ in L.HistStats._fields_] == [0, 8, 16, 24, 28, 32, 36, 40, 48, 56, 60]
    assert [M.SEGMENT_INFO_DTYPE.fields[n][1] for n, _ in L.SegmentInfo._fields_] == [0, 8, 12]
    assert (L.HIST_EMPTY, L.HIST_FLAT, L.GRAY_OUTSIDE, L.SEG_OTSU) == (1, 2, 4, -1)


def test_random_histograms():
    rng = np.random.default_rng(23)
    for k in range(500):
        kind = k % 5
        if kind == 0:        # dense, any counts
            h = rng.integers(0, 2000, 256)
        elif kind == 1:      # sparse
            h = rng.integers(0, 50, 256) * (rng.random(256) < 0.1)
        elif kind == 2:      # two humps
            x = np.arange(256)
            a, b = rng.integers(10, 120), rng.integers(130, 250)
            h = np.rint(900 * np.exp(-(x - a) ** 2 / 200.0) + 500 * np.exp(-(x - b) ** 2 / 90.0))
        elif kind == 3:      # few pixels
            h = np.bincount(rng.integers(0, 256, rng.integers(1, 6)), minlength=256)
        else:                # a band
            lo = rng.integers(0, 200)
            h = np.zeros(256)
            h[lo:lo + rng.integers(2, 56)] = rng.integers(1, 16384)
        h = h.astype(np.int64)
        assert h.sum() <= ref.MAX_N
        _check(h, f"random {k}")


def test_degenerate_and_tied_histograms():
    z = np.zeros(256, np.int64)
    e = _check(z, "empty")
    assert e["flags"] == L.HIST_EMPTY and all(e[f] == 0 for f in ref.STAT_FIELDS if f != "flags")
    for v in (0, 137, 255):
        h = z.copy()
        h[v] = 1000
        e = _check(h, f"flat {v}")
        assert e["flags"] == L.HIST_FLAT and e["otsu"] == e["min"] == e["max"] == e["median"] == v and e["stddev"] == 0.0
    h = z.copy()
    h[3] = 1
    e = _check(h, "one pixel")
    assert e["n"] == 1 and e["flags"] == L.HIST_FLAT and e["otsu"] == 3 and e["mean"] == 3.0
    # two spikes at a < b: every t in a .. b - 1 splits them alike; the answer is a
    for a, b, na, nb in [(10, 200, 70, 30), (0, 255, 1, 1), (0, 1, 5, 9), (254, 255, 4000, 1), (100, 101, 3, 3)]:
        h = z.copy()
        h[a], h[b] = na, nb
        e = _check(h, f"spikes {a} {b}")
        assert e["otsu"] == a and e["flags"] == 0 and e["min"] == a and e["max"] == b
    # a symmetric histogram: B(t) = B(254 - t) exactly; the smaller t of the best pair wins
    rng = np.random.default_rng(5)
    half = rng.integers(0, 300, 128)
    h = np.concatenate([half, half[::-1]]).astype(np.int64)
    e = _check(h, "symmetric")
    assert e["otsu"] <= 127
    h = z.copy()
    h[[20, 60, 195, 235]] = [50, 7, 7, 50]
    e = _check(h, "symmetric spikes")
    assert e["otsu"] == 60        # t = 60 .. 194 tie between the two middle spikes
    # the largest counts: 2^22 in one bin, and split between the end bins (the largest N)
    for v in (0, 200, 255):
        h = z.copy()
        h[v] = 1 << 22
        assert _check(h, f"full {v}")["flags"] == L.HIST_FLAT
    h = z.copy()
    h[0] = h[255] = 1 << 21
    e = _check(h, "split")
    assert e["otsu"] == 0 and e["mean"] == 127.5 and e["stddev"] == 127.5 and e["median"] == 0


def test_argument_errors_leave_the_output_untouched(fpm_lib):
    out = np.full(1, 7, M.HIST_STATS_DTYPE)
    before = out.tobytes()
    po = out.ctypes.data_as(C.POINTER(L.HistStats))
    ok = np.zeros(256, np.uint32)
    ph = ok.ctypes.data_as(C.POINTER(C.c_uint32))
    assert fpm_lib.fpm_hist_derive(None, po) == L.FPM_E_INVALID_ARG
    assert fpm_lib.fpm_hist_derive(ph, None) == L.FPM_E_INVALID_ARG
    for hist in ([(0, (1 << 22) + 1)], [(0, 1 << 22), (255, 1)], [(b, 1 << 31) for b in range(256)], [(7, 0xFFFFFFFF)]):
        h = np.zeros(256, np.uint32)
        for b, v in hist:
            h[b] = v
        assert fpm_lib.fpm_hist_derive(h.ctypes.data_as(C.POINTER(C.c_uint32)), po) == L.FPM_E_INVALID_ARG
    assert out.tobytes() == before
    assert fpm_lib.fpm_hist_derive(ph, po) == L.FPM_OK and out[0]["flags"] == L.HIST_EMPTY
    with pytest.raises(ValueError):
        M.hist_derive(np.zeros(255, np.uint32))
    with pytest.raises(ValueError):
        M.hist_derive(np.full(256, -1))
    many = M.hist_derive(np.ones((3, 2, 256), np.uint32))
    assert many.shape == (3, 2) and (many["n"] == 256).all() and (many["otsu"] == 127).all()


def test_planted_discs():
    """A bright part with four dark discs of known radii at the alignment tests' two planted poses, rendered by area
    coverage; the restatement's segmentation with Otsu's threshold, dark polarity.  The count is exact (a condition);
    every area lies within AREA_TOLERANCE of pi r^2."""
    tw, th = align_ref.TW, align_ref.TH
    worst = 0.0
    for lt, angle in align_ref.PLANTED:
        scene = ref.planted_scene(tw, th, lt, angle)
        info, e = ref.segment(scene, (0, 0, tw, th), lt, angle, "otsu", -1)
        assert info["flags"] == 0 and ref.DARK < info["threshold"] <= ref.BRIGHT
        _, recs, summary = blobs_ref.blobs(e, 0, 8, 4, 64)
        assert summary["n_blobs"] == len(ref.DISCS) == len(recs) and summary["n_components"] == len(ref.DISCS)
        for cx, cy, r in ref.DISCS:
            d = [math.hypot(b["sum_x"] / b["area"] - cx, b["sum_y"] / b["area"] - cy) for b in recs]
            b = recs[int(np.argmin(d))]
            dev = abs(int(b["area"]) - math.pi * r * r)
            print(f"pose {lt} {angle}: disc r {r}: area {int(b['area'])} against {math.pi * r * r:.2f} "
                  f"(deviation {dev:.2f}), centroid off by {min(d):.3f}, threshold {info['threshold']}")
            assert min(d) < 0.25
            assert dev <= AREA_TOLERANCE
            worst = max(worst, dev)
    print(f"largest deviation {worst:.3f}")
