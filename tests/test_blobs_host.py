"""Defect blobs, host side (no GPU): the reference labelling (tests/blobs_ref.py) on hand-counted cases and against
scipy, then fpm_blobs_host -- the two-pass union-find and the tail (filter, seed order, truncation, summary) -- against
the reference.  Every expectation is equality."""
import ctypes as C

import numpy as np
import pytest

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import blobs_ref as ref


def _ncomp(mask, conn):
    return len(np.unique(ref.label(mask, conn))) - (0 if np.all(mask) else 1)


# ---- the reference itself ---------------------------------------------------------------------------------------------
def test_reference_hand_counted():
    two = np.zeros((6, 6), np.uint8)
    two[0:3, 0:3] = 1
    two[3:6, 3:6] = 1   # touch at a corner
    assert _ncomp(two, 8) == 1 and _ncomp(two, 4) == 2
    lab = ref.label(two, 4)
    assert lab[0, 0] == 1 and lab[5, 5] == 3 * 6 + 3 + 1 and lab[0, 5] == 0
    cb = ref.checkerboard(130, 35)
    assert int(cb.sum()) == 2275
    assert _ncomp(cb, 8) == 1 and _ncomp(cb, 4) == 2275
    assert not ref.label(np.zeros((7, 9), np.uint8), 8).any()
    full = ref.label(np.ones((7, 9), np.uint8), 4)
    assert np.all(full == 1)
    for (y, x) in ((0, 0), (0, 8), (6, 0), (6, 8)):
        one = np.zeros((7, 9), np.uint8)
        one[y, x] = 1
        lab = ref.label(one, 8)
        assert lab[y, x] == y * 9 + x + 1 and int((lab > 0).sum()) == 1
    # the patterns do what their names say
    for w, h in ref.SHAPES[3:]:
        assert _ncomp(ref.spiral(w, h), 4) == 1 and _ncomp(ref.spiral(w, h), 8) == 1
        assert _ncomp(ref.comb(w, h), 4) == 1 and _ncomp(ref.comb_mirror(w, h), 4) == 1
        assert _ncomp(ref.u_shape(w, h), 4) == 1 and _ncomp(ref.s_shape(w, h), 4) == 1
        for d in (ref.diagonal(w, h), ref.anti_diagonal(w, h)):
            assert _ncomp(d, 8) == 1 and _ncomp(d, 4) == min(w, h)
        assert _ncomp(ref.frame_island(w, h), 8) == 2
    # corner pixels of neighbouring tiles touch across the border: columns {0}, {63, 64}, {127, 128, 129} and rows {0},
    # {15, 16}, {31, 32}, {34} form 3 x 4 groups
    assert int(ref.tile_corners(130, 35).sum()) == 6 * 6
    assert _ncomp(ref.tile_corners(130, 35), 4) == 12 and _ncomp(ref.tile_corners(130, 35), 8) == 12


def test_reference_records_by_hand():
    img = np.zeros((4, 5), np.uint8)
    img[1, 1:4] = (10, 20, 30)
    img[2, 3] = 5
    img[3, 0] = 7
    lab, recs, s = ref.blobs(img, 0, 4, 1, 8, hit=3)
    assert [tuple(int(x) for x in r) for r in recs] == [(3, 6, 4, 1, 1, 3, 2, 30, 65, 9, 5), (3, 15, 1, 0, 3, 0, 3, 7, 7, 0, 3)]
    assert s == dict(fg_pixels=5, n_components=2, n_blobs=2, n_returned=2, largest_area=4, flags=0, reserved=0)
    _, recs, s = ref.blobs(img, 6, 4, 2, 8)   # level 6 drops the 5; min_area 2 drops the 7
    assert [int(r["area"]) for r in recs] == [3] and s["n_components"] == 2 and s["n_blobs"] == 1


def test_reference_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    structs = {4: ndi.generate_binary_structure(2, 1), 8: ndi.generate_binary_structure(2, 2)}
    for _ in range(60):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 40))
        mask = rng.random((h, w)) < rng.random()
        for conn in (4, 8):
            lab = ref.label(mask, conn)
            sl, k = ndi.label(mask, structure=structs[conn])
            assert np.array_equal(lab > 0, sl > 0)
            # the same partition: the pairs (ours, scipy's) are a bijection
            pairs = np.unique(np.stack([lab[mask], sl[mask]]), axis=1)
            assert pairs.shape[1] == k == len(np.unique(pairs[0])) == len(np.unique(pairs[1]))
            # and the label is the component's first pixel
            for s in np.unique(lab[mask]):
                assert np.flatnonzero(lab.ravel() == s)[0] == s - 1


# ---- fpm_blobs_host ---------------------------------------------------------------------------------------------------
def test_struct_sizes(fpm_lib):
    assert C.sizeof(L.Blob) == 56 and M.BLOB_DTYPE.itemsize == 56
    assert C.sizeof(L.BlobSummary) == 32 and M.BLOB_SUMMARY_DTYPE.itemsize == 32
    assert [n for n, _ in L.Blob._fields_] == list(ref.FIELDS)
    assert [n for n, _ in L.BlobSummary._fields_] == list(ref.SUMMARY_FIELDS)


def _check_batch(imgs, level, conn, min_area, cap, allrecs):
    summary, blobs, labels = M.blobs_host(imgs, level=level, min_area=min_area, connectivity=conn, cap=cap, labels=True)
    for i, (lab, allr) in enumerate(allrecs):
        assert np.array_equal(labels[i], lab), i
        recs, s = ref.from_all(allr, lab, min_area, cap)
        why = ref.accept(summary[i], blobs[i], recs, s, cap)
        assert why is None, (i, why)
        # the host entry's truncation is the first cap by seed
        assert np.array_equal(ref.as_rec(blobs[i]), recs[:cap]), i


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_host_patterns(fpm_lib, w, h, conn):
    names, imgs, levels = ref.pattern_batch(w, h)
    allrecs = ref.pattern_reference(w, h, conn)
    for lv in sorted(set(levels)):
        sel = [i for i, x in enumerate(levels) if x == lv]
        sub = [(allrecs[i][0], _rehit(allrecs[i][1], k)) for k, i in enumerate(sel)]
        for min_area in (1, 2, 9):
            for cap in (1, 4096):
                _check_batch(imgs[sel], lv, conn, min_area, cap, sub)


def _rehit(recs, hit):
    out = recs.copy()
    out["hit"] = hit
    return out


def test_host_random_masks(fpm_lib):
    rng = np.random.default_rng(77)
    for k in range(200):
        w, h = int(rng.integers(1, 100)), int(rng.integers(1, 60))
        img = ((rng.random((h, w)) < rng.random()) * rng.integers(1, 256, (h, w))).astype(np.uint8)
        level = int(rng.choice((0, 0, 0, 60)))
        for conn in (4, 8):
            lab = ref.label(img.astype(np.int64) > level, conn)
            allr = ref.records(img, lab, 0)
            _check_batch(img, level, conn, (1, 2, 9)[k % 3], (1, 4096)[(k // 3) % 2], [(lab, allr)])


def test_host_strided_rows(fpm_lib):
    """rows stride apart, the bytes between them ignored"""
    rng = np.random.default_rng(3)
    n, w, h, stride = 2, 13, 7, 20
    buf = rng.integers(0, 256, (n, h, stride)).astype(np.uint8)
    summary = np.zeros(n, M.BLOB_SUMMARY_DTYPE)
    recs = np.zeros((n, 64), M.BLOB_DTYPE)
    rc = fpm_lib.fpm_blobs_host(L.u8ptr(buf), n, w, h, stride, 128, 8, 1, summary.ctypes.data_as(C.POINTER(L.BlobSummary)),
                                recs.ctypes.data_as(C.POINTER(L.Blob)), 64, None)
    assert rc == L.FPM_OK
    for i in range(n):
        _, exp, s = ref.blobs(buf[i, :, :w], 128, 8, 1, 64, hit=i)
        assert ref.accept(summary[i], recs[i, :summary["n_returned"][i]], exp, s, 64) is None
        assert not recs[i, summary["n_returned"][i]:].view(np.uint8).any()   # zero-filled behind the records


def test_host_truncation(fpm_lib):
    cb = ref.checkerboard(130, 35) * np.uint8(255)
    summary, blobs = M.blobs_host(cb, level=0, min_area=1, connectivity=4, cap=64)
    _, recs, s = ref.blobs(cb, 0, 4, 1, 64)
    assert summary["n_blobs"][0] == 2275 and summary["flags"][0] == L.BLOBS_TRUNCATED and len(blobs[0]) == 64
    assert ref.accept(summary[0], blobs[0], recs, s, 64) is None
    # the predicate refuses what the contract refuses
    bad = blobs[0].copy()
    bad[[3, 4]] = bad[[4, 3]]
    assert ref.accept(summary[0], bad, recs, s, 64) is not None
    bad = blobs[0].copy()
    bad["sum_x"][5] += 1
    assert ref.accept(summary[0], bad, recs, s, 64) is not None


def test_speckle_uses_no_capacity(fpm_lib):
    img, _ = speckle_scene()
    summary, blobs = M.blobs_host(img, level=0, min_area=4, connectivity=8, cap=8)
    assert summary["n_components"][0] == 10003 and summary["n_blobs"][0] == 3 and summary["flags"][0] == 0
    assert [int(b) for b in blobs[0]["area"]] == [9, 9, 9]


def speckle_scene():
    """10 000 isolated pixels and three 3 x 3 squares; also the squares' seeds"""
    w, h = 420, 206
    img = np.zeros((h, w), np.uint8)
    img[0:200:2, 0:200:2] = 9
    seeds = []
    for (x, y) in ((300, 10), (250, 100), (400, 200)):
        img[y:y + 3, x:x + 3] = 77
        seeds.append(y * w + x)
    return img, seeds


def test_argument_rejection(fpm_lib):
    img = np.zeros((4, 4), np.uint8)
    summary = np.zeros(1, M.BLOB_SUMMARY_DTYPE)
    recs = np.zeros(4, M.BLOB_DTYPE)
    ps, pr = summary.ctypes.data_as(C.POINTER(L.BlobSummary)), recs.ctypes.data_as(C.POINTER(L.Blob))

    def call(images=L.u8ptr(img), n=1, w=4, h=4, stride=4, level=0, conn=8, min_area=1, s=ps, r=pr, cap=4):
        return fpm_lib.fpm_blobs_host(images, n, w, h, stride, level, conn, min_area, s, r, cap, None)

    assert call() == L.FPM_OK
    for kw in (dict(images=None), dict(s=None), dict(r=None), dict(n=0), dict(n=65536), dict(w=0), dict(h=0),
               dict(w=4096, h=1025, stride=4096), dict(stride=3), dict(level=-1), dict(level=255), dict(conn=6),
               dict(conn=0), dict(min_area=0), dict(cap=0), dict(cap=65537), dict(n=65, cap=65536)):
        assert call(**kw) == L.FPM_E_INVALID_ARG, kw
    with pytest.raises(ValueError):
        M.blobs_host(img, connectivity=5)
    with pytest.raises(ValueError):
        M.blobs_host(img, cap=0)
