"""Defect blobs on the device (fpm_last_blobs / fpm_blobs_at / fpm_op_blobs): the labelling kernels against the Python
reference (tests/blobs_ref.py) on its pattern list, with dirty row padding, in rounds and on a reused context; the
truncation rule; the inspection chain end to end against last_inspect(image=True) + blobs_host; state and errors.
Every expectation is equality, except which records a truncated list holds (ref.accept states that rule)."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import synth
from fastest_image_pattern_matching_amd.matcher import BLOB_DTYPE, BLOB_SUMMARY_DTYPE, blobs_host
from tests import blobs_ref as ref
from tests.test_blobs_host import speckle_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


def _rehit(recs, hit):
    out = recs.copy()
    out["hit"] = hit
    return out


def _check_batch(m, imgs, level, conn, min_area, cap, allrecs):
    summary, blobs, labels = m.op_blobs(imgs, level=level, min_area=min_area, connectivity=conn, cap=cap, labels=True)
    for i, (lab, allr) in enumerate(allrecs):
        assert np.array_equal(labels[i], lab), i
        recs, s = ref.from_all(allr, lab, min_area, cap)
        why = ref.accept(summary[i], blobs[i], recs, s, cap)
        assert why is None, (i, why)
        if not s["flags"]:
            assert np.array_equal(ref.as_rec(blobs[i]), recs), i


def _same(a, b):
    """two op_blobs / last_blobs results, byte for byte"""
    assert a[0].tobytes() == b[0].tobytes()
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert x.tobytes() == y.tobytes()
    if len(a) > 2:
        assert np.array_equal(a[2], b[2])


# ---- 1. patterns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("w,h", ref.SHAPES)
def test_patterns(hip, w, h, conn):
    names, imgs, levels = ref.pattern_batch(w, h)
    allrecs = ref.pattern_reference(w, h, conn)
    for lv in sorted(set(levels)):
        sel = [i for i, x in enumerate(levels) if x == lv]
        sub = [(allrecs[i][0], _rehit(allrecs[i][1], k)) for k, i in enumerate(sel)]
        for min_area in (1, 2, 9):
            for cap in (1, 4096):
                _check_batch(hip, imgs[sel], lv, conn, min_area, cap, sub)


# ---- 2. the bytes beside the image are masked ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", ((63, 15), (65, 17)))
def test_padding_is_masked(hip, w, h):
    _, imgs, _ = ref.pattern_batch(w, h)
    padded = np.full((len(imgs), h, 128), 255, np.uint8)
    padded[:, :, :w] = imgs
    view = padded[:, :, :w]
    assert view.strides == (128 * h, 128, 1)
    for conn in (4, 8):
        dense = hip.op_blobs(imgs, level=0, min_area=1, connectivity=conn, cap=4096, labels=True)
        _same(hip.op_blobs(view, level=0, min_area=1, connectivity=conn, cap=4096, labels=True), dense)
        lab = ref.pattern_reference(w, h, conn)
        full = [i for i, x in enumerate(ref.pattern_batch(w, h)[2]) if x == 0]
        for i in full:
            assert np.array_equal(dense[2][i], lab[i][0]), i


# ---- 3. rounds and reuse ------------------------------------------------------------------------------------------------
def test_rounds_give_identical_bytes(hip):
    _, imgs, _ = ref.pattern_batch(130, 35)
    got = []
    try:
        for r in (1, 3, 0):
            hip.blobs_set_round(r)
            got.append(hip.op_blobs(imgs, level=0, min_area=1, connectivity=4, cap=4096, labels=True))
    finally:
        hip.blobs_set_round(0)
    assert int(got[0][0]["n_blobs"].max()) == 2275 and not got[0][0]["flags"].any()   # nothing truncated: determined
    _same(got[0], got[1])
    _same(got[0], got[2])
    with pytest.raises(ValueError):
        hip.blobs_set_round(-1)


def test_reuse_of_a_context(hip, gpu_matcher_factory):
    """257 x 50, then 5 x 3, then 257 x 50 again: the buffers shrink in use and are cleared per round"""
    big, small = ref.pattern_batch(257, 50)[1], ref.pattern_batch(5, 3)[1]
    kw = dict(level=0, min_area=1, connectivity=8, cap=4096, labels=True)
    fresh_big = gpu_matcher_factory().op_blobs(big, **kw)
    fresh_small = gpu_matcher_factory().op_blobs(small, **kw)
    assert not fresh_big[0]["flags"].any()
    m = gpu_matcher_factory()
    _same(m.op_blobs(big, **kw), fresh_big)
    _same(m.op_blobs(small, **kw), fresh_small)
    _same(m.op_blobs(big, **kw), fresh_big)


# ---- 4. truncation ------------------------------------------------------------------------------------------------------
def test_truncation(hip):
    cb = ref.checkerboard(130, 35) * np.uint8(255)
    summary, blobs = hip.op_blobs(cb, level=0, min_area=1, connectivity=4, cap=64)
    _, recs, s = ref.blobs(cb, 0, 4, 1, 64)
    assert summary["n_blobs"][0] == 2275 and summary["flags"][0] == L.BLOBS_TRUNCATED and len(blobs[0]) == 64
    assert ref.accept(summary[0], blobs[0], recs, s, 64) is None


def test_speckle_uses_no_capacity(hip):
    img, seeds = speckle_scene()
    summary, blobs = hip.op_blobs(img, level=0, min_area=4, connectivity=8, cap=8)
    assert summary["n_components"][0] == 10003 and summary["n_blobs"][0] == 3 and summary["flags"][0] == 0
    assert [int(b) for b in blobs[0]["area"]] == [9, 9, 9]
    assert [int(b) for b in blobs[0]["seed"]] == sorted(seeds)
    _same((summary, blobs), blobs_host(img, level=0, min_area=4, connectivity=8, cap=8))


# ---- 5. end to end ------------------------------------------------------------------------------------------------------
PX, PY = 130, 90


def _dark_spot(t):
    th, tw = t.shape
    dark = t < 100
    spots = [(bx, by) for by in range(4, th - 8) for bx in range(4, tw - 9) if dark[by:by + 4, bx:bx + 5].all()]
    assert spots
    return spots[len(spots) // 2]


def _frames(t):
    base = np.full((240, 320), 128, np.uint8)
    synth.paste(base, t, PX, PY)
    rng = np.random.default_rng(17)
    return [np.clip(base.astype(np.int32) + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8) for _ in range(9)]


def _trained(hip, t, frames):
    """the model from the 8 clean frames, then all 9 staged and searched"""
    hip.resetParams()
    hip._params.max_pos = 1
    assert hip.learnPattern(t)
    hip.stage(frames[:8])
    assert all(len(r) == 1 for r in hip.match_staged())
    assert hip.model_train_last(-1) == 8
    hip.stage(frames)
    res = hip.match_staged()
    assert all(len(r) == 1 and (r[0].ptLT, r[0].dMatchedAngle) == ((float(PX), float(PY)), 0.0) for r in res)


@pytest.mark.parametrize("normalize", (False, True))
def test_planted_defect_end_to_end(hip, templates, normalize):
    t = templates["Dst10"]
    bx, by = _dark_spot(t)
    frames = _frames(t)
    frames[8][PY + by:PY + by + 4, PX + bx:PX + bx + 5] = 255
    _trained(hip, t, frames)
    kw = dict(level=0, min_area=1, connectivity=8, cap=16)
    st, img = hip.last_inspect(-1, 8, 3.0, normalize=normalize, image=True)
    want = blobs_host(img, **kw)
    got = hip.last_blobs(-1, 8, 3.0, normalize=normalize, stats=True, **kw)
    _same(got[:2], want)
    summary, blobs, rows = got
    assert rows.tobytes() == st.tobytes()
    assert len(summary) == 9 and not summary["n_blobs"][:8].any() and all(len(b) == 0 for b in blobs[:8])
    assert summary["n_blobs"][8] == 1 and summary["fg_pixels"][8] == 20 and summary["flags"][8] == 0
    b = blobs[8][0]
    assert (b["hit"], b["area"], b["x0"], b["y0"], b["x1"], b["y1"]) == (8, 20, bx, by, bx + 4, by + 3)
    assert b["seed"] == by * t.shape[1] + bx
    at = hip.blobs_at(np.arange(9), [(PX, PY)] * 9, [0.0] * 9, 8, 3.0, normalize=normalize, stats=True, **kw)
    _same(at[:2], want)
    assert at[2].tobytes() == st.tobytes()


def test_two_blocks_touching_at_a_corner(hip, templates):
    t = templates["Dst10"]
    bx, by = _dark_spot(t)
    frames = _frames(t)
    frames[8][PY + by:PY + by + 2, PX + bx:PX + bx + 2] = 255
    frames[8][PY + by + 2:PY + by + 4, PX + bx + 2:PX + bx + 4] = 255
    _trained(hip, t, frames)
    img = hip.last_inspect(-1, 8, 3.0, image=True)[1]
    for conn, areas in ((8, [8]), (4, [4, 4])):
        kw = dict(level=0, min_area=1, connectivity=conn, cap=16)
        got = hip.last_blobs(-1, 8, 3.0, **kw)
        _same(got, blobs_host(img, **kw))
        assert not got[0]["n_blobs"][:8].any()
        assert [int(a) for a in got[1][8]["area"]] == areas and (got[1][8]["hit"] == 8).all()
    assert (got[1][8]["x0"][0], got[1][8]["y0"][0]) == (bx, by) and (got[1][8]["x1"][1], got[1][8]["y1"][1]) == (bx + 3, by + 3)


# ---- 6. state -------------------------------------------------------------------------------------------------------------
def test_errors_as_last_inspect(hip, templates):
    t = templates["Dst10"]
    frames = _frames(t)
    hip.resetParams()
    hip._params.max_pos = 1
    assert hip.learnPattern(t)          # a new template drops the model
    hip.stage(frames[:2])
    hip.match_staged()
    for call in (lambda: hip.last_inspect(-1), lambda: hip.last_blobs(-1), lambda: hip.blobs_at(0, [(PX, PY)], [0.0])):
        with pytest.raises(ValueError, match="no variation model"):
            call()
    assert hip.model_train_last(-1) == 2
    for kw in (dict(connectivity=6), dict(level=-1), dict(level=255), dict(min_area=0), dict(cap=0), dict(cap=65537),
               dict(cap=(1 << 21) + 1)):   # 2 hits x cap > 2^22
        with pytest.raises(ValueError):
            hip.last_blobs(-1, **kw)
        with pytest.raises(ValueError):
            hip.blobs_at([0, 1], [(PX, PY)] * 2, [0.0] * 2, **kw)
    # 65 poses x 65536 record slots > 2^22: refused by the entry itself, before anything is written
    n = 65
    idx, lt, ang = np.zeros(n, np.int32), np.tile(np.float32([PX, PY]), (n, 1)), np.zeros(n)
    summary, recs = np.zeros(1, BLOB_SUMMARY_DTYPE), np.zeros(1, BLOB_DTYPE)
    rc = hip._lib.fpm_blobs_at(hip._ctx, idx.ctypes.data_as(C.POINTER(C.c_int32)), lt.ctypes.data_as(C.POINTER(C.c_float)),
                               ang.ctypes.data_as(C.POINTER(C.c_double)), n, 8, 48, 0, 0, 8, 1, None,
                               summary.ctypes.data_as(C.POINTER(L.BlobSummary)), recs.ctypes.data_as(C.POINTER(L.Blob)),
                               65536)
    assert rc == L.FPM_E_INVALID_ARG and "2^22" in hip.last_error()
    assert not summary.view(np.uint8).any() and not recs.view(np.uint8).any()
    with pytest.raises(ValueError):
        hip.blobs_at(idx, lt, ang, cap=65536)
    with pytest.raises(ValueError):
        hip.last_blobs(-1, abs_threshold=256)
    with pytest.raises(ValueError):
        hip.last_blobs(7)               # no such source
    with pytest.raises(ValueError):
        hip.op_blobs(np.zeros((4, 4), np.uint8), connectivity=5)
    assert len(hip.last_blobs(-1)[0]) == 2   # and the context still works


def test_search_state_is_left_alone(hip, templates):
    t = templates["Dst10"]
    bx, by = _dark_spot(t)
    frames = _frames(t)
    frames[8][PY + by:PY + by + 4, PX + bx:PX + bx + 5] = 255
    _trained(hip, t, frames)

    def state():
        st, img = hip.last_inspect(-1, 8, 3.0, image=True)
        return st.tobytes(), img.tobytes(), hip.last_patches(-1)[0].tobytes(), [[r.as_tuple() for r in s] for s in hip.match_staged()]

    before = state()
    hip.last_blobs(-1, 8, 3.0, min_area=1)
    hip.op_blobs(ref.pattern_batch(65, 17)[1], min_area=1)
    assert state() == before
    assert hip.model_info() == (8, (0, 0, t.shape[1], t.shape[0]))


def test_profile_counts_one_launch_per_kernel_and_round(hip, templates):
    t = templates["Dst10"]
    frames = _frames(t)
    _trained(hip, t, frames)
    hip.profile(True)
    try:
        for rounds, per in ((1, 0), (3, 3), (9, 1)):
            hip.profile_reset()
            hip.blobs_set_round(per)
            hip.last_blobs(-1, 8, 3.0)
            got = [hip.blobs_profile(k) for k in range(5)]
            assert [g[1] for g in got] == [rounds] * 5, got
            assert all(g[0] > 0 and g[2] > 0 for g in got), got
            assert hip.model_profile(L.MODEL_INSPECT)[1] == 1
        hip.profile_reset()
        hip.op_blobs(ref.pattern_batch(65, 17)[1])     # the parity vehicle leaves the counters alone
        assert [hip.blobs_profile(k)[1] for k in range(5)] == [0] * 5
    finally:
        hip.blobs_set_round(0)
        hip.profile(False)
    with pytest.raises(ValueError):
        hip.blobs_profile(5)
