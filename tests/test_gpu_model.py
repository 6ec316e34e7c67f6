"""Variation model on the HIP path (fpm_model_* / fpm_last_inspect / fpm_inspect_at): per-pixel sums trained from hits on
the device, the mean / lo / hi planes derived from them, and hits held against those.  The expectation is the oracle's
warpAffine of fpm_patch_matrix's matrix, then Python integers (tests/model_ref.py).  Every comparison is ==."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import synth
from fastest_image_pattern_matching_amd.matcher import INSPECT_DTYPE, LearnError, merge_candidates, patch_matrix
from tests import model_ref as ref
from tests import oracle
from tests.cases import CASES, _run_both
from tests.fast_mode_ref import fast_reference
from tests.test_gpu_compare import EDGE_POSES
from tests.test_gpu_learn_device import assert_same_template, host_learned, snapshot
from tests.test_patch_host import poses as host_poses

pytestmark = pytest.mark.gpu

PARITY = {"dst10_multi": 3, "dst5_subpixel": 1, "top_is_layer0": 2, "dst4_overlap": 2}
SEMANTICS_MFC = 1
AK = [(0, 0.0), (8, 3.0), (255, 15.9375)]    # (a, kq) = (0, 0), (8, 48), (255, 255)


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


_scenes = {}


def _scene(templates, case):
    if case not in _scenes:
        make, prm = CASES[case]
        _scenes[case] = make(templates) + (prm,)
    return _scenes[case]


def _tuples(res):
    return [r.as_tuple() for r in res]


def _qt_poses(results):
    return [(r.ptLT, r.dMatchedAngle) for r in results]


def _patches(src, t, poses, rect):
    """(patches, template crop) for `poses` [(lt, angle)] on `src`; rect None = the whole template."""
    th, tw = t.shape
    x, y, w, h = rect if rect is not None else (0, 0, tw, th)
    T = np.ascontiguousarray(t[y:y + h, x:x + w])
    return [oracle.warp_affine(src, patch_matrix(src.shape[1], src.shape[0], lt, a, (x, y)), (w, h)) for lt, a in poses], T


def _expect_inspect(patches, T, lo, hi, normalize):
    rows, imgs = [], []
    for I in patches:
        v, gain, offset = ref.sample(I, T, normalize)
        row, e = ref.inspect(v, lo, hi, gain, offset)
        rows.append(row)
        imgs.append(e)
    return rows, np.array(imgs, np.uint8).reshape((len(patches),) + T.shape)


def _eq_sums(hip, n, S, Q, label):
    gs, gq = hip.model_sums()
    assert gs.dtype == gq.dtype == np.uint32
    assert np.array_equal(gs, S) and np.array_equal(gq, Q), label
    assert hip.model_info()[0] == n, label


# ---- tile and lane edges --------------------------------------------------------------------------------------------
EDGE_W = [1, 3, 4, 5, 63, 64, 65]
EDGE_H = [1, 15, 16, 17]


@pytest.mark.parametrize("sw", [161, 164])
def test_tile_and_lane_edges(hip, sw):
    sh = 119
    rng = np.random.default_rng(sw)
    src = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    tmpl = rng.integers(0, 256, (23, 71), dtype=np.uint8)
    hip.resetParams()
    assert hip.learnPattern(tmpl)
    hip.stage([src])
    ps = EDGE_POSES + host_poses()
    lts, angs = [p[0] for p in ps], [p[1] for p in ps]
    try:
        for w in EDGE_W:
            for h in EDGE_H:
                for x in (0, 1, 2, 3):
                    rect = (x, (x + h) % 5, w, h)
                    patches, T = _patches(src, tmpl, ps, rect)
                    for norm in (False, True):
                        tag = f"{rect} norm={norm}"
                        n, S, Q = ref.accumulate([ref.sample(I, T, norm)[0] for I in patches])
                        for chunk in (0, 1, 2, len(ps)):
                            hip.model_clear()
                            hip.model_set_chunk(chunk)
                            assert hip.model_train_at(0, lts, angs, rect, normalize=norm) == n
                            _eq_sums(hip, n, S, Q, f"{tag} chunk={chunk}")
                            assert hip.model_info() == (n, rect)
                        hip.model_set_chunk(2 if (w + h) % 2 else 0)    # an atomic add, or a plain one, onto a model
                        hip.model_train_at(0, lts, angs, rect, normalize=norm)
                        _eq_sums(hip, 2 * n, 2 * S, 2 * Q, tag + " twice")
                        for a, k in AK:
                            mean, lo, hi = ref.derive(2 * n, 2 * S, 2 * Q, a, ref.kq_of(k))
                            got = hip.model_images(a, k)
                            assert all(np.array_equal(g, e) for g, e in zip(got, (mean, lo, hi))), (tag, a, k)
                            rows, imgs = _expect_inspect(patches, T, lo, hi, norm)
                            st, img = hip.inspect_at(0, lts, angs, a, k, normalize=norm, image=True)
                            assert st.dtype == INSPECT_DTYPE
                            ref.assert_rows(st, rows, f"{tag} a={a} k={k}")
                            assert np.array_equal(img, imgs), (tag, a, k)
    finally:
        hip.model_set_chunk(0)


# ---- border path ----------------------------------------------------------------------------------------------------
def test_patches_that_leave_the_source(hip, templates):
    s, t, prm = _scene(templates, "top_is_layer0")
    assert s.shape == (160, 220)
    th, tw = t.shape
    hip.resetParams()
    assert hip.learnPattern(t)
    hip.stage([s])
    ps = [((-tw / 2.0, 70.0), 0.0), ((220.0 - tw / 2.0, 70.0), 0.0), ((93.0, -th / 2.0), 0.0), ((93.0, 160.0 - th / 2.0), 0.0),
          ((-10.5, 150.25), 37.0), ((1000.0, 1000.0), 0.0), ((101.5, 72.25), 37.0)]
    lts, angs = [p[0] for p in ps], [p[1] for p in ps]
    patches, T = _patches(s, t, ps, None)
    assert not patches[5].any() and all(p.any() for p in patches[:5])
    for norm in (False, True):
        n, S, Q = ref.accumulate([ref.sample(I, T, norm)[0] for I in patches])
        hip.model_clear()
        assert hip.model_train_at(0, lts, angs, normalize=norm) == 7
        _eq_sums(hip, n, S, Q, f"borders norm={norm}")
        mean, lo, hi = ref.derive_fast(n, S, Q, 8, 48)
        assert all(np.array_equal(g, e) for g, e in zip(hip.model_images(8, 3.0), (mean, lo, hi)))
        rows, imgs = _expect_inspect(patches, T, lo, hi, norm)
        st, img = hip.inspect_at(0, lts, angs, 8, 3.0, normalize=norm, image=True)
        ref.assert_rows(st, rows, f"borders norm={norm}")
        assert np.array_equal(img, imgs)


# ---- after a search -------------------------------------------------------------------------------------------------
def _check_last(hip, src, t, poses, label):
    """model_train_last(-1) then last_inspect of the search just run, against the reference at `poses`."""
    patches, T = _patches(src, t, poses, None)
    for norm in (False, True):
        tag = f"{label} norm={norm}"
        n, S, Q = ref.accumulate([ref.sample(I, T, norm)[0] for I in patches])
        hip.model_clear()
        assert hip.model_train_last(-1, normalize=norm) == len(poses)
        _eq_sums(hip, n, S, Q, tag)
        for a, k in ((8, 3.0), (0, 1.0)):
            mean, lo, hi = ref.derive_fast(n, S, Q, a, ref.kq_of(k))
            assert all(np.array_equal(g, e) for g, e in zip(hip.model_images(a, k), (mean, lo, hi))), tag
            rows, imgs = _expect_inspect(patches, T, lo, hi, norm)
            st, img = hip.last_inspect(0, a, k, normalize=norm, image=True)
            ref.assert_rows(st, rows, f"{tag} a={a} k={k}")
            assert np.array_equal(img, imgs), tag
            ref.assert_rows(hip.last_inspect(-1, a, k, normalize=norm), rows, tag + " no image")


@pytest.mark.parametrize("case", sorted(PARITY))
def test_model_of_results(hip, templates, case):
    s, t, prm = _scene(templates, case)
    gpu, orc, _, _ = _run_both(hip, s, t, **prm)
    assert len(orc) >= PARITY[case] and _tuples(gpu) == orc
    _check_last(hip, s, t, _qt_poses(gpu), case)


def test_mfc_semantics_and_bitwise_not(hip, templates):
    """The raw pose, not the converted result's, and the inverted plane the search ran on."""
    s, t, prm = _scene(templates, "dst3_range")
    inv = np.ascontiguousarray(255 - s)
    o = oracle.OracleMatcher()
    hip.resetParams()
    for k, v in {**prm, "semantics": SEMANTICS_MFC}.items():
        setattr(o.params, k, v)
        setattr(hip._params, k, v)
    hip._params.bitwise_not = 1
    for k, v in enumerate((-40.0, -1.0, 0.0, 40.0)):   # as tests/test_gpu_compare.py: the case's +-40 degrees as two ranges
        o.params.tolerance[k] = v
        hip._params.tolerance[k] = v
    assert o.learnPattern(t) and hip.learnPattern(t)
    gpu, orc = hip.match(inv), o.match(s)              # 255 - inv = s is what is searched, and what the model sees
    assert len(orc) >= 2 and _tuples(gpu) == orc
    assert all(abs(r.dMatchedAngle) < 40 for r in gpu)   # so the reported angle is the exact negation of dMatchAngle
    _check_last(hip, s, t, [(r.ptLT, -r.dMatchedAngle) for r in gpu], "mfc + bitwise not")


def test_fast_mode_uses_the_doubled_layer1_pose(hip, templates):
    s, t, prm = _scene(templates, "dst10_multi")
    th, tw = t.shape
    rec = fast_reference(t, s, prm)[0]
    hip.resetParams()
    for k, v in {**prm, "stop_layer": 1}.items():
        setattr(hip._params, k, v)
    assert hip.learnPattern(t)
    got = hip.match(s)
    exp = merge_candidates(hip._params, tw, th, rec)
    assert len(exp) >= 3 and _tuples(got) == _tuples(exp)
    _check_last(hip, s, t, _qt_poses(exp), "fast mode")


# ---- planted defect -------------------------------------------------------------------------------------------------
def test_planted_defect(hip, templates):
    t = templates["Dst10"]
    th, tw = t.shape
    dark = t < 100
    spots = [(bx, by) for by in range(4, th - 8) for bx in range(4, tw - 9) if dark[by:by + 4, bx:bx + 5].all()]
    assert spots
    bx, by = spots[len(spots) // 2]
    px, py = 130, 90
    base = np.full((240, 320), 128, np.uint8)
    synth.paste(base, t, px, py)
    rng = np.random.default_rng(17)
    frames = [np.clip(base.astype(np.int32) + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8) for _ in range(9)]
    frames[8][py + by:py + by + 4, px + bx:px + bx + 5] = 255
    pose = [((float(px), float(py)), 0.0)]
    # the two claims in the restatement first: no training frame leaves its own model, the ninth leaves it in the block only
    train = [_patches(f, t, pose, None)[0][0] for f in frames[:8]]
    n, S, Q = ref.accumulate(train)
    mean, lo, hi = ref.derive_fast(n, S, Q, 8, 48)
    rows = [ref.inspect(I, lo, hi)[0] for I in train]
    assert all(r["n_low"] + r["n_high"] == 0 for r in rows)
    bad, bad_img = ref.inspect(_patches(frames[8], t, pose, None)[0][0], lo, hi)
    assert (bad["n_low"], bad["n_high"]) == (0, 20) and (bad["x0"], bad["y0"], bad["x1"], bad["y1"]) == (bx, by, bx + 4, by + 3)
    # train on a batch, restage, inspect the next frame
    hip.resetParams()
    hip._params.max_pos = 1
    assert hip.learnPattern(t)
    hip.stage(frames[:8])
    res = hip.match_staged()
    assert all(len(r) == 1 and _qt_poses(r) == pose for r in res)
    assert hip.model_train_last(-1) == 8
    _eq_sums(hip, n, S, Q, "defect")
    st = hip.last_inspect(-1, 8, 3.0)
    ref.assert_rows(st, rows, "training frames")
    assert ((st["n_low"] + st["n_high"]) == 0).all() and (st["sum_excess"] == 0).all()
    assert (st["x0"] == tw).all() and (st["y0"] == th).all() and (st["x1"] == -1).all() and (st["y1"] == -1).all()
    hip.stage([frames[8]])
    assert hip.model_info() == (8, (0, 0, tw, th))     # restaging keeps the model
    assert _qt_poses(hip.match_staged()[0]) == pose
    st, img = hip.last_inspect(0, 8, 3.0, image=True)
    ref.assert_rows(st, [bad], "ninth frame")
    assert np.array_equal(img[0], bad_img)
    assert st[0]["n_high"] == 20 and st[0]["n_low"] == 0
    assert (st[0]["x0"], st[0]["y0"], st[0]["x1"], st[0]["y1"]) == (bx, by, bx + 4, by + 3)


# ---- counter cap ----------------------------------------------------------------------------------------------------
def test_counter_cap(hip):
    src = np.full((48, 64), 255, np.uint8)
    hip.resetParams()
    assert hip.learnPattern(np.random.default_rng(3).integers(0, 256, (8, 8), dtype=np.uint8))
    hip.stage([src])
    n = L.MODEL_MAX_SAMPLES
    lts = np.tile(np.array([[10.0, 10.0]], np.float32), (n, 1))
    assert hip.model_train_at(0, lts, np.zeros(n), (0, 0, 1, 1)) == n
    S, Q = hip.model_sums()
    assert S.shape == (1, 1) and int(S[0, 0]) == n * 255 and int(Q[0, 0]) == n * 65025
    r = L.PatchRect(0, 0, 1, 1)
    idx, lt, ang = np.zeros(1, np.int32), np.array([[10.0, 10.0]], np.float32), np.zeros(1)
    rc = hip._lib.fpm_model_train_at(hip._ctx, C.byref(r), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                     lt.ctypes.data_as(C.POINTER(C.c_float)), ang.ctypes.data_as(C.POINTER(C.c_double)), 1, 0)
    assert rc == L.FPM_E_CAPACITY
    S2, Q2 = hip.model_sums()
    assert hip.model_info() == (n, (0, 0, 1, 1)) and np.array_equal(S, S2) and np.array_equal(Q, Q2)
    assert [p.tolist() for p in hip.model_images(0, 0.0)] == [[[255]]] * 3


# ---- model_learn ----------------------------------------------------------------------------------------------------
def test_model_learn(gpu_matcher_factory, templates):
    t = templates["Dst10"]
    s = synth.noise(480, 360, 128, 10, 2024)
    synth.paste_rotated(s, t, 150, 140, 33.0)
    synth.paste_rotated(s, t, 330, 230, -120.0)
    th, tw = t.shape
    prm = dict(max_pos=2, tolerance_angle=180.0)
    rect = (2, 1, tw - 3, th - 2)                # same top layer as the template's: the sources stay staged
    a = gpu_matcher_factory(**prm)
    assert a.learnPattern(t)
    a.stage([s])
    first = a.match_staged()[0]
    assert len(first) == 2
    assert a.model_train_last(0, rect) == 2
    patches, _ = _patches(s, t, _qt_poses(first), rect)
    n, S, Q = ref.accumulate(patches)
    mean = ref.derive_fast(n, S, Q, 0, 0)[0]
    assert np.array_equal(a.model_images(0, 0.0)[0], mean)
    a.model_learn()
    assert a.model_info() == (2, (0, 0, rect[2], rect[3]))
    _eq_sums(a, n, S, Q, "after model_learn")
    sa = snapshot(a)
    assert sa["levels"][0][:2] == (mean.shape, mean.tobytes())
    b = host_learned(gpu_matcher_factory, mean, **prm)
    assert_same_template(sa, snapshot(b), "model_learn")
    # the last poses are dropped, the sources survive: the next search is the oracle's with the mean image
    with pytest.raises(ValueError, match="no search has run"):
        a.last_inspect(0)
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(mean)
    again, exp = a.match_staged()[0], o.match(s)
    assert len(exp) >= 1 and _tuples(again) == exp
    # a hit of the new template and the model's new rectangle sample the region the model was trained on
    assert a.model_train_last(0) == len(exp)
    more, _ = _patches(s, mean, _qt_poses(again), None)
    n2, S2, Q2 = ref.accumulate(patches + more)
    _eq_sums(a, n2, S2, Q2, "trained on after model_learn")
    # a model whose mean has another top layer than the slab's: the sources go, as after learn_at
    a.model_clear()
    a.model_train_at(0, [(150.0, 140.0)], [0.0], (0, 0, 12, 12))
    a.model_learn()
    assert a.template_info()[0] == 1 and a.model_info() == (1, (0, 0, 12, 12))
    with pytest.raises(RuntimeError, match="no staged sources"):
        a.match_staged()


# ---- state ----------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LearnError) as e:
        call()
    return e.value.code


def test_state_rules(gpu_matcher_factory, templates):
    t = templates["Dst10"]
    th, tw = t.shape
    s = synth.noise(320, 240, 128, 10, 300)
    synth.paste_rotated(s, t, 80, 70, 25.0)
    synth.paste_rotated(s, t, 230, 160, -140.0)
    m = gpu_matcher_factory(max_pos=3, tolerance_angle=180.0)
    n = C.c_int32(-1)
    assert m._lib.fpm_last_inspect(m._ctx, 0, 8, 48, 0, None, 0, C.byref(n), None, 0, 0) == L.FPM_E_NOT_LEARNED
    assert m.model_info() == (0, None)
    assert m.learnPattern(t)
    with pytest.raises(ValueError, match="no staged sources"):
        m.model_train_last()
    m.stage([s])
    with pytest.raises(ValueError, match="no search has run"):
        m.model_train_last()
    # no model: every entry that needs one is FPM_E_INVALID_ARG
    assert m._lib.fpm_last_inspect(m._ctx, 0, 8, 48, 0, None, 0, C.byref(n), None, 0, 0) == L.FPM_E_INVALID_ARG
    assert m._lib.fpm_model_sums(m._ctx, None, None) == L.FPM_E_INVALID_ARG
    assert m._lib.fpm_model_images(m._ctx, 8, 48, None, None, None, tw) == L.FPM_E_INVALID_ARG
    assert m._lib.fpm_model_learn(m._ctx) == L.FPM_E_INVALID_ARG
    for call in (m.model_sums, m.model_images, m.last_inspect, lambda: m.inspect_at(0, [(10.0, 10.0)], [0.0])):
        with pytest.raises(ValueError, match="no variation model"):
            call()
    assert _code(m.model_learn) == L.FPM_E_INVALID_ARG
    assert len(m.match_staged()[0]) == 2
    assert m.model_train_last() == 2 and m.model_train_at(0, [(10.0, 10.0)], [5.0]) == 1
    assert m.model_info() == (3, (0, 0, tw, th))
    # another rectangle, a bad one, bad thresholds and flags
    with pytest.raises(ValueError, match="another rectangle"):
        m.model_train_last(0, (1, 0, tw - 1, th))
    with pytest.raises(ValueError):
        m.model_train_last(0, (0, 0, tw + 1, th))
    added = C.c_int32(-1)
    assert m._lib.fpm_model_train_last(m._ctx, C.byref(L.PatchRect(1, 1, 4, 4)), 0, 0, C.byref(added)) == L.FPM_E_INVALID_ARG
    assert added.value == 0
    assert m._lib.fpm_model_train_last(m._ctx, None, 0, 2, C.byref(added)) == L.FPM_E_INVALID_ARG
    for a, kq, flags in [(-1, 48, 0), (256, 48, 0), (8, -1, 0), (8, 256, 0), (8, 48, 2)]:
        assert m._lib.fpm_last_inspect(m._ctx, 0, a, kq, flags, None, 0, C.byref(n), None, 0, 0) == L.FPM_E_INVALID_ARG
    with pytest.raises(ValueError):
        m.last_inspect(0, k=16.0)
    assert m.model_info()[0] == 3
    # capacity of the record buffer: the count, FPM_E_CAPACITY, nothing written
    out = np.zeros(2, INSPECT_DTYPE)
    rc = m._lib.fpm_last_inspect(m._ctx, 0, 8, 48, 0, out.ctypes.data_as(C.POINTER(L.InspectStats)), 1, C.byref(n), None, 0, 0)
    assert rc == L.FPM_E_CAPACITY and n.value == 2 and out.tobytes() == bytes(out.nbytes)
    # excess images with strides: the bytes outside are left alone
    st, dense = m.last_inspect(0, 0, 0.5, image=True)
    assert dense.any()
    buf = np.full((2, th + 1, tw + 7), 0xA5, np.uint8)
    rc = m._lib.fpm_last_inspect(m._ctx, 0, 0, 8, 0, out.ctypes.data_as(C.POINTER(L.InspectStats)), 2, C.byref(n),
                                 L.u8ptr(buf), tw + 7, (tw + 7) * (th + 1))
    assert rc == L.FPM_OK and out.tobytes() == st.tobytes() and np.array_equal(buf[:, :th, :tw], dense)
    buf[:, :th, :tw] = 0xA5
    assert (buf == 0xA5).all()
    # while a search is in flight
    m.match_staged_launch()
    for call in (m.model_train_last, lambda: m.model_train_at(0, [(10.0, 10.0)], [0.0]), m.last_inspect, m.model_sums,
                 m.model_images, lambda: m.inspect_at(0, [(10.0, 10.0)], [0.0]), m.model_clear):
        with pytest.raises(ValueError, match="in flight"):
            call()
    assert _code(m.model_learn) == L.FPM_E_INVALID_ARG
    m.match_staged_finish_array()
    assert m.model_info()[0] == 3
    # restaging keeps the model (inspection then needs a search, inspect_at does not); the learn entries drop it
    m.stage([s])
    assert m.model_info()[0] == 3 and len(m.inspect_at(0, [(10.0, 10.0)], [5.0])) == 1
    with pytest.raises(ValueError, match="no search has run"):
        m.last_inspect()
    m.match_staged_candidates()                        # a search without results
    none, img = m.last_inspect(-1, image=True)
    assert none.shape == (0,) and none.dtype == INSPECT_DTYPE and img.shape == (0, th, tw)
    assert m.learnPattern(t)
    assert m.model_info() == (0, None)
    m.stage([s])
    m.model_train_at(0, [(10.0, 10.0)], [5.0])
    assert m.model_info()[0] == 1
    m.learn_at(0, (10.0, 10.0), 5.0)
    assert m.model_info() == (0, None)
    m.model_train_at(0, [(10.0, 10.0)], [5.0])
    m.clearPattern()
    assert m.model_info() == (0, None)


# ---- profile --------------------------------------------------------------------------------------------------------
def test_profile_counts_the_launches(hip, templates):
    s, t, prm = _scene(templates, "dst10_multi")
    th, tw = t.shape
    gpu, orc, _, _ = _run_both(hip, s, t, **prm)
    n = len(gpu)
    assert n >= 3
    px = tw * th
    hip.profile(True)
    try:
        hip.profile_reset()
        assert hip.model_train_last(0) == n
        ms, launches, nbytes = hip.model_profile(L.MODEL_TRAIN)
        assert launches == 1 and nbytes == n * px + 8 * px and ms > 0
        hip.model_train_last(0)
        assert hip.model_profile(L.MODEL_TRAIN)[1] == 2
        hip.last_inspect(0, 8, 3.0)
        hip.last_inspect(0, 8, 3.0, image=True)        # the same key: no second prepare
        assert hip.model_profile(L.MODEL_PREPARE)[1:] == (1, px * (8 + 3))
        ms, launches, nbytes = hip.model_profile(L.MODEL_INSPECT)
        assert launches == 2 and nbytes == (3 + 4) * n * px and ms > 0
        hip.model_images(8, 2.0)
        hip.model_images(8, 2.0)
        assert hip.model_profile(L.MODEL_PREPARE)[1] == 2   # a new (a, kq)
        hip.model_train_last(0)
        hip.model_images(8, 2.0)
        assert hip.model_profile(L.MODEL_PREPARE)[1] == 3   # new sums
        # none of these is a launch of the two existing patch kernels
        assert hip.profile_get(L.K_PATCH)[1] == 0 and hip.profile_get(L.K_COMPARE)[1] == 0
        # normalised: the sums launch of k_patch_compare first, then one launch of the model's kernel
        hip.profile_reset()
        hip.last_inspect(0, 8, 2.0, normalize=True)
        assert hip.model_profile(L.MODEL_INSPECT)[1] == 1 and hip.model_profile(L.MODEL_PREPARE)[1] == 0
        assert hip.profile_get(L.K_COMPARE)[1:] == (1, 2 * n * px) and hip.profile_get(L.K_PATCH)[1] == 0
        assert len(L.KERNEL_NAMES) == 15
    finally:
        hip.profile(False)
