"""Template masks on the HIP path (fpm_mask_* and the MASK forms of k_patch_compare, k_patch_align, k_model_inspect): the
tools that compare, align and inspect a hit run over the used pixels only.  The expectation is tests/mask_ref.py: the
oracle's warpAffine of fpm_patch_matrix's matrix, then the existing references with a masked pixel adding nothing.
Every comparison is ==.  Shapes: a tile is 64 x 16, a wave holds 4 of its rows, a lane 4 pixels; the templates 67 x 35
and 130 x 33 put a rectangle's edge in every position of those."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from fastest_image_pattern_matching_amd import synth
from fastest_image_pattern_matching_amd.matcher import MaskError
from tests import align_ref
from tests import blobs_ref
from tests import compare_ref
from tests import mask_ref as ref
from tests import model_ref

pytestmark = pytest.mark.gpu

SIZES = [(67, 35), (130, 33)]                  # (tw, th)
SW, SH = 203, 157
# inside; inside and rotated; across the source's left edge; wholly outside
POSES = [((40.0, 30.0), 0.0), ((52.25, 41.5), 30.0), ((-20.5, 60.25), -17.0), ((1000.0, 1000.0), 0.0)]
LTS, ANGS = [p[0] for p in POSES], [p[1] for p in POSES]


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


@functools.lru_cache(maxsize=None)
def scene(tw, th):
    rng = np.random.default_rng(tw * 1000 + th)
    src, t = rng.integers(0, 256, (SH, SW), dtype=np.uint8), rng.integers(0, 256, (th, tw), dtype=np.uint8)
    src.setflags(write=False)
    t.setflags(write=False)
    return src, t


def rects(tw, th):
    """None; every tx & 3; the widths around a lane group and a tile; the template's last column inside."""
    out = [None] + [(x, (x + 1) % 3, tw - 5, th - 4) for x in (0, 1, 2, 3)]
    out += [(2, 1, w, 17) for w in (1, 3, 4, 5, 63, 64, 65)]
    out += [(tw - 6, 3, 6, th - 3), (tw - 1, 0, 1, th)]
    return out


@functools.lru_cache(maxsize=None)
def masks(tw, th):
    """{name: uint8 (th, tw)}; nonzero = used."""
    rng = np.random.default_rng(tw + th)
    v, u = np.mgrid[0:th, 0:tw]
    m = {"ones": np.ones((th, tw), np.uint8), "zeros": np.zeros((th, tw), np.uint8)}
    m["corners"] = blobs_ref.tile_corners(tw, th)              # the four corners of every tile, the image's among them
    m["column"] = (u == 5).astype(np.uint8)
    m["row"] = (v == 17).astype(np.uint8)
    m["checker1"] = ((u + v) % 2).astype(np.uint8)
    m["checker4"] = ((u // 4 + v) % 2).astype(np.uint8)        # lane groups wholly on and wholly off
    m["tile_off"] = np.ones((th, tw), np.uint8)
    m["tile_off"][16:32, 0:64] = 0                             # exactly one tile
    m["wave_off"] = np.ones((th, tw), np.uint8)
    m["wave_off"][4:8, :] = 0                                  # exactly one wave's four rows
    for d in (0.05, 0.5, 0.95):
        m[f"random{d}"] = (rng.random((th, tw)) < d).astype(np.uint8)
    m["ellipse"] = ref.ellipse(tw, th, (tw - 1) / 2.0, (th - 1) / 2.0, 0.45 * tw, 0.45 * th).astype(np.uint8)
    m["bytes"] = rng.choice(np.array([0, 1, 128, 255], np.uint8), (th, tw))   # 1, 128 and 255 count alike
    for a in m.values():
        a.setflags(write=False)
    return m


MASK_NAMES = sorted(masks(*SIZES[0]))


@functools.lru_cache(maxsize=None)
def patches(tw, th, rect):
    """The patches of POSES for the rectangle, and the template crop: computed once, shared, left unchanged."""
    src, t = scene(tw, th)
    x, y, w, h = rect
    out = [align_ref.patch(src, rect, lt, a) for lt, a in POSES]
    return out, np.ascontiguousarray(t[y:y + h, x:x + w])


def full(rect, tw, th):
    return rect if rect is not None else (0, 0, tw, th)


def setup(hip, tw, th, mask=None):
    src, t = scene(tw, th)
    hip.resetParams()
    assert hip.learnPattern(t)
    hip.stage([src])
    if mask is not None:
        hip.set_mask(mask)
    return src, t


# ---- 1. comparison ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MASK_NAMES)
@pytest.mark.parametrize("size", SIZES)
def test_compare(hip, size, name):
    tw, th = size
    mask = masks(tw, th)[name]
    setup(hip, tw, th, mask)
    assert hip.mask_info() == (tw, th, int((mask != 0).sum()), True)
    for rect in rects(tw, th):
        fr = full(rect, tw, th)
        I, T = patches(tw, th, fr)
        m = ref.crop(mask, fr)
        assert hip.mask_count(rect) == int(m.sum())
        for norm in (False, True):
            exp = [ref.compare(i, T, m, 16, norm) for i in I]
            rows, diffs = [e[0] for e in exp], np.array([e[1] for e in exp], np.uint8)
            tag = f"{name} {rect} norm={norm}"
            got, img = hip.compare_at(0, LTS, ANGS, rect, threshold=16, normalize=norm, diff=True)
            compare_ref.assert_rows(got, rows, tag)
            assert np.array_equal(img, diffs), tag
            compare_ref.assert_rows(hip.compare_at(0, LTS, ANGS, rect, threshold=16, normalize=norm), rows, tag + " no diff")


# ---- 2. alignment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MASK_NAMES)
@pytest.mark.parametrize("size", SIZES)
def test_align_sums(hip, size, name):
    tw, th = size
    mask = masks(tw, th)[name]
    src, t = setup(hip, tw, th, mask)
    for rect in rects(tw, th):
        fr = full(rect, tw, th)
        I, T = patches(tw, th, fr)
        for norm in (False, True):
            exp = [ref.align_sums(i, t, fr, mask, ref.table(i, T, ref.crop(mask, fr)) if norm else None) for i in I]
            got = hip.align_sums_at(0, LTS, ANGS, rect, normalize=norm)
            align_ref.assert_rows(got, exp, align_ref.SUM_FIELDS, f"{name} {rect} norm={norm}")


LOOP_MASKS = ["ones", "zeros", "ellipse", "checker1", "checker4", "tile_off", "wave_off", "random0.05", "random0.5", "bytes"]


@pytest.mark.parametrize("name", LOOP_MASKS)
@pytest.mark.parametrize("size", SIZES)
def test_align_loop(hip, size, name):
    tw, th = size
    mask = masks(tw, th)[name]
    src, t = setup(hip, tw, th, mask)
    # the whole template, every tx & 3, a tile filled exactly and one column more, the template's last columns
    for rect in [None] + rects(tw, th)[1:5] + [(2, 1, 64, 17), (2, 1, 65, 17), (tw - 6, 3, 6, th - 3)]:
        fr = full(rect, tw, th)
        for norm in (False, True):
            exp = [ref.align_loop(src, t, fr, mask, lt, a, 3, 2.0, norm) for lt, a in POSES]
            got = hip.align_at(0, LTS, ANGS, rect, iters=3, normalize=norm)
            align_ref.assert_rows(got, exp, align_ref.RESULT_FIELDS, f"{name} {rect} norm={norm}")


# ---- a searched batch: the *_last entries and adopt -----------------------------------------------------------------------
def test_last_entries_and_adopt(hip, templates):
    t = templates["Dst10"]
    th, tw = t.shape
    hits = [[(80, 70, 25.0), (230, 160, -140.0)], [], [(160, 120, 61.0)]]        # tests/test_gpu_align.py's batch
    srcs = []
    for k, hs in enumerate(hits):
        s = synth.noise(320, 240, 128, 10, 300 + k)
        for cx, cy, a in hs:
            synth.paste_rotated(s, t, cx, cy, a)
        srcs.append(s)
    mask = ref.ellipse(tw, th, (tw - 1) / 2.0, (th - 1) / 2.0, 0.42 * tw, 0.42 * th).astype(np.uint8)
    hip.resetParams()
    hip._params.max_pos = 3
    hip._params.tolerance_angle = 180.0
    assert hip.learnPattern(t)
    hip.set_mask(mask)
    hip.stage(srcs)
    res = hip.match_staged()
    assert [len(r) for r in res] == [2, 0, 1]
    idx = [k for k in range(3) for _ in res[k]]
    ps = [(r.ptLT, r.dMatchedAngle) for k in range(3) for r in res[k]]
    fr = (0, 0, tw, th)
    m = ref.crop(mask, fr)

    def rows_at(poses, norm):
        return [ref.compare(align_ref.patch(srcs[i], fr, lt, a), t, m, 16, norm)[0] for i, (lt, a) in zip(idx, poses)]

    for norm in (False, True):
        compare_ref.assert_rows(hip.last_compare(-1, normalize=norm), rows_at(ps, norm), f"last_compare norm={norm}")
        got = hip.align_last(-1, normalize=norm)
        exp = [ref.align_loop(srcs[i], t, fr, mask, lt, a, 3, 2.0, norm) for i, (lt, a) in zip(idx, ps)]
        align_ref.assert_rows(got, exp, align_ref.RESULT_FIELDS, f"align_last norm={norm}")
    got = hip.align_last(-1, adopt=True)
    align_ref.assert_rows(got, [ref.align_loop(srcs[i], t, fr, mask, lt, a, 3) for i, (lt, a) in zip(idx, ps)],
                          align_ref.RESULT_FIELDS, "align_last adopt")
    assert (got["best_eval"] > 0).any(), "no hit moved: the test shows nothing"
    adopted = [((float(g["lt_x"]), float(g["lt_y"])), float(g["angle"])) for g in got]
    compare_ref.assert_rows(hip.last_compare(-1), rows_at(adopted, False), "last_compare at the adopted poses")
    # last_inspect / last_blobs at the adopted poses, against a model of the same hits
    assert hip.model_train_last(-1) == 3
    n, S, Q = model_ref.accumulate([align_ref.patch(srcs[i], fr, lt, a) for i, (lt, a) in zip(idx, adopted)])
    gs, gq = hip.model_sums()
    assert np.array_equal(gs, S) and np.array_equal(gq, Q)
    _, lo, hi = model_ref.derive_fast(n, S, Q, 2, model_ref.kq_of(1.0))
    exp = [ref.inspect(align_ref.patch(srcs[i], fr, lt, a), lo, hi, m) for i, (lt, a) in zip(idx, adopted)]
    st, img = hip.last_inspect(-1, 2, 1.0, image=True)
    model_ref.assert_rows(st, [e[0] for e in exp], "last_inspect")
    assert np.array_equal(img, np.array([e[1] for e in exp], np.uint8))
    summary, blobs = hip.last_blobs(-1, 2, 1.0, min_area=1)
    for i, e in enumerate(exp):
        _, recs, sm = blobs_ref.blobs(e[1], 0, 8, 1, 64, hit=i)
        assert blobs_ref.accept(summary[i], blobs[i], recs, sm, 64) is None, i


# ---- planted truth: an elliptic part on a foreign background --------------------------------------------------------------
def test_planted_scene(hip):
    """DESIGN.md section 22's planted scene on the device: the rows == the masked loop, the masked error within twice the
    largest the reference reaches, and the inspection clean under the mask only."""
    mask, scenes = ref.planted()
    bound = 2.0 * max(e[2] for e in ref.planted_alignments())
    part = align_ref.smooth_scene(seed=13)
    for k, (sc, t, lt, a) in enumerate(scenes):
        hip.resetParams()
        assert hip.learnPattern(t)
        hip.set_mask(mask)
        # one model sample of the template frame from the seed-13 scene (trained under the mask: the planes ignore it)
        hip.stage([part])
        hip.model_clear()
        hip.model_train_at(0, [lt], [a])
        S, Q = hip.model_sums()
        taught = align_ref.patch(part, ref.PLANT_RECT, lt, a).astype(np.uint32)
        assert np.array_equal(S, taught) and np.array_equal(Q, taught * taught)
        hip.stage([sc])
        truth = align_ref.centre(sc.shape, ref.PLANT_RECT, lt, a)
        starts = align_ref.starts(lt, a)
        slts, sangs = [p[0] for p in starts], [p[1] for p in starts]

        def err(r):
            return float(np.hypot(*(align_ref.centre(sc.shape, ref.PLANT_RECT, (r["lt_x"], r["lt_y"]), r["angle"]) - truth)))

        got = hip.align_at(0, slts, sangs)
        align_ref.assert_rows(got, [ref.align_loop(sc, t, ref.PLANT_RECT, mask, l, g, 3) for l, g in starts],
                              align_ref.RESULT_FIELDS, f"scene {k} masked")
        hip.mask_enable(False)
        un = hip.align_at(0, slts, sangs)
        align_ref.assert_rows(un, [align_ref.loop(sc, t, ref.PLANT_RECT, l, g, 3) for l, g in starts], align_ref.RESULT_FIELDS,
                              f"scene {k} unmasked")
        for i, (l, g) in enumerate(starts):
            e0 = float(np.hypot(*(align_ref.centre(sc.shape, ref.PLANT_RECT, l, g) - truth)))
            print(f"scene {k} start {i}: {e0:.4f} px, unmasked {err(un[i]):.4f} px, masked {err(got[i]):.4f} px (bound {bound:.4f})")
            assert err(got[i]) < e0 and err(got[i]) < err(un[i]) and err(got[i]) <= bound
        # inspection at the planted pose: the foreign background is a defect without the mask, and none with it
        st = hip.inspect_at(0, [lt], [a])[0]
        assert st["n_low"] + st["n_high"] > 0 and st["n"] == align_ref.TW * align_ref.TH
        assert ref.box_reaches_a_corner(st, align_ref.TW, align_ref.TH), st     # a corner pixel of the frame is in the box
        assert hip.blobs_at(0, [lt], [a], min_area=1)[0]["n_blobs"][0] > 0
        hip.mask_enable(True)
        st = hip.inspect_at(0, [lt], [a])[0]
        assert st["n_low"] + st["n_high"] == 0 and st["n"] == int(mask.sum())
        summary, blobs = hip.blobs_at(0, [lt], [a], min_area=1)
        assert summary["n_blobs"][0] == 0 and summary["fg_pixels"][0] == 0 and len(blobs[0]) == 0


# ---- 3. inspection, blobs, normalised training -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bands(tw, th, rect):
    """(n, S, Q, lo, hi) of the unnormalised model of POSES over the rectangle, a = 8, k = 3."""
    I, _ = patches(tw, th, rect)
    n, S, Q = model_ref.accumulate(I)
    _, lo, hi = model_ref.derive_fast(n, S, Q, 8, model_ref.kq_of(3.0))
    return n, S, Q, lo, hi


@pytest.mark.parametrize("name", MASK_NAMES)
@pytest.mark.parametrize("size", SIZES)
def test_inspect_and_blobs(hip, size, name):
    tw, th = size
    mask = masks(tw, th)[name]
    src, t = setup(hip, tw, th, mask)
    # inspected poses: the trained ones moved a little, so that pixels leave their bands
    lts2 = [(lt[0] + 0.5, lt[1] - 0.25) for lt in LTS]
    for rect in rects(tw, th):
        fr = full(rect, tw, th)
        x, y, w, h = fr
        n, S, Q, lo, hi = bands(tw, th, fr)
        hip.model_clear()
        assert hip.model_train_at(0, LTS, ANGS, rect) == n
        gs, gq = hip.model_sums()
        assert np.array_equal(gs, S) and np.array_equal(gq, Q), f"{name} {rect}: the planes take every pixel"
        m = ref.crop(mask, fr)
        T = np.ascontiguousarray(t[y:y + h, x:x + w])
        I2 = [align_ref.patch(src, fr, lt, a) for lt, a in zip(lts2, ANGS)]
        for norm in (False, True):
            smp = [ref.sample(i, T, m, norm) for i in I2]
            exp = [ref.inspect(v, lo, hi, m, g, o) for v, g, o in smp]
            rows, imgs = [e[0] for e in exp], np.array([e[1] for e in exp], np.uint8)
            tag = f"{name} {rect} norm={norm}"
            st, img = hip.inspect_at(0, lts2, ANGS, 8, 3.0, normalize=norm, image=True)
            model_ref.assert_rows(st, rows, tag)
            assert np.array_equal(img, imgs), tag
            model_ref.assert_rows(hip.inspect_at(0, lts2, ANGS, 8, 3.0, normalize=norm), rows, tag + " no image")
            summary, blobs, st2 = hip.blobs_at(0, lts2, ANGS, 8, 3.0, normalize=norm, min_area=1, cap=64, stats=True)
            assert st2.tobytes() == st.tobytes()
            for i, e in enumerate(imgs):
                _, recs, s = blobs_ref.blobs(e, 0, 8, 1, 64, hit=i)
                why = blobs_ref.accept(summary[i], blobs[i], recs, s, 64)
                assert why is None, (tag, i, why)


@pytest.mark.parametrize("name", ["ellipse", "random0.5", "zeros"])
def test_normalised_training_uses_the_masked_tables(hip, name):
    tw, th = SIZES[1]
    mask = masks(tw, th)[name]
    src, t = setup(hip, tw, th, mask)
    for rect in (None, (3, 1, 70, 20)):
        fr = full(rect, tw, th)
        I, T = patches(tw, th, fr)
        m = ref.crop(mask, fr)
        n, S, Q = model_ref.accumulate([ref.sample(i, T, m, True)[0] for i in I])
        hip.model_clear()
        assert hip.model_train_at(0, LTS, ANGS, rect, normalize=True) == n
        gs, gq = hip.model_sums()
        assert np.array_equal(gs, S) and np.array_equal(gq, Q), (name, rect)


# ---- 4. all ones, disabled, cleared: today's bytes ---------------------------------------------------------------------------
def _all_outputs(hip, rect):
    out = []
    for norm in (False, True):
        st, img = hip.compare_at(0, LTS, ANGS, rect, normalize=norm, diff=True)
        out += [st.tobytes(), img.tobytes(), hip.align_sums_at(0, LTS, ANGS, rect, normalize=norm).tobytes(),
                hip.align_at(0, LTS, ANGS, rect, iters=2, normalize=norm).tobytes()]
        hip.model_clear()
        hip.model_train_at(0, LTS, ANGS, rect, normalize=norm)
        out += [a.tobytes() for a in hip.model_sums()]
        st, img = hip.inspect_at(0, [(lt[0] + 0.5, lt[1]) for lt in LTS], ANGS, normalize=norm, image=True)
        out += [st.tobytes(), img.tobytes()]
        # capacity for every component an image of this size can hold: of a truncated hit ANY cap records may come back
        summary, blobs = hip.blobs_at(0, [(lt[0] + 0.5, lt[1]) for lt in LTS], ANGS, normalize=norm, min_area=1, cap=2048)
        assert not summary["flags"].any()
        out += [summary.tobytes()] + [b.tobytes() for b in blobs]
    return out


def _launches(hip):
    return (hip.profile_get(L.K_COMPARE)[1], hip.model_profile(L.MODEL_TRAIN)[1], hip.model_profile(L.MODEL_INSPECT)[1],
            hip.align_profile()[1])


@pytest.mark.parametrize("size", SIZES)
def test_all_ones_disabled_and_cleared_change_nothing(hip, size):
    tw, th = size
    setup(hip, tw, th)
    for rect in (None, (3, 2, tw - 5, th - 4)):
        hip.clear_mask()
        hip.profile(True)
        try:
            hip.profile_reset()
            plain = _all_outputs(hip, rect)
            n_plain = _launches(hip)
            hip.set_mask(masks(tw, th)["ones"])
            hip.profile_reset()
            assert _all_outputs(hip, rect) == plain, "all ones"
            assert _launches(hip) == n_plain and min(n_plain) > 0
        finally:
            hip.profile(False)
        hip.set_mask(masks(tw, th)["random0.5"])
        assert _all_outputs(hip, rect) != plain
        hip.mask_enable(False)
        assert hip.mask_info() == (tw, th, int(masks(tw, th)["random0.5"].sum()), False)
        assert _all_outputs(hip, rect) == plain, "disabled"
        hip.mask_enable(True)
        assert _all_outputs(hip, rect) != plain
        hip.clear_mask()
        assert hip.mask_info() == (0, 0, 0, False) and hip.mask() is None
        assert _all_outputs(hip, rect) == plain, "cleared"


# ---- 5. nothing used ------------------------------------------------------------------------------------------------------
def test_no_used_pixel(hip):
    tw, th = SIZES[0]
    mask = np.array(masks(tw, th)["ones"])
    miss = (8, 4, 21, 9)
    mask[4:13, 8:29] = 0
    for m_, rect in ((masks(tw, th)["zeros"], None), (mask, miss)):
        setup(hip, tw, th, m_)
        x, y, w, h = full(rect, tw, th)
        assert hip.mask_count(rect) == 0
        for norm in (False, True):
            st, img = hip.compare_at(0, LTS, ANGS, rect, threshold=0, normalize=norm, diff=True)
            for f in compare_ref.FIELDS:
                want = {"x0": w, "y0": h, "x1": -1, "y1": -1, "gain": 1.0}.get(f, 0)
                assert (st[f] == want).all(), (f, st[f])
            assert not img.any()
            al = hip.align_at(0, LTS, ANGS, rect, normalize=norm)
            assert (al["flags"] == L.ALIGN_SINGULAR | L.ALIGN_KEPT_START).all() and (al["n_used"] == 0).all()
            assert al["lt_x"].tobytes() == np.float32([p[0] for p in LTS]).tobytes()
            assert al["lt_y"].tobytes() == np.float32([p[1] for p in LTS]).tobytes()
            assert al["angle"].tobytes() == np.float64(ANGS).tobytes() and (al["evals"] == 1).all()
            assert not any(hip.align_sums_at(0, LTS, ANGS, rect, normalize=norm)[f].any() for f in align_ref.SUM_FIELDS)
            hip.model_clear()
            hip.model_train_at(0, LTS[:1], ANGS[:1], rect, normalize=norm)
            ins, img = hip.inspect_at(0, LTS, ANGS, 0, 0.0, normalize=norm, image=True)
            for f in model_ref.FIELDS:
                want = {"x0": w, "y0": h, "x1": -1, "y1": -1, "gain": 1.0}.get(f, 0)
                assert (ins[f] == want).all(), (f, ins[f])
            assert not img.any()
    # a normalised training under no used pixel goes through the identity table: the pixels as sampled
    I, _ = patches(tw, th, miss)
    assert np.array_equal(hip.model_sums()[0], I[0].astype(np.uint32))


# ---- views, storage, counts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_device_views_equal_the_host_mask(hip, size):
    tw, th = size
    setup(hip, tw, th)
    mask = masks(tw, th)["bytes"]
    stored = ((mask != 0) * 255).astype(np.uint8)
    hip.set_mask(mask)
    assert np.array_equal(hip.mask(), stored) and hip.mask().dtype == np.uint8
    want = hip.compare_at(0, LTS, ANGS, normalize=True).tobytes()
    stride = tw + 8 + (tw % 2 == 0)                                         # odd
    for off in (1, 2, 3):
        buf = torch.full((off + th * stride + 64,), 77, dtype=torch.uint8, device="cuda")   # non-zero around the view
        view = torch.as_strided(buf, (th, tw), (stride, 1), off)
        view.copy_(torch.from_numpy(np.array(mask)).cuda())
        assert view.data_ptr() % 4 == off and stride % 2 == 1
        hip.clear_mask()
        hip.set_mask(view)
        assert np.array_equal(hip.mask(), stored), off
        assert hip.mask_info() == (tw, th, int((mask != 0).sum()), True)
        assert hip.compare_at(0, LTS, ANGS, normalize=True).tobytes() == want
    # bool tensors and arrays, and a host view with a wide row
    hip.set_mask(torch.from_numpy(mask != 0).cuda())
    assert np.array_equal(hip.mask(), stored)
    wide = np.full((th, tw + 13), 9, np.uint8)
    wide[:, 5:5 + tw] = mask
    hip.set_mask(wide[:, 5:5 + tw])
    assert np.array_equal(hip.mask(), stored)
    hip.set_mask(mask != 0)
    assert np.array_equal(hip.mask(), stored)
    for rect in [None, (0, 0, 1, 1), (3, 2, 40, 20), (tw - 1, th - 1, 1, 1), (1, 0, tw - 1, th)]:
        x, y, w, h = full(rect, tw, th)
        assert hip.mask_count(rect) == int((mask[y:y + h, x:x + w] != 0).sum()), rect


# ---- 6. lifetime --------------------------------------------------------------------------------------------------------------
def _search_outputs(hip):
    res = [[r.as_tuple() for r in s] for s in hip.match_staged()]
    cal = M.caliper(20.0, 15.0, 10.0, 30, 8)
    summary, edges = hip.last_calipers([cal], -1)
    return res, hip.last_patches(-1)[0].tobytes(), summary.tobytes(), edges.tobytes()


def test_lifetime(hip, templates):
    t = templates["Dst10"]
    th, tw = t.shape
    srcs = []
    for k, (cx, cy, a) in enumerate([(150, 140, 33.0), (200, 180, -120.0)]):
        s = synth.noise(400, 320, 128, 10, 40 + k)
        synth.paste_rotated(s, t, cx, cy, a)
        srcs.append(s)
    mask = ref.ellipse(tw, th, tw / 2.0, th / 2.0, 0.4 * tw, 0.4 * th).astype(np.uint8)
    stored = mask * np.uint8(255)

    def fresh():
        hip.resetParams()
        hip._params.max_pos = 1
        hip._params.tolerance_angle = 180.0
        assert hip.learnPattern(t)
        hip.stage(srcs)

    fresh()
    plain = _search_outputs(hip)
    assert all(len(r) == 1 for r in plain[0])
    hip.set_mask(mask)
    # staging, a search, the model's clearing and an alignment keep the mask; the search and the tools that do not honour it
    # give the same bytes with it
    hip.stage(srcs)
    assert _search_outputs(hip) == plain
    hip.model_clear()
    hip.align_last(-1, adopt=True)
    hip.stage_device([torch.from_numpy(s).cuda() for s in srcs])
    assert np.array_equal(hip.mask(), stored) and hip.mask_info()[3]
    # fpm_model_learn crops the mask to the model's rectangle
    rect = (5, 3, tw - 11, th - 7)
    hip.match_staged()
    assert hip.model_train_last(-1, rect) == 2
    hip.mask_enable(False)
    hip.model_learn()
    x, y, w, h = rect
    assert np.array_equal(hip.mask(), stored[y:y + h, x:x + w]) and hip.mask_info() == (w, h, int(mask[y:y + h, x:x + w].sum()), False)
    hip.mask_enable(True)
    assert hip.mask_count() == int(mask[y:y + h, x:x + w].sum())
    hip.stage(srcs)
    st = hip.compare_at([0], [(100.0, 100.0)], [0.0])
    assert st["n"][0] == hip.mask_count()
    # every learn entry drops it
    pose = ((100.0, 100.0), 10.0)
    dt = torch.from_numpy(np.ascontiguousarray(t)).cuda()
    for learn in (lambda: hip.learnPattern(t), lambda: hip.learn_device(dt), lambda: hip.learn_at(0, pose[0], pose[1]),
                  lambda: hip.learn_hit(0, 0), lambda: hip.clearPattern()):
        fresh()
        hip.match_staged()
        hip.set_mask(mask)
        assert hip.mask_info()[:2] == (tw, th)
        learn()
        assert hip.mask_info() == (0, 0, 0, False)


# ---- 7. argument and state errors ------------------------------------------------------------------------------------------
def test_errors_leave_the_previous_mask(gpu_matcher_factory):
    m = gpu_matcher_factory()
    tw, th = SIZES[0]
    src, t = scene(tw, th)
    mask = np.array(masks(tw, th)["ellipse"])
    p8 = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    n64, out = C.c_int64(-5), np.full((th, tw), 3, np.uint8)
    # no template
    assert m._lib.fpm_mask_set(m._ctx, p8, tw, th, tw) == L.FPM_E_NOT_LEARNED
    assert m._lib.fpm_mask_enable(m._ctx, 1) == L.FPM_E_NOT_LEARNED
    assert m._lib.fpm_mask_count(m._ctx, None, C.byref(n64)) == L.FPM_E_NOT_LEARNED and n64.value == -5
    with pytest.raises(MaskError) as e:
        m.set_mask(mask)
    assert e.value.code == L.FPM_E_NOT_LEARNED and m.mask_info() == (0, 0, 0, False)
    assert m.learnPattern(t)
    m.stage([src])
    # get / enable / count without a mask
    for call in (lambda: m.mask_enable(True), lambda: m.mask_count(), lambda: m.mask_count((0, 0, 2, 2))):
        with pytest.raises(MaskError) as e:
            call()
        assert e.value.code == L.FPM_E_INVALID_ARG
    assert m._lib.fpm_mask_get(m._ctx, L.u8ptr(out), tw) == L.FPM_E_INVALID_ARG and (out == 3).all()
    m.clear_mask()                                   # clearing nothing is fine
    m.set_mask(mask)
    before = (m.mask().tobytes(), m.mask_info(), m.compare_at(0, LTS, ANGS).tobytes())

    def intact():
        return (m.mask().tobytes(), m.mask_info(), m.compare_at(0, LTS, ANGS).tobytes()) == before

    other = np.ones((th + 1, tw + 1), np.uint8)
    dmask = torch.from_numpy(other).cuda()
    host = np.ones((th, tw), np.uint8)
    bad = [lambda: m._lib.fpm_mask_set(m._ctx, L.u8ptr(other), tw + 1, th, tw + 1),            # wrong size
           lambda: m._lib.fpm_mask_set(m._ctx, L.u8ptr(other), tw, th + 1, tw + 1),
           lambda: m._lib.fpm_mask_set(m._ctx, L.u8ptr(other), tw, th, tw - 1),                # stride below the width
           lambda: m._lib.fpm_mask_set(m._ctx, None, tw, th, tw),                              # null pointer
           lambda: m._lib.fpm_mask_set_device(m._ctx, None, tw, th, tw, None),
           lambda: m._lib.fpm_mask_set_device(m._ctx, dmask.data_ptr(), tw + 1, th + 1, tw + 1, None),
           lambda: m._lib.fpm_mask_set_device(m._ctx, dmask.data_ptr(), tw, th, tw - 1, None),
           lambda: m._lib.fpm_mask_set_device(m._ctx, host.ctypes.data, tw, th, tw, None),     # a host pointer
           lambda: m._lib.fpm_mask_get(m._ctx, None, tw),
           lambda: m._lib.fpm_mask_get(m._ctx, L.u8ptr(out), tw - 1),
           lambda: m._lib.fpm_mask_count(m._ctx, C.byref(L.PatchRect(1, 1, tw, th)), C.byref(n64)),
           lambda: m._lib.fpm_mask_count(m._ctx, None, None)]
    for k, call in enumerate(bad):
        assert call() == L.FPM_E_INVALID_ARG, k
        assert intact() and n64.value == -5 and (out == 3).all(), k
    for call in (lambda: m.set_mask(other), lambda: m.set_mask(dmask), lambda: m.mask_count((0, 0, tw + 1, 1))):
        with pytest.raises(MaskError) as e:
            call()
        assert e.value.code == L.FPM_E_INVALID_ARG and intact()
    with pytest.raises(TypeError):
        m.set_mask(np.ones((th, tw), np.float32))
    # a search in flight
    m.match_staged_launch()
    try:
        calls = [lambda: m._lib.fpm_mask_set(m._ctx, p8, tw, th, tw), lambda: m._lib.fpm_mask_clear(m._ctx),
                 lambda: m._lib.fpm_mask_enable(m._ctx, 0), lambda: m._lib.fpm_mask_get(m._ctx, L.u8ptr(out), tw),
                 lambda: m._lib.fpm_mask_count(m._ctx, None, C.byref(n64)),
                 lambda: m._lib.fpm_mask_set_device(m._ctx, dmask.data_ptr(), tw, th, tw, None)]
        for k, call in enumerate(calls):
            assert call() == L.FPM_E_INVALID_ARG and "in flight" in m.last_error(), k
        assert m.mask_info() == before[1]
    finally:
        m.match_staged_finish_array()
    assert intact() and n64.value == -5 and (out == 3).all()
    assert m._lib.fpm_mask_info(None, None, None, None, None) == L.FPM_E_INVALID_ARG


# ---- 8. determinism -----------------------------------------------------------------------------------------------------------
def test_job_order_does_not_matter(hip):
    tw, th = SIZES[1]
    setup(hip, tw, th, masks(tw, th)["random0.5"])
    rng = np.random.default_rng(5)
    k = 24
    lts = [(float(x), float(y)) for x, y in rng.uniform(-20.0, 120.0, (k, 2))]
    angs = [float(a) for a in rng.uniform(-180.0, 180.0, k)]
    hip.model_clear()
    hip.model_train_at(0, lts[:4], angs[:4])
    perm = rng.permutation(k)

    def run(order):
        l, a = [lts[i] for i in order], [angs[i] for i in order]
        out = []
        for norm in (False, True):
            st, img = hip.compare_at(0, l, a, normalize=norm, diff=True)
            ins, e = hip.inspect_at(0, l, a, normalize=norm, image=True)
            out += [st, img, hip.align_sums_at(0, l, a, normalize=norm), hip.align_at(0, l, a, iters=2, normalize=norm), ins, e]
        return out

    first, again, shuffled = run(range(k)), run(range(k)), run(perm)
    for a, b, c in zip(first, again, shuffled):
        assert a.tobytes() == b.tobytes()
        assert a[perm].tobytes() == c.tobytes()
