"""Learning on the device (fpm_learn_device / fpm_learn_at / fpm_learn_hit, k_tmpl_prep): a context that learns through
a new entry against a fresh context that learns the same pixels through fpm_learn -- the template's levels, statistics
and matrix-core operands byte for byte and bit for bit -- then searches with the learned template, the staged sources
that survive a device learn, and the state rules.  Every comparison is equality."""
import numpy as np
import pytest
import torch   # at collection time, before any test loads libfpm_hip.so: one HIP runtime for both (_lib.hip_runtimes)

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import images, synth
from fastest_image_pattern_matching_amd.matcher import LearnError
from tests import oracle

pytestmark = pytest.mark.gpu

SEMANTICS_MFC = 1   # FPM_SEMANTICS_MFC (include/fpm.h)
# (w, h): one pixel, narrower than a dword, one and two MFMA row chunks, operand rows of one, exactly one and two 64-byte
# blocks, several workgroups per level, odd level sizes down the pyramid
SIZES = [(1, 1), (3, 5), (17, 16), (63, 33), (64, 64), (65, 17), (130, 47), (257, 31), (200, 150)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def snapshot(m):
    """Everything a learned template is: fpm_template_info, every level (size, pixels, the three doubles as bit patterns,
    vecResultEqual1) and both operand arrays as they lie in device memory."""
    n, border = m.template_info()
    levels = []
    for l in range(n):
        px, mean, norm, inv_area, equal1 = m.template_level(l)
        levels.append((px.shape, px.tobytes(), float(mean).hex(), float(norm).hex(), float(inv_area).hex(), equal1))
    t8, tsum = m.template_operands()
    return {"info": (n, border), "levels": levels, "t8": t8.tobytes(), "tsum": tsum.tobytes()}


def assert_same_template(a, b, label):
    assert a["info"] == b["info"], (label, a["info"], b["info"])
    for l, (x, y) in enumerate(zip(a["levels"], b["levels"])):
        assert x[0] == y[0], (label, l, x[0], y[0])
        assert x[1] == y[1], f"{label}: level {l} pixels differ"
        assert x[2:] == y[2:], (label, l, x[2:], y[2:])
    assert len(a["t8"]) == len(b["t8"]) and len(a["tsum"]) == len(b["tsum"]), label
    if a["t8"] != b["t8"]:
        x, y = np.frombuffer(a["t8"], np.int8), np.frombuffer(b["t8"], np.int8)
        bad = np.flatnonzero(x != y)
        pytest.fail(f"{label}: operand slab differs at {len(bad)} of {len(x)} bytes, first at {bad[0]}")
    assert a["tsum"] == b["tsum"], f"{label}: row sums differ"


def host_learned(factory, px, **prm):
    """A fresh context that learns `px` through fpm_learn: the yardstick."""
    m = factory(**prm)
    assert m.learnPattern(np.ascontiguousarray(px))
    return m


# ---- operand parity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mra", [256, 64])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_operand_parity(gpu_matcher_factory, size, mra):
    w, h = size
    px = _noise(w, h, 1000 * w + h + mra)
    a = gpu_matcher_factory(min_reduce_area=mra)
    a.learn_device(_dev(px))
    assert a.isPatternLearned()
    b = host_learned(gpu_matcher_factory, px, min_reduce_area=mra)
    sa = snapshot(a)
    assert sa["levels"][0][:2] == ((h, w), px.tobytes())
    assert_same_template(sa, snapshot(b), f"{w}x{h} mra {mra}")


@pytest.mark.parametrize("value", [0, 77, 255])
def test_constant_image(gpu_matcher_factory, value):
    px = np.full((40, 50), value, np.uint8)
    a = gpu_matcher_factory(min_reduce_area=64)
    a.learn_device(_dev(px))
    sa = snapshot(a)
    assert all(lv[5] for lv in sa["levels"]) and sa["info"][1] == (255 if value < 128 else 0)
    assert_same_template(sa, snapshot(host_learned(gpu_matcher_factory, px, min_reduce_area=64)), f"constant {value}")


def test_no_stale_bytes_after_a_larger_template(gpu_matcher_factory):
    """The buffers are reused: a smaller template learned after a larger one leaves nothing of it in the padding, in the
    rows past the template or in the slack the correlation kernel prefetches."""
    a = gpu_matcher_factory(min_reduce_area=64)
    a.learn_device(_dev(_noise(130, 47, 5)))
    small = _noise(17, 16, 6)
    a.learn_device(_dev(small))
    assert_same_template(snapshot(a), snapshot(host_learned(gpu_matcher_factory, small, min_reduce_area=64)), "17x16 after 130x47")
    # and the other way round, on the same context: the buffers grow
    big = _noise(200, 150, 7)
    a.learn_device(_dev(big))
    assert_same_template(snapshot(a), snapshot(host_learned(gpu_matcher_factory, big, min_reduce_area=64)), "200x150 after 17x16")


def test_profile_counts_one_launch(gpu_matcher_factory):
    w, h = 130, 47
    a = gpu_matcher_factory()
    a.profile(True)
    a.profile_reset()
    a.learn_device(_dev(_noise(w, h, 8)))
    ms, launches, nbytes = a.profile_get(L.K_LEARN)
    # 130 x 47 at min_reduce_area 256 (getTopLayer: 6110 -> 1527 -> 381 -> 95 <= 256): four levels; per level the pixels
    # read, the operand rows of 64 * ceil(w / 64) bytes over round_up(h, 16) rows and one i32 per such row, then the 256
    # bytes of slack
    levels = [(130, 47, 48), (65, 24, 32), (33, 12, 16), (17, 6, 16)]
    exp = sum(lw * lh + 64 * ((lw + 63) // 64) * r + 4 * r for lw, lh, r in levels) + 256
    assert a.template_info()[0] == 4 and launches == 1 and nbytes == exp and ms > 0
    assert a.profile_get(L.K_PATCH)[1] == 0 and a.profile_get(L.K_PYR)[1] == 0   # events bracket only the new kernel


# ---- formats --------------------------------------------------------------------------------------------------------
def test_gray_view_with_odd_stride_and_unaligned_base(gpu_matcher_factory):
    w, h = 63, 33
    big = _dev(_noise(w + 38, h + 2, 9))            # row stride 101 bytes
    view = big[1:1 + h, 3:3 + w]
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 != 0
    a = gpu_matcher_factory()
    a.learn_device(view)
    assert_same_template(snapshot(a), snapshot(host_learned(gpu_matcher_factory, view.cpu().numpy())), "gray view")


@pytest.mark.parametrize("fmt", ["bgr_interleaved", "rgb_planar"])
def test_colour_formats(gpu_matcher_factory, fmt):
    rgb = np.random.default_rng(10).integers(0, 256, (47, 130, 3), dtype=np.uint8)   # (H, W, 3), R G B
    a = gpu_matcher_factory()
    if fmt == "bgr_interleaved":
        a.learn_device(_dev(rgb[..., ::-1]), channel_order="bgr")
    else:
        a.learn_device(_dev(rgb.transpose(2, 0, 1)), channel_order="rgb", layout="chw")
    gray = images.bgr_to_gray(rgb)
    assert_same_template(snapshot(a), snapshot(host_learned(gpu_matcher_factory, gray)), fmt)


# ---- search ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(templates):
    """The smoke scene: Dst10 pasted at two angles into 480 x 360 noise."""
    t = templates["Dst10"]
    s = synth.noise(480, 360, 128, 10, 2024)
    synth.paste_rotated(s, t, 150, 140, 33.0)
    synth.paste_rotated(s, t, 330, 230, -120.0)
    return t, s


def _tuples(res):
    return [r.as_tuple() for r in res]


def test_search_with_a_device_learned_template(gpu_matcher_factory, scene):
    t, s = scene
    prm = dict(max_pos=2, tolerance_angle=180.0)
    a = gpu_matcher_factory(**prm)
    a.learn_device(_dev(t))
    b = host_learned(gpu_matcher_factory, t, **prm)
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    got, ref, exp = _tuples(a.match(s)), _tuples(b.match(s)), o.match(s)
    assert len(exp) == 2 and got == ref and got == exp
    assert a.last_candidates(0).tobytes() == b.last_candidates(0).tobytes()


# ---- learn_at -------------------------------------------------------------------------------------------------------
def test_learn_at_equals_the_patch(gpu_matcher_factory, scene):
    t, s = scene
    th, tw = t.shape
    prm = dict(max_pos=2, tolerance_angle=180.0)
    a = gpu_matcher_factory(**prm)
    assert a.learnPattern(t)
    a.stage([s])
    lt, angle, rect = (101.25, 87.5), 33.0, (-3, -3, tw + 6, th + 6)
    patch = a.patches_at(0, [lt], [angle], rect)[0]
    assert patch.shape == (th + 6, tw + 6) and patch.std() > 0
    a.learn_at(0, lt, angle, rect)
    sa = snapshot(a)
    assert sa["levels"][0][:2] == (patch.shape, patch.tobytes())
    assert_same_template(sa, snapshot(host_learned(gpu_matcher_factory, patch, **prm)), "learn_at 33 degrees")
    # the sources are still staged (same top layer): an upright integer pose is the numpy crop
    x, y, w, h = 40, 25, 71, 50
    a.learn_at(0, (float(x), float(y)), 0.0, (0, 0, w, h))
    crop = np.ascontiguousarray(s[y:y + h, x:x + w])
    sa = snapshot(a)
    assert sa["levels"][0][:2] == ((h, w), crop.tobytes())
    assert_same_template(sa, snapshot(host_learned(gpu_matcher_factory, crop, **prm)), "learn_at crop")
    # 71 x 50 has Dst10's top layer too: rect None is now the new template's frame, on the sources staged at the start
    assert a.patches_at(0, [(float(x), float(y))], [0.0])[0].tobytes() == crop.tobytes()


def test_learn_at_through_the_warp_form(gpu_matcher_factory, scene):
    t, s = scene
    th, tw = t.shape
    a = gpu_matcher_factory()
    assert a.learnPattern(t)
    a.stage([s])
    a.setPatchForm(L.PATCH_FORM_WARP)
    lt, angle, rect = (200.5, 150.75), -120.0, (-3, -3, tw + 6, th + 6)
    patch = a.patches_at(0, [lt], [angle], rect)[0]
    a.learn_at(0, lt, angle, rect)
    assert_same_template(snapshot(a), snapshot(host_learned(gpu_matcher_factory, patch)), "learn_at, k_warp form")


# ---- learn_hit ------------------------------------------------------------------------------------------------------
def test_learn_hit_then_search_without_restaging(gpu_matcher_factory, scene):
    t, s = scene
    prm = dict(max_pos=2, tolerance_angle=180.0, semantics=SEMANTICS_MFC, subpixel=1)
    a = gpu_matcher_factory(**prm)
    assert a.learnPattern(t)
    a.stage([s])
    first = a.match_staged()[0]
    assert len(first) == 2
    patch = a.last_patches(0)[0]             # at the raw pose: not the converted result's under MFC semantics
    a.learn_hit(0)
    sa = snapshot(a)
    assert sa["levels"][0][:2] == (t.shape, patch.tobytes()) and patch.tobytes() != t.tobytes()
    b = host_learned(gpu_matcher_factory, patch, **prm)
    assert_same_template(sa, snapshot(b), "learn_hit")
    # the same template size: the sources stayed staged; the plan and the captured graph are rebuilt for the new template
    again = a.match_staged()[0]
    b.stage([s])
    ref = b.match_staged()[0]
    assert len(ref) >= 1 and _tuples(again) == _tuples(ref)
    assert _tuples(again) != _tuples(first)   # the new template's scores, not the old plan's
    assert a.last_candidates(0).tobytes() == b.last_candidates(0).tobytes()
    # patches and comparisons work on the kept sources too
    assert a.last_patches(0).tobytes() == b.last_patches(0).tobytes()
    assert a.last_compare(0).tobytes() == b.last_compare(0).tobytes()


# ---- state ----------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LearnError) as e:
        call()
    return e.value.code


def test_state_rules(gpu_matcher_factory, scene):
    t, s = scene
    th, tw = t.shape
    prm = dict(max_pos=2, tolerance_angle=180.0)
    m = gpu_matcher_factory(**prm)
    dt = _dev(t)
    # no template: the frame of the template learned now does not exist
    assert _code(lambda: m.learn_at(0, (10.0, 10.0), 0.0)) == L.FPM_E_NOT_LEARNED
    assert m.learnPattern(t)
    # nothing staged
    assert _code(lambda: m.learn_at(0, (10.0, 10.0), 0.0)) == L.FPM_E_INVALID_ARG
    assert _code(lambda: m.learn_hit(0)) == L.FPM_E_INVALID_ARG
    m.stage([s])
    assert _code(lambda: m.learn_hit(0)) == L.FPM_E_INVALID_ARG            # staged, not searched
    assert _code(lambda: m.learn_at(1, (10.0, 10.0), 0.0)) == L.FPM_E_INVALID_ARG   # source past the batch
    assert _code(lambda: m.learn_at(0, (float("nan"), 10.0), 0.0)) == L.FPM_E_INVALID_ARG
    before = snapshot(m)
    # while a staged search is in flight
    m.match_staged_launch()
    assert _code(lambda: m.learn_device(dt)) == L.FPM_E_INVALID_ARG
    assert _code(lambda: m.learn_at(0, (10.0, 10.0), 0.0)) == L.FPM_E_INVALID_ARG
    assert _code(lambda: m.learn_hit(0)) == L.FPM_E_INVALID_ARG
    counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [2]
    assert _code(lambda: m.learn_hit(2)) == L.FPM_E_INVALID_ARG            # index out of range
    assert _code(lambda: m.learn_hit(-1)) == L.FPM_E_INVALID_ARG
    assert _code(lambda: m.learn_hit(0, source=1)) == L.FPM_E_INVALID_ARG
    # a rejected call leaves the context as it was
    assert m.isPatternLearned() and snapshot(m) == before and len(m.last_patches(0)) == 2
    # after a device learn the last search's poses are gone until the next search
    m.learn_hit(1)
    with pytest.raises(ValueError, match="no search has run"):
        m.last_patches(0)
    with pytest.raises(ValueError, match="no search has run"):
        m.last_compare(0)
    assert _code(lambda: m.learn_hit(0)) == L.FPM_E_INVALID_ARG
    assert len(m.match_staged()[0]) >= 1 and len(m.last_patches(0)) >= 1   # still staged; searched again
    # a template whose top layer differs from the slab's: the sources are invalidated, as fpm_learn invalidates them
    assert m.template_info()[0] > 1
    m.learn_at(0, (150.0, 140.0), 0.0, (0, 0, 12, 12))
    assert m.template_info()[0] == 1
    with pytest.raises(RuntimeError, match="no staged sources"):
        m.match_staged()
    assert _code(lambda: m.learn_at(0, (10.0, 10.0), 0.0)) == L.FPM_E_INVALID_ARG
    crop = np.ascontiguousarray(s[140:152, 150:162])
    assert m.template_level(0)[0].tobytes() == crop.tobytes()
    m.stage([s])
    fresh = host_learned(gpu_matcher_factory, crop, **prm)
    fresh.stage([s])
    assert _tuples(m.match_staged()[0]) == _tuples(fresh.match_staged()[0])
    # a host pointer, a bad format: rejected before anything is touched
    kept = snapshot(m)
    rc = m._lib.fpm_learn_device(m._ctx, t.ctypes.data, tw, th, tw, 0, L.FMT_GRAY8, None)
    assert rc == L.FPM_E_INVALID_ARG
    assert m._lib.fpm_learn_device(m._ctx, dt.data_ptr(), tw, th, tw, 0, 99, None) == L.FPM_E_INVALID_ARG
    assert m._lib.fpm_learn_device(m._ctx, dt.data_ptr(), tw, th, tw - 1, 0, L.FMT_GRAY8, None) == L.FPM_E_INVALID_ARG
    assert snapshot(m) == kept
