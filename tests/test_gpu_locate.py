"""The sub-pattern locators on the HIP path (fpm_locate_at / fpm_last_locate): k_patch_locate's maps, raw records and
the derived results against the restatement of tests/locate_ref.py (the oracle's warpAffine of fpm_patch_matrix's
matrix, int64 sums, z and the tie rule in Python floats in the header's order).  Every comparison is ==."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  at collection time, before any test loads libfpm_hip.so: one HIP runtime for both

from fastest_image_pattern_matching_amd import _lib as L
from fastest_image_pattern_matching_amd import matcher as M
from tests import locate_ref as ref
from tests.cases import CASES
from tests.test_gpu_gray import FAR_POSE, POSES, SH, SW, TEMPLATES, mask_for

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 5, 63, 64, 65, 128]
HEIGHTS = [1, 15, 16, 17, 33]
RADII = [(0, 0), (1, 3), (3, 1), (0, 16), (16, 0), (3, 3), (1, 0), (0, 1), (16, 3), (1, 16)]


@pytest.fixture(scope="module")
def hip(gpu_matcher_factory):
    return gpu_matcher_factory()


def _source(seed=203):
    return np.random.default_rng(seed).integers(0, 256, (SH, SW), dtype=np.uint8)


def _template(tw, th):
    return np.random.default_rng(tw).integers(0, 256, (th, tw), dtype=np.uint8)


def features_for(tw, th):
    """Every width with every height the template allows, the radii in turn, every x & 3, the last column, the last
    row, both radii at their cap, and windows that leave the template on all four sides."""
    fs = []
    for i, w in enumerate(w for w in WIDTHS if w <= tw):
        for j, h in enumerate(h for h in HEIGHTS if h <= th):
            rx, ry = RADII[(i * len(HEIGHTS) + j) % len(RADII)]
            fs.append((min((i + j) % 4, tw - w), min((2 * i + j) % 3, th - h), w, h, rx, ry))
    fs += [(tw - 1, 0, 1, th, 3, 1), (0, th - 1, tw if tw <= 128 else 128, 1, 1, 3), (tw - 5, th - 3, 5, 3, 16, 16),
           (0, 0, 9, 7, 3, 3), (tw - 9, th - 7, 9, 7, 3, 3)] + [(x, x % 2, 9, 7, 2, 1) for x in range(1, 5)]
    assert len(fs) <= L.LOCATE_MAX_FEATURES and {f[0] & 3 for f in fs} == {0, 1, 2, 3}
    assert all(f[0] + f[2] <= tw and f[1] + f[3] <= th for f in fs) and any(f[4] != f[5] for f in fs)
    assert any(f[0] - f[4] < 0 for f in fs) and any(f[1] - f[5] < 0 for f in fs)
    assert any(f[0] + f[2] + f[4] > tw for f in fs) and any(f[1] + f[3] + f[5] > th for f in fs)
    return fs


def _feats(fs):
    return np.array([M.feature(*f) for f in fs], M.FEATURE_DTYPE)


_expected = {}


def _expect(key, src, tmpl, f, pose):
    """(raw dict with the entry's flag, maps, result dict) of (source key, feature, pose): computed once, shared."""
    k = (key, f, pose)
    if k not in _expected:
        x, y, w, h, rx, ry = f
        raw, maps = ref.locate(ref.window(src, f, *pose), tmpl[y:y + h, x:x + w], rx, ry)
        raw["flags"] = ref.outside(src.shape[1], src.shape[0], f, *pose)
        _expected[k] = (raw, maps, ref.derive(f, pose[0], pose[1], raw))
    return _expected[k]


def _check(got, key, src, tmpl, fs, poses, label=""):
    res, raw, maps = got
    assert res.shape == raw.shape == (len(poses), len(fs)) and maps.dtype == np.int32
    assert maps.shape == (len(poses), len(fs), 3, max((2 * f[4] + 1) * (2 * f[5] + 1) for f in fs))
    for i, pose in enumerate(poses):
        for k, f in enumerate(fs):
            eraw, emaps, eres = _expect(key, src, tmpl, f, pose)
            n = emaps[0].size
            where = f"{label} pose {i} {pose} feature {k} {f}"
            assert np.array_equal(maps[i, k, :, :n], emaps.reshape(3, n)) and not maps[i, k, :, n:].any(), where
            assert ref.raw_equal(raw[i, k], eraw), (where, ref.raw_dict(raw[i, k]), eraw)
            assert ref.result_equal(res[i, k], eres), (where, res[i, k], eres)
            assert res[i, k].tobytes() == M.locate_derive(_feats([f])[0], pose[0], pose[1], raw[i, k]).tobytes(), where


def _setup(hip, tw, th, srcs):
    hip.resetParams()
    t = _template(tw, th)
    assert hip.learnPattern(t)
    hip.stage(srcs)
    return t


def _at(poses, s=0):
    return [s] * len(poses), [p[0] for p in poses], [p[1] for p in poses]


@pytest.mark.parametrize("tw,th", TEMPLATES)
def test_parity(hip, tw, th):
    src = _source()
    t = _setup(hip, tw, th, [src])
    fs = features_for(tw, th)
    got = hip.locate_at(*_at(POSES), _feats(fs), raw=True, maps=True)
    _check(got, ("rand", tw), src, t, fs, POSES)
    res, raw, maps = got
    assert POSES[-1] == FAR_POSE                                    # wholly outside: every sum 0, at nominal, score 0
    assert not maps[-1].any() and not raw["dx"][-1].any() and not raw["dy"][-1].any() and not res["score"][-1].any()
    assert ((res["flags"][-1] & (L.LOCATE_FLAT | L.LOCATE_OUTSIDE)) == (L.LOCATE_FLAT | L.LOCATE_OUTSIDE)).all()
    assert (res["flags"][0] & L.LOCATE_OUTSIDE == 0).any() and (raw["dx"] != 0).any() and (raw["dy"] != 0).any()
    # the optional outputs change nothing
    assert hip.locate_at(*_at(POSES), _feats(fs)).tobytes() == res.tobytes()
    only_raw = hip.locate_at(*_at(POSES), _feats(fs), raw=True)
    assert only_raw[0].tobytes() == res.tobytes() and only_raw[1].tobytes() == raw.tobytes()


def test_largest_feature(hip):
    """128 x 128 with both radii 16: the whole LDS budget and the largest sums (a white source under a white template
    reaches 65025 * 16384)."""
    rng = np.random.default_rng(128)
    t = rng.integers(0, 256, (140, 150), dtype=np.uint8)
    t[5:133, 7:135] = 255
    srcs = [rng.integers(0, 256, (300, 320), dtype=np.uint8), np.full((300, 320), 255, np.uint8)]
    hip.resetParams()
    assert hip.learnPattern(t)
    hip.stage(srcs)
    fs = [(7, 5, 128, 128, 16, 16), (3, 2, 128, 127, 16, 15), (22, 12, 127, 128, 15, 16)]
    poses = [((60.0, 50.0), 0.0), ((150.25, 40.5), 30.0)]
    for s, src in enumerate(srcs):
        got = hip.locate_at(*_at(poses, s), _feats(fs), raw=True, maps=True)
        _check(got, ("big", s), src, t, fs, poses, f"source {s}")
    assert got[2][0, 0, 2].max() == 65025 * 16384


def test_tie_rule(hip):
    tw, th = TEMPLATES[0]
    vv, uu = np.mgrid[0:SH, 0:SW]
    srcs = [np.full((SH, SW), 90, np.uint8), np.zeros((SH, SW), np.uint8),
            (((uu % 4) * 37 + (vv % 4) * 11 + ((uu % 4) * (vv % 4)) * 5) % 256).astype(np.uint8),
            (((uu % 2) * 100 + (vv % 8) * 9) % 256).astype(np.uint8)]
    t = _setup(hip, tw, th, srcs)
    fs = [(2, 1, 20, 12, 4, 4), (5, 3, 33, 17, 8, 8), (0, 0, 7, 5, 4, 8), (9, 2, 16, 16, 2, 16)]
    poses = [((40.0, 30.0), 0.0), ((57.0, 41.0), 0.0)]             # whole pixels, upright: the window keeps the period
    for s, src in enumerate(srcs):
        res, raw, maps = got = hip.locate_at(*_at(poses, s), _feats(fs), raw=True, maps=True)
        _check(got, ("tie", s), src, t, fs, poses, f"source {s}")
        if s < 2:                                                   # constant: every offset ties at 0 -- at nominal
            assert not raw["dx"].any() and not raw["dy"].any() and not res["score"].any()
            assert (res["flags"] == L.LOCATE_FLAT).all()
        if s == 2:                                                  # period 4 both ways: the maps repeat, the peak is
            for k, f in enumerate(fs):                              # the repeat nearest to nominal
                nx, ny = 2 * f[4] + 1, 2 * f[5] + 1
                m = maps[0, k, :, :nx * ny].reshape(3, ny, nx)
                assert np.array_equal(m[:, 4:, 4:], m[:, :-4, :-4])
                assert abs(int(raw["dx"][0, k])) <= 2 and abs(int(raw["dy"][0, k])) <= 2


def test_64_features_permuted_and_alone(hip):
    tw, th = TEMPLATES[0]
    src = _source()
    _setup(hip, tw, th, [src])
    fs = features_for(tw, th)
    fs += [(k % 7, k % 5, 10 + 2 * (k % 25), 3 + k % 20, k % 5, (k * 3) % 7) for k in range(64 - len(fs))]
    assert len(fs) == 64
    poses = POSES[:4]
    res, raw, maps = hip.locate_at(*_at(poses), _feats(fs), raw=True, maps=True)
    perm = list(np.random.default_rng(9).permutation(64))
    pres, praw, pmaps = hip.locate_at(*_at(poses), _feats([fs[k] for k in perm]), raw=True, maps=True)
    assert pres.tobytes() == res[:, perm].tobytes() and praw.tobytes() == raw[:, perm].tobytes()
    assert np.array_equal(pmaps, maps[:, perm])
    for k in (0, 7, 21, 40, 63):
        ores, oraw, omaps = hip.locate_at(*_at(poses), _feats([fs[k]]), raw=True, maps=True)
        n = omaps.shape[3]
        assert ores[:, 0].tobytes() == res[:, k].tobytes() and oraw[:, 0].tobytes() == raw[:, k].tobytes(), k
        assert np.array_equal(omaps[:, 0], maps[:, k, :, :n]) and not maps[:, k, :, n:].any(), k


# ---- over the hits of a search ----------------------------------------------------------------------------------------
def _search(m, templates, bitwise_not=False):
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    m.resetParams()
    for k, v in prm.items():
        setattr(m._params, k, v)
    m.setBitwiseNot(bitwise_not)
    assert m.learnPattern(t)
    m.stage([np.ascontiguousarray(255 - s) if bitwise_not else s])
    res = m.match_staged()
    assert len(res[0]) == 3
    ps = [(r.ptLT, r.dMatchedAngle) for r in res[0]]     # Qt semantics: the raw pose
    return s, t, [p[0] for p in ps], [p[1] for p in ps]


def _hit_features(t):
    th, tw = t.shape
    return [(tw // 4, th // 4, min(64, tw // 2), min(48, th // 2), 8, 8), (3, 2, 21, 17, 3, 5), (tw - 9, th - 7, 9, 7, 2, 2)]


def _check_last(m, s, t, lts, angs, label):
    fs = _hit_features(t)
    got = m.last_locate(_feats(fs), source=0, raw=True, maps=True)
    poses = [(tuple(float(np.float32(v)) for v in lt), float(a)) for lt, a in zip(lts, angs)]
    _check(got, ("hit", label), s, t, fs, poses, label)
    at = m.locate_at(0, lts, angs, _feats(fs), raw=True, maps=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, at)), label
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, m.last_locate(_feats(fs), source=-1, raw=True, maps=True)))
    return got


def test_last_locate_after_a_search(hip, templates):
    s, t, lts, angs = _search(hip, templates)
    res, raw, maps = _check_last(hip, s, t, lts, angs, "raw poses")
    assert (res["score"][:, 0] > 0.9).all() and (np.hypot(res["ox"][:, 0], res["oy"][:, 0]) < 1.0).all()
    # a mask is not honoured: set, disabled or cleared, the same bytes
    th, tw = t.shape
    hip.set_mask(mask_for("ellipse", tw, th))
    masked = hip.last_locate(_feats(_hit_features(t)), raw=True, maps=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(masked, (res, raw, maps)))
    hip.mask_enable(False)
    assert hip.last_locate(_feats(_hit_features(t))).tobytes() == res.tobytes()
    hip.mask_enable(True)
    hip.clear_mask()
    # after adoption it samples at the aligned poses
    al = hip.align_last(0, adopt=True)
    assert (al["best_eval"] > 0).any(), "no hit moved: the test shows nothing"
    alt, aang = np.stack([al["lt_x"], al["lt_y"]], 1), al["angle"]
    got2 = _check_last(hip, s, t, [tuple(p) for p in alt.tolist()], aang.tolist(), "adopted")
    assert got2[2].tobytes() != maps.tobytes()


def test_last_locate_under_bitwise_not(hip, templates):
    s, t, lts, angs = _search(hip, templates, bitwise_not=True)     # staged: 255 - s; sampled: the inverted plane, s
    try:
        _check_last(hip, s, t, lts, angs, "bitwise_not")
    finally:
        hip.setBitwiseNot(False)


# ---- state ----------------------------------------------------------------------------------------------------------
def _results(m, n_src):
    n = (C.c_int32 * n_src)()
    m._lib.fpm_last_results(m._ctx, None, 0, n)
    out = (L.Result * max(sum(n), 1))()
    assert m._lib.fpm_last_results(m._ctx, out, sum(n), n) == L.FPM_OK
    return bytes(out), list(n)


def test_state_errors_and_profile(gpu_matcher_factory, templates):
    make, prm = CASES["dst10_multi"]
    s, t = make(templates)
    th, tw = t.shape
    m = gpu_matcher_factory(**prm)
    one = [(10.0, 10.0)]
    f1 = _feats([(3, 2, 21, 17, 3, 5)])
    for call in (lambda: m.last_locate(f1), lambda: m.locate_at(0, one, [0.0], f1)):
        with pytest.raises((ValueError, RuntimeError)):
            call()                                              # no template
    n = C.c_int32(-1)
    pf = f1.ctypes.data_as(C.POINTER(L.Feature))
    assert m._lib.fpm_last_locate(m._ctx, 0, pf, 1, None, None, None, 0, 0, C.byref(n)) == L.FPM_E_NOT_LEARNED
    assert m.learnPattern(t)
    for call in (lambda: m.last_locate(f1), lambda: m.locate_at(0, one, [0.0], f1)):
        with pytest.raises(ValueError, match="no staged sources"):
            call()
    m.stage([s])
    with pytest.raises(ValueError, match="no search has run"):
        m.last_locate(f1)
    assert m.locate_at(0, one, [5.0], f1).shape == (1, 1)       # poses of the caller's need no search
    m.match_staged_launch()
    for call in (lambda: m.last_locate(f1), lambda: m.locate_at(0, one, [0.0], f1)):
        with pytest.raises(ValueError, match="in flight"):
            call()
    counts, _ = m.match_staged_finish_array()
    assert counts.tolist() == [3]
    mask = mask_for("ellipse", tw, th)
    m.set_mask(mask)
    m.model_train_last(source=0)
    results, cands = _results(m, 1), m.last_candidates(0).tobytes()
    patches, model = m.last_patches(0).tobytes(), [a.tobytes() for a in m.model_sums()]
    compare = m.last_compare(0).tobytes()
    fs = _feats([(3, 2, 21, 17, 3, 5), (0, 0, 9, 7, 1, 0)])
    stride = 77
    res = np.frombuffer(bytearray(b"\xa5" * (80 * 6)), M.LOCATE_DTYPE).reshape(3, 2)
    raw = np.frombuffer(bytearray(b"\xa5" * (160 * 6)), M.LOCATE_RAW_DTYPE).reshape(3, 2)
    maps = np.full((3, 2, 3, stride), -1515870811, np.int32)
    sent = [a.tobytes() for a in (res, raw, maps)]
    pr, pw, pm = (res.ctypes.data_as(C.POINTER(L.LocateResult)), raw.ctypes.data_as(C.POINTER(L.LocateRaw)),
                  maps.ctypes.data_as(C.POINTER(C.c_int32)))

    def untouched():
        return [a.tobytes() for a in (res, raw, maps)] == sent

    def last(source=0, f=fs, nf=2, r=pr, w=pw, mp=pm, st=stride, cap=3):
        return m._lib.fpm_last_locate(m._ctx, source, f.ctypes.data_as(C.POINTER(L.Feature)) if f is not None else None, nf,
                                      r, w, mp, st, cap, C.byref(n))

    def at(idx=(0,), lt=((10.0, 10.0),), ang=(0.0,), f=fs, nf=2, r=pr, w=pw, mp=pm, st=stride):
        i, l, a = np.array(idx, np.int32), np.array(lt, np.float32), np.array(ang, np.float64)
        return m._lib.fpm_locate_at(m._ctx, i.ctypes.data_as(C.POINTER(C.c_int32)), l.ctypes.data_as(C.POINTER(C.c_float)),
                                    a.ctypes.data_as(C.POINTER(C.c_double)), len(i),
                                    f.ctypes.data_as(C.POINTER(L.Feature)) if f is not None else None, nf, r, w, mp, st)

    # the count-only call, then a capacity below the count: FPM_E_CAPACITY, nothing written
    assert last(r=None, w=None, mp=None, st=0, cap=0) == L.FPM_E_CAPACITY and n.value == 3
    assert last(cap=2) == L.FPM_E_CAPACITY and n.value == 3 and untouched()
    m.profile(True)
    try:
        m.profile_reset()

        def bad(**kw):
            f = fs.copy()
            for k, v in kw.items():
                f[k][1] = v
            return f

        bad_feats = [bad(x=-1), bad(y=-1), bad(w=0), bad(h=0), bad(w=129), bad(h=129), bad(x=tw - 8), bad(y=th - 6),
                     bad(rx=-1), bad(ry=-1), bad(rx=17), bad(ry=17), bad(reserved=(1, 0)), bad(reserved=(0, 1))]
        for f in bad_feats:
            assert last(f=f) == L.FPM_E_INVALID_ARG and at(f=f) == L.FPM_E_INVALID_ARG and untouched(), f[1]
        for kw in (dict(f=None), dict(nf=0), dict(nf=65), dict(r=None), dict(st=14), dict(source=1), dict(source=-2)):
            assert last(**kw) == L.FPM_E_INVALID_ARG and untouched(), kw
        for kw in (dict(f=None), dict(nf=0), dict(nf=65), dict(r=None), dict(st=14), dict(idx=(1,)), dict(idx=(-1,)),
                   dict(lt=((2e6, 10.0),)), dict(lt=((np.nan, 10.0),)), dict(ang=(np.inf,))):
            assert at(**kw) == L.FPM_E_INVALID_ARG and untouched(), kw
        assert last(st=14, mp=None) == L.FPM_OK                 # without maps the stride is not looked at
        res[:], raw[:] = (np.frombuffer(bytearray(b"\xa5" * len(b)), a.dtype).reshape(a.shape) for a, b in zip((res, raw), sent))
        with pytest.raises(ValueError):
            m.locate_at(0, one * 1025, [0.0] * 1025, np.repeat(f1, 64))     # 65 600 jobs
        with pytest.raises(ValueError):
            m.last_locate(np.repeat(f1, 65))
        assert untouched() and m.locate_profile()[1] == 1
        m.profile_reset()
        assert m.locate_profile() == (0.0, 0, 0)
        m.last_locate(fs)
        ms, launches, nbytes = m.locate_profile()
        windows = 3 * ((21 + 6) * (17 + 10) + 21 * 17 + (9 + 2) * 7 + 9 * 7)
        assert ms > 0 and launches == 1 and nbytes == windows + 6 * 160
        m.locate_at(0, one * 4, [5.0] * 4, fs, maps=True)
        assert m.locate_profile()[1] == 2 and m.locate_profile()[2] == nbytes + 4 * windows // 3 + 8 * (160 + 4 * 3 * 77)
        assert m.profile_get(L.K_PATCH)[1] == 0 and m.profile_get(L.K_COMPARE)[1] == 0
        assert len(L.KERNEL_NAMES) == 15 and len(L.PROFILE_NAMES) == 16     # no FPM_K_* index was added
    finally:
        m.profile(False)
    assert untouched()
    assert last() == L.FPM_OK and n.value == 3 and (raw["n"] == [[21 * 17, 9 * 7]] * 3).all() and not untouched()
    assert not maps[:, 1, :, 3:].any() and not maps[:, 0, :, 77:].any()
    # the search's records, the poses, the comparison, the model and the mask are what they were, and a following search
    # returns the same
    assert _results(m, 1) == results and m.last_candidates(0).tobytes() == cands and m.last_patches(0).tobytes() == patches
    assert [a.tobytes() for a in m.model_sums()] == model and np.array_equal(m.mask() != 0, mask != 0)
    assert m.last_compare(0).tobytes() == compare
    assert len(m.match_staged()[0]) == 3 and _results(m, 1) == results and m.last_candidates(0).tobytes() == cands
    m.stage([s])                                                # staged again, not searched
    with pytest.raises(ValueError, match="no search has run"):
        m.last_locate(fs)
    m.match_staged_candidates()                                 # a search without results
    assert m.last_locate(fs, source=-1).shape == (0, 2)
