"""The variation model restated in numpy and Python integers (include/fpm.h, "variation model"): the planes S and Q, what
is derived per pixel from them, and the inspection of a patch.  Shared by tests/test_model_host.py and
tests/test_gpu_model.py.  Everything is exact: Python integers and math.isqrt."""
import math

import numpy as np

from tests import compare_ref

FIELDS = ("n", "sum_excess", "n_low", "n_high", "max_excess", "x0", "y0", "x1", "y1", "gain", "offset")


def kq_of(k):
    """The sigma multiple in sixteenths, as the Python interface takes a float to it."""
    return int(round(float(k) * 16.0))


def derive1(n, S, Q, a, kq):
    """(mean, lo, hi) of one pixel from Python integers."""
    V = n * Q - S * S
    assert V >= 0 and kq * kq * V < 2 ** 63
    B = max(n * a, math.isqrt((kq * kq * V) >> 8))
    mean = (2 * S + n) // (2 * n)
    lo = max(0, -((B - S) // n))          # ceil((S - B) / n)
    hi = min(255, (S + B) // n)
    return mean, lo, hi


def sample(I, T=None, normalize=False):
    """(v, gain, offset): what the model sees of patch I -- the pixels, or LUT[pixels] with the table a normalised
    comparison with template crop T builds."""
    if not normalize:
        return I, 1.0, 0.0
    _, gain, offset, lut = compare_ref.derive(*compare_ref.sums(I, T), True)
    return lut[I], gain, offset


def accumulate(samples):
    """(n, S, Q) as int64 arrays for a list of uint8 images of one shape."""
    v = np.stack([s.astype(np.int64) for s in samples])
    return len(samples), v.sum(axis=0), (v * v).sum(axis=0)


def derive(n, S, Q, a, kq):
    """(mean, lo, hi) uint8 images from the planes."""
    h, w = S.shape
    out = np.zeros((3, h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            out[:, y, x] = derive1(n, int(S[y, x]), int(Q[y, x]), a, kq)
    return out[0], out[1], out[2]


def derive_fast(n, S, Q, a, kq):
    """derive() for large planes: one derive1 per distinct (S, Q) pair."""
    h, w = S.shape
    pairs, inv = np.unique(np.stack([S.ravel(), Q.ravel()], axis=1), axis=0, return_inverse=True)
    vals = np.array([derive1(n, int(s), int(q), a, kq) for s, q in pairs], np.uint8)
    out = vals[np.asarray(inv).ravel()].reshape(h, w, 3)
    return out[..., 0].copy(), out[..., 1].copy(), out[..., 2].copy()


def inspect(v, lo, hi, gain=1.0, offset=0.0):
    """({field: value}, excess image) of sampled values v (uint8) against the lo / hi images."""
    u, l, h_ = v.astype(np.int32), lo.astype(np.int32), hi.astype(np.int32)
    low, high = u < l, (u >= l) & (u > h_)
    e = np.where(low, l - u, np.where(high, u - h_, 0))
    h, w = v.shape
    out = e > 0
    assert np.array_equal(out, low | high)
    if out.any():
        ys, xs = np.nonzero(out)
        box = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
    else:
        box = (w, h, -1, -1)
    row = dict(n=h * w, sum_excess=int(e.sum()), n_low=int(low.sum()), n_high=int(high.sum()), max_excess=int(e.max()),
               x0=box[0], y0=box[1], x1=box[2], y1=box[3], gain=gain, offset=offset)
    return row, e.astype(np.uint8)


def assert_rows(got, exp, label):
    assert len(got) == len(exp), f"{label}: {len(got)} rows vs {len(exp)}"
    for i, e in enumerate(exp):
        for f in FIELDS:
            g = got[i][f].item()
            assert g == e[f], f"{label}: row {i} field {f}: {g!r} != {e[f]!r}"
