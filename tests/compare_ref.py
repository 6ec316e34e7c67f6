"""The patch comparison restated in numpy (include/fpm.h, "patch comparison"): Python integers for the sums and the
three determinants, np.float64 operations in the header's order for what is derived from them, np.rint for the table.
Shared by tests/test_compare_host.py and tests/test_gpu_compare.py."""
import numpy as np

FIELDS = ("n", "sum_i", "sum_ii", "sum_t", "sum_tt", "sum_it", "sum_abs", "n_over", "max_abs", "x0", "y0", "x1", "y1",
          "zncc", "gain", "offset")


def sums(I, T):
    """(n, sum_i, sum_ii, sum_t, sum_tt, sum_it) of two uint8 images of one shape, as Python integers."""
    assert I.shape == T.shape and I.dtype == T.dtype == np.uint8
    i, t = I.astype(np.int64).ravel(), T.astype(np.int64).ravel()
    return (int(i.size), int(i.sum()), int((i * i).sum()), int(t.sum()), int((t * t).sum()), int((i * t).sum()))


def derive(n, si, sii, st, stt, sit, normalize):
    """(zncc, gain, offset, lut) from the integer sums."""
    Di, Dt, N = n * sii - si * si, n * stt - st * st, n * sit - si * st
    assert max(abs(Di), abs(Dt), abs(N)) < 2 ** 63
    sdi, sdt = np.sqrt(np.float64(Di)), np.sqrt(np.float64(Dt))
    zncc = np.float64(N) / (sdi * sdt) if Di != 0 and Dt != 0 else np.float64(0.0)
    gain, offset = np.float64(1.0), np.float64(0.0)
    if normalize:
        gain = sdt / sdi if Di != 0 else np.float64(1.0)
        offset = (np.float64(st) - gain * np.float64(si)) / np.float64(n)
    v = np.arange(256, dtype=np.float64)
    prod = gain * v           # two ufunc calls: the product and the sum are rounded separately
    lut = np.minimum(255.0, np.maximum(0.0, np.rint(prod + offset))).astype(np.uint8)
    return float(zncc), float(gain), float(offset), lut


def stats(I, T, threshold, normalize):
    """({field: value}, difference image) of patch I against template crop T."""
    n, si, sii, st, stt, sit = sums(I, T)
    zncc, gain, offset, lut = derive(n, si, sii, st, stt, sit, normalize)
    d = np.abs(lut[I].astype(np.int32) - T.astype(np.int32))
    over = d > threshold
    h, w = I.shape
    if over.any():
        ys, xs = np.nonzero(over)
        box = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
    else:
        box = (w, h, -1, -1)
    row = dict(n=n, sum_i=si, sum_ii=sii, sum_t=st, sum_tt=stt, sum_it=sit, sum_abs=int(d.sum()),
               n_over=int(over.sum()), max_abs=int(d.max()), x0=box[0], y0=box[1], x1=box[2], y1=box[3], zncc=zncc,
               gain=gain, offset=offset)
    return row, d.astype(np.uint8)


def assert_rows(got, exp, label):
    """Every field of every row equal (==: the integers by construction, the f64 by the fixed operation order)."""
    assert len(got) == len(exp), f"{label}: {len(got)} rows vs {len(exp)}"
    for i, e in enumerate(exp):
        for f in FIELDS:
            g = got[i][f].item()
            assert g == e[f], f"{label}: row {i} field {f}: {g!r} != {e[f]!r}"
