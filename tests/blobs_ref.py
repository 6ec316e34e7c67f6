"""Reference for the defect blobs (include/fpm.h, "defect blobs"): connected components of the pixels above a level, in
plain Python and numpy (no scipy, no library).  A run-based two-pass union-find gives the label image (seed + 1, seed =
the smallest row-major index of the component); numpy sums give the records.  Also the patterns of the tests (the
shapes are chosen around a 64 x 16 tile: one lane, a partial tile, exact edges, one pixel past, ragged grids) and the
acceptance predicate of a truncated list."""
import functools

import numpy as np

FIELDS = ("hit", "seed", "area", "x0", "y0", "x1", "y1", "max_value", "sum_value", "sum_x", "sum_y")
SUMMARY_FIELDS = ("fg_pixels", "n_components", "n_blobs", "n_returned", "largest_area", "flags", "reserved")
REC = np.dtype([(f, np.int64) for f in FIELDS])
TRUNCATED = 1


def label(mask, connectivity):
    """int32 (h, w): seed + 1 of the pixel's component where ``mask`` is set, 0 elsewhere."""
    assert connectivity in (4, 8)
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    reach = 1 if connectivity == 8 else 0
    parent, runs = [], []   # per run: its parent run; (row, start, end) with end exclusive.  Ids ascend in row-major order

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    prev = []
    for v in range(h):
        edges = np.flatnonzero(np.diff(np.concatenate(([0], mask[v].astype(np.int8), [0]))))
        cur = []
        for s, e in zip(edges[0::2].tolist(), edges[1::2].tolist()):
            rid = len(parent)
            parent.append(rid)
            runs.append((v, s, e))
            cur.append(rid)
            for pid in prev:   # runs of the row above that touch [s, e): by an edge, or at 8 also by a corner
                _, ps, pe = runs[pid]
                if ps < e + reach and pe > s - reach:
                    a, b = find(rid), find(pid)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
        prev = cur
    out = np.zeros((h, w), np.int32)
    for rid, (v, s, e) in enumerate(runs):
        rv, rs, _ = runs[find(rid)]
        out[v, s:e] = rv * w + rs + 1
    return out


def records(img, labels, hit=0):
    """Every component's record, ascending seed: a REC array."""
    img = np.asarray(img, np.int64)
    h, w = img.shape
    fg = labels > 0
    seeds, inv = np.unique(labels[fg] - 1, return_inverse=True)
    out = np.zeros(len(seeds), REC)
    if not len(seeds):
        return out
    ys, xs = np.nonzero(fg)
    e = img[fg]
    k = len(seeds)
    out["hit"] = hit
    out["seed"] = seeds
    out["area"] = np.bincount(inv, minlength=k)
    for name, val in (("sum_value", e), ("sum_x", xs), ("sum_y", ys)):
        out[name] = np.bincount(inv, weights=val, minlength=k).astype(np.int64)   # < 2^53: exact
    for name, val, fn in (("x0", xs, np.minimum), ("y0", ys, np.minimum), ("x1", xs, np.maximum), ("y1", ys, np.maximum),
                          ("max_value", e, np.maximum)):
        acc = np.full(k, val.max() if fn is np.minimum else val.min(), np.int64)
        fn.at(acc, inv, val)
        out[name] = acc
    return out


def blobs(img, level, connectivity, min_area, cap, hit=0):
    """(labels, recs, summary) of one image by the contract: ``recs`` = every component with area >= min_area in
    ascending seed (NOT cut to cap), ``summary`` a dict of SUMMARY_FIELDS."""
    img = np.asarray(img)
    lab = label(img.astype(np.int64) > level, connectivity)
    allr = records(img, lab, hit)
    keep = allr[allr["area"] >= min_area]
    summary = dict(fg_pixels=int((lab > 0).sum()), n_components=len(allr), n_blobs=len(keep),
                   n_returned=min(len(keep), cap), largest_area=int(allr["area"].max()) if len(allr) else 0,
                   flags=TRUNCATED if len(keep) > cap else 0, reserved=0)
    return lab, keep, summary


def as_rec(a):
    """A structured array with FIELDS (any integer types) as a REC array."""
    out = np.zeros(len(a), REC)
    for f in FIELDS:
        out[f] = a[f]
    return out


def accept(summary_row, got, ref_recs, ref_summary, cap):
    """The contract's acceptance of one hit: the summary equal; not truncated: the records equal the reference's;
    truncated: cap records, each one of the reference's qualifying records, ascending and distinct by seed."""
    for f in SUMMARY_FIELDS:
        if int(summary_row[f]) != ref_summary[f]:
            return f"summary.{f}: got {int(summary_row[f])}, expected {ref_summary[f]}"
    got = as_rec(got)
    if len(got) != ref_summary["n_returned"]:
        return f"{len(got)} records, expected {ref_summary['n_returned']}"
    if not ref_summary["flags"] & TRUNCATED:
        return None if np.array_equal(got, ref_recs) else "records differ from the reference's"
    if len(got) != cap:
        return "a truncated list holds cap records"
    if not np.all(np.diff(got["seed"]) > 0):
        return "seeds not ascending and distinct"
    pos = np.searchsorted(ref_recs["seed"], got["seed"])
    if np.any(pos >= len(ref_recs)) or not np.array_equal(ref_recs[np.minimum(pos, len(ref_recs) - 1)], got):
        return "a record is none of the reference's qualifying records"
    return None


# ---- patterns (masks as uint8 0 / 1; callers scale them) --------------------------------------------------------------
def checkerboard(w, h):
    v, u = np.mgrid[0:h, 0:w]
    return ((u + v) % 2 == 0).astype(np.uint8)


def spiral(w, h):
    """A one-pixel-wide rectangular spiral filling the image (one pixel of gap between the turns)."""
    m = np.zeros((h, w), np.uint8)
    x0, y0, x1, y1 = 0, 0, w - 1, h - 1
    x, y = 0, 0
    m[0, 0] = 1
    d = 0
    while x0 <= x1 and y0 <= y1:
        if d == 0:
            m[y, x:x1 + 1] = 1; x = x1; y0 += 2
        elif d == 1:
            m[y:y1 + 1, x] = 1; y = y1; x1 -= 2
        elif d == 2:
            m[y, x0:x + 1] = 1; x = x0; y1 -= 2
        else:
            m[y0:y + 1, x] = 1; y = y0; x0 += 2
        d = (d + 1) % 4
    return m


def comb(w, h):
    """Teeth in every other column that join only along the last row."""
    m = np.zeros((h, w), np.uint8)
    m[:, 0::2] = 1
    m[h - 1, :] = 1
    return m


def comb_mirror(w, h):
    """Teeth in every other row that join only along the last column."""
    return np.ascontiguousarray(comb(h, w).T)


def u_shape(w, h):
    m = np.zeros((h, w), np.uint8)
    m[:, 0] = 1; m[:, w - 1] = 1; m[h - 1, :] = 1
    return m


def s_shape(w, h):
    m = np.zeros((h, w), np.uint8)
    mid = h // 2
    m[0, :] = 1; m[mid, :] = 1; m[h - 1, :] = 1
    m[0:mid + 1, 0] = 1
    m[mid:h, w - 1] = 1
    return m


def diagonal(w, h):
    m = np.zeros((h, w), np.uint8)
    k = np.arange(min(w, h))
    m[k, k] = 1
    return m


def anti_diagonal(w, h):
    return np.ascontiguousarray(diagonal(w, h)[:, ::-1])


def frame_island(w, h):
    m = np.zeros((h, w), np.uint8)
    m[0, :] = 1; m[h - 1, :] = 1; m[:, 0] = 1; m[:, w - 1] = 1
    if w >= 5 and h >= 5:
        m[h // 2, w // 2] = 1
    return m


def tile_corners(w, h, tw=64, th=16):
    """Isolated pixels in the four corners of every tw x th tile (cut by the image's edge)."""
    m = np.zeros((h, w), np.uint8)
    for y in sorted({y for t in range(0, h, th) for y in (t, min(t + th, h) - 1)}):
        for x in sorted({x for t in range(0, w, tw) for x in (t, min(t + tw, w) - 1)}):
            m[y, x] = 1
    return m


SHAPES = ((1, 1), (5, 3), (63, 15), (64, 16), (65, 17), (130, 35), (257, 50))
DENSITIES = (0.05, 0.4, 0.6, 0.95)
LEVELS = (0, 100, 254)


@functools.lru_cache(maxsize=None)
def pattern_batch(w, h):
    """``(names, images, levels)``: every pattern of the list at (w, h) as uint8 (n, h, w), and the level each is cut at.
    Mask patterns carry the values 0 / 200 + (u + 3 v) % 50 and are cut at level 0, so max_value and sum_value vary."""
    rng = np.random.default_rng(1000 * w + h)
    v, u = np.mgrid[0:h, 0:w]
    tone = (200 + (u + 3 * v) % 50).astype(np.uint8)
    names, imgs, levels = [], [], []
    for name, m in (("empty", np.zeros((h, w), np.uint8)), ("full", np.ones((h, w), np.uint8)),
                    ("checkerboard", checkerboard(w, h)), ("spiral", spiral(w, h)), ("comb", comb(w, h)),
                    ("comb_mirror", comb_mirror(w, h)), ("u", u_shape(w, h)), ("s", s_shape(w, h)),
                    ("anti_diagonal", anti_diagonal(w, h)), ("diagonal", diagonal(w, h)),
                    ("frame_island", frame_island(w, h)), ("tile_corners", tile_corners(w, h))):
        names.append(name); imgs.append(m * tone); levels.append(0)
    for d in DENSITIES:
        names.append(f"random_{d}"); imgs.append((rng.random((h, w)) < d) * tone); levels.append(0)
    values = rng.integers(0, 256, (h, w)).astype(np.uint8)
    for lv in LEVELS:
        names.append(f"values_{lv}"); imgs.append(values); levels.append(lv)
    out = np.ascontiguousarray(np.stack(imgs).astype(np.uint8))
    out.setflags(write=False)
    return tuple(names), out, tuple(levels)


@functools.lru_cache(maxsize=None)
def pattern_reference(w, h, connectivity):
    """Per image of pattern_batch(w, h): (labels, every component's record) -- computed once, shared, left unchanged."""
    _, imgs, levels = pattern_batch(w, h)
    out = []
    for i, (img, lv) in enumerate(zip(imgs, levels)):
        lab = label(img.astype(np.int64) > lv, connectivity)
        lab.setflags(write=False)
        out.append((lab, records(img, lab, i)))
    return out


def from_all(allr, lab, min_area, cap):
    """(recs, summary) for a filter and a capacity from every component's record."""
    keep = allr[allr["area"] >= min_area]
    return keep, dict(fg_pixels=int((lab > 0).sum()), n_components=len(allr), n_blobs=len(keep),
                      n_returned=min(len(keep), cap), largest_area=int(allr["area"].max()) if len(allr) else 0,
                      flags=TRUNCATED if len(keep) > cap else 0, reserved=0)
