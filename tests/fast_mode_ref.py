"""Expected fast-mode (fpm_params.stop_layer, MatchToolDlg.cpp:936-1054) candidate records, derived from the oracle's
trace of a NORMAL search -- TEST INFRASTRUCTURE ONLY.

The oracle searches down to layer 0 (its stop layer is fixed), but its trace holds every value fast mode returns, so the
expected records are picked from it with no arithmetic here.  For candidate i (`origin == i`, push order, as
`OracleMatcher.candidates()`), with L the top layer:

  top_score, angle_index, peak_rank, source   as in the normal-mode record;
  kept    1 iff the trace has a layer-0 row for i: a candidate enters layer 0 exactly when it passed layer 1's
          threshold (always, when L == 1);
  x, y    that layer-0 row's `lt`: the ptLT getRotatedROI got at layer 0, i.e. the layer-1 back-mapped Point2f (L >= 2)
          or the rotated top-layer ptLT (L == 1), doubled in float -- MatchToolDlg.cpp:1035 / :951;
  score, angle   L >= 2: the layer-1 row's score[imax], angle[imax];
                 L == 1: top_score and the layer-0 row's middle angle (the candidate's own top-layer angle);
  records with kept == 0 are zero past the four identity fields;
  L == 0: fast mode is the normal search (the stop layer is min(1, L)).
"""
import numpy as np

from fastest_image_pattern_matching_amd.matcher import CANDIDATE_DTYPE
from tests import oracle


def run_oracle(t, s, prm):
    """A traced normal-mode oracle search of `s` for `t` under `prm` (stop_layer / bitwise_not left out: the oracle has
    neither): (matcher, results, top layer L)."""
    prm = {k: v for k, v in prm.items() if k not in ("stop_layer", "bitwise_not")}
    o = oracle.OracleMatcher().set(**prm)
    assert o.learnPattern(t)
    o.set_trace(True)
    res = o.match(s)
    return o, res, len(o.template_levels()[0]) - 1


def fast_records(o, L):
    """Fast-mode candidate records of the oracle's last (traced) search; L = its top layer."""
    cands = o.candidates()
    if L == 0:
        return cands.copy()
    rows = {(int(r["origin"]), int(r["layer"])): r for r in o.trace()}
    out = np.zeros(len(cands), CANDIDATE_DTYPE)
    for f in ("top_score", "angle_index", "peak_rank", "source"):
        out[f] = cands[f]
    for i in range(len(cands)):
        r0 = rows.get((i, 0))
        if r0 is None:
            continue
        out["kept"][i] = 1
        out["x"][i], out["y"][i] = r0["lt"]
        if L >= 2:
            r1 = rows[(i, 1)]
            out["score"][i] = r1["score"][r1["imax"]]
            out["angle"][i] = r1["angle"][r1["imax"]]
        else:
            out["score"][i] = cands["top_score"][i]
            out["angle"][i] = r0["angle"][r0["n3"] // 2]
    return out


def fast_reference(t, s, prm):
    """(fast-mode records, normal-mode oracle matcher, normal-mode results, L) for one search."""
    o, res, L = run_oracle(t, s, prm)
    return fast_records(o, L), o, res, L
