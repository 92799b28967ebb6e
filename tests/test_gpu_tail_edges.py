"""Deterministic edge cases of the detection tail through yh_op_detect, bit for bit against the CPU oracle.
The cases come from tests/tail_cases.py; tests/test_tail_cases.py proves on the oracle alone that each of them does what it
claims (the pair it names is the only overlap, the score sits on the threshold, the cut runs through the tie group, ...), so
equality here is not vacuous. One test per case:

  a  K2's folded pair schedule: every pair (i, j) of K = 2 .. 10 as the only suppression, K = 1, no suppression, the corner
     pairs of K = 255 and 256 - also with most ranks suppressed, so that ranks past max_dets show in the detections
  b  K1 (81-class, generic odd and even class counts): conf_thresh one ulp below, on and one ulp above a score shared by 60
     priors; a single passing prior in lane 0 / lane 63 of a wave and in the first / last row of the ragged last workgroup
  c  conf_thresh = 0 and subnormal probabilities
  d  1, 2, 11, 24, 62 and 64 rows in K1's last workgroup
  e  16384 survivors in K3 (random and all tied); top_k - 1 / top_k / top_k + 1 candidates with a tie on the cut;
     max_dets - 1 / max_dets / max_dets + 1 (+ 3) survivors with a tie group over three classes on the cut
  f  K4's detection groups (gridDim.z = 8, 2, 1 at n = 1, 2 / 3, 8 / 9) with detection counts around the group size, crop windows
     off every edge, outside the map, over the whole map, of a pixel, and ending exactly on a pixel; an empty call and a full
     one after the largest (stale counters and masks)"""
import numpy as np
import pytest

import tail_cases as T

pytestmark = pytest.mark.gpu


def _engine(ya, oracle, case, cfg, max_batch):
    eng = ya.Engine(input_size=case["S"], max_batch=max_batch, use_graph=False, num_classes=case["C"], **cfg)
    pri, hp, wp = T.geometry(oracle, case["S"])
    assert eng.P == len(pri) and (eng.hp, eng.wp) == (hp, wp) and np.array_equal(eng.priors(), pri)   # the CPU self-check's priors
    return eng


def _run(eng, oracle, case, cfg, frames, refs):
    """One yh_op_detect call on the case's frames `frames`; every frame equals the oracle's (refs caches those per frame)."""
    pri = T.geometry(oracle, case["S"])[0]
    idx = list(frames)
    eng.op_detect(case["loc"][idx], case["conf"][idx], case["mask"][idx], case["proto"][idx])
    for k, f in enumerate(idx):
        if f not in refs:
            refs[f] = T.reference(oracle, case, f, pri, cfg)
        d, m = eng.detections(k)
        od, om = refs[f]
        assert T.tuples(d) == T.tuples(od), (case["id"], cfg, idx, k)
        assert np.array_equal(m, om), (case["id"], cfg, idx, k)


@pytest.mark.parametrize("cid", T.CASE_IDS)
def test_tail_edge_case(built, oracle, cid):
    import yolact_amd as ya
    S = T.CASES[T.CASE_IDS.index(cid)][1]
    pri, hp, wp = T.geometry(oracle, S)
    case = T.build(cid, pri, hp, wp)
    n = len(case["loc"])
    if cid.startswith("b_"):
        t = T.probe_score(case, oracle.detect, pri, case["C"])
        runs = [(cfg, [range(n)]) for cfg in T.threshold_cfgs(case, t)]
    elif cid.startswith("f_"):
        runs = [(case["cfg"], case["calls"])]
    else:
        runs = [(case["cfg"], [range(n)])]
    for cfg, calls in runs:
        eng = _engine(ya, oracle, case, cfg, max(len(c) for c in calls))
        try:
            refs = {}
            for frames in calls:
                _run(eng, oracle, case, cfg, frames, refs)
        finally:
            eng.close()
