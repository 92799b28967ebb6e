"""CPU: every case of tests/tfl_detect_cases.py does what it claims, and the restatement tests/tfl_detect_ref.py relates to
oracle.detect as DESIGN.md §11 "TFLite detections" says: equal to it, masks included, with power-of-two scales; equal on the
detections and on every mask pixel outside the band |S| < BAND with the scales 0.05 / 0.0173."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfl_detect_cases as K
import tfl_detect_ref as R


def _run(oracle, case, b=0, cfg=None, sums=False):
    return R.detect(oracle, R.image(case, b), case["quant"], case["priors"], cfg or case["cfg"], want_sums=sums)


@pytest.mark.parametrize("combo", list(K.COMBOS))
def test_power_of_two_scales_restatement_is_the_oracle(oracle, combo):
    kinds = K.COMBOS[combo]
    for zi in range(3):
        zps = tuple(0 if k == "f32" else K.ZPS[k][zi] for k in kinds)
        case = K.random_case(kinds, zps, 2, 6, 16, 16, 100 + zi)
        for b in range(2):
            dets, masks = _run(oracle, case, b)
            odets, omasks = R.oracle_on_values(oracle, R.image(case, b), case["quant"], case["priors"], case["cfg"])
            assert R.tuples(dets) == R.tuples(odets) and np.array_equal(masks, omasks)
            if zi == 1:
                assert len(dets) > 20 and masks.any() and not masks.all(), (combo, len(dets))


def test_odd_scales_agree_outside_the_band_and_the_band_is_met(oracle):
    in_band = 0
    for seed, case in ((0, K.band()), (1, K.random_case(K.COMBOS["all_u8"], (128, 128, 100, 17), 1, 6, 16, 16, 7, scales=K.ODD)),
                       (2, K.random_case(K.COMBOS["all_i8"], (0, 0, -3, -128), 1, 6, 16, 16, 8, scales=K.ODD))):
        dets, masks, S, win = _run(oracle, case, sums=True)
        odets, omasks = R.oracle_on_values(oracle, R.image(case, 0), case["quant"], case["priors"], case["cfg"])
        assert R.tuples(dets) == R.tuples(odets) and len(dets) >= 1
        far = np.abs(S) >= R.BAND
        assert np.array_equal(masks[far], omasks[far])
        in_band += int((win & ~far & (S != 0)).sum())
    assert in_band > 0


def test_band_case_rows(oracle):
    case = K.band()
    dets, masks, S, win = _run(oracle, case, sums=True)
    assert [d["prior"] for d in dets] == [40] and win[0].all()
    for row, want in case["rows"].items():
        assert (S[0, row] == want).all() and (masks[0, row] == (1 if want > 0 else 0)).all()
    assert (S[0, 0] == 0).all() and not masks[0, 0].any()          # S = 0 inside a crop window: off by rule 3


def test_ties(oracle):
    case = K.ties()
    dets, _ = _run(oracle, case)
    assert dets[0]["prior"] == 200
    tied = dets[1:]
    assert [(d["class_id"], d["prior"]) for d in tied] == case["tied"] and len({R.bits(d["score"]) for d in tied}) == 1


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_topk_cut(oracle, delta):
    case = K.topk_cut(8 + delta)
    dets, _ = _run(oracle, case)
    assert len(dets) == min(8 + delta, 8)
    kept = [d["prior"] for d in dets]
    assert len({R.bits(d["score"]) for d in dets[-2:]}) == 1
    if delta == 1:
        assert case["tie_priors"][2] not in kept and kept[-2:] == case["tie_priors"][:2]
    else:
        assert kept[-3:] == case["tie_priors"]


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_dets_cut(oracle, delta):
    case = K.dets_cut(6 + delta)
    dets, _ = _run(oracle, case)
    assert len(dets) == min(6 + delta, 6)
    want = case["tie_classes"][:2] if delta == 1 else case["tie_classes"]
    assert [d["class_id"] for d in dets[-len(want):]] == want and len({R.bits(d["score"]) for d in dets[-len(want):]}) == 1


def test_suppress_pair(oracle):
    for on in (False, True):
        case = K.suppress_pair(on)
        dets, _ = _run(oracle, case)
        assert [d["prior"] for d in dets] == ([20] if on else [20, 21])
        v = R.values(R.image(case, 0), case["quant"])
        boxes = K.decode(case["priors"][[20, 21]], v["loc"][[20, 21]])
        assert K.suppressors(boxes, 0.5) == ([[], [0]] if on else [[], []])


def test_threshold_group(oracle):
    case = K.threshold_group()
    dets, _ = _run(oracle, case)
    shared = [d for d in dets if d["prior"] in case["shared_priors"]]
    assert len(dets) == 6 and len(shared) == 5 and len({R.bits(d["score"]) for d in shared}) == 1
    below, on, above = K.thresholds(shared[0]["score"])
    for t, n in ((below, 6), (on, 1), (above, 1)):                  # (a candidate needs score > conf_thresh)
        assert len(_run(oracle, case, cfg=dict(case["cfg"], conf_thresh=t))[0]) == n


def test_empty_then_full(oracle):
    empty, full = K.empty_then_full()
    for b in range(2):
        assert _run(oracle, empty, b)[0] == []
        dets, masks = _run(oracle, full, b)
        assert len(dets) > 20 and masks.any()


def test_windows(oracle):
    case = K.windows()
    dets, masks, S, win = _run(oracle, case, sums=True)
    assert (S > 0).all() and np.array_equal(masks, win.astype(np.uint8))
    by_prior = {d["prior"]: i for i, d in enumerate(dets)}
    for pr, name in zip(case["at"], case["names"]):
        x0, x1, y0, y1 = K.WINDOWS[name][1]
        want = np.zeros((16, 16), bool)
        want[y0:y1, x0:x1] = True
        assert np.array_equal(win[by_prior[pr]], want), name


@pytest.mark.parametrize("sign", (1, -1))
def test_saturated(oracle, sign):
    for combo in ("all_u8", "all_i8", "u8proto_i8mask"):
        case = K.saturated(sign, K.COMBOS[combo])
        dets, masks, S, win = _run(oracle, case, sums=True)
        assert len(dets) >= 5 and (S == case["S"]).all() and abs(case["S"]) == 32 * 255 * 255
        assert np.array_equal(masks, win.astype(np.uint8) if sign > 0 else np.zeros_like(masks))
        assert all(np.isfinite(d["box"]).all() for d in dets)
