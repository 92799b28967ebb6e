"""The cases of tests/tail_cases.py, proven on the CPU oracle alone: every builder's inputs do what the case claims, so that the
bit-exact comparison of tests/test_gpu_tail_edges.py cannot pass vacuously (a suppressed rank really has one suppressor, a score
really sits on the threshold, a probability really is subnormal, a cut really runs through a tie group, ...)."""
import numpy as np
import pytest

import tail_cases as T

IDS = T.CASE_IDS


def _case(oracle, cid):
    S = T.CASES[IDS.index(cid)][1]
    pri, hp, wp = T.geometry(oracle, S)
    return T.build(cid, pri, hp, wp), pri, hp, wp


def _by_class(dets, class_id):
    return [d for d in dets if d["class_id"] == class_id]


def test_a_every_nms_pair_has_one_suppressor_and_is_visible(oracle):
    case, pri, _, _ = _case(oracle, "a_nms_pairs")
    subs = case["subs"]
    # the list the issue asks for: K = 1; K = 2 .. 10 without suppression and with every pair; six pairs at K = 255 and 256
    want = {(1, None, None)} | {(K, None, None) for K in range(2, 11)} | {(K, i, j) for K in range(2, 11) for j in range(K) for i in range(j)}
    for K in (255, 256):
        m = K // 2
        want |= {(K, 0, K - 1), (K, m - 1, m), (K, 0, m), (K, 3, m), (K, m, m + 1), (K, K - 2, K - 1)}
    assert {(s["K"], s["i"], s["j"]) for s in subs if not s["dense"]} == want
    assert {(s["K"], s["i"], s["j"]) for s in subs if s["dense"]} == {w for w in want if w[0] > 10}
    assert case["cfg"] == dict(top_k=256, max_dets=128, conf_thresh=0.05, nms_thresh=0.5)
    refs = [T.reference(oracle, case, f, pri)[0] for f in range(len(case["loc"]))]
    seen = set()
    for s in subs:
        K, i, j, pr = s["K"], s["i"], s["j"], s["priors"]
        assert (s["frame"], s["class_id"]) not in seen
        seen.add((s["frame"], s["class_id"]))
        got = _by_class(refs[s["frame"]], s["class_id"])
        sc = [d["score"] for d in got]
        assert all(a > b for a, b in zip(sc, sc[1:]))                       # distinct after f16 rounding and softmax
        if j is None:
            assert s["kept"] == pr
        else:
            assert s["sup"][j] == [i]                                       # i is the only box that overlaps j
            assert pr[j] not in s["kept"] and pr[i] in s["kept"]
        if not s["dense"]:
            assert s["kept"] == [p for r, p in enumerate(pr) if r != j]     # the other ranks do not miss
        if K > 10 and not s["dense"]:
            assert [d["prior"] for d in got] == s["kept"][:128] and len(refs[s["frame"]]) == 128
        else:
            # every survivor is in the output, and so would be one too many
            assert len(refs[s["frame"]]) <= 127
            assert [d["prior"] for d in got] == s["kept"]
        if s["dense"]:
            assert len(s["kept"]) <= 102 and j >= T.DENSE_BASE                  # (so ranks past max_dets are visible too)


@pytest.mark.parametrize("cid", [c for c in IDS if c.startswith("b_")])
def test_b_score_on_the_threshold(oracle, cid):
    case, pri, _, _ = _case(oracle, cid)
    C, P, cls, group = case["C"], len(pri), case["class_id"], case["group"]
    assert len(group) >= 40 and case["cfg"]["nms_thresh"] == 1.0 and case["cfg"]["max_dets"] == 128
    t = T.probe_score(case, oracle.detect, pri, C)
    cfgs = T.threshold_cfgs(case, t)
    th = [np.float32(c["conf_thresh"]) for c in cfgs]
    assert th[1] == t and th[0] < t < th[2] and np.nextafter(th[0], np.float32(1)) == t and np.nextafter(t, np.float32(1)) == th[2]
    lo, at, up = ([T.tuples(T.reference(oracle, case, f, pri, c)[0]) for f in range(5)] for c in cfgs)
    ingroup = [x for x in lo[0] if x[0] == cls and x[1] in group]
    assert sorted(x[1] for x in ingroup) == group and all(np.float32(x[2]) == t for x in ingroup)      # below: the whole group
    assert [x for x in lo[0] if x not in ingroup] == at[0] == up[0]                                  # on and above: none of it
    assert all(T.k1_place(C, p)[0] == 0 for p in group)                     # the group's waves hold nobody above the threshold:
    assert all(T.k1_place(C, x[1])[0] == 1 for x in at[0] if x[0] == cls)   # the class's other candidates are in the other workgroup
    others = [x[2] for x in at[0]]
    assert len(at[0]) >= 20 and min(others) > 2 * t and any(x[0] == cls for x in at[0])              # clearly above
    assert len(lo[0]) < 128
    last_wg = (P // 3 - 1) // 64
    for f, name, p in case["singles"]:
        wg, wave, lane = T.k1_place(C, p)
        if name == "lane0":
            assert lane == 0 and wg == 0
        elif name == "lane63":
            assert lane == 63 and wg == 0
        elif name == "ragged_first":
            assert wg == last_wg and p // 3 == last_wg * 64
        else:
            assert wg == last_wg and p // 3 == P // 3 - 1
        assert [x[1] for x in lo[f] if x[0] == cls] == [p]                                           # exactly one prior passes
        assert [x for x in lo[f] if x[0] != cls] == at[f] == up[f] and len(at[f]) > 0
        # every other prior is far below in that class: the row's class logit is OFF
        assert np.all(np.delete(case["conf"][f, :, cls + 1], p) == T.OFF)


@pytest.mark.parametrize("cid", [c for c in IDS if c.startswith("c_")])
def test_c_subnormal_probabilities_are_detections(oracle, cid):
    case, pri, _, _ = _case(oracle, cid)
    assert case["cfg"]["conf_thresh"] == 0.0
    conf = case["conf"][0]
    top = conf.max(1, keepdims=True)
    assert np.all((conf == top).sum(1) >= 2) and np.all((conf == top) | (conf <= top - 86.75))   # s >= 2, the rest 86.75+ below
    dets, _ = T.reference(oracle, case, 0, pri)
    sub = [d for d in dets if 0.0 < d["score"] < 2.0 ** -126]
    assert len(dets) == case["C"] - 1 and len(sub) >= case["C"] - 3
    assert len({d["score"] for d in sub}) >= 2


@pytest.mark.parametrize("cid", [c for c in IDS if c.startswith("d_")])
def test_d_ragged_last_workgroup_holds_detections(oracle, cid):
    case, pri, _, _ = _case(oracle, cid)
    P = len(pri)
    assert T.k1_last_rows(P) == T.RAGGED_SIZES[case["S"]]
    for f in range(2):
        dets, _ = T.reference(oracle, case, f, pri)
        got = {d["prior"] for d in dets}
        assert got & set(case["last_cell"]) and got & {0, 1, 2}
        assert len(dets) > 10


def test_e1_sixteen_thousand_survivors(oracle):
    case, pri, _, _ = _case(oracle, "e1_full_keys")
    assert case["C"] == 65 and case["cfg"]["top_k"] == 256 and len(pri) >= 256
    d0, _ = T.reference(oracle, case, 0, pri)
    d1, _ = T.reference(oracle, case, 1, pri)
    assert len(d0) == 128 and len(d1) == 128
    assert len({d["class_id"] for d in d0}) > 5 and len({d["score"] for d in d0}) > 5
    assert len({d["score"] for d in d1}) == 1 and [(d["class_id"], d["prior"]) for d in d1] == [(0, p) for p in range(128)]
    # every (class, prior) is a candidate: the lowest probability of either frame is above the threshold
    z = case["conf"].astype(np.float64)
    pr = np.exp(z) / np.exp(z).sum(2, keepdims=True)
    assert pr[:, :, 1:].min() > 2 * case["cfg"]["conf_thresh"]


@pytest.mark.parametrize("cid", [c for c in IDS if c.startswith("e2_")])
def test_e2_candidates_around_top_k(oracle, cid):
    case, pri, _, _ = _case(oracle, cid)
    tk = case["cfg"]["top_k"]
    assert [fr["m"] for fr in case["frames"]] == [tk - 1, tk, tk + 1]
    for f, fr in enumerate(case["frames"]):
        dets, _ = T.reference(oracle, case, f, pri)
        assert all(d["class_id"] == case["class_id"] for d in dets) and len(dets) <= 127
        assert [d["prior"] for d in dets] == fr["kept"]
        if fr["m"] >= 1:
            assert fr["ranked"][min(fr["m"], tk) - 1] in fr["kept"]               # the last rank inside the cut is a detection
    fr = case["frames"][2]
    a, b = fr["ranked"][tk - 1], fr["ranked"][tk]
    assert fr["logits"][tk - 1] == fr["logits"][tk] and a < b and a in fr["kept"] and b not in fr["kept"]   # a tie: prior order decides


@pytest.mark.parametrize("cid", [c for c in IDS if c.startswith("e3_")])
def test_e3_survivors_around_max_dets(oracle, cid):
    case, pri, _, _ = _case(oracle, cid)
    md = case["cfg"]["max_dets"]
    assert [fr["m"] for fr in case["frames"]][:3] == [md - 1, md, md + 1]
    for f, fr in enumerate(case["frames"]):
        m, tie = fr["m"], fr["tie"]
        dets, _ = T.reference(oracle, case, f, pri)
        assert len(dets) == min(m, md)
        full = T.reference(oracle, case, f, pri, dict(case["cfg"], max_dets=256))[0]
        assert len(full) == m                                                    # m survivors, nothing suppressed
        ts = {d["score"] for d in full if (d["class_id"], d["prior"]) in tie}
        assert len(ts) <= 1 and all(d["score"] > s for s in ts for d in full if (d["class_id"], d["prior"]) not in tie)
        kept = [(d["class_id"], d["prior"]) for d in dets if (d["class_id"], d["prior"]) in tie]
        assert len(tie) == min(6, m) and len({c for c, _ in tie}) == min(3, len(tie))
        if m <= md:
            assert sorted(kept) == sorted(tie)
        else:
            assert 0 < len(kept) < len(tie)                                      # the cut splits the tie group
            assert kept == sorted(tie)[:len(tie) - (m - md)]                     # class, then rank (= prior), decide
            assert kept != sorted(tie, key=lambda x: x[1])[:len(kept)]           # ... and prior order alone would not


@pytest.mark.parametrize("cid", [c for c in IDS if c.startswith("f_")])
def test_f_mask_groups_and_crop_windows(oracle, cid):
    case, pri, hp, wp = _case(oracle, cid)
    md, counts, kinds = case["cfg"]["max_dets"], case["counts"], case["kinds"]
    for z in (8, 2, 1):
        per = T.mask_group_size(md, z)
        assert {c for c in (0, 1, 3, 4, 5, per - 1, per, per + 1, md) if c <= md} <= set(counts)
    ns = {len(c) for c in case["calls"]}
    assert ns == set(T.MASK_BATCHES) and max(len(c) for c in case["calls"]) == 9
    nc = len(set(counts))
    assert sorted(counts[:nc]) == sorted(set(counts)) and all(c == md for c in counts[nc:])
    for n in T.MASK_BATCHES:                                                    # every count runs under every batch size
        assert {f for c in case["calls"][:-2] if len(c) == n for f in c} == set(range(nc))
    for c in case["calls"][:-2]:                                                # the frames of a call have different counts
        assert len({counts[f] for f in c}) == min(len(c), nc)
    assert all(counts[f] == 0 for f in case["calls"][-2]) and all(counts[f] == md for f in case["calls"][-1])
    assert len(case["calls"][-1]) == 9 and len(set(case["calls"][-1])) == 9
    assert np.all(case["proto"] > 0)
    pe, kx, ky = case["exact"]
    seen, first_row, last_row, pos_and_neg = set(), False, False, False
    for f, k in enumerate(counts):
        dets, masks = T.reference(oracle, case, f, pri)
        assert [d["prior"] for d in dets] == [p for p, _ in kinds[f]] and len(dets) == k
        for d, m, (p, kind) in zip(dets, masks, kinds[f]):
            seen.add(kind)
            acc = case["proto"][f].astype(np.float64) @ case["mask"][f, p].astype(np.float64)
            sure = np.abs(acc) > 1e-3
            if kind.startswith("out_"):
                assert not m.any()
            elif kind == "whole":
                assert np.array_equal(m[sure] > 0, acc[sure] > 0) and m.any() and not m.all()
                pos_and_neg = True
            else:
                assert m.any() and not np.array_equal(m[sure] > 0, acc[sure] > 0)          # a non-empty proper subset
                assert not (m[sure] > 0)[acc[sure] <= 0].any()
            if kind == "exact":
                x1, y2 = np.float32(d["box"][0]) * np.float32(wp), np.float32(d["box"][3]) * np.float32(hp)
                assert p == pe and x1 == kx and y2 == ky and 2 <= kx <= wp - 2 and 2 <= ky <= hp - 2
                cols, rows = np.nonzero(m.any(0))[0], np.nonzero(m.any(1))[0]
                assert cols.min() == kx - 1 and rows.max() == ky           # (coefficients >= 0: the mask is the window)
            first_row |= bool(m[0].any())
            last_row |= bool(m[-1].any())
    assert seen >= set(T.KINDS) and first_row and last_row and pos_and_neg
