"""The cases of tests/bneck_cases.py keep what tests/test_gpu_bneck_op.py rests on (CPU only). For every integer case:
  - sum |x| |w| + |bias| + |res| stays below 2^24 at each of the three stages, so every partial sum of every summation order is an
    integer float32 holds exactly, and bit equality with the kernels is the right bar;
  - every reference value is finite and below 65504 (no f16 overflow hides a difference);
  - at least a quarter of each of b, y and a' is nonzero and each has more than 8 distinct values (the ReLUs do not blank the case);
  - oracle.conv2d(..., f16=True) chained three times gives the same arrays: the numpy reference agrees with the oracle the
    rest of the suite trusts.
The dyadic case of every form has conditions of its own (test_dyadic_case_conditions): a bound of 2^22 on its grid, and rounding
that really happens at every stage.
These are conditions on the cases. A case that breaks one is changed; the bounds stay."""
import os
import re

import numpy as np
import pytest

import bneck_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE_CASES = [(planes, cid) for planes, form in ((64, "bneck_chain_f16<64,64,next>"), (64, "bneck_chain_f16<64,128,next,dual>"),
                                                  (128, "bneck_chain_f16<128,64,next>"), (256, B.XN))
               for cid in B.case_ids(form) if not cid.startswith(B.REAL) and not cid.startswith(B.DYADIC)]
DYADIC_CASES = [(64, B.DYADIC), (64, B.DYADIC + "_x2s1"), (128, B.DYADIC), (256, B.DYADIC)]


def test_forms_are_the_rows_of_the_kernel_table():
    """FORMS names every row of kBneckChains (csrc/bneck.hip) by the symbol bneck_symbol gives it, with the row's own key, plus
    bneck_xn_f16: a new row without cases fails here."""
    src = open(os.path.join(ROOT, "tiny-object-detection_amd", "csrc", "bneck.hip")).read()
    table = src[src.index("constexpr BneckChain kBneckChains[] = {"):]
    table = table[:table.index("};")]
    rows = re.findall(r"\{\s*(\d+),\s*(\d+),\s*(true|false),\s*(true|false),\s*bneck_chain_f16<[^>]*>,\s*\"([^\"]+)\"\s*\}", table)
    assert len(rows) == table.count("bneck_chain_f16<") // 2 == 11
    got = [(sym, int(pl), int(tm), nx == "true", du == "true") for pl, tm, nx, du, sym in rows]
    assert got == B.FORMS[:-1] and B.FORMS[-1] == (B.XN, 256, 64, True, False)
    assert '"bneck_xn_f16"' in src
    for sym, pl, tm, nx, du in got:
        assert sym == "bneck_chain_f16<%d,%d%s%s>" % (pl, tm, ",next" if nx else "", ",dual" if du else "")


def test_every_form_has_every_shape():
    for sym, planes, tm, nxt, dual in B.FORMS:
        ids = B.case_ids(sym)
        assert len(ids) == len(set(ids))
        for sid, n, H, W, stride, gap in B.SHAPES:
            if dual:
                assert f"{sid}_x2s1" in ids and f"{sid}_x2s2" in ids
            elif planes == 256:
                assert (sid in ids) == (stride == 1)
            else:
                assert sid in ids
        assert sum(i.startswith(B.REAL) for i in ids) == 1
        assert [i for i in ids if i.startswith(B.DYADIC)] == [B.DYADIC + ("_x2s1" if dual else "")]
    ms = {n * B.out_dim(H, s) * B.out_dim(W, s) for _, n, H, W, s, _ in B.SHAPES}
    assert {1, 63, 64, 70, 65, 128, 129, 255, 256, 257, 231, 646} <= ms
    assert all(H != W for _, n, H, W, s, _ in B.SHAPES if n > 1)


@pytest.mark.parametrize("planes,cid", PLANE_CASES, ids=[f"{p}-{c}" for p, c in PLANE_CASES])
def test_case_conditions(oracle, planes, cid):
    c = B.build(planes, cid)
    assert c["M"] == c["n"] * c["P"] * c["Q"]
    for k in ("a", "w2", "w3", "w1n", "res", "x2"):
        if c[k] is not None:
            assert c[k].dtype == np.float32 and np.array_equal(c[k], np.rint(c[k])), k
    lo, hi = (0, 3) if c["xn"] else (-3, 3)
    assert c["a"].min() >= lo and c["a"].max() <= hi
    assert all(np.abs(c[k]).max() <= 1 for k in ("w2", "w3", "w1n")) and all(np.abs(c[k]).max() <= 4 for k in ("bias2", "bias3", "bias1n"))
    assert np.abs(c["res"] if c["res"] is not None else c["x2"]).max() <= 5
    if c["x2"] is not None:   # x2 just covers the strided output grid; at stride2 = 2 its row length is not what a P / Q mix-up expects
        s2 = c["stride2"]
        assert c["x2"].shape[1:3] == ((c["P"], c["Q"]) if s2 == 1 else (2 * c["P"] - 1, 2 * c["Q"]))
        assert (c["P"] - 1) * s2 < c["x2"].shape[1] and (c["Q"] - 1) * s2 < c["x2"].shape[2]
    bounds, _ = B.stages(c, absolute=True)
    for i, s in enumerate(bounds):
        if s is not None:
            assert s.max() < 2.0 ** 24, (i, float(s.max()))
    ref = B.reference(c, oracle)
    for k in ("b", "y", "a_next"):
        v = ref[k]
        assert np.isfinite(v).all() and v.max() < 65504, k
        if not (c["xn"] and k == "b"):
            assert v.min() == 0
        assert np.count_nonzero(v) >= v.size / 4, (k, np.count_nonzero(v) / v.size)
        assert len(np.unique(v)) > 8 or (c["xn"] and k == "b"), k      # (bneck_xn_f16's b is the input: 0 .. 3)
    # the same three convolutions through the oracle
    one = lambda w: w[:, None, None, :]
    b = c["a"] if c["xn"] else oracle.conv2d(c["a"], c["w2"], c["bias2"], c["stride"], 1, None, 1, f16=True)
    k = np.concatenate([b, B._x2_rows(c)], -1) if c["x2"] is not None else b
    y = oracle.conv2d(k, one(c["w3"]), c["bias3"], 1, 0, c["res"], 1, f16=True)
    an = oracle.conv2d(y, one(c["w1n"]), c["bias1n"], 1, 0, None, 1, f16=True)
    assert np.array_equal(b, ref["b"]) and np.array_equal(y, ref["y"]) and np.array_equal(an, ref["a_next"])
    if c["xn"]:
        codes = ref["a_next8"]
        assert codes.shape == an.shape and len(np.unique(codes)) > 8 and len(np.unique(c["inv_scale"])) == 5
        for ch in (0, 63, 64, 255):   # per channel: the oracle's quantiser with that channel's scalar
            assert np.array_equal(codes[..., ch], oracle.quantize_e4m3(an[..., ch], float(c["inv_scale"][ch])))


@pytest.mark.parametrize("planes,cid", DYADIC_CASES, ids=[f"{p}-{c}" for p, c in DYADIC_CASES])
def test_dyadic_case_conditions(oracle, planes, cid):
    """The dyadic case of every form (bneck_cases.DYADIC_GRIDS). Per stage, with that stage's grid 2^-g:
      - every operand is f16-representable and a multiple of its grid, every bias a multiple of 2^-g;
      - (sum |x| |w| + |bias| + |res|) * 2^g < 2^22: every partial sum of every summation order is a multiple of 2^-g below
        2^(22 - g), an integer of at most 22 bits times 2^-g, which float32 holds exactly with two bits to spare - so a kernel's
        float32 accumulator is the exact sum whatever its order, and bit equality with reference() is the right bar;
      - every value is finite and below 65504, at least a quarter of b, y and a' is nonzero;
      - at least 10 % of the nonzero b, y and a' differ from their exact float64 value: the f16 rounding really happens;
      - y computed from an unrounded b, and a' from an unrounded y, differ from the reference on at least 5 % of its nonzero
        elements (the bar tests/test_dyadic_cases.py sets its mutants): a chain that keeps more than f16 between stages fails;
      - oracle.conv2d(..., f16=True) chained three times (float32 accumulation) gives the same arrays."""
    c = B.build(planes, cid)
    assert c["dyadic"] and not c["real"] and (c["n"], c["H"], c["W"]) == (3, 7, 11) and (c["x2"] is not None) == cid.endswith("_x2s1")
    g1, g2, g3 = c["g"]
    on_grid = lambda v, g: np.array_equal(v * 2.0 ** g, np.rint(v * 2.0 ** g))
    for k, g in (("a", g1), ("w2", g1), ("bias2", g1), ("x2", g1), ("w3", g2), ("bias3", g2), ("res", g2), ("w1n", g3), ("bias1n", g3)):
        if c[k] is not None and not (c["xn"] and k in ("w2", "bias2")):
            assert c[k].dtype == np.float32 and on_grid(c[k].astype(np.float64), g), k
            if not k.startswith("bias"):
                assert np.array_equal(c[k], B.h16(c[k])) and len(np.unique(c[k])) >= 3, k
    if c["xn"]:
        assert c["a"].min() == 0
    sums, (b, y, an) = B.stages(c)
    bounds, _ = B.stages(c, absolute=True)
    for name, s, bound, g, r in zip(("b", "y", "a_next"), sums, bounds, c["g"], (b, y, an)):
        if s is None:           # bneck_xn_f16: b is the input
            continue
        assert bound.max() * 2.0 ** g < 2.0 ** 22, (name, float(np.log2(bound.max()) + g))
        assert on_grid(s, g), name
        assert np.isfinite(r).all() and r.max() < 65504 and r.min() == 0, name
        nz = r != 0
        assert nz.sum() >= r.size / 4, (name, float(nz.mean()))
        rounded = (r.astype(np.float64) != np.maximum(s, 0)) & nz
        assert rounded.sum() >= 0.10 * nz.sum(), (name, float(rounded.sum() / nz.sum()))
    # a chain that hands b or y to the next stage unrounded (float32 in LDS or registers) differs where it can be seen
    d = lambda v: np.asarray(v, np.float64)
    differs = lambda got, want: ((got != want) & (want != 0)).sum() / (want != 0).sum()
    if not c["xn"]:
        wide = np.maximum(sums[0], 0)
        k = np.concatenate([wide, d(B._x2_rows(c))], -1) if c["x2"] is not None else wide
        y_wide = B.h16(np.maximum(k @ d(c["w3"]).T + d(c["bias3"]) + (d(c["res"]) if c["res"] is not None else 0.0), 0))
        assert differs(y_wide, y) >= 0.05
    assert differs(B.h16(np.maximum(np.maximum(sums[1], 0) @ d(c["w1n"]).T + d(c["bias1n"]), 0)), an) >= 0.05
    ref = B.reference(c, oracle)
    assert np.array_equal(ref["b"], b) and np.array_equal(ref["y"], y) and np.array_equal(ref["a_next"], an)
    one = lambda w: w[:, None, None, :]
    ob = c["a"] if c["xn"] else oracle.conv2d(c["a"], c["w2"], c["bias2"], c["stride"], 1, None, 1, f16=True)
    k = np.concatenate([ob, B._x2_rows(c)], -1) if c["x2"] is not None else ob
    oy = oracle.conv2d(k, one(c["w3"]), c["bias3"], 1, 0, c["res"], 1, f16=True)
    oan = oracle.conv2d(oy, one(c["w1n"]), c["bias1n"], 1, 0, None, 1, f16=True)
    assert np.array_equal(ob, b) and np.array_equal(oy, y) and np.array_equal(oan, an)
    if c["xn"]:
        assert ref["a_next8"].shape == an.shape and len(np.unique(ref["a_next8"])) > 8


def test_real_valued_cases_are_f16_and_cover_every_form():
    for sym, planes, tm, nxt, dual in B.FORMS:
        (cid,) = [i for i in B.case_ids(sym) if i.startswith(B.REAL)]
        c = B.build(planes, cid)
        assert c["real"] and (c["n"], c["H"], c["W"]) == (3, 7, 11) and (c["x2"] is not None) == dual
        for k in ("a", "w2", "w3", "w1n", "res", "x2"):
            if c[k] is not None:
                assert np.array_equal(c[k], B.h16(c[k])) and len(np.unique(c[k])) > 100, k
