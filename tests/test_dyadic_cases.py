"""The cases of tests/dyadic_cases.py keep what tests/test_gpu_rounding.py rests on (CPU only). For every case, with G = 12:
  - every operand is f16-representable and a multiple of its grid, every bias and residual a multiple of 2^-G;
  - (sum |x| |w| + |bias| + |res|) * 2^G < 2^22. Every product is a multiple of 2^-G, so every partial sum of every summation
    order is one too, and its magnitude is below that bound: an integer below 2^22 times 2^-G. float32 has 24 significant bits, so
    it holds each of them exactly, with two bits to spare. A kernel's float32 accumulator, the split-K slabs and their sum, the
    bias and residual additions are therefore all exact whatever their order, the value that reaches the final conversion is the
    exact one, and bit equality with one round-to-nearest-even of it is the right bar;
  - every reference value is finite and below 65504 (no f16 overflow hides a difference), at least a quarter are nonzero;
  - at least 10 % of the nonzero outputs differ from their exact float64 value: the rounding really happens;
  - at least 1 % of the nonzero outputs are exact ties between two f16 neighbours: ties-to-even is exercised;
  - each of the three mutants of the reference (rounds toward zero; f16 partial sums over the halves of K; rounds before bias and
    residual are added) differs from it on at least 5 % of the nonzero outputs: a kernel with that mistake fails the GPU test;
  - oracle.conv2d(..., f16=True), which accumulates in float32 in an order of its own, returns the same bits as the float64
    reference: on the CPU, proof that the data is exact in float32.
The fp8 cases (integer codes, fractional epilogue): the bound, the rounding share and the round-toward-zero mutant; the float32
expression of test_conv_fp8_exact_on_integers gives the reference's bits.
These are conditions on the cases. A case that breaks one is changed; the bounds stay. profiles/rounding_cases.txt holds each
case's actual shares (python tests/test_dyadic_cases.py prints them)."""
import numpy as np
import pytest

import dyadic_cases as D


def _on_grid(v, g):
    v = np.asarray(v, np.float64) * 2.0 ** g
    return np.array_equal(v, np.rint(v))


def _is_f16(v):
    return v.dtype == np.float32 and np.array_equal(v, v.astype(np.float16).astype(np.float32))


def test_cases_are_the_shapes_the_gpu_test_runs():
    assert len(D.CASE_IDS) == len(set(D.CASE_IDS)) and set(D.F16_IDS) | set(D.FP8_IDS) == set(D.CASE_IDS) and len(D.FP8_IDS) == 3
    for cid in D.CASE_IDS:
        c = D.build(cid)
        assert c["g"] == D.G == 12 and D.reference(c).shape == D.exact(c).shape == D.magnitude(c).shape
        assert not any(v.flags.writeable for v in c.values() if isinstance(v, np.ndarray))
        assert not D.reference(c).flags.writeable


def test_rounding_helpers():
    """rtz16 and is_tie on hand-made values: 1 + 2^-11 is the tie between 1 and 1 + 2^-10 (even: 1), 1 + 3 * 2^-11 the next one
    (even: 1 + 2^-9), both signs."""
    u = 2.0 ** -10
    v = np.array([1.0, 1 + u / 2, 1 + u, 1 + 3 * u / 2, 1 + u / 4, 1 + 3 * u / 4, -1 - u / 2, -1 - 3 * u / 4, 0.0, 2.0 ** -24 * 1.5])
    assert np.array_equal(D.rtz16(v), np.array([1, 1, 1 + u, 1 + u, 1, 1, -1, -1, 0, 2.0 ** -24], np.float32))
    assert np.array_equal(v.astype(np.float16).astype(np.float64), [1, 1, 1 + u, 1 + 2 * u, 1, 1 + u, -1, -1 - u, 0, 2.0 ** -23])
    assert D.is_tie(v).tolist() == [False, True, False, True, False, False, True, False, False, True]


@pytest.mark.parametrize("cid", D.F16_IDS)
def test_case_conditions(oracle, cid):
    c = D.build(cid)
    kind = c["kind"]
    for k in ("x", "x1", "x2", "w", "res"):
        if c.get(k) is not None:
            assert _is_f16(c[k]) and _on_grid(c[k], 6) and len(np.unique(c[k])) > 60, k
            assert np.abs(c[k]).max() <= (2.0 if k == "res" or (kind == "stem" and k == "x") else 0.5), k
    assert c["bias"].dtype == np.float32 and _on_grid(c["bias"], D.G) and np.abs(c["bias"]).max() <= 2 and not _on_grid(c["bias"], 8)
    assert D.magnitude(c).max() * 2.0 ** D.G < 2.0 ** 22, float(np.log2(D.magnitude(c).max()) + D.G)
    v, ref = D.exact(c), D.reference(c)
    assert _on_grid(v, D.G)
    assert np.isfinite(ref).all() and np.abs(ref).max() < 65504
    s = D.shares(c)
    assert s["nonzero"] >= 0.25, s
    assert s["rounded"] >= 0.10, s
    assert s["tie"] >= 0.01, s
    for name in D.MUTANTS:
        assert s[name] >= 0.05, (name, s)
    # the oracle: float32 accumulation, its own order
    if kind == "levels":
        n, cells, cin = c["x"].shape
        got, off = [], 0
        for sz in c["sizes"]:
            xl = c["x"][:, off:off + sz * sz].reshape(n, sz, sz, cin)
            got.append(oracle.conv2d(xl, c["w"], c["bias"], 1, c["pad"], None, c["act"], f16=True).reshape(n, sz * sz, -1))
            off += sz * sz
        got = np.concatenate(got, 1)
    elif kind == "dual":
        got = oracle.conv2d(D.dual_cat(c), c["w"][:, None, None, :], c["bias"], 1, 0, None, c["act"], f16=True)
    else:
        got = oracle.conv2d(c["x"], c["w"], c["bias"], c["stride"], c["pad"], c["res"], c["act"], f16=True)
    assert got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("cid", D.FP8_IDS)
def test_fp8_case_conditions(oracle, cid):
    c = D.build(cid)
    table = oracle.e4m3_decode_table()
    for k, lim in (("xi", 4), ("wi", 3)):      # the codes carry the integers exactly
        assert np.array_equal(c[k], np.rint(c[k])) and np.abs(c[k]).max() == lim and np.array_equal(table[oracle.quantize_e4m3(c[k])], c[k])
    assert set(np.log2(c["scale"]).tolist()) == set(range(-9, -3))
    assert _on_grid(c["bias"], D.G) and np.abs(c["bias"]).max() <= 2
    if c["res"] is not None:
        assert _is_f16(c["res"]) and _on_grid(c["res"], 10) and np.abs(c["res"]).max() <= 2
    assert D.magnitude(c).max() * 2.0 ** D.G < 2.0 ** 22
    ref = D.reference(c)
    assert _on_grid(D.exact(c), D.G) and np.isfinite(ref).all() and ref.max() < 65504
    s = D.shares(c)
    assert s["nonzero"] >= 0.25 and s["rounded"] >= 0.10 and s["rtz"] >= 0.05, s
    acc = oracle.conv2d(c["xi"], c["wi"], np.zeros(len(c["bias"]), np.float32), c["stride"], c["pad"], None, 0, f16=False)
    want = acc * c["scale"] + c["bias"]
    if c["res"] is not None:
        want = want + c["res"]
    assert want.dtype == np.float32 and np.array_equal(np.maximum(want, 0).astype(np.float16).astype(np.float32), ref)


def report():
    lines = ["case               nonzero  rounded  ties   rtz    f16_partials  round_before_side  log2(bound * 2^12)"]
    for cid in D.CASE_IDS:
        s = D.shares(D.build(cid))
        lines.append(f"{cid:18s} {s['nonzero']:7.3f} {s['rounded']:8.3f} {s['tie']:5.3f} {s['rtz']:6.3f} {s['f16_partials']:13.3f} {s['round_before_side']:18.3f} {s['bits']:19.2f}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
