"""The cases of tests/range_cases.py keep what tests/test_gpu_range.py rests on (CPU only). For every variant, with G = 12 and t the
channel's total exponent:
  - every scaled x, w and residual is still an f16 value, every bias a float32 multiple of the grid 2^(t - G);
  - (sum |x| |w| + |bias| + |res|) / 2^(t - G) < 2^22: the bound of tests/test_dyadic_cases.py, re-proved on the scaled tensors, so a
    float32 accumulator of any summation order holds the exact sum and bit equality with one rounding of it is the right bar;
  - the exact sums computed from the scaled tensors are the unscaled case's times 2^t (plus the bias moves), and the three
    subnormal placements give the same sums: one reference serves all three;
  - sub_x: every nonzero x is subnormal; sub_w: every nonzero w is; sub_out: every nonzero operand is normal;
  - subnormal family: at least 10 % of the outputs are nonzero subnormals, at least 5 % of the nonzero finite outputs exact ties,
    at least 16 nonzero sums round to zero, under ReLU at least 4 pre-activation sums lie in (-2^-25, 0) (expected +0), without
    activation at least 4 outputs are -0;
  - overflow family: at least 8 outputs exactly on 65520, 8 on the grid point below, 8 on 65504 (mirrored at -65520 without
    activation), at least 5 % inf; ovf_res: no conv + bias reaches 65504 alone, at least 8 outputs are inf; ovf_tanh: sums past
    +-65520, +0 sums, subnormal sums and sums that round to -0 on both sides of the tanh boundary;
  - each mutant aimed at a variant (flush_x, flush_w, flush_out, saturate, rtz) differs from the reference, by bits, on at least 5 %
    of the outputs; the sign mutant (round, then a max that keeps -0) on at least 4 elements;
  - oracle.conv2d(..., f16=True), float32 accumulation in an order of its own, gives the reference's bits: zeros' signs, inf and all.
Chains (one subnormal and one overflow case per form, shared by the forms of a plane count): test_chain_case_conditions.
These are conditions on the cases. A case that breaks one is changed; the bounds stay. profiles/range_cases.txt holds the census
(python tests/test_range_cases.py prints it)."""
import numpy as np
import pytest

import bneck_cases as B
import dyadic_cases as D
import range_cases as R
from bits import diff_bits, same_bits

_MIN_NORMAL = 2.0 ** -14


def _is_f16(v):
    return v.dtype == np.float32 and np.isfinite(v).all() and np.array_equal(v, v.astype(np.float16).astype(np.float32))


def test_same_bits_sees_zero_signs_and_nan_positions_only():
    nan2 = np.array([0xFFC00001], np.uint32).view(np.float32)[0]          # another sign and payload
    a = np.array([0.0, -0.0, np.nan, np.inf, 1.0], np.float32)
    same_bits(a, a.copy(), "self")
    same_bits(a, np.array([0.0, -0.0, nan2, np.inf, 1.0], np.float32), "nan payload")
    for other in ([-0.0, -0.0, np.nan, np.inf, 1.0], [0.0, 0.0, np.nan, np.inf, 1.0], [0.0, -0.0, 1.0, np.inf, 1.0], [0.0, -0.0, np.nan, np.inf, np.nan]):
        b = np.array(other, np.float32)
        assert diff_bits(a, b).sum() == 1
        with pytest.raises(AssertionError):
            same_bits(a, b, "differs")
    with pytest.raises(AssertionError):
        same_bits(a, a[:4], "shape")


def test_numpy_rounds_float64_to_f16_as_the_spec_does():
    v = np.array([65520.0, 65519.99, -65520.0, 2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, -2.0 ** -25, -2.0 ** -26])
    got = R.h16(v)
    same_bits(got, np.array([np.inf, 65504, -np.inf, 0.0, 2.0 ** -24, 2.0 ** -23, -0.0, -0.0], np.float32), "ends")
    same_bits(R.relu(np.array([-1.0, -0.0, 0.0, np.nan, 2.0])).astype(np.float32), np.array([0, 0, 0, 0, 2], np.float32), "relu")


def test_variants_cover_every_case():
    assert len(R.VARIANTS) == len(set(R.VARIANTS))
    for cid in D.CASE_IDS:
        fam = R.families(cid)
        assert "ovf" in fam and "sub_out" in fam and (D.CASES[cid][0] == "fp8" or set(R.SUB_FAMILIES) <= set(fam))
    assert "head_3x3/ovf_res" in R.VARIANTS and "big_256_512_k1/ovf_tanh" in R.VARIANTS


@pytest.mark.parametrize("vid", R.VARIANTS)
def test_variant_conditions(oracle, vid):
    c = R.build(vid)
    base, fam, fp8 = D.build(c["base"]), c["family"], c["kind"] == "fp8"
    grid = 2.0 ** (c["t"].astype(np.float64) - R.G)                       # per channel
    # operands
    ops = [k for k in ("x", "x1", "x2", "w") if c.get(k) is not None and not fp8]
    for k in ops + (["res"] if c["res"] is not None else []):
        assert _is_f16(c[k]), k
    assert c["bias"].dtype == np.float32 and np.array_equal(np.rint(c["bias"] / grid), c["bias"] / grid)
    if c["res"] is not None:
        q = c["res"].astype(np.float64) / grid
        assert np.array_equal(np.rint(q), q)
    for k in ops:
        nz = np.abs(c[k][c[k] != 0])
        if (fam == "sub_x" and k != "w") or (fam == "sub_w" and k == "w"):
            assert nz.max() < _MIN_NORMAL and len(nz) > 0.9 * c[k].size, k
        elif fam in R.SUB_FAMILIES:
            assert nz.min() >= _MIN_NORMAL, k
    if fp8:
        assert np.array_equal(c["xi"], base["xi"]) and np.array_equal(c["wi"], base["wi"]) and np.array_equal(np.log2(c["scale"]), np.rint(np.log2(c["scale"])))
    # the bound, on the scaled tensors
    assert R.magnitude_bits(vid) < 22
    # scaling carries the sums over: this variant's own tensors give base * 2^t (+ the moved biases, + ovf_res' wider residual)
    p = R._pre_of(c)
    if fam not in ("ovf_tanh", "ovf_res"):
        moved = R._moves(c["base"], fam == "ovf") if fam == "ovf" or c["base"] in R.SUB_MOVED else 0.0
        assert np.array_equal(p, R._base_pre(c["base"]) * 2.0 ** c["t"].astype(np.float64) + moved)
    assert np.array_equal(p, R.pre(vid))                                  # (sub_x, sub_w, sub_out: the shared sums)
    assert np.array_equal(np.rint(p / grid), p / grid) and np.array_equal(p.astype(np.float32).astype(np.float64), p)
    s = R.census(vid)
    if fam == "ovf_tanh":
        lin, th = p[..., :R.TANH_FROM], p[..., R.TANH_FROM:]
        for part in (lin, th):
            assert (part >= R.F16_OVF).sum() >= 8 and (part <= -R.F16_OVF).sum() >= 8 and (part == 0).sum() >= 8
            assert ((part != 0) & (np.abs(part) < _MIN_NORMAL)).sum() >= 8 and ((part < 0) & (part >= -2.0 ** -25)).sum() >= 8
        ref = R.reference(vid, oracle)
        assert np.isinf(ref[..., :R.TANH_FROM]).any() and np.abs(ref[..., R.TANH_FROM:]).max() == 1.0
        for tile_ch in (32, 64, 96, 128, 256):
            assert R.TANH_FROM % tile_ch != 0
        y0 = oracle.conv2d(c["x"], c["w"], c["bias"], 1, 0, None, 0, f16=True)
        y2 = oracle.conv2d(c["x"], c["w"], c["bias"], 1, 0, None, 2, f16=True)
        same_bits(np.where(np.arange(ref.shape[-1]) >= R.TANH_FROM, y2, y0), ref, vid)
        return
    ref = R.reference(vid)
    if fam in R.SUB_FAMILIES:
        assert s["subnormal"] >= 0.10 and s["tie"] >= 0.05 and s["to_zero"] >= 16, s
        assert (s["relu_neg_tiny"] if c["act"] else s["minus_zero"]) >= 4, s
        assert c["act"] == 0 or s["minus_zero"] == 0
    elif fam == "ovf":
        assert min(s["on_ovf"], s["below_ovf"], s["on_max"]) >= 8 and s["inf"] >= 0.05, s
        assert c["act"] or min(s["on_novf"], s["below_novf"], s["on_nmax"]) >= 8, s
        assert 1.5 * R.F16_MAX < s["max"] < 12 * R.F16_MAX, s
    else:
        assert s["alone_max"] < R.F16_MAX and s["res_over"] >= 8, s
        assert diff_bits(R.mutant_saturate(vid), ref).sum() == s["res_over"]
    for name in R.aimed(vid):
        assert s[name] >= (4 if name == "relu_after_round_keeps_sign" else 0.05), (name, s)
    # the oracle: float32 accumulation, its own order, ReLU before the rounding
    kind = c["kind"]
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
    elif fp8:
        acc = oracle.conv2d(c["xi"], c["wi"], np.zeros(len(c["bias"]), np.float32), c["stride"], c["pad"], None, 0, f16=False)
        want = acc * c["scale"] + c["bias"]
        if c["res"] is not None:
            want = want + c["res"]
        assert want.dtype == np.float32
        got = R.h16(R.relu(want))
    else:
        got = oracle.conv2d(c["x"], c["w"], c["bias"], c["stride"], c["pad"], c["res"], c["act"], f16=True)
    same_bits(got, ref, vid)


_CHAIN_FORMS = ["bneck_chain_f16<64,128,next,dual>", "bneck_chain_f16<64,256,next>", "bneck_chain_f16<128,128,next>", B.XN]


def test_chain_cases_cover_every_form():
    keys = {(R.chain_build(f, "sub")["planes"], R.chain_build(f, "sub")["id"]) for f in _CHAIN_FORMS}
    for form in B.FORM_IDS:
        for fam in R.CHAIN_FAMILIES:
            c = R.chain_build(form, fam)
            assert (c["planes"], c["id"].replace("/" + fam, "/sub")) in keys and (c["n"], c["H"], c["W"]) == (3, 7, 11)


@pytest.mark.parametrize("fam", R.CHAIN_FAMILIES)
@pytest.mark.parametrize("form", _CHAIN_FORMS)
def test_chain_case_conditions(oracle, form, fam):
    """Per stage i, with the unscaled case's grid 2^-g_i and the stage's exponent s_i: every operand is an f16 value, every finite sum
    a multiple of 2^(s_i - g_i) whose bound (sum |x| |w| + |bias| + |res|) is below 2^22 of them, so a float32 accumulator holds it
    exactly; an inf or NaN operand gives inf or NaN in every summation order (NaN if a NaN, an inf times zero or both infinities
    take part, else that infinity). sub: every a and every nonzero b is subnormal, at least 10 % of y and of a' are nonzero
    subnormals, at least 8 sums of y round to zero and 8 lie in (-2^-25, 0). ovf: b or y holds inf, a' holds at least 8 inf, at
    least 8 zeros behind a NaN sum, and finite values. A chain that flushes b, or saturates b and y, differs. The oracle's three
    convolutions, chained, give the same bits."""
    c = R.chain_build(form, fam)
    base = B.build(c["planes"], c["id"].split("/")[0])
    for k in ("a", "w2", "w3", "w1n", "res", "x2"):
        if c[k] is not None and not (c["xn"] and k == "w2"):
            assert _is_f16(c[k]) and len(np.unique(c[k])) >= 3, k
    with np.errstate(all="ignore"):
        sums, (b, y, an) = R.chain_stages(c)
        bounds, _ = R.chain_stages(c, absolute=True)
    sub = lambda r: (r != 0) & (np.abs(r) < _MIN_NORMAL)
    for name, s, bound, g, e in zip(("b", "y", "a_next"), sums, bounds, base["g"], c["s"]):
        if s is None:
            continue
        fin = np.isfinite(bound)
        grid = 2.0 ** (e - g)
        assert bound[fin].max() / grid < 2.0 ** 22, name
        assert np.array_equal(np.isfinite(s), fin) and np.array_equal(np.rint(s[fin] / grid), s[fin] / grid), name
    if fam == "sub":
        assert np.abs(c["a"]).max() < _MIN_NORMAL and np.isfinite(an).all()
        assert c["xn"] or (sub(b) == (b != 0)).all()
        assert sub(y).mean() >= 0.10 and sub(an).mean() >= 0.10
        v = R.relu(sums[1])
        assert ((v != 0) & (y == 0)).sum() >= 8 and ((sums[1] < 0) & (sums[1] > -2.0 ** -25)).sum() >= 8
        flushed = dict(c, a=R._flush(c["a"])) if c["xn"] else None
        if not c["xn"]:      # b flushed on its way to the second stage
            k = np.concatenate([R._flush(b), B._x2_rows(c)], -1) if c["x2"] is not None else R._flush(b)
            side = c["res"] if c["res"] is not None else 0.0
            y_flushed = R.h16(R.relu(k.astype(np.float64) @ c["w3"].astype(np.float64).T + c["bias3"] + side))
        else:
            y_flushed = R.chain_stages(flushed)[1][1]
        assert diff_bits(y_flushed, y).mean() >= 0.05
    else:
        assert np.isinf(b).any() or np.isinf(y).any()
        assert np.isinf(an).sum() >= 8 and (np.isnan(sums[2]) & (an == 0)).sum() >= 8 and (np.isfinite(an) & (an != 0)).sum() >= 8
        sat = lambda r: np.where(np.isinf(r), np.copysign(np.float32(R.F16_MAX), r), r)
        with np.errstate(all="ignore"):
            an_sat = R.h16(R.relu(sat(y).astype(np.float64) @ c["w1n"].astype(np.float64).T + c["bias1n"]))
        assert diff_bits(an_sat, an).sum() >= 8
    one = lambda w: w[:, None, None, :]
    ob = c["a"] if c["xn"] else oracle.conv2d(c["a"], c["w2"], c["bias2"], c["stride"], 1, None, 1, f16=True)
    k = np.concatenate([ob, B._x2_rows(c)], -1) if c["x2"] is not None else ob
    oy = oracle.conv2d(k, one(c["w3"]), c["bias3"], 1, 0, c["res"], 1, f16=True)
    oan = oracle.conv2d(oy, one(c["w1n"]), c["bias1n"], 1, 0, None, 1, f16=True)
    same_bits(ob, b, "b"), same_bits(oy, y, "y"), same_bits(oan, an, "a_next")
    ref = R.chain_reference(form, fam, oracle)
    same_bits(ref["y"], y, "reference y"), same_bits(ref["a_next"], an, "reference a_next")
    if c["xn"]:
        codes = ref["a_next8"]
        assert len(np.unique(codes)) > 8 and (codes == 0x7E).sum() >= 8       # saturated at 448
        if fam == "sub":
            assert ((codes > 0) & (codes < 0x08)).sum() >= 8                  # E4M3 subnormals: below 2^-6
        for ch in (0, 63, 64, 255):
            assert np.array_equal(codes[..., ch], oracle.quantize_e4m3(an[..., ch], float(c["inv_scale"][ch])))


def chain_report():
    lines = ["chain case                             stage  subnormal  to_zero  neg_tiny     inf  nan_sum"]
    for form in _CHAIN_FORMS:
        for fam in R.CHAIN_FAMILIES:
            c = R.chain_build(form, fam)
            with np.errstate(all="ignore"):
                sums, outs = R.chain_stages(c)
            for name, s, r in zip(("b", "y", "a_next"), sums, outs):
                if s is None:
                    continue
                v = R.relu(s)
                lines.append(f"{form:34s} {fam:3s} {name:6s} {float(((r != 0) & (np.abs(r) < _MIN_NORMAL)).mean()):9.3f} {int(((v != 0) & (r == 0) & np.isfinite(v)).sum()):8d} "
                             f"{int(((s < 0) & (s > -2.0 ** -25)).sum()):9d} {float(np.isinf(r).mean()):7.3f} {float(np.isnan(s).mean()):8.3f}")
    return "\n".join(lines)


def report():
    cols = ["bits", "subnormal", "tie", "to_zero", "relu_neg_tiny", "minus_zero", "inf", "on_ovf", "below_ovf", "on_max", "on_novf", "below_novf",
            "on_nmax"] + list(R.MUTANTS)
    lines = ["variant                      " + " ".join(f"{k[:13]:>13s}" for k in cols)]
    for vid in R.VARIANTS:
        s = R.census(vid)
        f = lambda v: "            -" if v is None else (f"{v:13.3f}" if isinstance(v, float) else f"{v:13d}")
        lines.append(f"{vid:28s} " + " ".join(f(s.get(k)) for k in cols))
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
    print()
    print(chain_report())
