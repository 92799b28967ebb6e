"""CPU: the cases of tests/tfl_cases.py are what they claim to be, before the GPU tests rely on them - oracle/tfl_oracle.py equals the
plain-integer statement of the fixed-point step on every accumulator the cases produce, the form cases reach every row of the
register-fed kernel's table, every case's own conditions hold, and three wrong references are each told apart by the tie cases."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfl_builder as B
import tfl_cases as K


def _oracle():
    import tfl_oracle as O
    return O


def _same_on(values, m, s):
    O = _oracle()
    v = np.unique(np.asarray(values, np.int64))
    got = O.mbqm(v, m, s)
    want = [K.mbqm(int(a), m, s) for a in v]
    assert [int(g) for g in got] == want, (m, s)
    return len(v)


def test_fixed_point_statement_known_answers():
    """The statement itself on values worked by hand: half up in the high multiplication, half away in the shift, both in a row."""
    h = 1 << 30                                      # the Q31 mantissa of every power of two
    assert [K.srdhm(x, h) for x in (-3, -2, -1, 0, 1, 2, 3)] == [-1, -1, 0, 0, 1, 1, 2]       # x / 2, halves toward +inf
    assert [K.rdbpot(x, 1) for x in (-3, -2, -1, 0, 1, 2, 3)] == [-2, -1, -1, 0, 1, 1, 2]     # x / 2, halves away from zero
    assert K.srdhm(K.I32_MIN, K.I32_MIN) == K.I32_MAX and K.srdhm(K.I32_MIN, K.I32_MAX) == -K.I32_MAX
    assert K.quantize_multiplier(2.0 ** -3) == (h, -2) and K.quantize_multiplier(2.0) == (h, 2)
    assert K.quantize_multiplier(1e-11) == (0, 0) and K.quantize_multiplier(2.0 ** -31)[0] == h
    assert K.mbqm(3, h, -2) == 1 and K.mbqm_once(3, h, -2) == 0                                # the double rounding
    assert K.mbqm(-3, h, -2) == 0 and K.mbqm_once(-3, h, -2) == 0 and K.mbqm(-5, h, -2) == -1
    assert K.mbqm(7, *K.quantize_multiplier(3.7)) == 26 and K.mbqm(-100, 0, 0) == 0
    O = _oracle()
    for ratio in K.TIE_RATIOS + (1.0, 2.0 ** -31, 0.999999, 1e-5, 255.0):
        assert O.quantize_multiplier(ratio) == K.quantize_multiplier(ratio)
        m, s = K.quantize_multiplier(ratio)
        big = (1 << 31 - max(s, 0)) - 1
        _same_on(list(range(-1100, 1101)) + [big, -big, big // 3, -(big // 3)], m, s)
    assert int(O._srdhm(np.array([K.I32_MIN]), K.I32_MIN)[0]) == K.I32_MAX


def test_form_cases_reach_every_row_of_the_table(built):
    """The restated conv_i8_direct_form maps the form cases - and their last-chunk variants - onto every row yh_tfl_direct_forms
    reports: a row added to kDirectForms without a case fails here. The variants the issue names are the ones found: fewer steps
    than the shallowest ring, exactly a ring, the deepest ring that n fills."""
    from yolact_amd import capi
    rows = capi.tfl_direct_forms()
    assert len(rows) >= 18 and all(d >= 1 and kk in (0, 1, 3) and (once or kk == 0) for d, once, kk in rows)
    assert len(set(rows)) == len(rows)
    hit = {}
    for kh, kw, ci in K.FORM_CASES:
        r = K.direct_form(rows, kh, kw, ci)
        assert r >= 0
        hit.setdefault(r, []).append((kh, kw, ci))
        for less in K.LAST_CHUNK:
            assert K.direct_form(rows, kh, kw, ci - less) == r, (kh, kw, ci, less)
    assert sorted(hit) == list(range(len(rows))), sorted(set(range(len(rows))) - set(hit))
    want = {(1, 1, 256): (4, True, 1), (1, 1, 320): (5, True, 1), (1, 1, 512): (8, True, 1), (1, 1, 768): (12, True, 1), (1, 1, 1152): (18, True, 1),
            (1, 1, 448): (4, False, 0), (1, 3, 128): (6, False, 0), (1, 1, 1024): (8, False, 0), (1, 3, 64): (4, False, 0),
            (2, 2, 64): (4, False, 0), (5, 5, 64): (5, False, 0), (3, 3, 256): (9, False, 0), (3, 3, 64): (9, True, 3), (3, 3, 128): (18, True, 3)}
    for case, row in want.items():
        assert rows[K.direct_form(rows, *case)] == row, case
    # a table with one more looped ring has a row no case reaches: the check above would fail
    for extra in ((10, False, 0), (10, True, 1)):
        more = rows + [extra]
        assert len(more) - 1 not in {K.direct_form(more, *c) for c in K.FORM_CASES}


def test_form_and_group_cases_oracle_equals_the_statement():
    rng = np.random.default_rng(5)
    n = 0
    for kh, kw, ci in K.FORM_CASES:
        for less in K.LAST_CHUNK:
            m = K.form_model(kh, kw, ci - less, rng)
            x = rng.integers(0, 256, (1, 3, 5, ci - less), dtype=np.uint8)
            acc, padded = K.conv_acc(m, x)
            mult, shift = K.conv_multiplier(m)
            assert np.abs(acc).max() << max(shift, 0) < 1 << 31
            n += _same_on(acc, mult, shift)
            if (kh, kw) != (1, 1):
                assert (padded > 0).any()
            assert m.tensors[m.outputs[0]].shape == (1, 3, 5, 17)
        g = K.group_model(kh, kw, ci, rng)
        assert [g.tensors[o].shape for o in g.outputs] == [(1, 3, 5, 17), (1, 3, 5, 16), (1, 2, 3, 1)]
    assert n > 10000


@pytest.mark.parametrize("ratio", K.TIE_RATIOS)
def test_tie_cases_conditions(ratio):
    """Every accumulator g (p - 128) occurs; the oracle equals the statement on all of them; each power-of-two ratio holds at
    least 16 exact half-integers of each sign among the outputs that are not saturated, and an output where two roundings differ
    from one. Ratios 2^-3 and 2^-6 saturate nothing. (At 2^-1 the case as the issue states it must saturate: |g (p - 128)| reaches
    896, 448 codes from the zero point - so the ties are counted among the outputs strictly inside the clamp range.)"""
    O = _oracle()
    for ci, dw in ((3, False), (4, False), (16, False), (64, False), (8, True)):
        m, x = K.tie_model(ci, ratio, depthwise=dw)
        acc, _ = K.conv_acc(m, x) if ci in (3, 8) else (None, None)
        if acc is not None:
            want = np.array(K.TIE_GAINS)[None, None, :] * (np.arange(256).reshape(16, 16, 1) - 128)
            assert np.array_equal(acc, want)
        mult, shift = K.conv_multiplier(m)
        if ratio in K.TIE_POW2 or ratio == 2.0:
            assert (mult, shift) == K.quantize_multiplier(ratio)
        val = O.run_model(m, {0: x})[m.outputs[0]]
        g = np.array(K.TIE_GAINS)
        for p in range(0, 256, 5):
            for c in range(8):
                a = int(g[c]) * (p - 128)
                assert val[0, p // 16, p % 16, c] == min(255, max(0, K.mbqm(a, mult, shift) + 128))
    mult, shift = K.quantize_multiplier(ratio)
    accs = sorted({g * (p - 128) for g in K.TIE_GAINS for p in range(256)})
    assert max(abs(a) for a in accs) << max(shift, 0) < 1 << 31
    _same_on(accs, mult, shift)
    if ratio in K.TIE_POW2:
        pos, neg, sat, differ = K.tie_census(ratio)
        assert pos >= 16 and neg >= 16 and differ >= 1, (pos, neg, sat, differ)
        if ratio != 0.5:
            assert sat == 0
        else:
            assert sat == sum(not 0 < K.round_half_away(Fraction(a, 2) + Fraction(1, 4)) + 128 < 255 for gg in K.TIE_GAINS for a in [gg * (p - 128) for p in range(256)])
    if ratio == 1e-11:
        assert (mult, shift) == (0, 0) and all(K.mbqm(a, mult, shift) == 0 for a in accs)
    if ratio in (2.0, 3.7):
        assert shift > 0                                                      # the left-shift branch


def test_three_wrong_references_are_told_apart_by_the_tie_cases():
    """srdhm rounding half away from zero, one rounding of the exact product, and a float32 round(acc * scale) each differ from the
    statement on some output of the power-of-two tie cases - and from each other - so a kernel (or an oracle) built on any of them fails."""
    def outputs(f, ratios):
        out = []
        for ratio in ratios:
            m, s = K.quantize_multiplier(ratio)
            out += [min(255, max(0, f(g * (p - 128), m, s, ratio) + 128)) for g in K.TIE_GAINS for p in range(256)]
        return out
    fs = [lambda a, m, s, r: K.mbqm(a, m, s), lambda a, m, s, r: K.mbqm_srdhm_away(a, m, s), lambda a, m, s, r: K.mbqm_once(a, m, s),
          lambda a, m, s, r: K.mbqm_f32(a, r)]
    true = outputs(fs[0], K.TIE_POW2)
    for i, f in enumerate(fs[1:]):
        assert outputs(f, K.TIE_POW2) != true, i          # the power-of-two cases alone expose each of them
    # (on a power of two a float32 product IS one rounding of the exact product: those two part at 0.75 and 3.7)
    every = [outputs(f, K.TIE_RATIOS[:-1]) for f in fs]
    for i in range(len(every)):
        for j in range(i):
            assert every[i] != every[j], (i, j)


@pytest.mark.parametrize("ci", K.CORNER_CIS + (8,))
def test_zero_point_corner_cases_conditions(ci):
    """Per (zx, zw, zo): 14 of the 20 pixels have padded taps; no accumulator leaves int32 after the left shift; with random data AND
    random weights at most half the reference's outputs sit at a clamp end; the oracle equals the statement on every accumulator of
    every weight and data variant."""
    O = _oracle()
    rng = np.random.default_rng(100 + ci)
    dw = ci == 8
    for zx, zw in K.CORNER_ZPS:
        for zo in K.CORNER_ZOS:
            models, x0 = K.corner_models(ci, zx, zw, zo, rng, depthwise=dw)
            xs = [x0] + K.corner_inputs(ci, rng)[1:]
            for mi, m in enumerate(models):
                mult, shift = K.conv_multiplier(m)
                for xi, x in enumerate(xs):
                    acc, padded = K.conv_acc(m, x)
                    assert int((padded > 0).sum()) == 14 and padded.size == 20
                    assert int(np.abs(acc).max()) << max(shift, 0) < 1 << 31
                    _same_on(acc, mult, shift)
                    if mi == 0 and xi == 0:
                        val = O.run_model(m, {0: x})[m.outputs[0]]
                        assert np.isin(val, (0, 255)).mean() <= 0.5, (zx, zw, zo)
                        assert len(np.unique(val)) >= 10                  # (not a constant image)


def test_elementwise_domains_oracle_equals_the_statement():
    """ADD on all 65 536 pairs and RELU / RELU6 / QUANTIZE on all 256 codes: the oracle against the integer statement, per parameter
    set; the sets hold what they claim (zero points 0 and 255, a ratio of 64, both clamp ends reached, a clamp from RELU6)."""
    O = _oracle()
    a, b = np.repeat(np.arange(256), 256).astype(np.uint8), np.tile(np.arange(256), 256).astype(np.uint8)
    assert len(K.ADD_SETS) >= 6 and len(K.UNARY_SETS) >= 6
    both_ends = relu6 = False
    for ps in K.ADD_SETS:
        sa, za, sb, zb, so, zo, act = ps
        want = K.add_exact(ps)
        assert np.array_equal(O.add_u8(a, za, sa, b, zb, sb, zo, so, act).reshape(256, 256), want), ps
        both_ends = both_ends or ((want == 0).mean() > 0.2 and (want == 255).mean() > 0.2)
        relu6 = relu6 or (act == 3 and 0 < want.max() < 255)
    assert both_ends and relu6
    assert {0, 255} <= {p[1] for p in K.ADD_SETS} and {0, 255} <= {p[3] for p in K.ADD_SETS} and any(p[0] / p[2] == 64 for p in K.ADD_SETS)
    assert {0, 255} <= {p[1] for p in K.UNARY_SETS} and {0, 255} <= {p[3] for p in K.UNARY_SETS}
    assert any(p[0] > p[2] for p in K.UNARY_SETS) and any(p[0] < p[2] for p in K.UNARY_SETS) and any(p[0] / p[2] in (0.5, 0.125) for p in K.UNARY_SETS)
    codes = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    for code in ("RELU", "RELU6", "QUANTIZE"):
        for ps in K.UNARY_SETS:
            m = K.unary_model(code, ps)
            assert np.array_equal(O.run_model(m, {0: codes})[m.outputs[0]].reshape(-1), K.unary_exact(code, ps)), (code, ps)
    for scale, zo in ((0.5, 128), (0.125, 0), (2.0, 255)):
        x = K.quantize_f32_cases(scale, zo)
        assert np.isfinite(x).all() and (np.abs(x[np.abs(x) > 1e-30].astype(np.float64) / scale) <= 2.0 ** 24).all()
        got = O.quantize_f32(x, zo, scale)
        assert np.array_equal(got, K.quantize_f32_exact(x, scale, zo)), (scale, zo)
        assert got.min() == 0 and got.max() == 255


def test_every_case_model_serialises_and_validates(built):
    """Every builder's model goes through the product's flatbuffer reader (parse + validate_graph, no GPU)."""
    from yolact_amd import capi
    rng = np.random.default_rng(3)
    models = [K.form_model(1, 3, 64, rng), K.group_model(2, 2, 64, rng), K.tie_model(4, 0.5)[0], K.tie_model(8, 2.0, depthwise=True)[0],
              K.corner_models(4, 0, 255, 0, rng)[0][1], K.copy_model(17, rng), K.unaligned_concat_model(1, 3, "conv", rng)[0],
              K.unaligned_concat_model(2, 1, "dw", rng)[0], K.folded_model("conv", 16, 6, "add", rng, "aq", "act")[0],
              K.folded_model("resize", 6, 6, "tanh", rng)[0], K.add_model(K.ADD_SETS[0], folded=True), K.unary_model("CONCATENATION", K.UNARY_SETS[1]),
              K.unary_model("RELU6", K.UNARY_SETS[0]), K.quantize_f32_model(5, 0.5, 128), K.resize_model(7, 7, 3, 3, False, True),
              K.conv_model(9, 7, 4, 5, 3, 3, dil=(2, 1), padding=1, rng=rng)]
    for i, m in enumerate(models):
        ok, nt, no, msg = capi.tfl_validate(B.serialize(m))
        assert ok and nt == len(m.tensors) and no == len(m.ops), (i, msg)


def test_oracle_dilation_and_absent_bias():
    """run_model passes dil_h / dil_w through and takes a convolution without a bias operand: against the exact accumulators."""
    O = _oracle()
    rng = np.random.default_rng(9)
    for dw in (False, True):
        for dil, padding in (((2, 2), 0), ((2, 1), 1), ((1, 1), 0)):
            m = K.conv_model(9, 7, 8, 5, 3, 3, x_zp=77, w_zp=130, y_zp=100, dil=dil, padding=padding, depthwise=dw, rng=rng)
            assert len(m.ops[0].inputs) == 2
            x = rng.integers(0, 256, (1, 9, 7, 8), dtype=np.uint8)
            acc, _ = K.conv_acc(m, x)
            K.fit_output_scale(m, acc)
            mult, shift = K.conv_multiplier(m)
            want = np.array([min(255, max(0, K.mbqm(int(a), mult, shift) + 100)) for a in acc.reshape(-1)], np.uint8).reshape(acc.shape)
            got = O.run_model(m, {0: x})[m.outputs[0]]
            assert got.shape == (1,) + acc.shape and np.array_equal(got[0], want)
            if padding == 1 and dil == (2, 1):
                assert acc.shape[:2] == (5, 5)
