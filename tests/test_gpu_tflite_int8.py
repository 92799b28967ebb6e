"""-m gpu: the TFLite executor on int8 tensors and per-channel weight scales (DESIGN.md section 11 "TFLite int8"). Every comparison
is array_equal on bytes against tests/tfl_q_ref.py, with one and two images per invoke; each case asserts the kernel family, the row
of the table of forms, grouped and folded (yh_tfl_op_info) and the output type and per-channel tables (yh_tfl_op_quant) first."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfl_builder_q as BQ
import tfl_cases as K
import tfl_q_cases as Q
import tfl_q_ref as R
from tfl_builder_q import Model, Op, T

pytestmark = pytest.mark.gpu

I8PC = (True, True)        # yh_tfl_op_quant of an int8 convolution: int8 output, per-channel tables


def _tune(dot, **more):
    t = dict(more)
    if dot != 3:
        t["tfl_dot"] = dot
    return t or None


def _both_shift_signs(m, op=0):
    o = m.ops[op]
    tx, tw, ty = (m.tensors[i] for i in (o.inputs[0], o.inputs[1], o.outputs[0]))
    shifts = [R.quantize_multiplier(R.f32(tx.scale) * s / R.f32(ty.scale))[1] for s in R.scales_of(tw)]
    return min(shifts) < 0 < max(shifts)


def _families(m, dot, rows=None):
    out = {}
    for i, o in enumerate(m.ops):
        w = m.tensors[o.inputs[1]].shape
        if o.code == "CONV_2D":
            fam = Q.expected_conv_family(w[1], w[2], w[3], dot)
            row = K.direct_form(rows, w[1], w[2], w[3]) if (rows and fam == "conv_i8_direct") else (-1 if fam != "conv_i8_direct" else None)
        else:
            fam, row = K.expected_dw_family(w[1], w[2], w[3], o.opts.get("depth_multiplier", 1), dot), -1
        out[i] = (fam, row, False, False)
    return out


@pytest.mark.parametrize("case", K.FORM_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_every_row_of_the_table_single_int8(built, case):
    """The smallest convolution that selects each row of kDirectForms, as int8: x (2, 3, 5, Ci) with the row's Ci and its last-chunk
    variants, Co = 17 (a ragged channel tile, byte stores, tables padded), per-channel scales on both sides of 1, zx at both ends
    and 0 with SAME padding (a padded tap carries the byte of zx), weights -128 and 127, both clamp ends hit. On the reference:
    exchanging any two channels' multipliers changes a byte. The native register-fed form reports the row the uint8 form reports;
    then the LDS tiles (Ci % 64 == 0), px8 / scalar under tfl_dot = 1, scalar under 0."""
    from yolact_amd import capi
    rows = capi.tfl_direct_forms()
    kh, kw, ci = case
    rng = np.random.default_rng(kh * 100000 + kw * 10000 + ci + 7)
    for less in K.LAST_CHUNK:
        for zx in Q.ZXS:
            c = ci - less
            m, x, acc = Q.form_model(kh, kw, c, rng, zx)
            w = m.tensors[1].data
            assert w.min() == -128 and w.max() == 127 and m.tensors[1].per_channel
            assert _both_shift_signs(m) and Q.multipliers_matter(m, acc), (case, less, zx)
            wants = Q.reference_images(m, x)
            ys = np.stack([wants[i][m.outputs[0]] for i in range(2)])
            assert ys.min() == -128 and ys.max() == 127
            for dot in (3, 2, 1, 0):
                fams = _families(m, dot, rows)
                assert (dot == 3) == (fams[0][0] == "conv_i8_direct") and (fams[0][0] == "conv_i8_lds") == (dot == 2 and c % 64 == 0)
                if dot == 2 and c % 64 != 0:
                    continue          # (the same kernel as under tfl_dot = 1)
                Q.gpu_check(m, x, wants, _tune(dot), fams, {0: I8PC}, label=(case, less, zx, dot))
    print("int8 form case %dx%dx%d: row %d" % (kh, kw, ci, K.direct_form(rows, kh, kw, ci)))


@pytest.mark.parametrize("case", K.FORM_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_every_row_of_the_table_grouped_int8(built, case):
    """Three int8 convolutions of one form with different multiplier tables and biases in one launch (tfl_group on) and as three
    (off): each equals its own reference, so a table read from another member's record fails."""
    from yolact_amd import capi
    rows = capi.tfl_direct_forms()
    kh, kw, ci = case
    rng = np.random.default_rng(kh * 100000 + kw * 10000 + ci + 8)
    m, x = Q.group_model(kh, kw, ci, rng, Q.ZXS[ci % 3])
    wants = Q.reference_images(m, x)
    row = K.direct_form(rows, kh, kw, ci)
    quants = {i: (True, m.tensors[m.ops[i].inputs[1]].per_channel) for i in range(3)}
    assert [q[1] for q in quants.values()] == [True, True, False]      # (Co = 1: one scale - the table is read, 'per channel' is not reported)
    Q.gpu_check(m, x, wants, None, {i: ("conv_i8_direct", row, True, False) for i in range(3)}, quants, label=case)
    Q.gpu_check(m, x, wants, dict(tfl_group=0), {i: ("conv_i8_direct", row, False, False) for i in range(3)}, quants, label=case)


def test_uint8_and_int8_convolutions_never_share_a_group(built):
    """Two uint8 and two int8 convolutions of one form at one depth of the plan (each pair behind a QUANTIZE of the graph input):
    all four report 'in a group', and the plan has four launches - the two QUANTIZEs, the uint8 pair, the int8 pair."""
    import yolact_amd as ya
    rng = np.random.default_rng(3)
    m = Model()
    xu = m.add(T("x", (1, 3, 5, 64), "u8", scale=0.05, zp=128))
    xi = m.add(T("xi", (1, 3, 5, 64), "i8", scale=0.05, zp=0))
    xq = m.add(T("xq", (1, 3, 5, 64), "u8", scale=0.05, zp=128))
    m.ops += [Op("QUANTIZE", [xu], [xi]), Op("QUANTIZE", [xu], [xq])]
    x = rng.integers(0, 256, (2, 3, 5, 64), dtype=np.uint8)
    for k in range(2):
        one = K.conv_model(3, 5, 64, 16, 1, 1, rng=rng, bias=rng.integers(-900, 900, 16))
        ids = [xq] + [m.add(T(t.name, t.shape, t.dtype, data=t.data, scale=t.scale, zp=t.zp)) for t in one.tensors[1:]]
        m.ops.append(Op("CONV_2D", ids[:3], [ids[3]], **one.ops[0].opts))
        m.outputs.append(ids[3])
        one, _, _ = Q.form_model(1, 1, 64, rng, 0, co=16)
        Q.fit_output_scale(one, (x ^ 0x80).view(np.int8))
        ids = [xi] + [m.add(t) for t in one.tensors[1:]]
        m.ops.append(Op("CONV_2D", ids[:3], [ids[3]], **one.ops[0].opts))
        m.outputs.append(ids[3])
    m.inputs = [xu]
    fams = {i: ("conv_i8_direct", None, True, False) for i in range(2, 6)}
    Q.gpu_check(m, x, None, None, fams, {2: (False, False), 3: I8PC, 4: (False, False), 5: I8PC})
    eng = ya.TfliteEngine(BQ.serialize(m))
    assert eng.plan_summary()["launches_per_invoke"] == 4
    eng.close()


def _fitted(m, x):
    Q.fit_output_scale(m, x)
    return m


@pytest.mark.parametrize("zx", Q.ZXS)
def test_other_convolution_families_int8(built, zx):
    """The LDS tiles under tfl_dot = 2 (Ci 64 and 128, 3 x 3 and 1 x 1, Co 17 and 64), the px8 stem (3 x 3, stride 2, Ci = 3), the
    scalar kernel (Ci = 5: 7 x 1, and dilation 2 past the px8 kernel's LDS), depthwise four-channels-per-lane and scalar (8 and 6
    channels, depth multiplier 1 and 2, stride 1 and 2): per-channel scales, 9 x 8 pixels, one and two images."""
    rng = np.random.default_rng(200 + zx)
    for ci in (64, 128):
        for k in (3, 1):
            for co in (17, 64):
                x = rng.integers(-128, 128, (2, 9, 8, ci)).astype(np.int8)
                m = _fitted(Q.conv_model(9, 8, ci, co, k, k, zx=zx, zo=5, bias=rng.integers(-900, 900, co), rng=rng), x)
                Q.gpu_check(m, x, None, dict(tfl_dot=2), {0: ("conv_i8_lds", -1, False, False)}, {0: I8PC}, label=("lds", ci, k, co))
    x = rng.integers(-128, 128, (2, 17, 16, 3)).astype(np.int8)
    m = _fitted(Q.conv_model(17, 16, 3, 9, 3, 3, zx=zx, zo=-9, stride=(2, 2), bias=rng.integers(-900, 900, 9), rng=rng), x)
    Q.gpu_check(m, x, None, None, {0: ("conv_px8", -1, False, False)}, {0: I8PC}, label="stem")
    Q.gpu_check(m, x, None, dict(tfl_dot=0), {0: ("conv_scalar", -1, False, False)}, {0: I8PC}, label="stem scalar")
    x = rng.integers(-128, 128, (2, 9, 8, 5)).astype(np.int8)
    m = _fitted(Q.conv_model(9, 8, 5, 9, 7, 1, zx=zx, zo=3, bias=rng.integers(-900, 900, 9), rng=rng), x)
    Q.gpu_check(m, x, None, dict(tfl_dot=0), {0: ("conv_scalar", -1, False, False)}, {0: I8PC}, label="7x1")
    Q.gpu_check(m, x, None, None, {0: ("conv_px8", -1, False, False)}, {0: I8PC}, label="7x1 px8")
    x = rng.integers(-128, 128, (2, 9, 8, 5)).astype(np.int8)
    m = _fitted(Q.conv_model(9, 8, 5, 9, 11, 11, zx=zx, zo=3, dil=(2, 2), bias=rng.integers(-900, 900, 9), rng=rng), x)
    Q.gpu_check(m, x, None, None, {0: ("conv_scalar", -1, False, False)}, {0: I8PC}, label="dilated, 605 weights per channel")
    for ci, dm, stride, fam in ((8, 1, 1, "dw_c4"), (8, 1, 2, "dw_c4"), (6, 1, 1, "dw_scalar"), (6, 2, 2, "dw_scalar"), (8, 2, 1, "dw_scalar")):
        x = rng.integers(-128, 128, (2, 9, 8, ci)).astype(np.int8)
        m = _fitted(Q.conv_model(9, 8, ci, 0, 3, 3, zx=zx, zo=-4, stride=(stride, stride), bias=rng.integers(-900, 900, ci * dm), depthwise=True, dm=dm, rng=rng), x)
        assert m.tensors[1].per_channel and m.tensors[1].qdim == 3
        Q.gpu_check(m, x, None, None, {0: (fam, -1, False, False)}, {0: I8PC}, label=("dw", ci, dm, stride))
        Q.gpu_check(m, x, None, dict(tfl_dot=0), {0: ("dw_scalar", -1, False, False)}, {0: I8PC}, label=("dw scalar", ci, dm, stride))


GEOMETRY = [dict(k=(3, 3), dil=(2, 2), padding=0), dict(k=(3, 3), dil=(2, 2), padding=1), dict(k=(3, 3), dil=(2, 1), padding=0),
            dict(k=(3, 3), dil=(2, 1), padding=1), dict(k=(1, 3)), dict(k=(3, 1)), dict(k=(2, 2)), dict(k=(3, 3), stride=(1, 2)),
            dict(k=(3, 3), stride=(2, 1)), dict(k=(3, 3), bias=False), dict(k=(2, 2), dil=(2, 1), stride=(1, 2), bias=False, padding=1)]


@pytest.mark.parametrize("geo", GEOMETRY, ids=lambda g: "-".join("%s%s" % (k, v) for k, v in g.items()).replace(" ", ""))
def test_geometry_every_int8_family(built, geo):
    """The geometry list of test_geometry_every_family on the int8 families: a 9 x 7 input, Ci = 3, 4, 16, 64 under every tfl_dot
    that selects another kernel, depthwise 8 channels."""
    rng = np.random.default_rng(len(str(geo)) + 1)
    kh, kw = geo["k"]
    for ci, dw in ((3, False), (4, False), (16, False), (64, False), (8, True)):
        co = 8 if dw else 9
        x = rng.integers(-128, 128, (2, 9, 7, ci)).astype(np.int8)
        m = Q.conv_model(9, 7, ci, co, kh, kw, zx=int(rng.choice(Q.ZXS)), zo=int(rng.integers(-21, 22)), stride=geo.get("stride", (1, 1)),
                         dil=geo.get("dil", (1, 1)), padding=geo.get("padding", 0), bias=rng.integers(-900, 900, co) if geo.get("bias", True) else None,
                         depthwise=dw, rng=rng)
        Q.fit_output_scale(m, x)
        wants, seen = Q.reference_images(m, x), set()
        for dot in (3, 2, 1, 0):
            fams = _families(m, dot)
            if fams[0][0] not in seen:
                seen.add(fams[0][0])
                Q.gpu_check(m, x, wants, _tune(dot), fams, {0: I8PC}, label=(geo, ci, dot))


FOLD_PRODUCERS = [("conv", 3, 3), ("conv", 3, 0), ("conv", 16, 3), ("conv", 64, 2), ("dw", 8, 3), ("dw", 6, 3), ("resize", 6, 3)]
FOLDED_FAMILY = {"RELU6": "requant", "TANH": "lut", "ADD": "add", "QUANTIZE": "requant"}


@pytest.mark.parametrize("producer,ci,dot", FOLD_PRODUCERS, ids=lambda v: str(v))
def test_folded_chains_int8(built, producer, ci, dot):
    """int8 producer -> RELU6 / TANH (table indices -128 and 127 reached) / TANH -> ADD and TANH -> QUANTIZE to uint8 (the chain goes
    on past the int8 table) / ADD with an int8 operand from an earlier launch or a constant / QUANTIZE to uint8, folded into the producer's epilogue: once per family, Co = 6 and 8, two images. tfl_fuse = 1 and 0
    give equal bytes, both the reference's; the folded operator reports 'folded' and the producer's own tensor is never written."""
    rng = np.random.default_rng(ci * 10 + dot + 1)
    fam = {"conv": Q.expected_conv_family(3, 3, ci, dot), "dw": K.expected_dw_family(3, 3, ci, 1, dot), "resize": "resize"}[producer]
    for co in ((6, 8) if producer == "conv" else (ci,)):
        for tail in Q.CHAIN_TAILS:
            if producer == "resize" and (tail == "add_act" or tail[:4] == "tanh"):
                continue
            m, x, prod, folded = Q.chain_model(producer, ci, co, tail, rng)
            wants = Q.reference_images(m, x)
            if tail[:4] == "tanh":
                mid = np.stack([wants[i][m.ops[prod].outputs[0]] for i in range(2)])
                assert mid.min() == -128 and mid.max() == 127
            fams = {prod: (fam, None, False, False)}
            fams.update({f: (FOLDED_FAMILY[m.ops[f].code], -1, False, True) for f in folded})
            quants = {prod: (True, producer != "resize")}
            quants.update({f: (m.tensors[m.ops[f].outputs[0]].dtype == "i8", False) for f in folded})
            fused = Q.gpu_check(m, x, wants, _tune(dot), fams, quants, label=(producer, ci, co, tail), tensors=True)
            plain_f = {f: (v[0], v[1], v[2], False) for f, v in fams.items()}
            plain = Q.gpu_check(m, x, wants, _tune(dot, tfl_fuse=0), plain_f, quants, label=("unfused", producer, ci, co, tail), tensors=True)
            assert all(np.array_equal(a, b) for a, b in zip(fused, plain))


def test_uint8_convolution_quantize_to_int8_int8_convolution(built):
    """A type change in the middle of a graph: uint8 convolution -> QUANTIZE to int8 -> int8 convolution. The QUANTIZE folds into
    the uint8 convolution's epilogue (its stores take the value's low byte); tfl_fuse 1 and 0 give equal bytes."""
    rng = np.random.default_rng(9)
    for co in (6, 8):
        m, x = Q.u8_quantize_i8_model(16, co, rng)
        fams = {0: ("conv_i8_direct", None, False, False), 1: ("requant", -1, False, False), 2: (Q.expected_conv_family(3, 3, co, 3), None, False, False)}     # (the second convolution's Ci is the first's Co: 6 runs px8)
        quants = {0: (False, False), 1: (True, False), 2: I8PC}
        a = Q.gpu_check(m, x, None, None, {**fams, 1: ("requant", -1, False, True)}, quants, tensors=True)
        b = Q.gpu_check(m, x, None, dict(tfl_fuse=0), fams, quants, tensors=True)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_element_wise_operators_alone_int8(built):
    """ADD on every (a, b) pair at the corners of both ranges; the four QUANTIZE directions where every other input is a tie of
    mbqm; DEQUANTIZE; RELU, RELU6, TANH over all 256 values; PAD filling with zp -128; RESHAPE of a constant."""
    xi = np.tile(np.arange(-128, 128).astype(np.int8), (2, 1))
    xu = np.tile(np.arange(256).astype(np.uint8), (2, 1))
    for za, zb, zo in ((-128, -128, -128), (127, 127, 127), (-128, 127, 0), (127, -128, 5)):
        for act in (0, 1, 3):
            m = Q.add_model(0.04, za, 0.07, zb, 0.09, zo, act)
            Q.gpu_check(m, np.concatenate([Q.add_input()] * 2), None, None, {0: ("add", -1, False, False)}, {0: (True, False)}, label=("add", za, zb, zo, act))
    directions = {("u8", "i8"): (xu, ((0.5, 1.0, 128, 0), (0.5, 1.0, 3, -1), (0.1, 0.1, 128, 0), (0.75, 0.1, 255, -128), (0.1, 0.75, 0, 127))),
                  ("i8", "u8"): (xi, ((0.5, 1.0, 0, 128), (0.5, 1.0, 3, 0), (0.1, 0.1, 0, 128), (0.75, 0.1, 127, 0), (0.1, 0.75, -128, 255))),
                  ("i8", "i8"): (xi, ((0.5, 1.0, 0, 0), (0.5, 1.0, 3, -1), (0.1, 0.1, 0, 0), (0.75, 0.1, 127, -128), (0.1, 0.75, -128, 127)))}
    for (dt_in, dt_out), (x, sets) in directions.items():       # (scale ratio 1/2: every other input is a tie)
        for si, so, zi, zo in sets:
            m = Q.unary_model("QUANTIZE", dt_in, dt_out, si, zi, so, zo, n=256)
            Q.gpu_check(m, x, None, None, {0: ("requant", -1, False, False)}, {0: (dt_out == "i8", False)}, label=("quantize", dt_in, dt_out, si, so))
    f = np.tile(np.concatenate([np.linspace(-40, 40, 201), (np.arange(-20, 20) + 0.5) * 0.25, [1000.0, -1000.0]]).astype(np.float32), (2, 1))
    for zo in (-128, 0, 127):
        Q.gpu_check(Q.unary_model("QUANTIZE", "f32", "i8", None, 0, 0.25, zo, n=f.shape[1]), f, None, None, {0: ("quantize_f32", -1, False, False)}, {0: (True, False)})
    for zi in (-128, 3, 127):
        Q.gpu_check(Q.unary_model("DEQUANTIZE", "i8", "f32", 0.37, zi, None, 0, n=256), xi, None, None, {0: ("dequantize", -1, False, False)}, {0: (None, False)})
        for code, fam in (("RELU", "requant"), ("RELU6", "requant"), ("TANH", "lut")):
            for si, so, zo in ((0.05, 0.03, -128), (0.5, 4.0, 127), (1 / 32, 1 / 128, 0)):
                Q.gpu_check(Q.unary_model(code, "i8", "i8", si, zi, so, zo, n=256), xi, None, None, {0: (fam, -1, False, False)}, {0: (True, False)}, label=(code, zi, si))
    m = Model()
    a = m.add(T("a", (1, 2, 3, 2), "i8", scale=0.1, zp=-128))
    pd = m.add(T("p", (4, 2), "i32", data=[[0, 0], [1, 0], [0, 2], [0, 1]]))
    b = m.add(T("b", (1, 3, 5, 3), "i8", scale=0.1, zp=-128))
    m.ops.append(Op("PAD", [a, pd], [b]))
    m.inputs, m.outputs = [a], [b]
    got = Q.gpu_check(m, np.arange(-12, 12).astype(np.int8).reshape(2, 2, 3, 2), None, None, {0: ("pad", -1, False, False)}, {0: (True, False)})
    assert (got[0] == -128).sum() >= 2 * (45 - 12)
    for n in (1, 17, 4113):
        m = Model()
        c = m.add(T("c", (n,), "i8", data=np.arange(n) % 256 - 128, scale=0.1, zp=0))
        x0 = m.add(T("x", (1, 4), "i8", scale=0.1, zp=0))
        r = m.add(T("r", (1, n), "i8", scale=0.1, zp=0))
        y0 = m.add(T("y", (1, 4), "i8", scale=0.1, zp=0))
        m.ops += [Op("RESHAPE", [c], [r], new_shape=[1, n]), Op("RELU", [x0], [y0])]
        m.inputs, m.outputs = [x0], [y0, r]
        Q.gpu_check(m, np.zeros((1, 1, 4), np.int8), None, None, {0: ("copy", -1, False, False)}, nbs=(1,))


@pytest.mark.parametrize("producer,dot", [("conv", 3), ("conv", 2), ("dw", 3)])
@pytest.mark.parametrize("lead,row", [(1, 1), (2, 1), (1, 3), (1, 5)])
def test_int8_concatenation_in_place_at_an_unaligned_byte(built, producer, dot, lead, row):
    """tfl_cases.unaligned_concat_model as int8: the producer (Co = 8: packed stores where the address allows) writes its part
    straight into the concatenated tensor behind lead x row constant bytes, so the part starts at an odd byte; fused equals plain."""
    rng = np.random.default_rng(lead * 10 + row)
    dw = producer == "dw"
    ci, co = (8, 8) if dw else (64, 8)
    x = rng.integers(-128, 128, (2, 3, 5, ci)).astype(np.int8)
    m = Q.conv_model(3, 5, ci, co, 3, 3, zx=-7, zo=9, bias=rng.integers(-500, 500, co), depthwise=dw, rng=rng)
    Q.fit_output_scale(m, x)
    y = m.ops[0].outputs[0]
    ty, n = m.tensors[y], 3 * 5 * co
    r = m.add(T("r", (1, n // row, row), "i8", scale=ty.scale, zp=ty.zp))
    m.ops.append(Op("RESHAPE", [y], [r], new_shape=[1, n // row, row]))
    c = m.add(T("lead", (1, lead, row), "i8", data=rng.integers(-128, 128, (1, lead, row)), scale=ty.scale, zp=ty.zp))
    out = m.add(T("cat", (1, lead + n // row, row), "i8", scale=ty.scale, zp=ty.zp))
    m.ops.append(Op("CONCATENATION", [c, r], [out], axis=1))
    m.outputs = [out]
    fam = "dw_c4" if dw else ("conv_i8_direct" if dot == 3 else "conv_i8_lds")
    fused = Q.gpu_check(m, x, None, _tune(dot), {0: (fam, None, False, False)}, {0: I8PC}, tensors=True)
    plain = Q.gpu_check(m, x, None, _tune(dot, tfl_fuse=0), {0: (fam, None, False, False)}, {0: I8PC}, tensors=True)
    assert np.array_equal(fused[0], plain[0])
    import yolact_amd as ya
    eng = ya.TfliteEngine(BQ.serialize(m), tune=_tune(dot))
    with pytest.raises(ya.YhError) as e:       # written in place: the producer's own tensor no longer exists
        eng.tensor(y, ty.shape, np.int8)
    assert e.value.code == ya.capi.ESTATE
    eng.close()


def test_int8_concatenation_with_another_scale_is_refused(built):
    """TFLite rescales only uint8 parts: an int8 CONCATENATION whose part has another scale is refused, by the reference too."""
    import yolact_amd as ya
    m = Model()
    a = m.add(T("a", (1, 4), "i8", scale=0.1, zp=0))
    c = m.add(T("c", (1, 4), "i8", data=[1, 2, 3, 4], scale=0.2, zp=0))
    y = m.add(T("y", (1, 8), "i8", scale=0.1, zp=0))
    m.ops.append(Op("CONCATENATION", [a, c], [y], axis=1))
    m.inputs, m.outputs = [a], [y]
    with pytest.raises(ya.YhError) as e:
        ya.TfliteEngine(BQ.serialize(m))
    assert "every int8 input must have the output's scale and zero point" in str(e.value)
    with pytest.raises(R.Refused):
        Q.reference_images(m, np.zeros((1, 1, 4), np.int8))


def test_integer_resize_int8(built):
    """The sizes of tfl_cases.resize_cases in the three modes with inputs at -128, -1, 0 and 127 (and random bytes)."""
    rng = np.random.default_rng(4)
    for h, w, ho, wo, align, hp, xu in K.resize_cases(rng):
        for fill in ("ends", "random"):
            x = rng.choice(np.array([-128, -1, 0, 127], np.int8), (2,) + xu.shape[1:]) if fill == "ends" else rng.integers(-128, 128, (2,) + xu.shape[1:]).astype(np.int8)
            Q.gpu_check(Q.resize_model(h, w, ho, wo, align, hp), x, None, None, {0: ("resize", -1, False, False)}, {0: (True, False)}, label=(h, w, ho, wo, align, hp, fill))


def test_whole_graphs_int8_twins(built):
    """The int8 / per-channel twin of mobilenet_like(S = 64, C = 6) - uint8 input behind a QUANTIZE, int8 body, output 4 behind a
    QUANTIZE to uint8, output 0 behind a DEQUANTIZE - of random DAGs, int8 throughout, and of random DAGs with uint8 and int8
    regions joined by QUANTIZE (tfl_models_q.mixed_twin): every tensor the plan still writes equals the reference
    (a folded one says so), fused and grouped (default) and plain."""
    import tfl_models as M
    import tfl_models_q as MQ
    rng = np.random.default_rng(7)
    twin = Q.int8_twin(M.mobilenet_like(rng, S=64, C=6), rng)
    x = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    wants = Q.reference_images(twin, x)
    assert twin.tensors[twin.outputs[4]].dtype == "u8" and twin.tensors[twin.outputs[0]].dtype == "f32"
    quants = {i: I8PC for i, o in enumerate(twin.ops) if o.code in ("CONV_2D", "DEPTHWISE_CONV_2D")}
    quants[0] = (True, False)
    Q.gpu_check(twin, x, wants, None, None, quants, tensors=True, label="mobilenet twin")
    Q.gpu_check(twin, x, wants, dict(tfl_fuse=0, tfl_group=0), None, quants, tensors=True, label="mobilenet twin, plain")
    for seed in range(3):
        rng = np.random.default_rng(1000 + seed)
        twin = Q.int8_twin(M.random_dag(rng, n_ops=36), rng, dequant_output=None, quant_output=0)
        x = rng.integers(0, 256, (2,) + twin.tensors[twin.inputs[0]].shape[1:], dtype=np.uint8)
        wants = Q.reference_images(twin, x)
        Q.gpu_check(twin, x, wants, None, tensors=True, label=("dag twin", seed))
        Q.gpu_check(twin, x, wants, dict(tfl_fuse=0, tfl_group=0), tensors=True, label=("dag twin, plain", seed))
    for seed in range(4):      # uint8 and int8 regions joined by QUANTIZE: every fold, group and ADD meets both types
        rng = np.random.default_rng(2000 + seed)
        twin = MQ.mixed_twin(M.random_dag(rng, n_ops=36), rng)
        kinds = {(o.code, twin.tensors[o.outputs[0]].dtype) for o in twin.ops}
        assert {("CONV_2D", "u8"), ("CONV_2D", "i8"), ("QUANTIZE", "u8"), ("QUANTIZE", "i8")} <= kinds
        x = rng.integers(0, 256, (2,) + twin.tensors[twin.inputs[0]].shape[1:], dtype=np.uint8)
        wants = Q.reference_images(twin, x)
        a = Q.gpu_check(twin, x, wants, None, tensors=True, label=("mixed dag", seed))
        b = Q.gpu_check(twin, x, wants, dict(tfl_fuse=0, tfl_group=0), tensors=True, label=("mixed dag, plain", seed))
        assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_refusals_at_create_int8(built):
    import yolact_amd as ya
    rng = np.random.default_rng(5)

    def refused(m, words):
        with pytest.raises(ya.YhError) as e:
            ya.TfliteEngine(BQ.serialize(m))
        assert words in str(e.value), str(e.value)

    m = Q.conv_model(3, 5, 16, 4, 1, 1, rng=rng, xdtype="u8", wdtype="u8", zw=128, zx=128)       # uint8 with per-channel weight scales
    refused(m, "uint8 activations with per-channel weight scales")
    m = Q.conv_model(3, 5, 16, 4, 1, 1, rng=rng, wdtype="u8", zw=128, sw=0.01)                    # int8 activations, uint8 weights
    refused(m, "int8 activations with uint8 weights")
    refused(Q.add_model(0.04, 0, 0.07, 128, 0.09, 0, dt="i8", dt_b="u8"), "tensors of one type")
