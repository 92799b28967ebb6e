"""-m gpu: every kernel form of the TFLite executor, named and checked. yh_tfl_op_info says which kernel an operator runs on, so each
case asserts the family (and, for the register-fed int8 convolution, the row of its table of forms and whether it ran in a group)
before it compares the bytes with oracle/tfl_oracle.py. The cases and their conditions: tests/tfl_cases.py, tests/test_tfl_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfl_builder as B
import tfl_cases as K

pytestmark = pytest.mark.gpu

DOTS = (3, 2, 1, 0)


def _tune(dot, **more):
    t = dict(more)
    if dot != 3:
        t["tfl_dot"] = dot          # (3 is the default: that plan runs with no field set)
    return t or None


def _conv_families(model, dot, rows=None):
    """{op: (family, row, grouped, folded)} of a model of lone convolutions under tfl_dot."""
    out = {}
    for i, o in enumerate(model.ops):
        w = model.tensors[o.inputs[1]].shape
        if o.code == "CONV_2D":
            fam = K.expected_conv_family(w[1], w[2], w[3], dot)
            row = K.direct_form(rows, w[1], w[2], w[3]) if (rows and fam == "conv_i8_direct") else (-1 if fam != "conv_i8_direct" else None)
        else:
            fam, row = K.expected_dw_family(w[1], w[2], w[3], o.opts.get("depth_multiplier", 1), dot), -1
        out[i] = (fam, row, False, False)
    return out


@pytest.mark.parametrize("case", K.FORM_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_every_row_of_the_table_single(built, case):
    """The smallest convolution that selects each row of kDirectForms (3 x 5 pixels, SAME, Co = 17: two channel tiles, byte stores)
    and its last-chunk variants (Ci 4, 12, 60 less), one and two images: family and row as reported, bytes equal to the oracle; then
    the same layer on the LDS tiles (Ci % 64 == 0 only), the dot-product kernels and the scalar kernel."""
    from yolact_amd import capi
    rows = capi.tfl_direct_forms()
    kh, kw, ci = case
    rng = np.random.default_rng(kh * 100000 + kw * 10000 + ci)
    for less in K.LAST_CHUNK:
        c = ci - less
        m = K.form_model(kh, kw, c, rng)
        x = rng.integers(0, 256, (2, 3, 5, c), dtype=np.uint8)
        wants, blob = K.oracle_images(m, x), bytes(B.serialize(m))
        for dot in DOTS:
            fams = _conv_families(m, dot, rows)
            assert (dot == 3) == (fams[0][0] == "conv_i8_direct") and (fams[0][0] == "conv_i8_lds") == (dot == 2 and c % 64 == 0)
            K.gpu_check(m, x, wants, _tune(dot), fams, blob=blob, label=(case, less))
        print("form case %dx%dx%d: row %d %s" % (kh, kw, c, fams[0][1] if dot == 3 else K.direct_form(rows, kh, kw, c), rows[K.direct_form(rows, kh, kw, c)]))


@pytest.mark.parametrize("case", K.FORM_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_every_row_of_the_table_grouped(built, case):
    """Three independent convolutions of one row on one input (Co 17, 16, 1; the last with stride 2: three M, three tile counts):
    all three report 'in a group' under the default tuning and 'single' under tfl_group = 0; both equal the oracle on every output."""
    from yolact_amd import capi
    rows = capi.tfl_direct_forms()
    kh, kw, ci = case
    rng = np.random.default_rng(kh * 100000 + kw * 10000 + ci + 1)
    m = K.group_model(kh, kw, ci, rng)
    x = rng.integers(0, 256, (2, 3, 5, ci), dtype=np.uint8)
    wants, blob = K.oracle_images(m, x), bytes(B.serialize(m))
    row = K.direct_form(rows, kh, kw, ci)
    K.gpu_check(m, x, wants, None, {i: ("conv_i8_direct", row, True, False) for i in range(3)}, blob=blob, label=case)
    K.gpu_check(m, x, wants, dict(tfl_group=0), {i: ("conv_i8_direct", row, False, False) for i in range(3)}, blob=blob, label=case)
    print("group case %dx%dx%d: row %d grouped and single" % (kh, kw, ci, row))


PX8 = [(2, 16, 16, "conv_px8"), (3, 9, 19, "conv_scalar"), (513, 1, 1, "conv_scalar"), (3, 3, 3, "conv_px8"), (5, 3, 3, "conv_px8")]


@pytest.mark.parametrize("ci,kh,kw,fam", PX8, ids=lambda v: str(v))
def test_px8_and_its_fall_to_the_scalar_kernel(built, ci, kh, kw, fam):
    """tfl_conv_u8_px8 holds kh kw Ci <= 512 weights per channel in LDS: 512 exactly is taken (16 x 16 x 2), 513 falls to the scalar
    kernel (9 x 19 x 3; 1 x 1 x 513); Ci = 3 and 5 at 3 x 3. Co = 1, 8, 9 (around the 8-channel block), 255 and 257 output pixels
    (around the 256-pixel workgroup), one and two images; tfl_dot = 0 runs the scalar kernel on all of them."""
    assert (kh * kw * ci <= 512) == (fam == "conv_px8") and kh * kw * ci in (512, 513, 27, 45)
    rng = np.random.default_rng(ci * 1000 + kh)
    for co in (1, 8, 9):
        for h, w in ((15, 17), (1, 257)):
            m = K.conv_model(h, w, ci, co, kh, kw, x_zp=int(rng.integers(0, 256)), w_zp=int(rng.integers(0, 256)), y_zp=120,
                             bias=rng.integers(-900, 900, co), rng=rng)
            x = rng.integers(0, 256, (2, h, w, ci), dtype=np.uint8)
            K.fit_output_scale(m, K.conv_acc(m, x[:1])[0])
            wants, blob = K.oracle_images(m, x), bytes(B.serialize(m))
            K.gpu_check(m, x, wants, None, {0: (fam, -1, False, False)}, blob=blob, label=(ci, kh, kw, co, h))
            K.gpu_check(m, x, wants, dict(tfl_dot=0), {0: ("conv_scalar", -1, False, False)}, blob=blob, label=(ci, kh, kw, co, h))
    print("px8 case Ci %d %dx%d: %s" % (ci, kh, kw, fam))


def test_dot4_dot1_and_depthwise_families(built):
    """tfl_dot = 1: Ci = 16 runs the dot-product kernel with K split over four waves, Ci = 20 the one-wave form; depthwise 3 x 3 with
    Co = 8 runs four channels per lane, Co = 6, depth multiplier 2 and 5 x 5 the scalar kernel. 9 x 8 pixels (two 64-pixel blocks)."""
    rng = np.random.default_rng(77)
    for ci, fam in ((16, "conv_dot4"), (20, "conv_dot1")):
        m = K.conv_model(9, 8, ci, 9, 3, 3, x_zp=3, w_zp=250, y_zp=130, bias=rng.integers(-900, 900, 9), rng=rng)
        x = rng.integers(0, 256, (2, 9, 8, ci), dtype=np.uint8)
        K.fit_output_scale(m, K.conv_acc(m, x[:1])[0])
        wants = K.oracle_images(m, x)
        assert K.expected_conv_family(3, 3, ci, 1) == fam
        for dot in DOTS:
            K.gpu_check(m, x, wants, _tune(dot), _conv_families(m, dot), label=(ci, dot))
    for ci, dm, k, fam in ((8, 1, 3, "dw_c4"), (6, 1, 3, "dw_scalar"), (4, 2, 3, "dw_scalar"), (8, 1, 5, "dw_scalar")):
        m = K.conv_model(9, 8, ci, 0, k, k, x_zp=7, w_zp=201, y_zp=99, bias=rng.integers(-900, 900, ci * dm), depthwise=True, dm=dm, rng=rng)
        x = rng.integers(0, 256, (2, 9, 8, ci), dtype=np.uint8)
        K.fit_output_scale(m, K.conv_acc(m, x[:1])[0])
        wants = K.oracle_images(m, x)
        K.gpu_check(m, x, wants, None, {0: (fam, -1, False, False)}, label=(ci, dm, k))
        K.gpu_check(m, x, wants, dict(tfl_dot=0), {0: ("dw_scalar", -1, False, False)}, label=(ci, dm, k))
        print("depthwise case C %d dm %d %dx%d: %s" % (ci, dm, k, k, fam))


GEOMETRY = [dict(k=(3, 3), dil=(2, 2), padding=0), dict(k=(3, 3), dil=(2, 2), padding=1), dict(k=(3, 3), dil=(2, 1), padding=0),
            dict(k=(3, 3), dil=(2, 1), padding=1), dict(k=(1, 3)), dict(k=(3, 1)), dict(k=(2, 2)), dict(k=(3, 3), stride=(1, 2)),
            dict(k=(3, 3), stride=(2, 1)), dict(k=(3, 3), bias=False), dict(k=(2, 2), dil=(2, 1), stride=(1, 2), bias=False, padding=1)]


@pytest.mark.parametrize("geo", GEOMETRY, ids=lambda g: "-".join("%s%s" % (k, v) for k, v in g.items()).replace(" ", ""))
def test_geometry_every_family(built, geo):
    """Dilation 2 and (2, 1), SAME and VALID; kernels 1 x 3, 3 x 1, 2 x 2; strides (1, 2) and (2, 1); a convolution without a bias
    operand - on a 9 x 7 input, on every kernel family that takes it (Ci = 3, 4, 16, 64 under every tfl_dot; depthwise 8 channels),
    one and two images."""
    rng = np.random.default_rng(len(str(geo)))
    kh, kw = geo["k"]
    for ci, dw in ((3, False), (4, False), (16, False), (64, False), (8, True)):
        co = 8 if dw else 9
        m = K.conv_model(9, 7, ci, co, kh, kw, x_zp=int(rng.integers(0, 256)), w_zp=int(rng.integers(0, 256)), y_zp=int(rng.integers(60, 200)),
                         stride=geo.get("stride", (1, 1)), dil=geo.get("dil", (1, 1)), padding=geo.get("padding", 0),
                         bias=rng.integers(-900, 900, co) if geo.get("bias", True) else None, depthwise=dw, rng=rng)
        assert (len(m.ops[0].inputs) == 2) == (not geo.get("bias", True))
        x = rng.integers(0, 256, (2, 9, 7, ci), dtype=np.uint8)
        K.fit_output_scale(m, K.conv_acc(m, x[:1])[0])
        wants, blob = K.oracle_images(m, x), bytes(B.serialize(m))
        seen = set()
        for dot in DOTS:
            fams = _conv_families(m, dot)
            if fams[0][0] in seen:
                continue
            seen.add(fams[0][0])
            K.gpu_check(m, x, wants, _tune(dot), fams, blob=blob, label=(geo, ci, dot))
    print("geometry case %s: passed on every family" % (geo,))


FOLD_PRODUCERS = [("conv", 3, 3), ("conv", 3, 0), ("conv", 16, 3), ("conv", 16, 1), ("conv", 20, 1), ("conv", 64, 2), ("dw", 8, 3), ("dw", 6, 3), ("resize", 6, 3)]


@pytest.mark.parametrize("producer,ci,dot", FOLD_PRODUCERS, ids=lambda v: str(v))
def test_folded_operators_per_family(built, producer, ci, dot):
    """conv -> ADD -> RELU6 (the convolution's output as either operand; the other a constant or an earlier activation) and conv ->
    TANH, folded into the producer's epilogue: once per convolution family and once behind RESIZE_BILINEAR, Co = 6 and 8, two images.
    The fused plan equals the oracle and the tfl_fuse = 0 plan, and the folded operators report 'folded'. (The constant operand is
    the case that found the batch plan reading past a constant: image 1 must meet the same constant.)"""
    import yolact_amd as ya
    rng = np.random.default_rng(ci * 10 + dot)
    fam = {"conv": K.expected_conv_family(3, 3, ci, dot), "dw": K.expected_dw_family(3, 3, ci, 1, dot), "resize": "resize"}[producer]
    for co in ((6, 8) if producer == "conv" else (ci,)):
        variants = [("add", o, k) for o in ("qa", "aq") for k in ("const", "act") if not (producer == "resize" and k == "act")] + [("tanh", "qa", "const")]
        for tail, order, other in variants:
            m, folded = K.folded_model(producer, ci, co, tail, rng, order, other)
            x = rng.integers(0, 256, (2,) + m.tensors[m.inputs[0]].shape[1:], dtype=np.uint8)
            wants, blob = K.oracle_images(m, x), bytes(B.serialize(m))
            prod = folded[0] - 1
            fams = {prod: (fam, None, False, False)}
            fams.update({f: ({"ADD": "add", "RELU6": "requant", "TANH": "lut"}[m.ops[f].code], -1, False, True) for f in folded})
            fused = K.gpu_check(m, x, wants, _tune(dot), fams, blob=blob, label=(producer, ci, co, tail, order, other))
            plain_f = {f: (v[0], v[1], v[2], False) for f, v in fams.items()}
            plain = K.gpu_check(m, x, wants, _tune(dot, tfl_fuse=0), plain_f, blob=blob, label=("unfused", producer, ci, co, tail))
            assert all(np.array_equal(a, b) for a, b in zip(fused, plain))
            eng = ya.TfliteEngine(blob, tune=_tune(dot))
            with pytest.raises(ya.YhError) as e:       # the producer's own tensor is never written
                eng.tensor(m.ops[prod].outputs[0], m.tensors[m.ops[prod].outputs[0]].shape, np.uint8)
            assert e.value.code == ya.capi.ESTATE
            eng.close()
    print("folded case %s Ci %d tfl_dot %d: %s" % (producer, ci, dot, fam))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4113])
def test_reshape_of_a_constant_runs_the_copy_kernel(built, n):
    """tfl_copy_bytes serves only a RESHAPE of a constant (an activation's RESHAPE shares the buffer): 16-byte body and byte tail
    around 16 and around a 256-lane block of 16-byte words; one and two images (each image gets the constant)."""
    rng = np.random.default_rng(n)
    m = K.copy_model(n, rng)
    x = rng.integers(0, 256, (2, 2, 2, 4), dtype=np.uint8)
    wants = K.oracle_images(m, x)
    assert np.array_equal(wants[1][m.outputs[0]].reshape(-1), m.tensors[1].data)
    K.gpu_check(m, x, wants, None, {0: ("copy", -1, False, False), 1: ("requant", -1, False, False)}, label=n)


@pytest.mark.parametrize("producer,dot", [("conv", 3), ("conv", 2), ("dw", 3)])
@pytest.mark.parametrize("lead,row", [(1, 1), (2, 1), (1, 3), (1, 5)])
def test_in_place_concatenation_part_at_an_unaligned_byte(built, producer, dot, lead, row):
    """A CONCATENATION along axis 1 whose in-place part starts at byte 1, 2, 3 (and 5) of the output, behind a constant part: the
    int8 convolution's epilogue (register-fed and LDS tiles) and the four-channel depthwise kernel take their byte-store branch. The
    part is folded (reading the producer's tensor gives YH_ESTATE); the output equals the oracle for one and two images - in image 1
    the part starts at another byte again (the whole row is odd)."""
    import yolact_amd as ya
    rng = np.random.default_rng(lead * 10 + row)
    m, y = K.unaligned_concat_model(lead, row, producer, rng)
    assert (lead * row) % 4 != 0
    x = rng.integers(0, 256, (2,) + m.tensors[0].shape[1:], dtype=np.uint8)
    wants, blob = K.oracle_images(m, x), bytes(B.serialize(m))
    fam = "dw_c4" if producer == "dw" else ("conv_i8_direct" if dot == 3 else "conv_i8_lds")
    K.gpu_check(m, x, wants, _tune(dot), {0: (fam, None, False, False), 2: ("concat", -1, False, False)}, blob=blob, label=(producer, dot, lead, row))
    eng = ya.TfliteEngine(blob, tune=_tune(dot))
    with pytest.raises(ya.YhError) as e:
        eng.tensor(y, m.tensors[y].shape, np.uint8)
    assert e.value.code == ya.capi.ESTATE and "folded" in str(e.value)
    assert eng.op_info(1) == dict(family=None, row=-1, grouped=False, folded=True)      # the RESHAPE shares its input's buffer
    eng.close()
    K.gpu_check(m, x, wants, _tune(dot, tfl_fuse=0), {0: (fam, None, False, False)}, blob=blob, label=("unfused", producer, dot, lead, row))
