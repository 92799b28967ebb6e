"""-m gpu: the quantisation edges of the TFLite executor - rounding ties of both signs at both stages of the requantisation, a left
shift and a vanishing multiplier, zero points and data at 0 and 255 in every convolution family's zero-point algebra, and the
element-wise operators over their whole domain - bit for bit against oracle/tfl_oracle.py, which tests/test_tfl_cases.py holds to the
plain-integer statement of tests/tfl_cases.py on these very cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfl_builder as B
import tfl_cases as K

pytestmark = pytest.mark.gpu

DOTS = (3, 2, 1, 0)


def _tune(dot):
    return None if dot == 3 else dict(tfl_dot=dot)


def _family(model, dot):
    o = model.ops[0]
    w = model.tensors[o.inputs[1]].shape
    if o.code == "CONV_2D":
        return K.expected_conv_family(w[1], w[2], w[3], dot)
    return K.expected_dw_family(w[1], w[2], w[3], o.opts.get("depth_multiplier", 1), dot)


def _every_family(model, x, wants, label, more=()):
    """The model under every tfl_dot that selects another kernel family; returns the families run."""
    blob, seen = bytes(B.serialize(model)), []
    for dot in DOTS:
        fam = _family(model, dot)
        if fam in seen:
            continue
        seen.append(fam)
        K.gpu_check(model, x, wants, _tune(dot), {0: (fam, None, False, False)}, nbs=(len(x),), blob=blob, label=(label, dot), more=more)
    return seen


@pytest.mark.parametrize("ratio", K.TIE_RATIOS, ids=lambda r: "%g" % r)
def test_tie_sweep_every_convolution_family(built, ratio):
    """Accumulators g (p - 128) for every byte p and g in (1, -1, 2, -2, 3, -3, 5, -7) through a 1 x 1 convolution (Ci = 3, 4, 16, 64)
    and its depthwise analogue, in every kernel family: ratios 2^-1, 2^-3, 2^-6 put ties of both signs at both rounding stages (half
    up in the high multiplication, half away from zero in the shift, 3 / 8 -> 1 by the double rounding); 0.75; 2.0 and 3.7 take the
    left-shift branch; at 1e-11 the multiplier is (0, 0) and every output is the zero point."""
    seen = set()
    for ci, dw in ((3, False), (4, False), (16, False), (64, False), (8, True)):
        m, x = K.tie_model(ci, ratio, depthwise=dw)
        wants = K.oracle_images(m, x)
        want = wants[0][m.outputs[0]]
        mult, shift = K.conv_multiplier(m)
        for p in (0, 1, 125, 127, 129, 131, 255):          # the statement itself, on the spot
            for c, g in enumerate(K.TIE_GAINS):
                assert want[0, p // 16, p % 16, c] == min(255, max(0, K.mbqm(g * (p - 128), mult, shift) + 128))
        if ratio == 1e-11:
            assert (want == 128).all()
        seen |= set(_every_family(m, x, wants, (ratio, ci)))
    assert seen == {"conv_px8", "conv_scalar", "conv_i8_direct", "conv_dot1", "conv_dot4", "conv_i8_lds", "dw_c4", "dw_scalar"}
    print("tie case ratio %g: multiplier %s, census (ties > 0, ties < 0, saturated, two roundings != one) %s; families %s"
          % (ratio, K.quantize_multiplier(ratio), K.tie_census(ratio) if ratio in K.TIE_POW2 else "-", sorted(seen)))


@pytest.mark.parametrize("zx,zw", K.CORNER_ZPS)
@pytest.mark.parametrize("ci", K.CORNER_CIS + (8,))
def test_zero_point_corners_every_family(built, ci, zx, zw):
    """(zx, zw) in {0, 255}^2 and (128, 128), zo in {0, 255, 128}, data all 0 / all 255 / random, weights all 0 / all 255 / random,
    3 x 3 SAME on 5 x 4 pixels (14 of 20 with padded taps), Co = 9: the dot-product kernel's n Ci zx zw - zw sum(x), the int8
    kernels' xterm / cterm and the padded tap fed zx, against the oracle in every family the layer can run on. The three data variants
    run as two invokes of one engine: two images, then one."""
    rng = np.random.default_rng(100 + ci)          # (the generator tests/test_tfl_cases.py checks the conditions with)
    dw = ci == 8
    fams = set()
    for pair in K.CORNER_ZPS:
        for zo in K.CORNER_ZOS:
            models, x0 = K.corner_models(ci, pair[0], pair[1], zo, rng, depthwise=dw)
            xs = np.concatenate([x0] + K.corner_inputs(ci, rng)[1:])
            if pair != (zx, zw):
                continue
            for m in models:
                wants = K.oracle_images(m, xs)
                fams |= set(_every_family(m, xs[:2], wants[:2], (ci, zx, zw, zo), more=[(xs[2:], wants[2:])]))
    print("corner case Ci %d zx %d zw %d: families %s" % (ci, zx, zw, sorted(fams)))
    assert len(fams) == (2 if ci in (3, 8) else (4 if ci % 64 == 0 else 3))


@pytest.mark.parametrize("ps", K.ADD_SETS, ids=lambda p: "-".join("%g" % v for v in p))
def test_add_on_all_code_pairs_alone_and_folded(built, ps):
    """ADD on all 65 536 (a, b) code pairs - the stand-alone kernel against the oracle, and the same ADD folded behind an identity
    1 x 1 convolution (ratio 1, zo = zx) against the stand-alone kernel."""
    x = K.add_input()
    alone = K.add_model(ps)
    wants = K.oracle_images(alone, x)
    a = K.gpu_check(alone, x, wants, None, {0: ("add", -1, False, False)}, nbs=(1,), label=ps)[0]
    assert np.array_equal(a.reshape(256, 256), K.add_exact(ps))
    fm = K.add_model(ps, folded=True)
    fw = K.oracle_images(fm, x)
    assert np.array_equal(fw[0][fm.ops[0].outputs[0]], x)          # the identity convolution reproduces every code
    for dot in (3, 0):
        f = K.gpu_check(fm, x, fw, _tune(dot), {0: ("conv_px8" if dot else "conv_scalar", -1, False, False), 1: ("add", -1, False, True)}, nbs=(1,), label=ps)[0]
        assert np.array_equal(f, a)


@pytest.mark.parametrize("code", K.UNARY_CODES)
def test_unary_operators_on_all_codes(built, code):
    """RELU, RELU6, QUANTIZE (u8 -> u8), TANH, DEQUANTIZE and the CONCATENATION rescale on all 256 codes, per parameter set: zero
    points 0 and 255, ratios above and below 1, powers of two (ties)."""
    fam = {"RELU": "requant", "RELU6": "requant", "QUANTIZE": "requant", "TANH": "lut", "DEQUANTIZE": "dequantize", "CONCATENATION": "concat"}[code]
    x = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    for ps in K.UNARY_SETS:
        m = K.unary_model(code, ps)
        wants = K.oracle_images(m, x)
        got = K.gpu_check(m, x, wants, None, {0: (fam, -1, False, False)}, nbs=(1,), label=(code, ps))[0]
        if code in ("RELU", "RELU6", "QUANTIZE"):
            assert np.array_equal(got.reshape(-1), K.unary_exact(code, ps))
        if code == "TANH" and ps[1] not in (0, 255) and ps[3] not in (0, 255):
            assert len(np.unique(got)) > 50            # (with a zero point at an end of the range the table is one-sided or flat)
    print("unary case %s: %d parameter sets on 256 codes, family %s" % (code, len(K.UNARY_SETS), fam))


@pytest.mark.parametrize("scale,zo", [(0.5, 128), (0.125, 0), (2.0, 255)])
def test_quantize_from_float32(built, scale, zo):
    """Exact half-integers times the scale of both signs, +-0, subnormals, the clamp edges +- 1/2, |x / scale| up to 2^24."""
    x = K.quantize_f32_cases(scale, zo)
    m = K.quantize_f32_model(len(x), scale, zo)
    xs = x.reshape(1, 1, len(x), 1)
    wants = K.oracle_images(m, xs)
    got = K.gpu_check(m, xs, wants, None, {0: ("quantize_f32", -1, False, False)}, nbs=(1,), label=(scale, zo))[0]
    assert np.array_equal(got.reshape(-1), K.quantize_f32_exact(x, scale, zo))


def test_resize_bilinear_edges(built):
    """7 -> 3 (downscale), 1 x 1 -> 4 x 4, Ho = 1 with align_corners, x2 on codes 0 / 255 and on neighbours that differ by an odd
    number (the midpoints are v + 1/2 exactly), with and without half_pixel_centers."""
    rng = np.random.default_rng(12)
    for h, w, ho, wo, align, hp, x in K.resize_cases(rng):
        m = K.resize_model(h, w, ho, wo, align, hp)
        xs = np.concatenate([x, x[:, ::-1]])
        wants = K.oracle_images(m, xs)
        K.gpu_check(m, xs, wants, None, {0: ("resize", -1, False, False)}, label=(h, w, ho, wo, align, hp))
    print("resize cases: %d passed" % len(K.resize_cases(rng)))
