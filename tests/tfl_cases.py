"""Cases for the TFLite executor's kernel forms and quantisation edges (tests/test_tfl_cases.py on the CPU,
tests/test_gpu_tflite_forms.py and tests/test_gpu_tflite_quant.py on the GPU): model builders on tfl_builder, the conditions every
case must satisfy, and an exact statement of gemmlowp's fixed-point step in Python integers and fractions.Fraction only.

    srdhm(a, b)   = floor((a b + 2^30) / 2^31), INT_MAX at a = b = INT_MIN      (one rounding, half UP, toward +inf)
    rdbpot(x, e)  = x / 2^e rounded half AWAY from zero
    mbqm(x, m, s) = rdbpot(srdhm(x 2^max(s, 0), m), max(-s, 0))                  (two roundings: 3 at ratio 2^-3 gives 1, not 0)
"""
import math
from fractions import Fraction

import numpy as np

from tfl_builder import Model, Op, T

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


# ------------------------------------------------------------------ the exact statement and its mutants
def round_half_away(q):
    """A Fraction to the nearest integer, halves away from zero."""
    q = Fraction(q)
    n = math.floor(abs(q) + Fraction(1, 2))
    return n if q >= 0 else -n


def srdhm(a, b):
    if a == I32_MIN and b == I32_MIN:
        return I32_MAX
    return (a * b + (1 << 30)) >> 31          # Python's >> is floor division


def rdbpot(x, e):
    if e == 0:
        return x
    n = (abs(x) + (1 << (e - 1))) >> e
    return n if x >= 0 else -n


def mbqm(x, m, s):
    return rdbpot(srdhm(x * (1 << max(s, 0)), m), max(-s, 0))


def mbqm_srdhm_away(x, m, s):
    """Mutant: the high multiplication rounds half away from zero."""
    return rdbpot(round_half_away(Fraction(x * (1 << max(s, 0)) * m, 1 << 31)), max(-s, 0))


def mbqm_once(x, m, s):
    """Mutant: ONE rounding (half away from zero) of the exact product x m / 2^(31 - s)."""
    return round_half_away(Fraction(x * m) * Fraction(2) ** (s - 31))


def mbqm_f32(x, ratio):
    """Mutant: float32 round(acc * scale)."""
    v = np.float32(np.float32(x) * np.float32(ratio))
    return int(np.floor(v + np.float32(0.5)) if v >= 0 else np.ceil(v - np.float32(0.5)))


def f32(s):
    return float(np.float32(s))


def quantize_multiplier(m):
    """tflite::QuantizeMultiplier(double) -> (Q31 mantissa, shift); (0, 0) below 2^-31."""
    if m == 0.0:
        return 0, 0
    q, shift = math.frexp(m)
    qf = int(math.floor(q * (1 << 31) + 0.5))
    if qf == (1 << 31):
        qf //= 2
        shift += 1
    return (0, 0) if shift < -31 else (qf, shift)


def conv_multiplier(model, op=0):
    o = model.ops[op]
    x, w, y = (model.tensors[i] for i in (o.inputs[0], o.inputs[1], o.outputs[0]))
    return quantize_multiplier(f32(x.scale) * f32(w.scale) / f32(y.scale))


# ------------------------------------------------------------------ the table of forms, restated
def direct_form(rows, kh, kw, ci):
    """conv_i8_direct_form (csrc/tflite_kernels.hip) on rows [(D, once, KK)]: the one-pass row of exactly n steps and this extent;
    else a looped row - where one-pass rows of n steps exist for other extents only, the deepest ring that n fills, otherwise the
    ring that pads n least, the deepest among equals; a ring deeper than n only when all are."""
    n = kh * kw * ((ci + 63) // 64)
    kk = 1 if (kh, kw) == (1, 1) else (3 if (kh, kw) == (3, 3) else 0)
    exact = False
    looped = [(i, d) for i, (d, once, _) in enumerate(rows) if not once]
    for i, (d, once, k) in enumerate(rows):
        if once and d == n and k == kk:
            return i
        exact = exact or (once and d == n)
    fit = [(i, d) for i, d in looped if d <= n]
    if not fit:
        return min(looped, key=lambda t: t[1])[0] if looped else -1
    if exact:
        return max(fit, key=lambda t: t[1])[0]
    return min(fit, key=lambda t: ((n + t[1] - 1) // t[1] * t[1] - n, -t[1]))[0]


# (kh, kw, Ci): the smallest convolution that selects each row; the shapes the suite already ran, then the eight rows nothing reached,
# then the looped rows' variants: fewer steps than the shallowest ring (1x3 x 64: n = 3 on D = 4), n = D, the deepest ring n fills
FORM_CASES = [(3, 3, 64), (3, 3, 128), (1, 1, 64), (1, 1, 128), (1, 1, 192), (1, 1, 384), (1, 1, 576), (1, 1, 960),
              (1, 1, 256), (1, 1, 320), (1, 1, 512), (1, 1, 768), (1, 1, 1152),
              (1, 1, 448), (1, 3, 128), (1, 1, 1024), (1, 3, 64), (2, 2, 64), (5, 5, 64), (3, 3, 256)]
LAST_CHUNK = (0, 4, 12, 60)     # channels below the case's Ci: the last 64-channel chunk holds 64, 60, 52 and 4


def expected_conv_family(kh, kw, ci, dot):
    """What a small CONV_2D is expected to run on under yh_tuning.tfl_dot (the claim the tests hold yh_tfl_op_info to)."""
    k = kh * kw * ci
    if dot >= 3 and ci % 4 == 0:
        return "conv_i8_direct"
    if dot >= 2 and ci % 64 == 0:
        return "conv_i8_lds"
    if dot >= 1 and ci % 4 == 0 and k * 65025 < (1 << 31):
        return "conv_dot4" if ci % 16 == 0 else "conv_dot1"
    if dot >= 1 and k <= 512:
        return "conv_px8"
    return "conv_scalar"


def expected_dw_family(kh, kw, co, dm, dot):
    return "dw_c4" if dot >= 1 and dm == 1 and (kh, kw) == (3, 3) and co % 4 == 0 else "dw_scalar"


# ------------------------------------------------------------------ geometry and exact accumulators
def out_geometry(h, w, kh, kw, stride, dil, padding):
    def same(i, k, s, d):
        o = -(-i // s)
        return o, max((o - 1) * s + (k - 1) * d + 1 - i, 0) // 2
    if padding == 0:
        (ho, ph), (wo, pw) = same(h, kh, stride[0], dil[0]), same(w, kw, stride[1], dil[1])
    else:
        ho, wo = (h - ((kh - 1) * dil[0] + 1) + stride[0]) // stride[0], (w - ((kw - 1) * dil[1] + 1) + stride[1]) // stride[1]
        ph = pw = 0
    return ho, wo, ph, pw


def conv_acc(model, x, op=0):
    """The int64 accumulators (bias included) of convolution `op` of `model` on input values x [1, H, W, Ci]: sums of
    (x - zx)(w - zw) over the taps inside the image - exact, and the count of padded taps per pixel."""
    o = model.ops[op]
    tx, tw = model.tensors[o.inputs[0]], model.tensors[o.inputs[1]]
    dw = o.code == "DEPTHWISE_CONV_2D"
    w = tw.data.astype(np.int64) - tw.zp
    _, h, ww, ci = x.shape
    kh, kw = w.shape[1], w.shape[2]
    co = w.shape[3] if dw else w.shape[0]
    stride, dil = (o.opts["stride_h"], o.opts["stride_w"]), (o.opts.get("dil_h", 1), o.opts.get("dil_w", 1))
    ho, wo, ph, pw = out_geometry(h, ww, kh, kw, stride, dil, o.opts["padding"])
    xi = x[0].astype(np.int64) - tx.zp
    acc = np.zeros((ho, wo, co), np.int64)
    padded = np.zeros((ho, wo), np.int64)
    src = np.repeat(np.arange(ci), o.opts.get("depth_multiplier", 1)) if dw else None
    for oy in range(ho):
        for ox in range(wo):
            for r in range(kh):
                for s in range(kw):
                    iy, ix = oy * stride[0] - ph + r * dil[0], ox * stride[1] - pw + s * dil[1]
                    if not (0 <= iy < h and 0 <= ix < ww):
                        padded[oy, ox] += 1
                        continue
                    acc[oy, ox] += xi[iy, ix][src] * w[0, r, s] if dw else w[:, r, s, :] @ xi[iy, ix]
    if len(o.inputs) > 2 and o.inputs[2] >= 0:
        acc += model.tensors[o.inputs[2]].data.astype(np.int64)
    return acc, padded


# ------------------------------------------------------------------ builders
def conv_model(h, w, ci, co, kh, kw, x_zp=128, w_zp=128, y_zp=128, sx=0.05, sw=0.01, so=0.08, stride=(1, 1), dil=(1, 1), padding=0,
               act=0, weights=None, bias=None, depthwise=False, dm=1, rng=None):
    """One CONV_2D / DEPTHWISE_CONV_2D. weights: an array, or None for random bytes from rng; bias: an int array, None for no bias
    OPERAND (two inputs)."""
    m = Model()
    x = m.add(T("x", (1, h, w, ci), "u8", scale=sx, zp=x_zp))
    if depthwise:
        co = ci * dm
    wshape = (1, kh, kw, co) if depthwise else (co, kh, kw, ci)
    wd = rng.integers(0, 256, wshape, dtype=np.uint8) if weights is None else np.asarray(weights, np.uint8).reshape(wshape)
    wt = m.add(T("w", wshape, "u8", data=wd, scale=sw, zp=w_zp))
    ins = [x, wt]
    if bias is not None:
        ins.append(m.add(T("b", (co,), "i32", data=np.asarray(bias, np.int32), scale=sx * sw, zp=0)))
    ho, wo, _, _ = out_geometry(h, w, kh, kw, stride, dil, padding)
    y = m.add(T("y", (1, ho, wo, co), "u8", scale=so, zp=y_zp))
    opts = dict(padding=padding, stride_h=stride[0], stride_w=stride[1], act=act, dil_h=dil[0], dil_w=dil[1])
    if depthwise:
        opts["depth_multiplier"] = dm
    m.ops.append(Op("DEPTHWISE_CONV_2D" if depthwise else "CONV_2D", ins, [y], **opts))
    m.inputs, m.outputs = [x], [y]
    return m


def fit_output_scale(model, acc, codes=100):
    """Sets the output scale from the reference's own accumulators so that the largest |acc| lands `codes` codes from the zero point."""
    o = model.ops[0]
    tx, tw, ty = (model.tensors[i] for i in (o.inputs[0], o.inputs[1], o.outputs[0]))
    ty.scale = f32(tx.scale) * f32(tw.scale) * max(int(np.abs(acc).max()), 1) / codes
    return model


def form_model(kh, kw, ci, rng, co=17, stride=(1, 1)):
    """The form cases' layer: 3 x 5 pixels, SAME, Co = 17 (two channel tiles, the second with one live channel; byte stores)."""
    m = conv_model(3, 5, ci, co, kh, kw, x_zp=int(rng.integers(1, 255)), w_zp=int(rng.integers(1, 255)), y_zp=int(rng.integers(100, 156)),
                   stride=stride, bias=rng.integers(-2000, 2000, co), act=int(rng.choice([0, 1, 3])), rng=rng)
    x = rng.integers(0, 256, (1, 3, 5, ci), dtype=np.uint8)
    return fit_output_scale(m, conv_acc(m, x)[0])


def group_model(kh, kw, ci, rng):
    """Three independent convolutions of one form on one input - Co 17, 16 and 1, the last with stride 2 (so three different M
    and tile counts) - and three outputs."""
    m = Model()
    x = m.add(T("x", (1, 3, 5, ci), "u8", scale=0.05, zp=int(rng.integers(1, 255))))
    xv = rng.integers(0, 256, (1, 3, 5, ci), dtype=np.uint8)
    for co, stride in ((17, (1, 1)), (16, (1, 1)), (1, (2, 2))):
        one = conv_model(3, 5, ci, co, kh, kw, x_zp=m.tensors[x].zp, w_zp=int(rng.integers(1, 255)), y_zp=int(rng.integers(100, 156)),
                         stride=stride, bias=rng.integers(-2000, 2000, co), rng=rng)
        fit_output_scale(one, conv_acc(one, xv)[0])
        ids = [x] + [m.add(t) for t in one.tensors[1:]]
        m.ops.append(Op("CONV_2D", ids[:3], [ids[3]], **one.ops[0].opts))
        m.outputs.append(ids[3])
    m.inputs = [x]
    return m


TIE_GAINS = (1, -1, 2, -2, 3, -3, 5, -7)
TIE_RATIOS = (2.0 ** -1, 2.0 ** -3, 2.0 ** -6, 0.75, 2.0, 3.7, 1e-11)
TIE_POW2 = TIE_RATIOS[:3]


def tie_model(ci, ratio, depthwise=False):
    """A 1 x 1 convolution on 16 x 16 pixels whose accumulators are g (p - 128) for every byte p and every g of TIE_GAINS: channel 0
    of pixel p holds p, the other channels the zero point; all weights but channel 0's equal the weights' zero point. Depthwise: 8
    channels that all hold p, a 3 x 3 kernel whose centre tap is zw + g (so that the four-channel kernel takes it)."""
    sx, sw = 0.5, 0.25
    if depthwise:
        w = np.full((1, 3, 3, 8), 128, np.uint8)
        w[0, 1, 1, :] = 128 + np.array(TIE_GAINS)
        m = conv_model(16, 16, 8, 8, 3, 3, sx=sx, sw=sw, so=sx * sw / ratio, weights=w, bias=np.zeros(8), depthwise=True)
        x = np.repeat(np.arange(256, dtype=np.uint8), 8).reshape(1, 16, 16, 8)
    else:
        w = np.full((8, 1, 1, ci), 128, np.uint8)
        w[:, 0, 0, 0] = 128 + np.array(TIE_GAINS)
        m = conv_model(16, 16, ci, 8, 1, 1, sx=sx, sw=sw, so=sx * sw / ratio, weights=w, bias=np.zeros(8))
        x = np.full((1, 16, 16, ci), 128, np.uint8)
        x[0, :, :, 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return m, x


def tie_census(ratio):
    """For a power-of-two ratio: over the tie case's 2048 accumulators, the unsaturated outputs whose exact value acc * ratio is a
    half-integer (positive, negative), the saturated outputs, and the unsaturated ones where the two roundings of mbqm differ from
    one rounding of the exact product. Fractions throughout."""
    m, s = quantize_multiplier(ratio)
    pos = neg = sat = differ = 0
    for g in TIE_GAINS:
        for p in range(256):
            acc = g * (p - 128)
            exact = Fraction(acc) * Fraction(ratio)
            out = mbqm(acc, m, s) + 128
            if not 0 < out < 255:
                sat += 1
                continue
            if exact.denominator == 2:
                pos, neg = pos + (exact > 0), neg + (exact < 0)
            differ += mbqm(acc, m, s) != mbqm_once(acc, m, s)
    return pos, neg, sat, differ


CORNER_ZPS = ((0, 0), (0, 255), (255, 0), (255, 255), (128, 128))
CORNER_ZOS = (0, 255, 128)
CORNER_CIS = (3, 4, 16, 64, 192)
CORNER_FILLS = ("random", 0, 255)


def corner_inputs(ci, rng):
    shape = (1, 5, 4, ci)
    return [rng.integers(0, 256, shape, dtype=np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)]


def corner_models(ci, zx, zw, zo, rng, depthwise=False):
    """3 x 3, SAME, 5 x 4 pixels (14 of 20 with padded taps), Co = 9 (depthwise: 8 channels): three models - random weights, all 0,
    all 255 - that share the bias and the output scale chosen on the random one from the reference's own accumulators: the quartile
    of the accumulators facing a clamp end at the zero point is moved onto it by the bias, the largest |acc| is 100 codes away."""
    co = 8 if depthwise else 9
    x = corner_inputs(ci, rng)[0]
    wshape = (1, 3, 3, co) if depthwise else (co, 3, 3, ci)
    wr = rng.integers(0, 256, wshape, dtype=np.uint8)
    base = conv_model(5, 4, ci, co, 3, 3, x_zp=zx, w_zp=zw, y_zp=zo, weights=wr, bias=np.zeros(co), depthwise=depthwise)
    acc, _ = conv_acc(base, x)
    shift = 0 if zo == 128 else int(-np.quantile(acc, 0.25 if zo == 0 else 0.75))
    bias = np.full(co, shift, np.int64)
    out = []
    for fill in CORNER_FILLS:
        wd = wr if fill == "random" else np.full(wshape, fill, np.uint8)
        m = conv_model(5, 4, ci, co, 3, 3, x_zp=zx, w_zp=zw, y_zp=zo, weights=wd, bias=bias, depthwise=depthwise)
        out.append(fit_output_scale(m, acc + shift, codes=100))
    return out, x


def copy_model(n, rng):
    """RESHAPE of a constant of n bytes as a graph output (the one operator that launches tfl_copy_bytes), beside a RELU of the input."""
    m = Model()
    x = m.add(T("x", (1, 2, 2, 4), "u8", scale=0.05, zp=120))
    c = m.add(T("c", (n,), "u8", data=rng.integers(0, 256, n, dtype=np.uint8), scale=0.05, zp=12))
    y = m.add(T("y", (1, n), "u8", scale=0.05, zp=12))
    r = m.add(T("r", (1, 2, 2, 4), "u8", scale=0.03, zp=10))
    m.ops.append(Op("RESHAPE", [c], [y], new_shape=[1, n]))
    m.ops.append(Op("RELU", [x], [r]))
    m.inputs, m.outputs = [x], [y, r]
    return m


def unaligned_concat_model(lead, row, producer, rng):
    """CONCATENATION along axis 1 of a constant [1, lead, row] and a convolution's output seen through RESHAPE as [1, n / row, row]:
    the in-place part starts at byte lead * row of every image (image 1: lead * row more than the whole row of image 0).
    producer: "conv" (int8 MFMA convolution, Ci 64, Co 8) or "dw" (depthwise 3 x 3, 8 channels)."""
    dw = producer == "dw"
    ci, co = (8, 8) if dw else (64, 8)
    m = conv_model(3, 5, ci, co, 3, 3, x_zp=121, w_zp=133, y_zp=117, bias=rng.integers(-500, 500, co), depthwise=dw, rng=rng)
    fit_output_scale(m, conv_acc(m, rng.integers(0, 256, (1, 3, 5, ci), dtype=np.uint8))[0])
    y = m.ops[0].outputs[0]
    ty = m.tensors[y]
    n = 3 * 5 * co
    assert n % row == 0
    r = m.add(T("r", (1, n // row, row), "u8", scale=ty.scale, zp=ty.zp))
    m.ops.append(Op("RESHAPE", [y], [r], new_shape=[1, n // row, row]))
    c = m.add(T("lead", (1, lead, row), "u8", data=rng.integers(0, 256, (1, lead, row), dtype=np.uint8), scale=ty.scale, zp=ty.zp))
    out = m.add(T("cat", (1, lead + n // row, row), "u8", scale=ty.scale, zp=ty.zp))
    m.ops.append(Op("CONCATENATION", [c, r], [out], axis=1))
    m.outputs = [out]
    return m, y


def _rescale_output(one, so):
    """The same ratio with the output scale `so` (the weights' scale takes the factor): +-100 codes = +-3 at 0.03, where tanh is not
    flat and an ADD's operands are of one size."""
    one.tensors[1].scale *= so / one.tensors[3].scale
    one.tensors[2].scale = one.tensors[0].scale * one.tensors[1].scale
    one.tensors[3].scale = so


def folded_model(producer, ci, co, tail, rng, order="qa", other="const"):
    """producer -> ADD -> RELU6 (tail "add": the producer's output as operand a (order "qa") or b ("aq"), the other operand a constant
    or an activation made by an earlier 1 x 1 convolution) or producer -> TANH (tail "tanh"). producer: "conv" 3 x 3, "dw" 3 x 3,
    "resize" (RESIZE_BILINEAR 3 x 2 -> 6 x 4: co = ci)."""
    m = Model()
    sc = lambda: float(rng.uniform(0.02, 0.08))
    zp = lambda: int(rng.integers(90, 160))
    H, W = (3, 2) if producer == "resize" else (6, 4)
    x = m.add(T("x", (1, H, W, ci), "u8", scale=0.05, zp=zp()))
    xv = rng.integers(0, 256, (1, H, W, ci), dtype=np.uint8)
    if producer in ("dw", "resize"):
        co = ci
    oth = None
    if tail == "add" and other == "act":      # made first: complete when the producer's launch reads it
        assert producer != "resize"
        one = conv_model(H, W, ci, co, 1, 1, x_zp=m.tensors[x].zp, w_zp=zp(), y_zp=zp(), bias=rng.integers(-500, 500, co), rng=rng)
        fit_output_scale(one, conv_acc(one, xv)[0])
        _rescale_output(one, 0.025)
        ids = [x] + [m.add(t) for t in one.tensors[1:]]
        m.ops.append(Op("CONV_2D", ids[:3], [ids[3]], **one.ops[0].opts))
        oth = ids[3]
        m.outputs.append(oth)
    if producer == "resize":
        sz = m.add(T("sz", (2,), "i32", data=[6, 4]))
        q = m.add(T("q", (1, 6, 4, co), "u8", scale=0.05, zp=m.tensors[x].zp))
        m.ops.append(Op("RESIZE_BILINEAR", [x, sz], [q], half_pixel_centers=True))
    else:
        one = conv_model(6, 4, ci, co, 3, 3, x_zp=m.tensors[x].zp, w_zp=zp(), y_zp=zp(), bias=rng.integers(-500, 500, co),
                         depthwise=producer == "dw", rng=rng)
        fit_output_scale(one, conv_acc(one, xv)[0])
        _rescale_output(one, 0.03)
        ids = [x] + [m.add(t) for t in one.tensors[1:]]
        m.ops.append(Op(one.ops[0].code, ids[:3], [ids[3]], **one.ops[0].opts))
        q = ids[3]
    shp = (1, 6, 4, co)
    folded = []
    if tail == "add":
        if oth is None:
            oth = m.add(T("k", shp, "u8", data=rng.integers(0, 256, shp, dtype=np.uint8), scale=sc(), zp=zp()))
        a = m.add(T("a", shp, "u8", scale=0.045, zp=zp()))
        m.ops.append(Op("ADD", [q, oth] if order == "qa" else [oth, q], [a], act=0))
        y = m.add(T("y", shp, "u8", scale=0.04, zp=int(rng.integers(20, 60))))
        m.ops.append(Op("RELU6", [a], [y]))
        folded = [len(m.ops) - 2, len(m.ops) - 1]
    else:
        y = m.add(T("y", shp, "u8", scale=1 / 128, zp=128))
        m.tensors[q].scale = 1 / 64 if producer == "resize" else m.tensors[q].scale
        m.ops.append(Op("TANH", [q], [y]))
        folded = [len(m.ops) - 1]
    m.inputs = [x]
    m.outputs.append(y)
    return m, folded


# ------------------------------------------------------------------ element-wise operators over their whole domain
# ADD: (a scale, a zp, b scale, b zp, y scale, y zp, act). The suite's own; equal scales; 1 : 64; zero points 0 and 255; an output
# scale small enough to saturate both ends; RELU6; and the mirror of 1 : 64.
ADD_SETS = [(0.04, 120, 0.07, 100, 0.09, 110, 0), (0.05, 128, 0.05, 128, 0.1, 128, 0), (0.5, 128, 0.5 / 64, 128, 0.5, 128, 0),
            (0.03, 0, 0.02, 255, 0.04, 0, 0), (0.03, 255, 0.02, 0, 0.04, 255, 0), (0.1, 128, 0.1, 128, 0.01, 128, 0),
            (0.04, 100, 0.03, 90, 0.047, 20, 3), (0.5 / 64, 7, 0.5, 200, 0.25, 128, 1)]


def add_model(ps, folded=False):
    """ADD of a 256 x 256 x 1 activation (row index = its code) and a constant (column index = its code): all 65 536 pairs. folded:
    the activation comes out of an identity 1 x 1 convolution (ratio 1, zo = zx: every code reproduced), so the ADD is folded."""
    sa, za, sb, zb, so, zo, act = ps
    m = Model()
    shp = (1, 256, 256, 1)
    x = m.add(T("x", shp, "u8", scale=sa, zp=za))
    a = x
    if folded:
        w = m.add(T("w", (1, 1, 1, 1), "u8", data=[129], scale=1.0, zp=128))
        b = m.add(T("b", (1,), "i32", data=[0], scale=sa, zp=0))
        a = m.add(T("a", shp, "u8", scale=sa, zp=za))
        m.ops.append(Op("CONV_2D", [x, w, b], [a], padding=0, stride_h=1, stride_w=1, act=0))
    c = m.add(T("c", shp, "u8", data=np.tile(np.arange(256, dtype=np.uint8), 256), scale=sb, zp=zb))
    y = m.add(T("y", shp, "u8", scale=so, zp=zo))
    m.ops.append(Op("ADD", [a, c], [y], act=act))
    m.inputs, m.outputs = [x], [y]
    return m


def add_input():
    return np.repeat(np.arange(256, dtype=np.uint8), 256).reshape(1, 256, 256, 1)


def add_exact(ps):
    """reference_ops::Add on all pairs from the integer statement: [256][256] codes."""
    sa, za, sb, zb, so, zo, act = ps
    twice = 2.0 * max(f32(sa), f32(sb))
    (m1, s1), (m2, s2) = quantize_multiplier(f32(sa) / twice), quantize_multiplier(f32(sb) / twice)
    mo, so_ = quantize_multiplier(twice / ((1 << 20) * f32(so)))
    lo, hi = act_range(act, so, zo)
    v1 = [mbqm((a - za) << 20, m1, s1) for a in range(256)]
    v2 = [mbqm((b - zb) << 20, m2, s2) for b in range(256)]
    memo = {}
    out = np.zeros((256, 256), np.uint8)
    for a in range(256):
        for b in range(256):
            s = v1[a] + v2[b]
            if s not in memo:
                memo[s] = min(hi, max(lo, mbqm(s, mo, so_) + zo))
            out[a, b] = memo[s]
    return out


def act_range(act, scale, zp):
    def q(v):
        d = float(np.float32(v) / np.float32(scale))
        return zp + int(math.floor(d + 0.5) if d >= 0 else math.ceil(d - 0.5))
    lo, hi = 0, 255
    if act == 1:
        lo = max(lo, q(0.0))
    elif act == 3:
        lo, hi = max(lo, q(0.0)), min(hi, q(6.0))
    return lo, hi


# unary operators: (input scale, input zp, output scale, output zp): zero points 0 and 255, ratio above and below 1, powers of two
UNARY_SETS = [(0.05, 120, 0.03, 10), (0.05, 0, 0.11, 255), (0.05, 255, 0.02, 0), (0.5, 128, 1.0, 128), (0.5, 100, 4.0, 30),
              (0.25, 128, 0.125, 128), (0.02, 30, 0.02, 30)]
UNARY_CODES = ("RELU", "RELU6", "QUANTIZE", "TANH", "DEQUANTIZE", "CONCATENATION")


def unary_model(code, ps):
    """One element-wise operator on a [1, 16, 16, 1] activation that holds every code once. CONCATENATION: the activation (rescaled to
    the output's quantisation) beside a constant part that already has it."""
    si, zi, so, zo = ps
    m = Model()
    shp = (1, 16, 16, 1)
    x = m.add(T("x", shp, "u8", scale=si, zp=zi))
    if code == "DEQUANTIZE":
        y = m.add(T("y", shp, "f32"))
        m.ops.append(Op(code, [x], [y]))
    elif code == "CONCATENATION":
        c = m.add(T("c", shp, "u8", data=np.arange(256, dtype=np.uint8)[::-1], scale=so, zp=zo))
        y = m.add(T("y", (1, 16, 16, 2), "u8", scale=so, zp=zo))
        m.ops.append(Op(code, [x, c], [y], axis=3))
    else:
        if code == "TANH":
            si, so, zo = si / 8, 1 / 128, 128 if zo not in (0, 255) else zo
            m.tensors[x].scale = si
        y = m.add(T("y", shp, "u8", scale=so, zp=zo))
        m.ops.append(Op(code, [x], [y]))
    m.inputs, m.outputs = [x], [y]
    return m


def unary_exact(code, ps):
    """RELU / RELU6 / QUANTIZE on all 256 codes from the integer statement."""
    si, zi, so, zo = ps
    m, s = quantize_multiplier(f32(si) / f32(so))
    lo, hi = act_range({"RELU": 1, "RELU6": 3, "QUANTIZE": 0}[code], so, zo)
    return np.array([min(hi, max(lo, mbqm(q - zi, m, s) + zo)) for q in range(256)], np.uint8)


def quantize_f32_cases(scale, zo):
    """float32 inputs of QUANTIZE: exact half-integers times the scale (a power of two: the products are exact) of both signs, +-0,
    subnormals, the two clamp edges +- 1/2, and |x / scale| up to 2^24."""
    k = np.arange(-300, 301, dtype=np.float64) + 0.5
    edges = np.array([-zo - 0.5, -zo + 0.5, -zo - 0.49, 255 - zo - 0.5, 255 - zo + 0.5, 255 - zo + 0.49, 255 - zo - 0.51])
    big = np.array([2.0 ** 24, -2.0 ** 24, 2.0 ** 23 + 0.5, -(2.0 ** 23) - 0.5, 2.0 ** 22 + 0.5])
    v = np.concatenate([k, edges, big, np.arange(-40, 41) / 4.0]) * scale
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, -1.1754942e-38], np.float32)
    return np.concatenate([v.astype(np.float32), tiny])


def quantize_f32_model(n, scale, zo):
    m = Model()
    x = m.add(T("x", (1, 1, n, 1), "f32"))
    y = m.add(T("y", (1, 1, n, 1), "u8", scale=scale, zp=zo))
    m.ops.append(Op("QUANTIZE", [x], [y]))
    m.inputs, m.outputs = [x], [y]
    return m


def quantize_f32_exact(x, scale, zo):
    """round-half-away(x / scale) + zo, clamped - in Fractions (scale a power of two: the float32 division is exact)."""
    out = []
    for v in x:
        q = Fraction(float(v)) / Fraction(float(np.float32(scale)))
        if abs(q) < Fraction(1, 4):
            q = Fraction(0)          # (subnormals: far below half a code whatever the division does with them)
        out.append(min(255, max(0, round_half_away(q) + zo)))
    return np.array(out, np.uint8)


# RESIZE_BILINEAR: (H, W, Ho, Wo, align_corners, half_pixel_centers, input)
def resize_cases(rng):
    odd = np.zeros((1, 4, 4, 2), np.uint8)     # neighbours that differ by an odd number: x2 midpoints are v + 1/2 exactly
    odd[0, :, :, 0] = np.array([[10, 11, 14, 19], [13, 20, 21, 28], [200, 255, 254, 1], [0, 255, 0, 255]])
    odd[0, :, :, 1] = odd[0, :, :, 0].T
    ends = rng.choice(np.array([0, 255], np.uint8), (1, 4, 4, 2))
    out = []
    for hp in (False, True):
        out += [(7, 7, 3, 3, False, hp, rng.integers(0, 256, (1, 7, 7, 2), dtype=np.uint8)),
                (1, 1, 4, 4, False, hp, rng.integers(0, 256, (1, 1, 1, 2), dtype=np.uint8)),
                (4, 4, 8, 8, False, hp, ends), (4, 4, 8, 8, False, hp, odd)]
    out += [(5, 4, 1, 7, True, False, rng.integers(0, 256, (1, 5, 4, 2), dtype=np.uint8)), (4, 4, 8, 8, True, False, odd)]
    return out


def resize_model(h, w, ho, wo, align, half_pixel, c=2):
    m = Model()
    x = m.add(T("x", (1, h, w, c), "u8", scale=0.1, zp=3))
    sz = m.add(T("s", (2,), "i32", data=[ho, wo]))
    y = m.add(T("y", (1, ho, wo, c), "u8", scale=0.1, zp=3))
    m.ops.append(Op("RESIZE_BILINEAR", [x, sz], [y], align_corners=align, half_pixel_centers=half_pixel))
    m.inputs, m.outputs = [x], [y]
    return m


# ------------------------------------------------------------------ running a case on the GPU (the -m gpu files)
def oracle_images(model, x):
    """The oracle's value of every tensor, per image of x [n, ...]."""
    import tfl_oracle as O
    return [O.run_model(model, {model.inputs[0]: x[i:i + 1]}) for i in range(len(x))]


def gpu_check(model, x, wants, tune=None, families=None, nbs=(1, 2), blob=None, label="", more=()):
    """One engine on `model` under `tune`: for 1 and 2 images per invoke, every operator of `families` {op: (family, row, grouped,
    folded)} reports exactly that (row None: not compared), and every output equals wants[image][tensor] byte for byte. Returns the
    outputs of the last invoke. more: further (x, wants) batches run on the same engine."""
    import yolact_amd as ya
    from tfl_builder import serialize
    eng = ya.TfliteEngine(blob if blob is not None else bytes(serialize(model)), tune=tune)
    try:
        for nb, x, wants in [(nb, x, wants) for nb in nbs] + [(len(mx), mx, mw) for mx, mw in more]:
            eng.set_batch(nb)
            eng.set_input(np.ascontiguousarray(x[:nb]))
            eng.invoke()
            for op, (fam, row, grouped, folded) in (families or {}).items():
                info = eng.op_info(op)
                got = (info["family"], info["row"] if row is not None else None, info["grouped"], info["folded"])
                assert got == (fam, row, grouped, folded), (label, tune, nb, op, info)
            outs = []
            for k, o in enumerate(model.outputs):
                got = eng.output(k)
                outs.append(got)
                for i in range(nb):
                    want = np.asarray(wants[i][o])
                    assert got.dtype == want.dtype and np.array_equal(got.reshape(nb, -1)[i], want.reshape(-1)), \
                        (label, tune, nb, model.tensors[o].name, i)
        return outs
    finally:
        eng.close()
