"""The value-level reference of the TFLite operator set: what an operator MEANS in real numbers - TEST INFRASTRUCTURE ONLY.

    output code  ~  round(real result / output scale) + output zero point, clamped to the activation's range

The two restatements (the uint8 oracle under oracle/, the int8 / per-channel reference under tests/) and the executor's kernels are compared bit for bit with each other;
this module is what all three are compared with. It is written from the operators' published definitions only and imports none of
them: from the test models it takes the data classes (tfl_builder.Model / tfl_builder_q.Model: tensors with shape, dtype, data,
scale, zp; operators with code, inputs, outputs, opts) and nothing else. Convolutions are torch-CPU float64 conv2d with explicit
asymmetric F.pad, groups = Ci for depthwise, and dilation; everything else is numpy float64.

real(model, op, vals) gives, per output element of operator `op` on the input arrays vals {tensor index: array [n, ...]} (constants
are taken from the model), a Real:

    t        the exact result in output-code units BEFORE the zero point (float64)
    delta    the half-width of the band around a rounding boundary inside which the fixed-point or float32 route may legitimately
             land one code away (float64, broadcast against t)
    zo       the output zero point
    lo, hi   the activation clamp in codes: the real bounds 0, 6, +-1 as codes, inside the type's range

and the one rule every comparison uses is check(got, t, delta, zo, lo, hi), with u = t + zo:

    off a boundary (u further than delta from the nearest half-integer):   got == clamp(nearest integer to u)
    inside the band:                                                        got is clamp(floor u) or clamp(ceil u)

It returns the share of elements inside the band. Exact ties lie inside the band on purpose: the tie rules are pinned bit for bit
by tests/test_gpu_tflite_quant.py and tests/test_tflite_int8_ref.py. DEQUANTIZE's result is float32 and comes back as a RealF32
(real, bound): |got - real| <= bound.

Scales are float32 in the file; every formula starts from that float32 value promoted to float64.

delta, derived (never tuned)
----------------------------
Fixed-point requantisation (CONV_2D, DEPTHWISE_CONV_2D, QUANTIZE between quantised types, RELU, RELU6; per channel where the
weights are). The route computes x M 2^(shift - 31) with the ratio = M 2^(shift - 31), (M, shift) from frexp of the ratio, M rounded
to 31 bits; r = max(0, -shift) is the right shift.

    delta = (2^-(r + 1) if r > 0 else 0)  +  |t| 2^-30  +  1e-9

  1. the rounding before the shift: the high multiplication rounds x M / 2^31 to an integer that is still 2^r times the output
     code, an error of at most 1/2 there = 2^-(r + 1) codes; then the shift rounds again. The second rounding can fall on the other
     side only where the exact value is that close to its boundary. With r = 0 there is one rounding and no such term.
  2. the mantissa: M = round(q 2^31) with q in [1/2, 1) is off by at most 1/2 in 2^30, a relative error of 2^-31; 2^-30 covers it
     and the float64 product that forms the ratio.
  3. float64 slack of this module's own evaluation of t.

ADD. Both inputs are brought to the scale 2 max(sa, sb) / 2^20 by a requantisation each, summed, and the sum requantised with the
ratio 2 max(sa, sb) / (2^20 so). One unit of the intermediate scale is that ratio in output codes. The input with the larger scale
has the ratio 1/2 exactly: no error. The other has a right shift r >= 1: 1/2 unit from the shift, 2^-(r + 1) <= 1/4 from the
rounding before it, and |v| 2^-31 <= 2^27 2^-31 = 1/16 from its mantissa: below one unit together. So

    delta = 2 max(sa, sb) / (2^20 so)  +  the requantisation term above for the ratio 2 max(sa, sb) / (2^20 so)

Float32 routes: (number of float32 roundings) x 2^-24 x (the magnitude each rounding acts on), + 1e-9.
  QUANTIZE from float32: v = x / scale (1), v + 0.5 before the floor (1), on |t| + 1:                 2 x 2^-24 x (|t| + 1)
  DEQUANTIZE (RealF32): scale x (q - zp), the difference exact (1), on |real|:                          1 x 2^-24 x |real|
  TANH table: x = si (q - zi) (1; tanh' <= 1 and |x| tanh'(x) < 1/2, so at most 1/2 2^-24 of the full scale), y = float32(tanh x) (1,
    and up to 3 more for the tanh routine's own error), 1 / so (1), y x that (1), + 0.5 before the floor (1), each on at most the
    full scale 1 / so codes:                                                                            8 x 2^-24 x (1 / so + 1)
  CONCATENATION with rescaling (uint8 only): 1 / so (1), s x that (1), the offset -z sc (1), x sc (1), their sum (1), + 0.5 (1), one to
    spare for a fused multiply-add done either way, each on at most 255 s / so + 1 codes:              7 x 2^-24 x (255 s / so + 1)
  uint8 RESIZE_BILINEAR: per axis the position takes 3 roundings (the step in / out; (o + 0.5) x step; - 0.5), each at most 2^-24 of
    the extent, and a position error e moves the value by at most 255 e: 6 roundings on 255 max(H, W); the value takes 10 more (1 - f
    per axis: 2; two products per corner weight and one with the pixel, the worst corner counted: 4; three sums: 3; + 0.5: 1) on at
    most 255:                                                                          2^-24 x (6 x 255 max(H, W) + 10 x 255)

int8 RESIZE_BILINEAR is TFLite's 10-bit integer kernel: its positions are rounded to 1 / 1024, so in general it lies MORE than one
code from the real interpolation. This module covers only sizes whose steps are exact in 10 bits - 1024 H / Ho an integer (even,
with half_pixel_centers, where the kernel halves it), or for align_corners 1024 (H - 1) / (Ho - 1) an integer - and raises
ValueError for any other. At such sizes the integer kernel evaluates the exact interpolation and only the final rounding is left:
delta = 1e-9. Every other size stays with the bit-exact restatement tests (tests/test_tflite_int8_ref.py, test_gpu_tflite_int8.py).

PAD (fills with the code of real 0: the zero point), RESHAPE, and CONCATENATION of parts that share the output's scale and zero
point: equality, expressed as t = the expected code - zo (an integer) with delta = 1e-9.
"""
import math

import numpy as np

RANGE = {"u8": (0, 255), "i8": (-128, 127)}
CAP = 0.05          # the largest share of a case's elements that may lie inside the band
_SLACK = 1e-9
_U = 2.0 ** -24     # one float32 rounding, relative


# ------------------------------------------------------------------ the rule
def judge(got, t, delta, zo, lo, hi):
    """(share inside the band, elements wrong OFF the band, elements wrong INSIDE it) of got against u = t + zo."""
    got = np.asarray(got).astype(np.int64)
    u = np.asarray(t, np.float64) + zo
    assert got.shape == u.shape, (got.shape, u.shape)
    delta = np.broadcast_to(np.asarray(delta, np.float64), u.shape)
    fl = np.floor(u)
    inband = np.abs(u - fl - 0.5) <= delta
    near = np.clip(np.floor(u + 0.5), lo, hi).astype(np.int64)
    down, up = np.clip(fl, lo, hi).astype(np.int64), np.clip(np.ceil(u), lo, hi).astype(np.int64)
    bad_off = ~inband & (got != near)
    bad_in = inband & (got != down) & (got != up)
    return float(inband.mean()), int(bad_off.sum()), int(bad_in.sum())


def check(got, t, delta, zo, lo, hi, label=""):
    """The rule of the module's docstring; returns the share of elements inside the band."""
    share, bad_off, bad_in = judge(got, t, delta, zo, lo, hi)
    if bad_off or bad_in:
        g = np.asarray(got).astype(np.int64)
        u = np.asarray(t, np.float64) + zo
        near = np.clip(np.floor(u + 0.5), lo, hi)
        k = np.flatnonzero((g != near).reshape(-1))[:8]
        raise AssertionError("%s: %d elements off the band and %d inside it differ from the real result; first (index, got, u): %s" %
                             (label, bad_off, bad_in, [(int(i), int(g.reshape(-1)[i]), float(u.reshape(-1)[i])) for i in k]))
    return share


class Real:
    kind = "q"

    def __init__(self, t, delta, zo, lo, hi):
        self.t, self.delta, self.zo, self.lo, self.hi = np.asarray(t, np.float64), delta, int(zo), int(lo), int(hi)

    def judge(self, got):
        return judge(np.asarray(got).reshape(self.t.shape), self.t, self.delta, self.zo, self.lo, self.hi)

    def check(self, got, label=""):
        return check(np.asarray(got).reshape(self.t.shape), self.t, self.delta, self.zo, self.lo, self.hi, label)


class RealF32:
    kind = "f32"

    def __init__(self, value, bound):
        self.value, self.bound = np.asarray(value, np.float64), np.asarray(bound, np.float64)

    def judge(self, got):
        bad = np.abs(np.asarray(got, np.float64).reshape(self.value.shape) - self.value) > self.bound
        return 0.0, int(bad.sum()), 0

    def check(self, got, label=""):
        assert np.asarray(got).dtype == np.float32, (label, np.asarray(got).dtype)
        _, bad, _ = self.judge(got)
        assert bad == 0, "%s: %d float32 elements further from the real value than the bound" % (label, bad)
        return 0.0


# ------------------------------------------------------------------ tensors' parameters
def f32(s):
    return float(np.float32(s))


def scales_of(t):
    return np.array([f32(s) for s in np.atleast_1d(t.scale)], np.float64)


def scale_of(t):
    s = scales_of(t)
    assert len(s) == 1, t.name
    return float(s[0])


def zp_of(t):
    return int(np.atleast_1d(t.zp)[0])


def right_shift(ratio):
    """r = max(0, -shift), (M, shift) from frexp of the ratio (a mantissa that rounds up to 1 moves the shift by one)."""
    q, e = math.frexp(float(ratio))
    if math.floor(q * 2.0 ** 31 + 0.5) == 2.0 ** 31:
        e += 1
    return max(0, -e)


def requant_delta(t, ratios):
    """The fixed-point term; ratios: a scalar or one per channel (the last axis of t)."""
    r = np.array([right_shift(v) for v in np.atleast_1d(ratios)], np.float64)
    first = np.where(r > 0, 2.0 ** -(r + 1), 0.0)
    return (first if first.size > 1 else float(first[0])) + np.abs(t) * 2.0 ** -30 + _SLACK


def act_bounds(act, so, zo, dtype):
    """The clamp in codes: act 0 none, 1 RELU [0, inf), 2 RELU_N1_TO_1 [-1, 1], 3 RELU6 [0, 6], inside the type's range."""
    def q(v):
        c = v / so
        n = math.floor(abs(c) + 0.5)
        if abs(abs(c) - math.floor(abs(c)) - 0.5) < 1e-4:
            raise ValueError("the bound %g lies on a rounding boundary of the scale %r: choose another scale" % (v, so))
        return zo + (n if c >= 0 else -n)
    lo, hi = RANGE[dtype]
    if act == 1:
        lo = max(lo, q(0.0))
    elif act == 2:
        lo, hi = max(lo, q(-1.0)), min(hi, q(1.0))
    elif act == 3:
        lo, hi = max(lo, q(0.0)), min(hi, q(6.0))
    elif act != 0:
        raise ValueError("activation %r" % (act,))
    return lo, hi


# ------------------------------------------------------------------ operators
def same_padding(n, k, stride, dil):
    """SAME: out = ceil(n / stride); the total padding is split with the ODD pixel behind (bottom / right)."""
    out = -(-n // stride)
    total = max((out - 1) * stride + (k - 1) * dil + 1 - n, 0)
    return out, total // 2, total - total // 2


def conv_real(x, zx, w, zw, bias, stride, dil, padding, depth_multiplier=None):
    """The integer accumulators as exact float64: x [n, H, W, Ci]; w OHWI [Co, kh, kw, Ci], or depthwise [1, kh, kw, Ci * dm] with
    output channel ic * dm + m (torch's grouped convolution with groups = Ci orders its outputs the same way). -> [n, Ho, Wo, Co]."""
    import torch
    import torch.nn.functional as F
    xs = torch.from_numpy(np.ascontiguousarray(x.astype(np.float64) - zx)).permute(0, 3, 1, 2)
    ci = xs.shape[1]
    wz = w.astype(np.float64) - np.asarray(zw, np.float64)
    if depth_multiplier is None:
        ws, groups = torch.from_numpy(np.ascontiguousarray(wz)).permute(0, 3, 1, 2), 1                  # OHWI -> OIHW
    else:
        assert w.shape[0] == 1 and w.shape[3] == ci * depth_multiplier, (w.shape, ci, depth_multiplier)
        ws, groups = torch.from_numpy(np.ascontiguousarray(wz)).permute(3, 0, 1, 2), ci                 # [Ci dm, 1, kh, kw]
    kh, kw = int(ws.shape[2]), int(ws.shape[3])
    if padding == 0:      # SAME
        _, pt, pb = same_padding(xs.shape[2], kh, stride[0], dil[0])
        _, pl, pr = same_padding(xs.shape[3], kw, stride[1], dil[1])
        xs = F.pad(xs, (pl, pr, pt, pb))                                                               # zeros: x - zx of a padded tap
    y = F.conv2d(xs.contiguous(), ws.contiguous(), None, stride=tuple(stride), dilation=tuple(dil), groups=groups)
    acc = y.permute(0, 2, 3, 1).numpy()
    return acc if bias is None else acc + np.asarray(bias, np.float64)


def _positions(n, no, align, half_pixel):
    o = np.arange(no, dtype=np.float64)
    if align and no > 1:
        p = o * ((n - 1) / (no - 1))
    elif half_pixel:
        p = (o + 0.5) * (n / no) - 0.5
    else:
        p = o * (n / no)
    p = np.clip(p, 0.0, n - 1.0)          # a position outside the image reads its edge pixel
    i0 = np.floor(p).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), p - i0


def resize_real(x, ho, wo, align, half_pixel):
    """Bilinear interpolation of x [n, H, W, C] (float64) at the published positions."""
    _, h, w, _ = x.shape
    y0, y1, fy = _positions(h, ho, align, half_pixel)
    x0, x1, fx = _positions(w, wo, align, half_pixel)
    xf = x.astype(np.float64)
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    top = xf[:, y0][:, :, x0] * (1 - fx) + xf[:, y0][:, :, x1] * fx
    bot = xf[:, y1][:, :, x0] * (1 - fx) + xf[:, y1][:, :, x1] * fx
    return top * (1 - fy) + bot * fy


def dyadic_resize(n, no, align, half_pixel):
    """The 10-bit step of the int8 kernel is exact."""
    num, den = (1024 * (n - 1), no - 1) if (align and no > 1) else (1024 * n, no)
    return num % den == 0 and not (half_pixel and not align and (num // den) % 2)


def _arr(model, vals, i):
    if i in vals:
        return np.asarray(vals[i])
    d = model.tensors[i].data
    assert d is not None, "operator input %d (%s) was not given" % (i, model.tensors[i].name)
    return d


def real(model, op, vals):
    """The Real (RealF32 for DEQUANTIZE) of operator `op` (an index) of `model` on vals {tensor index: array [n, ...]}."""
    o = model.ops[op]
    T = model.tensors
    ins, opts = o.inputs, o.opts
    ty = T[o.outputs[0]]
    code = o.code
    x = _arr(model, vals, ins[0])
    n = x.shape[0] if T[ins[0]].data is None else 1
    if code == "DEQUANTIZE":
        v = scale_of(T[ins[0]]) * (x.astype(np.float64) - zp_of(T[ins[0]]))
        return RealF32(v, 1 * _U * np.abs(v) + 1e-30)
    so, zo = scale_of(ty), zp_of(ty)
    lo, hi = RANGE[ty.dtype]
    if code in ("CONV_2D", "DEPTHWISE_CONV_2D"):
        tx, tw = T[ins[0]], T[ins[1]]
        bias = _arr(model, vals, ins[2]) if len(ins) > 2 and ins[2] >= 0 else None
        dm = opts.get("depth_multiplier", 1) if code[0] == "D" else None
        zw = np.atleast_1d(tw.zp)
        assert len(zw) == 1 or not zw.any()
        acc = conv_real(x, zp_of(tx), _arr(model, vals, ins[1]), int(zw[0]), bias, (opts["stride_h"], opts["stride_w"]),
                        (opts.get("dil_h", 1), opts.get("dil_w", 1)), opts["padding"], dm)
        sw = scales_of(tw)
        assert len(sw) in (1, acc.shape[-1]), (len(sw), acc.shape)
        ratios = scale_of(tx) * sw / so               # the real value of one accumulator unit of channel oc, in output codes
        t = acc * ratios
        lo, hi = act_bounds(opts.get("act", 0), so, zo, ty.dtype)
        return Real(t, requant_delta(t, ratios), zo, lo, hi)
    if code == "ADD":
        ta, tb = T[ins[0]], T[ins[1]]
        a, b = x.astype(np.float64), _arr(model, vals, ins[1]).astype(np.float64)
        sa, sb = scale_of(ta), scale_of(tb)
        t = ((a - zp_of(ta)) * sa + (b - zp_of(tb)) * sb) / so
        unit = 2.0 * max(sa, sb) / (2.0 ** 20 * so)
        lo, hi = act_bounds(opts.get("act", 0), so, zo, ty.dtype)
        return Real(t, unit + requant_delta(t, unit), zo, lo, hi)
    if code in ("RELU", "RELU6") or (code == "QUANTIZE" and T[ins[0]].dtype != "f32"):
        si = scale_of(T[ins[0]])
        t = (x.astype(np.float64) - zp_of(T[ins[0]])) * (si / so)
        lo, hi = act_bounds({"RELU": 1, "RELU6": 3, "QUANTIZE": 0}[code], so, zo, ty.dtype)
        return Real(t, requant_delta(t, si / so), zo, lo, hi)
    if code == "QUANTIZE":
        assert x.dtype == np.float32
        t = x.astype(np.float64) / so
        return Real(t, 2 * _U * (np.abs(t) + 1) + _SLACK, zo, lo, hi)
    if code == "TANH":
        t = np.tanh((x.astype(np.float64) - zp_of(T[ins[0]])) * scale_of(T[ins[0]])) / so
        return Real(t, 8 * _U * (1.0 / so + 1) + _SLACK, zo, lo, hi)
    if code == "PAD":
        pads = [(int(p), int(q)) for p, q in _arr(model, vals, ins[1])]
        assert pads[0] == (0, 0)
        want = np.pad(x.astype(np.int64), pads, constant_values=zo)          # real 0 as a code
        return Real(want - zo, _SLACK, zo, lo, hi)
    if code == "RESHAPE":
        return Real(x.astype(np.int64).reshape((n,) + tuple(ty.shape[1:])) - zo, _SLACK, zo, lo, hi)
    if code == "CONCATENATION":
        axis = opts["axis"] if opts["axis"] >= 0 else opts["axis"] + len(ty.shape)
        assert axis > 0
        ts, ds = [], []
        for i in ins:
            v = _arr(model, vals, i).astype(np.float64)
            if T[i].data is not None:
                v = np.broadcast_to(v, (n,) + v.shape[1:])
            s, z = scale_of(T[i]), zp_of(T[i])
            if z == zo and np.float32(s) == np.float32(so):
                ts.append(v - z)
                ds.append(np.full(v.shape, _SLACK))
            else:
                assert ty.dtype == "u8", "int8 concatenation rescales nothing"
                ts.append((v - z) * (s / so))
                ds.append(np.full(v.shape, 7 * _U * (255 * s / so + 1) + _SLACK))
        return Real(np.concatenate(ts, axis), np.concatenate(ds, axis), zo, lo, hi)
    if code == "RESIZE_BILINEAR":
        tx = T[ins[0]]
        assert np.float32(scale_of(tx)) == np.float32(so) and zp_of(tx) == zo, "RESIZE_BILINEAR keeps its input's quantisation"
        size = _arr(model, vals, ins[1])
        hn, wn = int(size[0]), int(size[1])
        align, hp = bool(opts.get("align_corners", False)), bool(opts.get("half_pixel_centers", False))
        _, h, w, _ = x.shape
        t = resize_real(x, hn, wn, align, hp) - zo
        if ty.dtype == "i8":
            if not (dyadic_resize(h, hn, align, hp) and dyadic_resize(w, wn, align, hp)):
                raise ValueError("int8 RESIZE_BILINEAR %dx%d -> %dx%d: the 10-bit steps are not exact; not covered here" % (h, w, hn, wn))
            return Real(t, _SLACK, zo, lo, hi)
        return Real(t, _U * (6 * 255 * max(h, w) + 10 * 255) + _SLACK, zo, lo, hi)
    raise NotImplementedError(code)
