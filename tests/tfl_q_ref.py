"""numpy restatement of the executor's pinned meaning of int8 / per-channel TFLite models (DESIGN.md section 11 "TFLite int8"):
TEST INFRASTRUCTURE ONLY. Written from the definitions, operator by operator, not from the kernels; it shares only the fixed-point
primitives (mbqm, quantize_multiplier) with oracle/tfl_oracle.py. The definitions restate TFLite's int8 reference kernels from
memory - no TFLite runtime is available to pin them - and are the project's own contract, like SURVEY Appendix C.

Every function takes and returns arrays of the tensor's own dtype (np.int8 / np.uint8 / np.float32); uint8 tensors follow the same
formulas with the type range [0, 255] (where tests/test_tflite_int8_ref.py proves them equal to tfl_oracle's uint8 functions), except
RESIZE_BILINEAR and CONCATENATION with rescaling, which exist for uint8 only in tfl_oracle and are taken from there.
"""
import math

import numpy as np

import tfl_oracle as O
from tfl_oracle import mbqm, quantize_multiplier

RANGE = {"i8": (-128, 127), "u8": (0, 255)}
O_NP = {"i8": np.int8, "u8": np.uint8}


def f32(s):
    return float(np.float32(s))


def scales_of(t):
    return [f32(s) for s in np.atleast_1d(t.scale)]


def zp_of(t):
    return int(np.atleast_1d(t.zp)[0])


def act_range(act, scale, zp, dtype):
    """The activation-range rule with the type range of `dtype`: act 0 none, 1 RELU, 2 RELU_N1_TO_1, 3 RELU6."""
    def q(v):
        d = float(np.float32(v) / np.float32(scale))
        return zp + int(math.floor(d + 0.5) if d >= 0 else math.ceil(d - 0.5))
    lo, hi = RANGE[dtype]
    if act == 1:
        lo = max(lo, q(0.0))
    elif act == 3:
        lo, hi = max(lo, q(0.0)), min(hi, q(6.0))
    elif act == 2:
        lo, hi = max(lo, q(-1.0)), min(hi, q(1.0))
    return lo, hi


def _conv_out(acc, sx, sws, so, zo, act, dtype):
    """y = clamp(mbqm(acc, M[oc], S[oc]) + zo, lo, hi), (M, S)[oc] = quantize_multiplier(sx * sw[oc] / so); acc [..., Co] int64."""
    co = acc.shape[-1]
    sws = list(sws) * co if len(sws) == 1 else sws
    lo, hi = act_range(act, so, zo, dtype)
    out = np.empty(acc.shape, np.int64)
    for oc in range(co):
        m, s = quantize_multiplier(f32(sx) * f32(sws[oc]) / f32(so))
        out[..., oc] = mbqm(acc[..., oc], m, s) + zo
    return np.clip(out, lo, hi).astype(O_NP[dtype])


def conv_acc(x, zx, w, zw, bias, stride, padding, dil, depth_multiplier=None):
    """acc = sum over the in-bounds taps of (x - zx)(w - zw) + bias[oc]; x [1,H,W,Ci]; w [Co,kh,kw,Ci], or depthwise [1,kh,kw,Ci*dm]
    with output channel oc = ic * dm + m."""
    dw = depth_multiplier is not None
    _, h, ww, ci = x.shape
    kh, kw = w.shape[1], w.shape[2]
    co = w.shape[3] if dw else w.shape[0]
    ho, wo, ph, pw = O._geom(h, ww, kh, kw, stride[0], stride[1], dil[0], dil[1], padding)
    xi, wi = x[0].astype(np.int64) - zx, w.astype(np.int64) - zw
    acc = np.zeros((ho, wo, co), np.int64)
    for oy in range(ho):
        for ox in range(wo):
            for r in range(kh):
                for s in range(kw):
                    iy, ix = oy * stride[0] - ph + r * dil[0], ox * stride[1] - pw + s * dil[1]
                    if 0 <= iy < h and 0 <= ix < ww:
                        acc[oy, ox] += np.repeat(xi[iy, ix], depth_multiplier) * wi[0, r, s] if dw else wi[:, r, s, :] @ xi[iy, ix]
    return acc + (0 if bias is None else bias.astype(np.int64))


def conv(x, tx, w, tw, bias, ty, stride, padding, act, dil=(1, 1), depth_multiplier=None):
    acc = conv_acc(x, zp_of(tx), w, zp_of(tw), bias, stride, padding, dil, depth_multiplier)
    return _conv_out(acc, tx.scale, scales_of(tw), ty.scale, zp_of(ty), act, ty.dtype)[None]


def add(a, ta, b, tb, ty, act):
    """The uint8 arithmetic (left shift 20) on the true integers, clamped to the output type's activation range."""
    twice = 2.0 * max(f32(ta.scale), f32(tb.scale))
    m1, s1 = quantize_multiplier(f32(ta.scale) / twice)
    m2, s2 = quantize_multiplier(f32(tb.scale) / twice)
    mo, so = quantize_multiplier(twice / ((1 << 20) * f32(ty.scale)))
    lo, hi = act_range(act, ty.scale, zp_of(ty), ty.dtype)
    v1 = mbqm((a.astype(np.int64) - zp_of(ta)) * (1 << 20), m1, s1)
    v2 = mbqm((b.astype(np.int64) - zp_of(tb)) * (1 << 20), m2, s2)
    return np.clip(mbqm(v1 + v2, mo, so) + zp_of(ty), lo, hi).astype(O_NP[ty.dtype])


def requant(x, tx, ty, act=0):
    """QUANTIZE between quantised types, RELU (act 1), RELU6 (act 3): clamp(mbqm(x - zi, M, S) + zo, range), (M, S) from si / so."""
    m, s = quantize_multiplier(f32(tx.scale) / f32(ty.scale))
    lo, hi = act_range(act, ty.scale, zp_of(ty), ty.dtype)
    return np.clip(mbqm(x.astype(np.int64) - zp_of(tx), m, s) + zp_of(ty), lo, hi).astype(O_NP[ty.dtype])


def quantize_f32(x, ty):
    v = (x.astype(np.float32) / np.float32(ty.scale)).astype(np.float32)
    r = np.where(v >= 0, np.floor(v + np.float32(0.5)), np.ceil(v - np.float32(0.5)))
    lo, hi = RANGE[ty.dtype]
    return np.clip(r.astype(np.int64) + zp_of(ty), lo, hi).astype(O_NP[ty.dtype])


def dequantize(x, tx):
    return (np.float32(tx.scale) * (x.astype(np.int32) - zp_of(tx)).astype(np.float32)).astype(np.float32)


def tanh(x, tx, ty):
    """The 256-entry table rule, one entry per value q of the input type."""
    inv = np.float32(1.0) / np.float32(ty.scale)
    lo, hi = RANGE[ty.dtype]
    first = RANGE[tx.dtype][0]
    table = np.zeros(256, np.int64)
    for q in range(first, first + 256):
        v = np.float32(tx.scale) * np.float32(q - zp_of(tx))
        r = float(np.float32(np.float32(math.tanh(float(v))) * inv))
        table[q - first] = min(hi, max(lo, int(math.floor(r + 0.5) if r >= 0 else math.ceil(r - 0.5)) + zp_of(ty)))
    return table[x.astype(np.int64) - first].astype(O_NP[ty.dtype])


def _tdiv(a, b):
    """C++ integer division: truncates toward zero."""
    return abs(a) // abs(b) * (1 if (a >= 0) == (b > 0) else -1)


def resize_bilinear_i8(x, ho, wo, align_corners=False, half_pixel=False):
    """TFLite's integer kernel in 10-bit fixed point."""
    _, h, w, c = x.shape

    def step(i, o):
        return _tdiv((1 << 10) * (i - 1) + (o - 1) // 2, o - 1) if align_corners and o > 1 else _tdiv((1 << 10) * i + o // 2, o)

    def pos(o, st, n):
        i = o * st + st // 2 - (1 << 9) if half_pixel else o * st
        p0 = min(max(_tdiv(i, 1 << 10), 0), n - 1)      # (the upper bound: only where the definition would read past the image)
        p1 = min(_tdiv(i + (1 << 10) - 1, 1 << 10), n - 1)
        return p0, p1, i - (1 << 10) * p0

    sh, sw = step(h, ho), step(w, wo)
    out = np.zeros((1, ho, wo, c), np.int8)
    xi = x[0].astype(np.int64)
    for oy in range(ho):
        y0, y1, fy = pos(oy, sh, h)
        for ox in range(wo):
            x0, x1, fx = pos(ox, sw, w)
            for ch in range(c):
                v = int(xi[y0, x0, ch]) * (1024 - fy) * (1024 - fx) + int(xi[y1, x0, ch]) * fy * (1024 - fx) + \
                    int(xi[y0, x1, ch]) * (1024 - fy) * fx + int(xi[y1, x1, ch]) * fy * fx
                out[0, oy, ox, ch] = np.int64(_tdiv(v + ((1 << 19) if v > 0 else -(1 << 19)), 1 << 20)).astype(np.int8)
    return out


class Refused(Exception):
    """The model is one the executor must refuse."""


def run_model(model, inputs):
    """Every tensor's value of a model of tfl_builder_q tensors (or tfl_builder's: uint8 with scalar parameters)."""
    T = model.tensors
    val = {i: t.data for i, t in enumerate(T) if t.data is not None}
    val.update(inputs)
    for op in model.ops:
        ins, outs, o = op.inputs, op.outputs, op.opts
        ty = T[outs[0]]
        if op.code in ("CONV_2D", "DEPTHWISE_CONV_2D"):
            tx, tw = T[ins[0]], T[ins[1]]
            bias = val[ins[2]] if len(ins) > 2 and ins[2] >= 0 else None
            val[outs[0]] = conv(val[ins[0]], tx, val[ins[1]], tw, bias, ty, (o["stride_h"], o["stride_w"]), o["padding"], o.get("act", 0),
                                (o.get("dil_h", 1), o.get("dil_w", 1)), o.get("depth_multiplier", 1) if op.code[0] == "D" else None)
        elif op.code == "ADD":
            val[outs[0]] = add(val[ins[0]], T[ins[0]], val[ins[1]], T[ins[1]], ty, o.get("act", 0))
        elif op.code == "PAD":
            val[outs[0]] = np.pad(val[ins[0]], [(int(a), int(b)) for a, b in val[ins[1]]], constant_values=O_NP[ty.dtype](zp_of(ty)))
        elif op.code == "RESIZE_BILINEAR":
            size = val[ins[1]]
            fn = resize_bilinear_i8 if ty.dtype == "i8" else O.resize_bilinear_u8
            val[outs[0]] = fn(val[ins[0]], int(size[0]), int(size[1]), o.get("align_corners", False), o.get("half_pixel_centers", False))
        elif op.code == "TANH":
            val[outs[0]] = tanh(val[ins[0]], T[ins[0]], ty)
        elif op.code in ("RELU", "RELU6"):
            val[outs[0]] = requant(val[ins[0]], T[ins[0]], ty, 1 if op.code == "RELU" else 3)
        elif op.code == "CONCATENATION":
            axis = o["axis"] if o["axis"] >= 0 else o["axis"] + len(ty.shape)
            if ty.dtype == "u8":
                val[outs[0]] = O.concat_u8([val[i] for i in ins], [(zp_of(T[i]), T[i].scale) for i in ins], zp_of(ty), ty.scale, axis)
            else:
                if ty.dtype == "i8" and any(zp_of(T[i]) != zp_of(ty) or np.float32(T[i].scale) != np.float32(ty.scale) for i in ins):
                    raise Refused("int8 concatenation with another scale or zero point")
                val[outs[0]] = np.concatenate([val[i] for i in ins], axis=axis)
        elif op.code == "RESHAPE":
            val[outs[0]] = val[ins[0]].reshape(ty.shape)
        elif op.code == "QUANTIZE":
            val[outs[0]] = quantize_f32(val[ins[0]], ty) if T[ins[0]].dtype == "f32" else requant(val[ins[0]], T[ins[0]], ty)
        elif op.code == "DEQUANTIZE":
            val[outs[0]] = dequantize(val[ins[0]], T[ins[0]])
        else:
            raise NotImplementedError(op.code)
    return val
