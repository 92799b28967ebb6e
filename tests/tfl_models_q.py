"""int8 / per-channel twins of the uint8 models of tests/tfl_models.py, as today's converter would write them (int8_twin), and the
twin of the full-size MobileNetV2-FPN-YOLACT stand-in that tools/time_tflite.py --int8 times. No oracle is imported here: tools/
load this module."""
import numpy as np

import tfl_models as M
from tfl_builder_q import Model, Op, T


def spread_scales(co, rng, base=0.01):
    """One weight scale per channel, a factor 16 apart end to end and in random order: no two channels share a multiplier, and
    with the output scale fitted to the largest (fit_output_scale) the smallest still spans a few dozen codes."""
    return (base * 2.0 ** (rng.permutation(co) * (4.0 / max(co - 1, 1)) - 2.0)).astype(np.float32)


def int8_twin(u8_model, rng, dequant_output=0, quant_output=4):
    """The int8 / per-channel twin of a uint8 model of tests/tfl_models.py, as today's converter would write it: a uint8 graph input
    behind a QUANTIZE, every activation int8 (same scale, zero point - 128), convolution weights int8 with zero point 0 and one scale
    per output channel, other uint8 constants as int8, output `quant_output` behind a QUANTIZE to uint8 and output `dequant_output`
    behind a DEQUANTIZE. Tensors that TFLite's int8 kernels want equally quantised (RESIZE_BILINEAR, PAD, RESHAPE: input and output;
    CONCATENATION: every input and the output) are given one record. Operator k of the uint8 model is operator k + 1 of the twin."""
    src = u8_model
    weights = {op.inputs[1]: op.code for op in src.ops if op.code in ("CONV_2D", "DEPTHWISE_CONV_2D")}
    m = Model()
    for i, t in enumerate(src.tensors):
        if t.dtype != "u8":
            m.add(T(t.name, t.shape, t.dtype, data=t.data, scale=t.scale, zp=t.zp))
        elif i in weights:
            co = t.shape[3] if weights[i][0] == "D" else t.shape[0]
            m.add(T(t.name, t.shape, "i8", data=(t.data.astype(np.int16) - 128).astype(np.int8), scale=spread_scales(co, rng, t.scale) if co > 1 else t.scale,
                    zp=0, qdim=3 if weights[i][0] == "D" and co > 1 else 0))
        else:
            m.add(T(t.name, t.shape, "i8", data=None if t.data is None else (t.data ^ 0x80).view(np.int8), scale=t.scale, zp=t.zp - 128))
    same = list(range(len(m.tensors)))

    def find(a):
        while same[a] != a:
            a = same[a]
        return a
    for op in src.ops:
        tied = op.inputs[:1] + op.outputs if op.code in ("RESIZE_BILINEAR", "PAD", "RESHAPE") else (op.inputs + op.outputs if op.code == "CONCATENATION" else [])
        for t in tied[1:]:
            same[find(t)] = find(tied[0])
    for i, t in enumerate(m.tensors):
        if t.dtype == "i8" and find(i) != i:
            t.scale, t.zp = m.tensors[find(i)].scale, m.tensors[find(i)].zp
    tin = src.tensors[src.inputs[0]]
    xin = m.add(T("input_u8", tin.shape, "u8", scale=tin.scale, zp=tin.zp))
    m.ops.append(Op("QUANTIZE", [xin], [src.inputs[0]]))
    m.ops += [Op(op.code, list(op.inputs), list(op.outputs), **op.opts) for op in src.ops]
    m.inputs, m.outputs = [xin], list(src.outputs)
    if quant_output is not None and quant_output < len(m.outputs):
        t = m.tensors[m.outputs[quant_output]]
        y = m.add(T(t.name + "_u8", t.shape, "u8", scale=t.scale, zp=int(np.atleast_1d(t.zp)[0]) + 128))
        m.ops.append(Op("QUANTIZE", [m.outputs[quant_output]], [y]))
        m.outputs[quant_output] = y
    if dequant_output is not None:
        t = m.tensors[m.outputs[dequant_output]]
        y = m.add(T(t.name + "_f32", t.shape, "f32"))
        m.ops.append(Op("DEQUANTIZE", [m.outputs[dequant_output]], [y]))
        m.outputs[dequant_output] = y
    return m


def mixed_twin(u8_model, rng, keep=0.4):
    """A twin with uint8 AND int8 regions joined by QUANTIZE: every operator stays uint8 with probability `keep` (a RESHAPE takes
    its input's type), else it is int8_twin's; where an operator reads an activation of the other type a QUANTIZE with the same
    scale and the zero point 128 apart is put in front of it (once per tensor: the conversion is exact), and a constant is stored
    in the type of each reader. The graph input is uint8, an output has the type of its producer. Tensors tied by int8_twin keep
    their one record in both types."""
    src = u8_model
    full = int8_twin(src, rng, dequant_output=None, quant_output=None)       # (tensor i of src is tensor i of full)
    weights = {op.inputs[1] for op in src.ops if op.code in ("CONV_2D", "DEPTHWISE_CONV_2D")}
    m, ver, made = Model(), {}, {src.inputs[0]: "u8"}

    def version(i, ty):
        t, f = src.tensors[i], full.tensors[i]
        if t.dtype != "u8":
            return T(t.name, t.shape, t.dtype, data=t.data, scale=t.scale, zp=t.zp)
        if ty == "i8":
            return T(f.name, f.shape, "i8", data=f.data, scale=f.scale, zp=f.zp, qdim=f.qdim)
        if i in weights:
            return T(t.name, t.shape, "u8", data=t.data, scale=t.scale, zp=t.zp)
        return T(t.name + "_u8", t.shape, "u8", data=t.data, scale=f.scale, zp=int(np.atleast_1d(f.zp)[0]) + 128)

    def get(i, ty):
        if i < 0:
            return i
        t = src.tensors[i]
        key = (i, ty if t.dtype == "u8" else None)
        if key not in ver:
            ver[key] = m.add(version(i, ty))
            if t.dtype == "u8" and t.data is None and made[i] != ty:          # an activation of the other type: convert it here
                m.ops.append(Op("QUANTIZE", [get(i, made[i])], [ver[key]]))
        return ver[key]

    for op in src.ops:
        ty = "u8" if rng.random() < keep else "i8"
        if op.code == "RESHAPE":
            ty = made.get(op.inputs[0], "i8")
        ins = [get(i, ty) for i in op.inputs]
        for o in op.outputs:
            made[o] = ty
        m.ops.append(Op(op.code, ins, [get(o, ty) for o in op.outputs], **op.opts))
    m.inputs, m.outputs = [get(src.inputs[0], "u8")], [get(o, made[o]) for o in src.outputs]
    return m


def mobilenetv2_yolact_q(rng, **kw):
    """tfl_models.mobilenetv2_yolact as int8: a uint8 input behind a QUANTIZE, output 4 behind a QUANTIZE to uint8."""
    return int8_twin(M.mobilenetv2_yolact(rng, **kw), rng, dequant_output=None, quant_output=4)


def reader_models():
    """Two small per-channel models for the reader: a CONV_2D (scales along dimension 0) and a DEPTHWISE_CONV_2D (dimension 3), each
    with a per-channel bias. What tests/test_tflite_int8_ref.py validates and what tools/tfl_reader_models.py writes out for the
    stand-alone sanitizer program (tools/tfl_reader_check.cpp)."""
    rng = np.random.default_rng(11)
    out = []
    for dw in (False, True):
        m, co = Model(), 8 if dw else 6
        wshape = (1, 3, 3, 8) if dw else (6, 3, 3, 8)
        sw = spread_scales(co, rng)
        x = m.add(T("x", (1, 4, 4, 8), "i8", scale=0.05, zp=-3))
        w = m.add(T("w", wshape, "i8", data=rng.integers(-128, 128, wshape), scale=sw, zp=0, qdim=3 if dw else 0))
        b = m.add(T("b", (co,), "i32", data=rng.integers(-50, 50, co), scale=np.float32(0.05) * sw, zp=0))
        y = m.add(T("y", (1, 4, 4, co), "i8", scale=0.9, zp=4))
        opts = dict(padding=0, stride_h=1, stride_w=1, act=0, dil_h=1, dil_w=1)
        if dw:
            opts["depth_multiplier"] = 1
        m.ops.append(Op("DEPTHWISE_CONV_2D" if dw else "CONV_2D", [x, w, b], [y], **opts))
        m.inputs, m.outputs = [x], [y]
        out.append(m)
    return out
