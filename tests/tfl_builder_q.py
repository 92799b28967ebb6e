"""The flatbuffer WRITER of tests/tfl_builder.py for the models today's converter writes: int8 tensors and per-channel
quantisation (a scale vector, a zero-point vector and quantized_dimension in QuantizationParameters: field ids 2, 3 and 6).

It reuses tfl_builder's objects and layout and defines its own tensor class and serialize. A T here takes dtype "i8", `scale` and
`zp` as a scalar or a sequence, and `qdim`; `n_scales` / `n_zps` (tests of the reader only) forge the LENGTH WORD of the scale /
zero-point vector after the file is laid out, leaving its elements as they are.
"""
import struct

import numpy as np

from tfl_builder import BUILTIN, OPTIONS_TYPE, Model, Op, _layout, _options, _Str, _Table, _Vec   # noqa: F401 (Model, Op: re-exported)

TENSOR_TYPE = {"f32": 0, "i32": 2, "u8": 3, "i8": 9}
NP_TYPE = {"f32": np.float32, "i32": np.int32, "u8": np.uint8, "i8": np.int8}


class T:
    def __init__(self, name, shape, dtype="i8", data=None, scale=None, zp=0, qdim=0, n_scales=None, n_zps=None):
        self.name, self.shape, self.dtype, self.qdim = name, tuple(int(s) for s in shape), dtype, int(qdim)
        self.scale, self.zp = scale, zp
        self.n_scales, self.n_zps = n_scales, n_zps
        self.data = None if data is None else np.ascontiguousarray(data, NP_TYPE[dtype]).reshape(self.shape)

    @property
    def scales(self):
        return None if self.scale is None else [float(s) for s in np.atleast_1d(self.scale)]

    @property
    def zps(self):
        return [int(z) for z in np.atleast_1d(self.zp)]

    @property
    def per_channel(self):
        return self.scale is not None and len(self.scales) > 1


def serialize(model, spans=None):
    """spans: a list that receives (first byte, one past the last) of every quantisation table and of its two vectors."""
    codes = sorted({op.code for op in model.ops}, key=lambda c: BUILTIN[c])
    buffers = [_Table({})]   # buffer 0: the empty sentinel
    tensors, forged, quants = [], [], []
    for t in model.tensors:
        bidx = 0
        if t.data is not None:
            buffers.append(_Table({0: ("off", _Vec("B", list(t.data.tobytes()), data_align=16))}))
            bidx = len(buffers) - 1
        q = None
        if t.scale is not None:
            sv, zv = _Vec("f", t.scales), _Vec("q", t.zps, data_align=8)
            if t.n_scales is not None:
                forged.append((sv, t.n_scales))
            if t.n_zps is not None:
                forged.append((zv, t.n_zps))
            q = _Table({2: ("off", sv), 3: ("off", zv), 6: ("i", t.qdim) if t.qdim else None})
            quants += [q, sv, zv]
        tensors.append(_Table({0: ("off", _Vec("i", list(t.shape))), 1: ("b", TENSOR_TYPE[t.dtype]), 2: ("I", bidx),
                               3: ("off", _Str(t.name)), 4: ("off", q) if q else None}))
    ops = []
    for op in model.ops:
        opt = _options(op)
        ops.append(_Table({0: ("I", codes.index(op.code)), 1: ("off", _Vec("i", op.inputs)), 2: ("off", _Vec("i", op.outputs)),
                           3: ("B", OPTIONS_TYPE[op.code]) if opt is not None else None, 4: ("off", opt) if opt is not None else None}))
    sub = _Table({0: ("off", _Vec("off", tensors)), 1: ("off", _Vec("i", model.inputs)), 2: ("off", _Vec("i", model.outputs)),
                  3: ("off", _Vec("off", ops)), 4: ("off", _Str("main"))})
    opcodes = [_Table({0: ("b", min(BUILTIN[c], 127)), 2: ("i", 1), 3: ("i", BUILTIN[c])}) for c in codes]
    root = _Table({0: ("I", 3), 1: ("off", _Vec("off", opcodes)), 2: ("off", _Vec("off", [sub])),
                   3: ("off", _Str("yolact_hip synthetic int8 test model")), 4: ("off", _Vec("off", buffers))})
    order, end = _layout(root)
    buf = bytearray(end)
    for o in order:
        o.emit(buf)
    if spans is not None:
        spans += [(o.pos, o.pos + o.size()) for o in quants]
    for vec, n in forged:
        struct.pack_into("<I", buf, vec.len_pos, n)
    struct.pack_into("<I", buf, 0, root.tpos)
    buf[4:8] = b"TFL3"
    return bytes(buf)
