"""The models of the int8 / per-channel tests (tests/test_tflite_int8_ref.py, tests/test_gpu_tflite_int8*.py): builders on
tfl_builder_q, their reference values from tfl_q_ref, and the GPU check they share."""
import numpy as np

import tfl_builder_q as BQ
import tfl_q_ref as R
from tfl_builder_q import Model, Op, T
from tfl_cases import out_geometry
from tfl_models_q import int8_twin, spread_scales   # noqa: F401 (the twins live with the models: tools/ load them without the oracle)

ZXS = (-128, 0, 127)            # the input zero points every convolution case runs with: a padded tap carries that byte


def conv_model(h, w, ci, co, kh, kw, zx=0, zo=0, sx=0.05, sw=None, so=0.08, stride=(1, 1), dil=(1, 1), padding=0, act=0, weights=None,
               bias=None, depthwise=False, dm=1, rng=None, xdtype="i8", wdtype="i8", zw=0):
    """One int8 CONV_2D / DEPTHWISE_CONV_2D; sw: a scalar (one scale) or one per output channel (default: spread_scales)."""
    m = Model()
    x = m.add(T("x", (1, h, w, ci), xdtype, scale=sx, zp=zx))
    if depthwise:
        co = ci * dm
    wshape = (1, kh, kw, co) if depthwise else (co, kh, kw, ci)
    if weights is None:
        weights = rng.integers(-128, 128, wshape) if wdtype == "i8" else rng.integers(0, 256, wshape)
        if wdtype == "i8":
            weights.flat[0], weights.flat[-1] = -128, 127      # both ends of the weight range are legal
    sw = spread_scales(co, rng) if sw is None else sw
    wt = m.add(T("w", wshape, wdtype, data=weights, scale=sw, zp=zw, qdim=3 if depthwise and np.ndim(sw) else 0))
    ins = [x, wt]
    if bias is not None:
        ins.append(m.add(T("b", (co,), "i32", data=np.asarray(bias, np.int32), scale=np.float32(sx) * np.asarray(sw, np.float32), zp=0)))
    ho, wo, _, _ = out_geometry(h, w, kh, kw, stride, dil, padding)
    y = m.add(T("y", (1, ho, wo, co), xdtype, scale=so, zp=zo))
    opts = dict(padding=padding, stride_h=stride[0], stride_w=stride[1], act=act, dil_h=dil[0], dil_w=dil[1])
    if depthwise:
        opts["depth_multiplier"] = dm
    m.ops.append(Op("DEPTHWISE_CONV_2D" if depthwise else "CONV_2D", ins, [y], **opts))
    m.inputs, m.outputs = [x], [y]
    return m


def conv_real(model, x, op=0):
    """The accumulators of convolution `op` on images x [n, ...] as real numbers per channel: acc * sx * sw[oc] (float64)."""
    o = model.ops[op]
    tx, tw = model.tensors[o.inputs[0]], model.tensors[o.inputs[1]]
    bias = model.tensors[o.inputs[2]].data if len(o.inputs) > 2 else None
    acc = np.stack([R.conv_acc(x[i:i + 1], R.zp_of(tx), tw.data, R.zp_of(tw), bias, (o.opts["stride_h"], o.opts["stride_w"]), o.opts["padding"],
                               (o.opts.get("dil_h", 1), o.opts.get("dil_w", 1)), o.opts.get("depth_multiplier", 1) if o.code[0] == "D" else None)
                    for i in range(len(x))])
    sws = np.array(R.scales_of(tw) * (acc.shape[-1] if len(R.scales_of(tw)) == 1 else 1))
    return acc, acc * R.f32(tx.scale) * sws


def fit_output_scale(model, x, op=0, codes=300):
    """Sets the output scale from the reference's own accumulators: the largest |acc sx sw[oc]| lands `codes` codes from the zero
    point - with |zo| < 22 more than twice past both ends of int8, so both clamps are hit when the other sign comes half as far.
    Returns the accumulators."""
    acc, real = conv_real(model, x, op)
    model.tensors[model.ops[op].outputs[0]].scale = float(np.abs(real).max()) / codes
    return acc


def multipliers_matter(model, acc, op=0):
    """On the reference: for every pair of output channels, giving each the other's multiplier changes at least one output byte (so
    a kernel that reads a neighbour's table entry cannot pass). acc: conv_real's accumulators."""
    o = model.ops[op]
    tx, tw, ty = (model.tensors[i] for i in (o.inputs[0], o.inputs[1], o.outputs[0]))
    sws = R.scales_of(tw)
    co = acc.shape[-1]
    own = R._conv_out(acc, tx.scale, sws, ty.scale, R.zp_of(ty), o.opts.get("act", 0), ty.dtype)
    for a in range(co):
        with_others = [R._conv_out(acc[..., a:a + 1], tx.scale, [sws[b]], ty.scale, R.zp_of(ty), o.opts.get("act", 0), ty.dtype) for b in range(co)]
        for b in range(co):
            if b != a and np.array_equal(with_others[b][..., 0], own[..., a]) and np.array_equal(
                    R._conv_out(acc[..., b:b + 1], tx.scale, [sws[a]], ty.scale, R.zp_of(ty), o.opts.get("act", 0), ty.dtype)[..., 0], own[..., b]):
                return False
    return True


def form_model(kh, kw, ci, rng, zx, co=17, stride=(1, 1), n=2, **kw_more):
    """The form cases' layer on n images of 3 x 5 pixels: SAME, Co = 17 (two channel tiles, the second with one live channel; byte
    stores; tables padded), per-channel scales, the output scale fitted. With K in the hundreds every fitted multiplier is far below 1
    (a right shift); so one channel (random, where Co > 1) holds a single weight 1 and a small bias - |acc| <= 275 - and a scale that
    makes its multiplier 2.5: a left shift of 2; and two channels mirror each other (both clamp ends). Returns (model, x, accumulators)."""
    m = conv_model(3, 5, ci, co, kh, kw, zx=zx, zo=int(rng.integers(-21, 22)), stride=stride, bias=rng.integers(-2000, 2000, co), rng=rng, **kw_more)
    x = rng.integers(-128, 128, (n, 3, 5, ci)).astype(np.int8)
    tw, tb = m.tensors[1], m.tensors[2]
    fine = int(rng.integers(3, co - 1)) if co > 4 else None      # (channels 0 and co - 1 hold the weights -128 and 127, 1 and 2 are the pair below)
    if fine is not None:
        tw.data[fine] = 0
        tw.data[fine, kh // 2, kw // 2, int(rng.integers(ci))] = 1
        tb.data[fine] = int(rng.integers(-20, 21))
        # both clamp ends: channels 1 and 2 get the two largest scales and opposite weights and biases, so what one reaches on one
        # side the other reaches on the other
        tw.data[1] = np.clip(tw.data[1], -127, 127)
        tw.data[2], tb.data[2] = -tw.data[1], -tb.data[1]
        sc = np.array(tw.scale, np.float32)
        for ch, rank in ((1, -1), (2, -2)):
            k = int(np.argsort(sc)[rank])
            sc[ch], sc[k] = sc[k], sc[ch]
        tw.scale = sc
    acc = fit_output_scale(m, x)
    if fine is not None:
        tw.scale = np.array(tw.scale, np.float32)
        tw.scale[fine] = np.float32(2.5 * R.f32(m.tensors[3].scale) / R.f32(m.tensors[0].scale))
    return m, x, acc


def group_model(kh, kw, ci, rng, zx):
    """Three independent int8 convolutions of one form on one input - Co 17, 16 and 1, the last with stride 2 - each with its own
    multiplier tables and bias, and three outputs."""
    m = Model()
    x = m.add(T("x", (1, 3, 5, ci), "i8", scale=0.05, zp=zx))
    xv = rng.integers(-128, 128, (2, 3, 5, ci)).astype(np.int8)
    for co, stride in ((17, (1, 1)), (16, (1, 1)), (1, (2, 2))):
        one, _, _ = form_model(kh, kw, ci, rng, zx, co=co, stride=stride)
        fit_output_scale(one, xv)
        ids = [x] + [m.add(t) for t in one.tensors[1:]]
        m.ops.append(Op("CONV_2D", ids[:3], [ids[3]], **one.ops[0].opts))
        m.outputs.append(ids[3])
    m.inputs = [x]
    return m, xv


def unary_model(code, dt_in, dt_out, si, zi, so, zo, n=300):
    m = Model()
    x = m.add(T("x", (1, n), dt_in, scale=None if dt_in == "f32" else si, zp=zi))
    y = m.add(T("y", (1, n), dt_out, scale=None if dt_out == "f32" else so, zp=zo))
    m.ops.append(Op(code, [x], [y]))
    m.inputs, m.outputs = [x], [y]
    return m


def add_model(sa, za, sb, zb, so, zo, act=0, dt="i8", dt_b=None):
    m = Model()
    a = m.add(T("a", (1, 256, 256), dt, scale=sa, zp=za))
    first = R.RANGE[dt_b or dt][0]
    b = m.add(T("b", (1, 256, 256), dt_b or dt, data=np.tile(np.arange(first, first + 256), (256, 1)), scale=sb, zp=zb))
    y = m.add(T("y", (1, 256, 256), dt, scale=so, zp=zo))
    m.ops.append(Op("ADD", [a, b], [y], act=act))
    m.inputs, m.outputs = [a], [y]
    return m


def add_input(dt="i8"):
    first = R.RANGE[dt][0]
    return np.tile(np.arange(first, first + 256)[:, None], (1, 256)).astype(R.O_NP[dt])[None]   # every (a, b) pair of the two ranges


def resize_model(h, w, ho, wo, align, half_pixel, c=2):
    m = Model()
    x = m.add(T("x", (1, h, w, c), "i8", scale=0.1, zp=3))
    sz = m.add(T("s", (2,), "i32", data=[ho, wo]))
    y = m.add(T("y", (1, ho, wo, c), "i8", scale=0.1, zp=3))
    m.ops.append(Op("RESIZE_BILINEAR", [x, sz], [y], align_corners=align, half_pixel_centers=half_pixel))
    m.inputs, m.outputs = [x], [y]
    return m


def reference_images(model, x):
    """tfl_q_ref's value of every tensor, per image of x [n, ...]."""
    return [R.run_model(model, {model.inputs[0]: x[i:i + 1]}) for i in range(len(x))]


def gpu_check(model, x, wants=None, tune=None, families=None, quants=None, nbs=(1, 2), label="", tensors=False):
    """One engine on `model` under `tune`: for 1 and 2 images per invoke, every operator of `families` {op: (family, row, grouped,
    folded)} and of `quants` {op: (signed, per_channel)} reports exactly that (row None: not compared), and every output equals the
    reference byte for byte; tensors: so does every tensor the plan still writes (a folded one says so). Returns the last outputs."""
    import yolact_amd as ya
    wants = reference_images(model, x) if wants is None else wants
    eng = ya.TfliteEngine(BQ.serialize(model), tune=tune)
    try:
        for nb in nbs:
            eng.set_batch(nb)
            eng.set_input(np.ascontiguousarray(x[:nb]))
            eng.invoke()
            for op, (fam, row, grouped, folded) in (families or {}).items():
                info = eng.op_info(op)
                got = (info["family"], info["row"] if row is not None else None, info["grouped"], info["folded"])
                assert got == (fam, row, grouped, folded), (label, tune, nb, op, info)
            for op, want in (quants or {}).items():
                q = eng.op_quant(op)
                assert (q["signed"], q["per_channel"]) == want, (label, tune, nb, op, q)
            outs = []
            for k, o in enumerate(model.outputs):
                got = eng.output(k)
                outs.append(got)
                for i in range(nb):
                    want = np.asarray(wants[i][o])
                    assert got.dtype == want.dtype and np.array_equal(got.reshape(nb, -1)[i], want.reshape(-1)), \
                        (label, tune, nb, model.tensors[o].name, i)
            gone = 0
            for t in sorted({o for op in model.ops for o in op.outputs}) if tensors else ():
                tt = model.tensors[t]
                try:
                    got = eng.tensor(t, tt.shape, BQ.NP_TYPE[tt.dtype])
                except ya.YhError as e:
                    assert e.code == ya.capi.ESTATE and "folded" in str(e), (label, t, tt.name, str(e))
                    gone += 1
                    continue
                for i in range(nb):
                    assert np.array_equal(got.reshape(nb, -1)[i], np.asarray(wants[i][t]).reshape(-1)), (label, tune, nb, tt.name, i)
        return outs
    finally:
        eng.close()


def expected_conv_family(kh, kw, ci, dot):
    """What a small int8 CONV_2D runs on under yh_tuning.tfl_dot: the uint8 rule without the dot-product kernels, which have no
    signed form - under tfl_dot = 1 an int8 convolution runs the px8 kernel while its weights fit LDS, else the scalar kernel."""
    if dot >= 3 and ci % 4 == 0:
        return "conv_i8_direct"
    if dot >= 2 and ci % 64 == 0:
        return "conv_i8_lds"
    return "conv_px8" if dot >= 1 and kh * kw * ci <= 512 else "conv_scalar"


CHAIN_TAILS = ("relu6", "tanh", "tanh_add", "tanh_quant", "add_act", "add_const", "quant_u8")


def chain_model(producer, ci, co, tail, rng):
    """x int8 [1, 5, 6, ci] -> producer -> tail, the tail folded into the producer's launch under tfl_fuse: producer "conv" (3 x 3
    SAME, per-channel), "dw" (3 x 3, co = ci) or "resize" (5 x 6 -> 10 x 12, co = ci); tail RELU6, TANH, TANH -> ADD with a constant,
    TANH -> QUANTIZE to uint8, ADD with an int8 operand
    from an earlier launch (a 1 x 1 convolution of x, first in the file; not behind the resize) or with a constant, QUANTIZE to uint8.
    Returns (model, x [2, ...], producer's operator index, the folded operators)."""
    x = rng.integers(-128, 128, (2, 5, 6, ci)).astype(np.int8)
    m = Model()
    xi = m.add(T("x", (1, 5, 6, ci), "i8", scale=0.05, zp=int(rng.integers(-20, 20))))

    def conv(kh, depthwise=False):
        one = conv_model(5, 6, ci, co, kh, kh, zx=m.tensors[xi].zp, zo=int(rng.integers(-21, 22)), bias=rng.integers(-2000, 2000, co), depthwise=depthwise, rng=rng)
        fit_output_scale(one, x)
        ids = [xi] + [m.add(t) for t in one.tensors[1:]]
        m.ops.append(Op(one.ops[0].code, ids[:3], [ids[3]], **one.ops[0].opts))
        return ids[3]

    other = conv(1) if tail == "add_act" else None
    if other is not None:
        m.tensors[other].name = "other"
    if producer == "resize":
        co = ci
        sz = m.add(T("s", (2,), "i32", data=[10, 12]))
        y = m.add(T("up", (1, 10, 12, ci), "i8", scale=0.05, zp=m.tensors[xi].zp))
        m.ops.append(Op("RESIZE_BILINEAR", [xi, sz], [y], half_pixel_centers=True))
    else:
        y = conv(3, producer == "dw")
    prod = len(m.ops) - 1
    ty = m.tensors[y]
    if tail == "relu6":
        z = m.add(T("z", ty.shape, "i8", scale=6.0 / 200, zp=-100))
        m.ops.append(Op("RELU6", [y], [z]))
    elif tail[:4] == "tanh":
        ty.scale = R.f32(ty.scale) * 300 / 600      # (fitted at 300 codes: now every |value| past a fifth of the largest clamps - indices -128 and 127)
        z = m.add(T("z", ty.shape, "i8", scale=1 / 128, zp=0))
        m.ops.append(Op("TANH", [y], [z]))
        if tail == "tanh_add":       # the chain goes on past the table: its entry must come back as the int8 value
            c = m.add(T("other", ty.shape, "i8", data=rng.integers(-128, 128, ty.shape), scale=0.01, zp=int(rng.integers(-30, 30))))
            z2 = m.add(T("z2", ty.shape, "i8", scale=0.015, zp=int(rng.integers(-30, 30))))
            m.ops.append(Op("ADD", [z, c], [z2], act=0))
            z = z2
        elif tail == "tanh_quant":
            z2 = m.add(T("z2", ty.shape, "u8", scale=1 / 100, zp=131))
            m.ops.append(Op("QUANTIZE", [z], [z2]))
            z = z2
    elif tail in ("add_act", "add_const"):
        if other is None:
            other = m.add(T("other", ty.shape, "i8", data=rng.integers(-128, 128, ty.shape), scale=0.07, zp=int(rng.integers(-30, 30))))
        z = m.add(T("z", ty.shape, "i8", scale=0.12, zp=int(rng.integers(-30, 30))))
        m.ops.append(Op("ADD", [other, y] if rng.integers(2) else [y, other], [z], act=int(rng.choice([0, 1, 3]))))
    else:
        z = m.add(T("z", ty.shape, "u8", scale=R.f32(ty.scale) * 1.5, zp=120))
        m.ops.append(Op("QUANTIZE", [y], [z]))
    m.inputs, m.outputs = [xi], [z]
    return m, x, prod, list(range(prod + 1, len(m.ops)))


def u8_quantize_i8_model(ci, co, rng):
    """uint8 convolution -> QUANTIZE to int8 -> int8 convolution (per-channel): a type change in the middle of a graph."""
    import tfl_cases as K
    x = rng.integers(0, 256, (2, 5, 6, ci), dtype=np.uint8)
    first = K.conv_model(5, 6, ci, co, 3, 3, x_zp=131, w_zp=120, y_zp=128, bias=rng.integers(-2000, 2000, co), rng=rng)
    K.fit_output_scale(first, K.conv_acc(first, x[:1])[0])
    m = Model()
    for t in first.tensors:
        m.add(T(t.name, t.shape, t.dtype, data=t.data, scale=t.scale, zp=t.zp))
    m.ops.append(Op("CONV_2D", [0, 1, 2], [3], **first.ops[0].opts))
    q = m.add(T("q", m.tensors[3].shape, "i8", scale=R.f32(m.tensors[3].scale) * 0.75, zp=-5))
    m.ops.append(Op("QUANTIZE", [3], [q]))
    mid = np.stack([R.run_model(m, {0: x[i:i + 1]})[q][0] for i in range(2)])
    second = conv_model(5, 6, co, 5, 3, 3, zx=-5, zo=7, sx=m.tensors[q].scale, bias=rng.integers(-2000, 2000, 5), rng=rng)
    fit_output_scale(second, mid)
    ids = [q] + [m.add(t) for t in second.tensors[1:]]
    m.ops.append(Op("CONV_2D", ids[:3], [ids[3]], **second.ops[0].opts))
    m.inputs, m.outputs = [0], [ids[3]]
    return m, x
