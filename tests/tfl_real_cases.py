"""Cases of the value-level tests (tests/test_tfl_real_ref.py on the CPU, tests/test_gpu_tflite_real.py on the GPU): single-operator
models on tfl_builder_q in the three quantisations "u8", "i8" (one weight scale) and "i8pc" (one per output channel), scaled from
tfl_real_ref's own float64 results so that few outputs lie near a rounding boundary, and the teacher-forced walk over a whole graph.
No restatement is imported here: what a test compares with tfl_real_ref is the test's own business."""
import numpy as np

import tfl_builder_q as BQ
import tfl_real_ref as R
from tfl_builder_q import Model, Op, T

NP = BQ.NP_TYPE
ACT_TYPE = {"u8": "u8", "i8": "i8", "i8pc": "i8"}


def codes(dt, rng, shape):
    lo, hi = R.RANGE[dt]
    return rng.integers(lo, hi + 1, shape).astype(NP[dt])


def all_codes(dt):
    lo, hi = R.RANGE[dt]
    return np.arange(lo, hi + 1).astype(NP[dt])


def spread64(co, rng):
    """One weight scale per channel, a factor 2^6.5 apart end to end, in random order: the right shifts differ between channels."""
    return (0.002 * 2.0 ** (rng.permutation(co) * (6.5 / max(co - 1, 1)))).astype(np.float32)


def conv_case(dt, rng, h=9, w=7, ci=4, co=9, k=(3, 3), stride=(1, 1), dil=(1, 1), padding=0, act=0, bias=True, depthwise=False, dm=1, n=2):
    """One CONV_2D / DEPTHWISE_CONV_2D and n input images. sx in [0.01, 0.1], sw in [0.001, 0.02] (per channel: spread64); the
    output scale puts the largest |real result| over the images 100 codes from the zero point - under RELU6 it is 6 / 64.3 instead
    (the clamp at 64 codes, off a rounding boundary) and the weights' scales take the factor."""
    a = ACT_TYPE[dt]
    kh, kw = k
    if depthwise:
        co = ci * dm
    wshape = (1, kh, kw, co) if depthwise else (co, kh, kw, ci)
    zx = int(rng.integers(1, 255)) + R.RANGE[a][0]
    zw = int(rng.integers(1, 255)) if dt == "u8" else 0
    zo = int(rng.integers(100, 157)) + R.RANGE[a][0] if dt == "u8" else int(rng.integers(-21, 22))
    sx = float(np.float32(rng.uniform(0.01, 0.1)))
    sw = spread64(co, rng) if dt == "i8pc" else np.float32(rng.uniform(0.001, 0.02))
    m = Model()
    xi = m.add(T("x", (1, h, w, ci), a, scale=sx, zp=zx))
    wi = m.add(T("w", wshape, a, data=codes(a, rng, wshape), scale=sw, zp=zw, qdim=3 if depthwise and dt == "i8pc" else 0))
    ins = [xi, wi]
    if bias:
        ins.append(m.add(T("b", (co,), "i32", data=rng.integers(-2000, 2000, co), scale=np.float32(sx) * np.asarray(sw, np.float32), zp=0)))
    x = codes(a, rng, (n, h, w, ci))
    acc = R.conv_real(x, zx, m.tensors[wi].data, zw, m.tensors[ins[2]].data if bias else None, stride, dil, padding, dm if depthwise else None)
    top = float(np.abs(acc * (sx * R.scales_of(m.tensors[wi]))).max())
    if act == 3:
        so = 6.0 / 64.3
        m.tensors[wi].scale = (np.asarray(sw, np.float64) * (100.0 * so / top)).astype(np.float32)
        if np.ndim(sw) == 0:
            m.tensors[wi].scale = np.float32(m.tensors[wi].scale)
    else:
        so = top / 100.0
    if bias:
        m.tensors[ins[2]].scale = np.float32(sx) * np.asarray(m.tensors[wi].scale, np.float32)
    yi = m.add(T("y", (1,) + acc.shape[1:], a, scale=float(np.float32(so)), zp=zo))
    opts = dict(padding=padding, stride_h=stride[0], stride_w=stride[1], act=act, dil_h=dil[0], dil_w=dil[1])
    if depthwise:
        opts["depth_multiplier"] = dm
    m.ops.append(Op("DEPTHWISE_CONV_2D" if depthwise else "CONV_2D", ins, [yi], **opts))
    m.inputs, m.outputs = [xi], [yi]
    return m, x


def conv_right_shifts(model, op=0):
    o = model.ops[op]
    tx, tw, ty = (model.tensors[i] for i in (o.inputs[0], o.inputs[1], o.outputs[0]))
    return [R.right_shift(r) for r in R.scale_of(tx) * R.scales_of(tw) / R.scale_of(ty)]


# two incommensurate (sa, sb, so) per type; zero points per type below
ADD_SCALES = ((0.04, 0.07, 0.09), (0.013, 0.2, 0.21))
ADD_ZPS = {"u8": (120, 100, 110), "i8": (-8, 28, -18)}


def add_case(dt, scales, act=0, n=2):
    """ADD of a [1, 256, 256, 1] activation (row = its code) and a constant (column = its code): all 65 536 pairs; image 1 holds the
    rows in reverse order."""
    (sa, sb, so), (za, zb, zo) = scales, ADD_ZPS[dt]
    m = Model()
    shp = (1, 256, 256, 1)
    a = m.add(T("a", shp, dt, scale=sa, zp=za))
    b = m.add(T("b", shp, dt, data=np.tile(all_codes(dt), 256), scale=sb, zp=zb))
    y = m.add(T("y", shp, dt, scale=so, zp=zo))
    m.ops.append(Op("ADD", [a, b], [y], act=act))
    m.inputs, m.outputs = [a], [y]
    x0 = np.repeat(all_codes(dt), 256).reshape(shp)
    return m, np.concatenate([x0, x0[:, ::-1]])[:n]


# (input scale, input zp offset from the range's start, output scale, output zp offset): ratios 5/3 (a left shift), 0.77 (no shift) and
# 0.03 (a right shift of 6: 2^-6 of all values lie in the band). Ratios in [2^-5, 1/2) have a right shift below 5 and cannot meet the cap.
UNARY_SETS = ((0.05, 120, 0.03, 10), (0.05, 131, 0.065, 117), (0.003, 100, 0.1, 128))


def unary_case(code, dt_in, dt_out, ps, n=2):
    """RELU / RELU6 / QUANTIZE / TANH / DEQUANTIZE on every code of dt_in (image 1: in reverse order); QUANTIZE from float32 on 256
    values of 0.37 .. 150 codes of both signs (so both clamps are met)."""
    si, zi, so, zo = ps
    m = Model()
    shp = (1, 16, 16, 1)
    if dt_in == "f32":
        x = m.add(T("x", shp, "f32"))
        k = np.arange(256, dtype=np.float64) - 127.63
        v = (k * 1.171 * so).astype(np.float32).reshape(shp)
        xs = np.concatenate([v, (v * np.float32(0.731))[:, ::-1]])
    else:
        x = m.add(T("x", shp, dt_in, scale=si, zp=zi + R.RANGE[dt_in][0]))
        v = all_codes(dt_in).reshape(shp)
        xs = np.concatenate([v, v[:, ::-1, ::-1]])
    if dt_out == "f32":
        y = m.add(T("y", shp, "f32"))
    else:
        y = m.add(T("y", shp, dt_out, scale=so, zp=zo + R.RANGE[dt_out][0]))
    m.ops.append(Op(code, [x], [y]))
    m.inputs, m.outputs = [x], [y]
    return m, xs[:n]


def tanh_case(dt, n=2):
    return unary_case("TANH", dt, dt, (0.03, 131, 1.0 / 128, 128), n)


def pad_case(dt, rng, n=2):
    """PAD on all four sides (top 1, bottom 2, left 2, right 1) with a zero point that is not the code 0."""
    z = 77 + R.RANGE[dt][0] + (0 if dt == "u8" else 100)      # u8 77; i8 49
    m = Model()
    x = m.add(T("x", (1, 5, 6, 4), dt, scale=0.1, zp=z))
    p = m.add(T("p", (4, 2), "i32", data=[[0, 0], [1, 2], [2, 1], [0, 0]]))
    y = m.add(T("y", (1, 8, 9, 4), dt, scale=0.1, zp=z))
    m.ops.append(Op("PAD", [x, p], [y]))
    m.inputs, m.outputs = [x], [y]
    return m, codes(dt, rng, (n, 5, 6, 4))


def concat_case(dt, rng, rescale, n=2):
    """CONCATENATION along the channels of the activation, a constant of 6 channels and one of 2; rescale (uint8): the first constant
    carries another scale and zero point."""
    off = R.RANGE[dt][0]
    m = Model()
    x = m.add(T("x", (1, 3, 3, 4), dt, scale=0.05, zp=120 + off))
    c = m.add(T("c", (1, 3, 3, 6), dt, data=codes(dt, rng, (1, 3, 3, 6)), scale=0.08 if rescale else 0.05, zp=(90 if rescale else 120) + off))
    d = m.add(T("d", (1, 3, 3, 2), dt, data=codes(dt, rng, (1, 3, 3, 2)), scale=0.05, zp=120 + off))
    y = m.add(T("y", (1, 3, 3, 12), dt, scale=0.05, zp=120 + off))
    m.ops.append(Op("CONCATENATION", [x, c, d], [y], axis=3))
    m.inputs, m.outputs = [x], [y]
    return m, codes(dt, rng, (n, 3, 3, 4))


def reshape_case(dt, rng, n=2):
    m = Model()
    x = m.add(T("x", (1, 4, 4, 6), dt, scale=0.05, zp=12))
    y = m.add(T("y", (1, 16, 6), dt, scale=0.05, zp=12))
    m.ops.append(Op("RESHAPE", [x], [y], new_shape=[1, 16, 6]))
    m.inputs, m.outputs = [x], [y]
    return m, codes(dt, rng, (n, 4, 4, 6))


# (H, W, Ho, Wo): the uint8 sizes (5 x 7 -> 9 x 13 has the steps 1/2 under align_corners: 5 x 7 -> 7 x 11 is there for that mode's
# rounding), and the sizes whose 10-bit steps are exact (the only ones int8 is covered at)
RESIZE_U8 = ((5, 7, 9, 13), (4, 4, 8, 8), (5, 7, 7, 11))
RESIZE_I8 = {"plain": ((4, 4, 8, 8), (8, 6, 4, 3), (3, 3, 4, 4)), "half_pixel": ((4, 4, 8, 8), (8, 6, 4, 3)), "align": ((5, 5, 9, 9), (3, 5, 5, 9))}
MODES = {"plain": (False, False), "align": (True, False), "half_pixel": (False, True)}


def resize_case(dt, rng, h, w, ho, wo, mode, n=2, c=3):
    """RESIZE_BILINEAR. At a dyadic size (steps exact in 10 bits) every interpolation weight is a multiple of 1/16 or coarser, so
    random codes would put a large share of the outputs on exact ties: there the codes are 16 k + one constant (every output an integer;
    neighbours differ by 16 or more, so a weight wrong by 1/16 moves a code). Elsewhere the codes are random and the rounding takes part."""
    align, hp = MODES[mode]
    lo, hi = R.RANGE[dt]
    m = Model()
    x = m.add(T("x", (1, h, w, c), dt, scale=0.1, zp=3))
    s = m.add(T("s", (2,), "i32", data=[ho, wo]))
    y = m.add(T("y", (1, ho, wo, c), dt, scale=0.1, zp=3))
    m.ops.append(Op("RESIZE_BILINEAR", [x, s], [y], align_corners=align, half_pixel_centers=hp))
    m.inputs, m.outputs = [x], [y]
    if R.dyadic_resize(h, ho, align, hp) and R.dyadic_resize(w, wo, align, hp):
        xs = (lo + 16 * rng.integers(0, 16, (n, h, w, c)) + int(rng.integers(0, 16))).astype(NP[dt])
    else:
        xs = codes(dt, rng, (n, h, w, c))
    return m, xs


# ------------------------------------------------------------------ whole graphs
def tame_right_shifts(model, least=6):
    """Re-scales a graph for the cap: a convolution whose smallest right shift r is below `least` has 2^-r of its outputs in the band
    (2^-4 is over the cap, 2^-5 near it on a small tensor), so its weights' scales are multiplied by 2^-(least - r). The weights
    belong to that operator alone: nothing else in the graph changes but the size of its real result. Returns the operators re-scaled."""
    done = []
    for k, o in enumerate(model.ops):
        if o.code in ("CONV_2D", "DEPTHWISE_CONV_2D"):
            r = min(conv_right_shifts(model, k))
            if r < least:
                tw = model.tensors[o.inputs[1]]
                tw.scale = (np.asarray(tw.scale, np.float32) * np.float32(2.0 ** -(least - r))).astype(np.float32) if np.ndim(tw.scale) else \
                    float(np.float32(tw.scale) * np.float32(2.0 ** -(least - r)))
                done.append(k)
    return done


def exact_ties(real):
    """The share of a Real's elements whose value t + zo is a half-integer exactly (to 1e-9)."""
    u = real.t + real.zo
    return float((np.abs(u - np.floor(u) - 0.5) < 1e-9).mean())


def teacher_forced(model, read, label=""):
    """Every operator of `model` alone: its real result on the arrays read(i) of its OWN input tensors against read(output). read(i):
    tensor i as [n, ...] (constants are taken from the model). One-code differences cannot accumulate this way. Returns
    {operator index: (code, share inside the band)}; every operator is checked and none may exceed the cap.

    One operator of the model family cannot meet the cap as it stands: RESIZE_BILINEAR 4 x 4 -> 8 x 8 takes midpoints (a + b) / 2 of
    neighbouring codes, an exact tie wherever a + b is odd - 10 to 20 % of its outputs on the graph's own activations, whatever the
    seed or the scales (27 % on random codes). There the cap is held to the band WITHOUT the exact ties (nothing but float32 noise is
    left: 0 in practice), each tie must still be floor or ceil, and the share with the ties is what is returned and printed. The
    single-operator resize cases meet the cap as it stands (codes 16 k + c at dyadic sizes)."""
    shares = {}
    for k, op in enumerate(model.ops):
        vals = {i: read(i) for i in op.inputs if i >= 0 and model.tensors[i].data is None}
        got = read(op.outputs[0])
        real = R.real(model, k, vals)
        share = real.check(got, label=(label, k, op.code, model.tensors[op.outputs[0]].name))
        capped = share
        if op.code == "RESIZE_BILINEAR":
            (h, w), (ho, wo) = model.tensors[op.inputs[0]].shape[1:3], model.tensors[op.outputs[0]].shape[1:3]
            mode = (bool(op.opts.get("align_corners", False)), bool(op.opts.get("half_pixel_centers", False)))
            if R.dyadic_resize(h, ho, *mode) and R.dyadic_resize(w, wo, *mode):
                capped = share - exact_ties(real)
        assert capped <= R.CAP, (label, k, op.code, share, capped)
        shares[k] = (op.code, share)
    assert sorted(shares) == list(range(len(model.ops)))
    return shares


def by_kind(shares):
    """{operator code: (operators, largest share)} of teacher_forced's result."""
    out = {}
    for code, s in shares.values():
        c, top = out.get(code, (0, 0.0))
        out[code] = (c + 1, max(top, s))
    return out


def engine_reader(eng, model, nb):
    def read(i):
        t = model.tensors[i]
        return eng.tensor(i, t.shape, NP[t.dtype]).reshape((nb,) + tuple(t.shape[1:]))
    return read


def device_check(model, x, families, tune=None, nbs=(1, 2), label="", max_images=2):
    """One engine on a single-operator `model` under `tune`: for every image count the operator reports the family of `families`
    {op: family} and the device's output tensor passes tfl_real_ref's rule on the input it was given, with at most CAP of the
    elements in the band. Returns the largest share."""
    import yolact_amd as ya
    eng = ya.TfliteEngine(BQ.serialize(model), tune=tune, max_images=max_images)
    top = 0.0
    try:
        for nb in nbs:
            eng.set_batch(nb)
            eng.set_input(np.ascontiguousarray(x[:nb]))
            eng.invoke()
            for op, fam in families.items():
                info = eng.op_info(op)
                assert info["family"] == fam and not info["folded"], (label, tune, nb, op, info)
            read = engine_reader(eng, model, nb)
            for k, op in enumerate(model.ops):
                share = R.real(model, k, {model.inputs[0]: x[:nb]}).check(read(op.outputs[0]), label=(label, tune, nb))
                assert share <= R.CAP, (label, tune, nb, share)
                top = max(top, share)
    finally:
        eng.close()
    return top
