"""CPU: the pinned meaning of int8 / per-channel TFLite models (tests/tfl_q_ref.py, DESIGN.md section 11 "TFLite int8") and the
reader's side of it (csrc/tflite_model.h through yh_tfl_validate, no GPU).

The restatement is pinned three ways: with single-scale weights every operator but RESIZE_BILINEAR is the uint8 oracle's operator
on the bytes XOR 0x80 (the isomorphism x' = x + 128); a per-channel convolution is, channel by channel, the single-scale one with
that channel's scale; the integer resize has hand-derived answers."""
import numpy as np
import pytest

import tfl_builder as B
import tfl_builder_q as BQ
import tfl_models_q as MQ
import tfl_oracle as O
import tfl_q_cases as Q
import tfl_q_ref as R
from tfl_builder_q import Model, Op, T


def u8_twin(m):
    """Every int8 byte XOR 0x80, every zero point + 128 (int8 weights zp 0 <-> uint8 weights zp 128), as a tfl_builder model."""
    t = B.Model()
    for x in m.tensors:
        if x.dtype == "i8":
            t.add(B.T(x.name, x.shape, "u8", data=None if x.data is None else x.data.view(np.uint8) ^ 0x80, scale=R.scales_of(x)[0], zp=R.zp_of(x) + 128))
        else:
            t.add(B.T(x.name, x.shape, x.dtype, data=x.data, scale=None if x.scale is None else R.scales_of(x)[0], zp=R.zp_of(x)))
    t.ops = [B.Op(op.code, list(op.inputs), list(op.outputs), **op.opts) for op in m.ops]
    t.inputs, t.outputs = list(m.inputs), list(m.outputs)
    return t


def _iso(m, x):
    got = R.run_model(m, {m.inputs[0]: x})[m.outputs[0]]
    xin = x.view(np.uint8) ^ 0x80 if x.dtype == np.int8 else x
    want = O.run_model(u8_twin(m), {m.inputs[0]: xin})[m.outputs[0]]
    if got.dtype == np.int8:
        assert want.dtype == np.uint8 and np.array_equal(got.view(np.uint8) ^ 0x80, want)
    else:
        assert got.dtype == want.dtype and np.array_equal(got, want)


ZPS = [(-128, -128), (-128, 127), (127, -128), (127, 127), (0, 3)]     # (input, output): both ends of the range


@pytest.mark.parametrize("zx,zo", ZPS)
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_single_scale_operators_are_the_uint8_oracle_on_flipped_bytes(zx, zo, act):
    rng = np.random.default_rng(1000 * act + (zx + 128) + 2 * (zo + 128))
    x = rng.integers(-128, 128, (1, 5, 6, 8)).astype(np.int8)
    for dw in (False, True):
        m = Q.conv_model(5, 6, 8, 5, 3, 3, zx=zx, zo=zo, sw=0.01, so=0.5, act=act, bias=rng.integers(-500, 500, 8 if dw else 5), depthwise=dw, rng=rng)
        Q.fit_output_scale(m, x)
        _iso(m, x)
        m = Q.conv_model(5, 6, 8, 5, 3, 3, zx=zx, zo=zo, sw=0.01, stride=(2, 1), dil=(1, 2), padding=1, act=act, depthwise=dw, dm=2 if dw else 1, rng=rng)
        Q.fit_output_scale(m, x)
        _iso(m, x)
    _iso(Q.add_model(0.04, zx, 0.07, zo, 0.09, zo, act), Q.add_input())
    _iso(Q.add_model(0.5, zx, 0.5 / 64, 5, 0.5, zo, act), Q.add_input())


@pytest.mark.parametrize("zi,zo", ZPS)
def test_element_wise_operators_are_the_uint8_oracle_on_flipped_bytes(zi, zo):
    x = np.arange(-128, 128).astype(np.int8).reshape(1, 256)
    for code in ("RELU", "RELU6", "QUANTIZE", "TANH"):
        for si, so in ((0.05, 0.03), (0.5, 4.0), (0.02, 0.02), (1 / 128, 1 / 128)):
            _iso(Q.unary_model(code, "i8", "i8", si, zi, so, zo, n=256), x)
    _iso(Q.unary_model("DEQUANTIZE", "i8", "f32", 0.37, zi, None, 0, n=256), x)
    f = np.concatenate([np.linspace(-40, 40, 201), (np.arange(-20, 20) + 0.5) * 0.25]).astype(np.float32)[None]   # (ties of x / scale)
    _iso(Q.unary_model("QUANTIZE", "f32", "i8", None, 0, 0.25, zo, n=f.size), f)
    m = Model()
    a = m.add(T("a", (1, 2, 3, 2), "i8", scale=0.1, zp=zi))
    pd = m.add(T("p", (4, 2), "i32", data=[[0, 0], [1, 0], [0, 2], [0, 1]]))
    b = m.add(T("b", (1, 3, 5, 3), "i8", scale=0.1, zp=zi))
    c = m.add(T("c", (1, 3, 5, 3), "i8", data=np.arange(45) - 20, scale=0.1, zp=zi))
    d = m.add(T("d", (1, 3, 5, 6), "i8", scale=0.1, zp=zi))
    e = m.add(T("e", (1, 90), "i8", scale=0.1, zp=zi))
    m.ops += [Op("PAD", [a, pd], [b]), Op("CONCATENATION", [b, c], [d], axis=3), Op("RESHAPE", [d], [e], new_shape=[1, 90])]
    m.inputs, m.outputs = [a], [e]
    _iso(m, np.arange(-6, 6).astype(np.int8).reshape(1, 2, 3, 2))


def test_quantize_between_the_types_at_the_ties_of_mbqm():
    """u8 -> i8 and i8 -> u8 with equal scales and zero points 128 apart are the identity on the value: bytes XOR 0x80; with scale
    ratio 1/2 (M = 2^30, no shift: one rounding, in SaturatingRoundingDoublingHighMul) every odd input is a tie; its nudge is 2^30 for a
    product >= 0 and 1 - 2^30 below, and the division truncates: +63.5 -> 64, -63.5 -> -63 - a tie goes UP, (v + 1) >> 1."""
    xu = np.arange(256).astype(np.uint8)[None]
    got = R.run_model(Q.unary_model("QUANTIZE", "u8", "i8", 0.1, 128, 0.1, 0, n=256), {0: xu})[1]
    assert np.array_equal(got.view(np.uint8) ^ 0x80, xu)
    xi = np.arange(-128, 128).astype(np.int8)[None]
    got = R.run_model(Q.unary_model("QUANTIZE", "i8", "u8", 0.1, 0, 0.1, 128, n=256), {0: xi})[1]
    assert np.array_equal(got ^ 0x80, xi.view(np.uint8))
    got = R.run_model(Q.unary_model("QUANTIZE", "i8", "i8", 0.5, 0, 1.0, 0, n=256), {0: xi})[1]
    v = xi.astype(np.int64)
    assert np.array_equal(got, ((v + 1) >> 1).astype(np.int8))
    got = R.run_model(Q.unary_model("QUANTIZE", "u8", "i8", 0.5, 3, 1.0, -1, n=256), {0: xu})[1]
    v = xu.astype(np.int64) - 3
    assert np.array_equal(got, np.clip(((v + 1) >> 1) - 1, -128, 127).astype(np.int8))


@pytest.mark.parametrize("dw", [False, True], ids=["conv", "depthwise"])
def test_per_channel_is_the_single_scale_operator_channel_by_channel(dw):
    rng = np.random.default_rng(5 + dw)
    x = rng.integers(-128, 128, (1, 6, 5, 4)).astype(np.int8)
    m = Q.conv_model(6, 5, 4, 7, 3, 3, zx=-7, zo=11, act=1, bias=rng.integers(-900, 900, 8 if dw else 7), depthwise=dw, dm=2, stride=(2, 1), rng=rng)
    Q.fit_output_scale(m, x)
    tw, tb = m.tensors[1], m.tensors[2]
    assert tw.per_channel and len(set(R.scales_of(tw))) == tw.shape[3 if dw else 0]
    want = R.run_model(m, {0: x})[m.outputs[0]]
    for oc in range(want.shape[-1]):
        if dw:   # channel oc = ic * dm + m reads input channel oc // 2: the one-channel depthwise layer on that channel
            one = Q.conv_model(6, 5, 1, 1, 3, 3, zx=-7, zo=11, act=1, sw=R.scales_of(tw)[oc], so=m.tensors[m.outputs[0]].scale, bias=tb.data[oc:oc + 1],
                               weights=tw.data[..., oc:oc + 1], depthwise=True, dm=1, stride=(2, 1))
            got = R.run_model(one, {0: x[..., oc // 2:oc // 2 + 1]})[one.outputs[0]]
        else:
            one = Q.conv_model(6, 5, 4, 1, 3, 3, zx=-7, zo=11, act=1, sw=R.scales_of(tw)[oc], so=m.tensors[m.outputs[0]].scale, bias=tb.data[oc:oc + 1],
                               weights=tw.data[oc:oc + 1], stride=(2, 1))
            got = R.run_model(one, {0: x})[one.outputs[0]]
        assert not one.tensors[1].per_channel and np.array_equal(got[..., 0], want[..., oc]), oc


def _resize(x, ho, wo, **kw):
    x = np.asarray(x, np.int8)
    return R.resize_bilinear_i8(x.reshape((1,) + x.shape + (1,)), ho, wo, **kw)[0, :, :, 0].tolist()


def test_integer_resize_known_answers():
    """Hand-derived from the definition. A 1 x 2 row [a, b] to 1 x 4: the row step is 1024 (H = Ho = 1: y0 = y1 = 0, fy = 0), so
    v = (a (1024 - fx) + b fx) 1024 and out = trunc((v +- 2^19) / 2^20) = trunc(s / 1024 +- 1/2) with s = a (1024 - fx) + b fx."""
    a, b = -128, 127
    # plain: step = (1024 * 2 + 4 / 2) / 4 = 2050 / 4 = 512; ix = 0, 512, 1024, 1536
    #   ox 0: x0 = x1 = 0, fx = 0: s = -128 * 1024 -> trunc(-128.5) = -128
    #   ox 1: x0 = 0, x1 = (512 + 1023) / 1024 = 1, fx = 512: s = (-128 + 127) 512 = -512, v = -2^19 exactly: trunc(-0.5 - 0.5) = -1
    #   ox 2: x0 = 1, x1 = 2047 / 1024 = 1, fx = 0: s = 127 * 1024 -> trunc(127.5) = 127
    #   ox 3: x0 = 1, x1 = min(2559 / 1024, 1) = 1, fx = 512: s = 127 * 1024 -> 127
    assert _resize([[a, b]], 1, 4) == [[-128, -1, 127, 127]]
    # align_corners: step = (1024 * 1 + 3 / 2) / 3 = 1025 / 3 = 341; ix = 0, 341, 682, 1023; x0 = 0, x1 = 1 for ox >= 1
    #   ox 1: fx = 341: s = -128 * 683 + 127 * 341 = -44117 -> trunc(-43.08 - 0.5) = -43
    #   ox 2: fx = 682: s = -128 * 342 + 127 * 682 = 42838 -> trunc(41.83 + 0.5) = 42
    #   ox 3: fx = 1023: s = -128 + 127 * 1023 = 129793 -> trunc(126.75 + 0.5) = 127
    assert _resize([[a, b]], 1, 4, align_corners=True) == [[-128, -43, 42, 127]]
    # half-pixel centres: step 512, ix = 512 ox + 256 - 512 = -256, 256, 768, 1280
    #   ox 0: x0 = max(-256 / 1024, 0) = 0, x1 = 767 / 1024 = 0, fx = -256: s = -128 * 1280 - 128 * (-256) = -128 * 1024 -> -128
    #   ox 1: x0 = 0, x1 = 1279 / 1024 = 1, fx = 256: s = -128 * 768 + 127 * 256 = -65792 -> trunc(-64.25 - 0.5) = -64
    #   ox 2: x0 = 0, x1 = 1791 / 1024 = 1, fx = 768: s = -128 * 256 + 127 * 768 = 64768 -> trunc(63.25 + 0.5) = 63
    #   ox 3: x0 = 1, x1 = min(2303 / 1024, 1) = 1, fx = 256: s = 127 * 1024 -> 127
    assert _resize([[a, b]], 1, 4, half_pixel=True) == [[-128, -64, 63, 127]]
    # the rounding tie, both signs (plain, ox 1: s = (a + b) 512, v = (a + b) 2^19): a + b = 1 -> v = 2^19 -> trunc(0.5 + 0.5) = 1;
    # a + b = -1 -> v = -2^19 -> trunc(-0.5 - 0.5) = -1
    assert _resize([[0, 1]], 1, 4) == [[0, 1, 1, 1]]
    assert _resize([[-1, 0]], 1, 4) == [[-1, -1, 0, 0]]
    # y1 clamped to H - 1: a 2 x 1 column to 4 x 1, step 512; oy 3: iy = 1536, y0 = 1, y1 = min(2559 / 1024 = 2, 1) = 1, fy = 512:
    # both rows read are row 1 -> 127; oy 1 is the -2^19 tie again
    assert _resize([[a], [b]], 4, 1) == [[-128], [-1], [127], [127]]
    # where the bound on x0 takes effect: a 1 x 2 row to 1 x 3000. step = (2048 + 1500) / 3000 = 1, ix = ox; from ox = 2048 on
    # x0 = ix / 1024 = 2 is past the last column - the definition alone would read x[2]. Bounded to 1 (and x1 = min(.., 1) = 1) both
    # taps are column 1 whatever fx is: (1024 - fx) b + fx b = 1024 b -> b. The same from ox = 1024 (x0 = x1 = 1 unbounded).
    wide = _resize([[a, b]], 1, 3000)[0]
    assert wide[0] == a and wide[1024:] == [b] * (3000 - 1024) and len(wide) == 3000


# ------------------------------------------------------------------ the reader, through yh_tfl_validate
def _pc_model(rng, dw=False):
    return MQ.reader_models()[1 if dw else 0]


def test_reader_takes_per_channel_int8_models(built):
    import yolact_amd as ya
    for m in MQ.reader_models():
        ok, nt, no, msg = ya.tfl_validate(BQ.serialize(m))
        assert ok and (nt, no) == (len(m.tensors), len(m.ops)), msg
    import tfl_models as M
    twin = Q.int8_twin(M.mobilenet_like(np.random.default_rng(0)), np.random.default_rng(1))
    ok, nt, no, msg = ya.tfl_validate(BQ.serialize(twin))
    assert ok and (nt, no) == (len(twin.tensors), len(twin.ops)), msg


def test_reader_refusals_name_the_tensor_or_the_operator(built):
    import yolact_amd as ya
    rng = np.random.default_rng(12)

    def refused(mutate, *words, dw=False):
        m = _pc_model(rng, dw)
        mutate(m)
        ok, _, _, msg = ya.tfl_validate(BQ.serialize(m))
        assert not ok and all(w in msg for w in words), (words, msg)

    refused(lambda m: setattr(m.tensors[1], "scale", m.tensors[1].scales[:5]), "scale vector", "tensor w")             # 5 scales for 6 channels
    refused(lambda m: setattr(m.tensors[2], "scale", m.tensors[2].scales[:2]), "scale vector", "tensor b")             # the bias's vector is checked too
    refused(lambda m: setattr(m.tensors[1], "zp", [0, 0, 0]), "zero-point vector", "tensor w")                          # 3 zero points for 6 scales
    refused(lambda m: setattr(m.tensors[1], "qdim", 4), "quantized_dimension", "tensor w")
    refused(lambda m: setattr(m.tensors[3], "scale", [0.1] * 6) or setattr(m.tensors[3], "qdim", 3), "not a constant", "y")   # an activation
    refused(lambda m: setattr(m.tensors[1], "qdim", 3) or setattr(m.tensors[1], "scale", m.tensors[1].scales + [0.1, 0.2]),
            "dimension 0 (CONV_2D)", "tensor w", "operator 0")                                                           # 8 scales along Ci
    refused(lambda m: setattr(m.tensors[1], "qdim", 1) or setattr(m.tensors[1], "scale", [0.1, 0.2, 0.3]),
            "3 (DEPTHWISE_CONV_2D)", "tensor w", "operator 0", dw=True)
    refused(lambda m: setattr(m.tensors[1], "zp", [0, 0, 0, 0, 1, 0]), "zero point 0", "tensor w", "operator 0")
    refused(lambda m: setattr(m.tensors[1], "zp", -1) or setattr(m.tensors[1], "scale", 0.01), "zero point 0", "tensor w")   # single scale, zp -1
    # a per-channel constant that is no convolution's weights or bias (an ADD's operand) would be computed with element 0: refused
    m = Q.add_model(0.04, 0, 0.07, 0, 0.09, 0)
    m.tensors[1].scale, m.tensors[1].qdim = [0.07] * 255 + [0.08], 2
    ok, _, _, msg = ya.tfl_validate(BQ.serialize(m))
    assert not ok and "not a convolution's weights or bias" in msg and "tensor b" in msg, msg


def test_forged_quantisation_vector_lengths_are_errors_not_crashes(built):
    import yolact_amd as ya
    rng = np.random.default_rng(13)
    for field in ("n_scales", "n_zps"):
        for n in (7, 1 << 20, (1 << 30) - 1, 0xFFFFFFFF):
            m = _pc_model(rng)
            setattr(m.tensors[1], field, n)
            ok, _, _, msg = ya.tfl_validate(BQ.serialize(m))
            assert not ok and msg, (field, n)
    m = _pc_model(rng)
    spans = []
    blob = BQ.serialize(m, spans)
    assert len(spans) == 3 * 4
    for lo, hi in spans:                       # truncated anywhere inside a quantisation record: an answer, ok or not
        for cut in range(lo, hi + 1):
            ya.tfl_validate(blob[:cut])
