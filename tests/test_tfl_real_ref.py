"""Both restatements of the TFLite operator set (oracle/tfl_oracle.py for uint8, tests/tfl_q_ref.py for int8 and per-channel) against
the value-level reference tests/tfl_real_ref.py: output ~ round(real result / output scale) + zero point, operator by operator.
The restatements were written from memory of TFLite's kernels by the hand that wrote the executor's kernels, and every other test
compares the two bit for bit; this file pins what an operator MEANS - the side of SAME padding's odd pixel, OHWI, the depthwise
channel order, which per-channel scale belongs to which channel, the resize modes, ADD's three scales, PAD's fill - to float64
arithmetic that shares no code with either. Then it shows that the reference can tell: eight deliberately wrong readings, each a
small patched copy of a restatement, are all rejected OFF the band. No GPU."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import tfl_models as M
import tfl_oracle as O
import tfl_q_ref as Q
import tfl_real_cases as C
import tfl_real_ref as R
from tfl_models_q import int8_twin

TYPES = ("u8", "i8", "i8pc")


def restatements(dt):
    """The restatements that evaluate a model of quantisation dt: both for uint8 (one formula set, two hands-off implementations)."""
    return (("tfl_oracle", O.run_model), ("tfl_q_ref", Q.run_model)) if dt == "u8" else (("tfl_q_ref", Q.run_model),)


def restated(run, model, x):
    """The restatement's output tensor 0 for every image of x."""
    return np.concatenate([np.asarray(run(model, {model.inputs[0]: x[i:i + 1]})[model.outputs[0]]) for i in range(len(x))])


def check_case(dt, model, x, label):
    """Every restatement of dt on the one-operator model against the real reference; the share in the band, capped."""
    real = R.real(model, 0, {model.inputs[0]: x})
    share = 0.0
    for name, run in restatements(dt):
        share = real.check(restated(run, model, x), label=(name, label))
        assert share <= R.CAP, (label, share)
    return share


# ------------------------------------------------------------------ convolutions
def _geometries():
    out = []
    for padding in (0, 1):
        for stride in ((1, 1), (2, 2), (1, 2), (2, 1)):
            for hw in ((8, 8), (9, 7)):
                out.append(dict(hw=hw, k=(3, 3), stride=stride, padding=padding))
    for dil in ((2, 2), (2, 1)):
        for padding in (0, 1):
            out.append(dict(hw=(9, 7), k=(3, 3), dil=dil, padding=padding))
    for k in ((1, 1), (1, 3), (2, 2)):
        out += [dict(hw=(9, 7), k=k, stride=(1, 1), padding=0), dict(hw=(8, 8), k=k, stride=(2, 2), padding=0),
                dict(hw=(9, 7), k=k, stride=(2, 1), padding=1)]
    for i, g in enumerate(out):      # activation, bias and depth multiplier go round independently of the geometry
        g.update(act=(0, 1, 3)[i % 3], bias=i % 4 != 3, dm=1 + i % 2)
    return out


GEOMETRIES = _geometries()


def _gid(g):
    return "%dx%d-k%dx%d-s%d%d-d%d%d-%s-act%d-%s-dm%d" % (g["hw"] + g["k"] + g.get("stride", (1, 1)) + g.get("dil", (1, 1)) +
                                                         ("SAME" if g["padding"] == 0 else "VALID", g["act"], "bias" if g["bias"] else "nobias", g["dm"]))


def test_the_case_list_covers_what_it_claims():
    G = GEOMETRIES
    for padding in (0, 1):
        for stride in ((1, 1), (2, 2), (1, 2), (2, 1)):
            for hw in ((8, 8), (9, 7)):
                assert any(g["padding"] == padding and g.get("stride") == stride and g["hw"] == hw for g in G)
    assert {g.get("dil") for g in G} >= {(2, 2), (2, 1)} and {g["k"] for g in G} == {(1, 1), (3, 3), (1, 3), (2, 2)}
    for key, vals in (("act", (0, 1, 3)), ("bias", (True, False)), ("dm", (1, 2)), ("padding", (0, 1))):
        for v in vals:      # each with a stride-2 SAME case of an odd total padding among them
            assert any(g[key] == v for g in G), (key, v)
    # SAME with an odd total padding (the odd pixel) exists on an even extent (3 x 3 under stride 2: 9 and 7 pad evenly there) and
    # on an odd one (the 2 x 2 kernel under stride 1)
    def odd_pixel(g):
        pads = [R.same_padding(n, k, s, d) for n, k, s, d in zip(g["hw"], g["k"], g.get("stride", (1, 1)), g.get("dil", (1, 1)))]
        return g["padding"] == 0 and any(front != back for _, front, back in pads)
    assert {(g["hw"], g.get("stride", (1, 1))[0]) for g in G if odd_pixel(g)} >= {((8, 8), 2), ((9, 7), 1)}


@pytest.mark.parametrize("geo", GEOMETRIES, ids=_gid)
def test_convolutions_mean_what_float64_says(geo):
    """CONV_2D and DEPTHWISE_CONV_2D in uint8, int8 and int8 per channel: every output off a rounding boundary is the float64
    convolution (torch, explicit asymmetric padding) rounded to nearest and clamped; per channel the right shifts differ."""
    shares = []
    for dt in TYPES:
        for dw in (False, True):
            rng = np.random.default_rng(zlib.crc32(repr((_gid(geo), dt, dw)).encode()))
            m, x = C.conv_case(dt, rng, h=geo["hw"][0], w=geo["hw"][1], ci=4, co=9, k=geo["k"], stride=geo.get("stride", (1, 1)),
                               dil=geo.get("dil", (1, 1)), padding=geo["padding"], act=geo["act"], bias=geo["bias"], depthwise=dw,
                               dm=geo["dm"])
            if dt == "i8pc":
                sw = R.scales_of(m.tensors[1])
                assert sw.max() / sw.min() >= 64 and len(set(C.conv_right_shifts(m))) > 1, (sw, C.conv_right_shifts(m))
            assert min(C.conv_right_shifts(m)) >= 5, C.conv_right_shifts(m)
            shares.append(check_case(dt, m, x, (_gid(geo), dt, "dw" if dw else "conv")))
    print("conv %s: band share %.4f (largest of %d cases)" % (_gid(geo), max(shares), len(shares)))


# ------------------------------------------------------------------ element-wise operators
@pytest.mark.parametrize("dt", ("u8", "i8"))
@pytest.mark.parametrize("scales", C.ADD_SCALES, ids=str)
def test_add_on_all_pairs(dt, scales):
    """ADD over all 256^2 code pairs, no activation and RELU6: this also confirms ADD's band (the two input roundings at the 2^20
    scale plus the final requantisation) against both restatements."""
    for act in (0, 3):
        m, x = C.add_case(dt, scales, act=act, n=1)
        share = check_case(dt, m, x, ("add", dt, scales, act))
        print("ADD %s %s act %d: band share %.4f" % (dt, scales, act, share))


@pytest.mark.parametrize("ps", C.UNARY_SETS, ids=str)
def test_requantising_operators_on_all_codes(ps):
    """QUANTIZE in the four type directions, RELU and RELU6 in both types, on all 256 codes."""
    for code, pairs in (("QUANTIZE", (("u8", "u8"), ("u8", "i8"), ("i8", "u8"), ("i8", "i8"))), ("RELU", (("u8", "u8"), ("i8", "i8"))),
                        ("RELU6", (("u8", "u8"), ("i8", "i8")))):
        for di, do in pairs:
            m, x = C.unary_case(code, di, do, ps, n=1)
            share = check_case("i8" if "i8" in (di, do) else "u8", m, x, (code, di, do, ps))
            print("%s %s -> %s %s: band share %.4f" % (code, di, do, ps, share))


@pytest.mark.parametrize("dt", ("u8", "i8"))
def test_float32_edges_and_the_tanh_table(dt):
    """QUANTIZE from float32, DEQUANTIZE (|got - real| within one float32 rounding) and TANH on all 256 codes."""
    for ps in C.UNARY_SETS[:2]:
        m, x = C.unary_case("QUANTIZE", "f32", dt, ps)
        print("QUANTIZE f32 -> %s: band share %.4f" % (dt, check_case(dt, m, x, ("quantize_f32", dt, ps))))
        m, x = C.unary_case("DEQUANTIZE", dt, "f32", ps)
        check_case(dt, m, x, ("dequantize", dt, ps))
    m, x = C.tanh_case(dt)
    want = R.real(m, 0, {m.inputs[0]: x})
    assert np.ptp(want.t) > 250 and (np.diff(want.t.reshape(2, -1)[0]) >= 0).all()      # the table rises with the code, over the whole range
    print("TANH %s: band share %.4f" % (dt, check_case(dt, m, x, ("tanh", dt))))


@pytest.mark.parametrize("dt", ("u8", "i8"))
def test_pad_concatenation_reshape(dt):
    rng = np.random.default_rng(5)
    for name, (m, x) in (("pad", C.pad_case(dt, rng)), ("concat", C.concat_case(dt, rng, False)), ("reshape", C.reshape_case(dt, rng))):
        assert check_case(dt, m, x, (name, dt)) == 0.0
    if dt == "u8":
        m, x = C.concat_case(dt, rng, True)
        print("CONCATENATION uint8 with rescaling: band share %.4f" % check_case(dt, m, x, ("concat rescale",)))


@pytest.mark.parametrize("mode", sorted(C.MODES))
def test_resize_bilinear_three_modes(mode):
    """uint8 at 5x7 -> 9x13 and 4x4 -> 8x8; int8 at the sizes whose 10-bit steps are exact (any other is refused by the reference)."""
    rng = np.random.default_rng(len(mode))
    for h, w, ho, wo in C.RESIZE_U8:
        m, x = C.resize_case("u8", rng, h, w, ho, wo, mode)
        print("RESIZE_BILINEAR u8 %s %dx%d -> %dx%d: band share %.4f" % (mode, h, w, ho, wo, check_case("u8", m, x, ("resize", mode, h, w))))
    for h, w, ho, wo in C.RESIZE_I8[mode]:
        assert R.dyadic_resize(h, ho, *C.MODES[mode]) and R.dyadic_resize(w, wo, *C.MODES[mode])
        m, x = C.resize_case("i8", rng, h, w, ho, wo, mode)
        print("RESIZE_BILINEAR i8 %s %dx%d -> %dx%d: band share %.4f" % (mode, h, w, ho, wo, check_case("i8", m, x, ("resize", mode, h, w))))
    m, x = C.resize_case("i8", rng, 5, 7, 9, 11, mode)
    with pytest.raises(ValueError):
        R.real(m, 0, {m.inputs[0]: x})


# ------------------------------------------------------------------ whole graphs, teacher-forced on the restatements' own tensors
GRAPH_SEED = 3


def graphs():
    u8 = M.mobilenet_like(np.random.default_rng(GRAPH_SEED), S=64, C=6)
    i8 = int8_twin(M.mobilenet_like(np.random.default_rng(GRAPH_SEED), S=64, C=6), np.random.default_rng(GRAPH_SEED + 1))
    for m in (u8, i8):      # re-scaled for the cap: no convolution keeps a right shift below 6
        C.tame_right_shifts(m)
        assert min(min(C.conv_right_shifts(m, k)) for k, o in enumerate(m.ops) if "CONV" in o.code) >= 6
    return u8, i8


def graph_input(n):
    return np.random.default_rng(GRAPH_SEED + 2).integers(0, 256, (n, 64, 64, 3), dtype=np.uint8)


@pytest.mark.parametrize("which", ("u8", "i8pc"))
def test_whole_graph_every_operator_on_its_own_inputs(which):
    """mobilenet_like(S = 64, C = 6) and its int8 / per-channel twin: every operator's output in the restatement's run against the
    real result on that run's own input tensors - every layer of the model family at its real shapes and scales, under the cap."""
    model = graphs()[which == "i8pc"]
    vals = (O.run_model if which == "u8" else Q.run_model)(model, {model.inputs[0]: graph_input(1)})
    shares = C.teacher_forced(model, lambda i: np.asarray(vals[i]), which)
    assert len(shares) == len(model.ops)
    print("whole graph %s: %d operators; by kind (count, largest band share): %s" % (which, len(shares), C.by_kind(shares)))


# ------------------------------------------------------------------ detection power: eight wrong readings
def _conv_copy(model, x, front=False, swapped=False, oihw=False, reverse=False):
    """A copy of the restated convolution on one image x [1, H, W, Ci], with four switches that each misread the definition: SAME
    padding's odd pixel in FRONT; the depthwise output channel m Ci + ic; the weights' bytes read as OIHW; the per-channel scales in
    reverse order. With no switch it is the restatement (asserted where it is used)."""
    o = model.ops[0]
    tx, tw, ty = (model.tensors[i] for i in (o.inputs[0], o.inputs[1], o.outputs[0]))
    dw, dm = o.code[0] == "D", o.opts.get("depth_multiplier", 1)
    wd = tw.data
    if oihw:
        co, kh, kw, ci = wd.shape
        wd = wd.reshape(co, ci, kh, kw).transpose(0, 2, 3, 1)
    w = wd.astype(np.int64) - Q.zp_of(tw)
    _, h, ww, ci = x.shape
    kh, kw = w.shape[1], w.shape[2]
    co = w.shape[3] if dw else w.shape[0]
    stride, dil = (o.opts["stride_h"], o.opts["stride_w"]), (o.opts.get("dil_h", 1), o.opts.get("dil_w", 1))

    def geom(n, k, s, d):
        if o.opts["padding"] == 1:
            return (n - ((k - 1) * d + 1) + s) // s, 0
        out = -(-n // s)
        total = max((out - 1) * s + (k - 1) * d + 1 - n, 0)
        return out, (total - total // 2 if front else total // 2)
    (ho, ph), (wo, pw) = geom(h, kh, stride[0], dil[0]), geom(ww, kw, stride[1], dil[1])
    src = (np.arange(co) % ci if swapped else np.arange(co) // dm) if dw else None
    xi = x[0].astype(np.int64) - Q.zp_of(tx)
    acc = np.zeros((ho, wo, co), np.int64)
    for oy in range(ho):
        for ox in range(wo):
            for r in range(kh):
                for s in range(kw):
                    iy, ix = oy * stride[0] - ph + r * dil[0], ox * stride[1] - pw + s * dil[1]
                    if 0 <= iy < h and 0 <= ix < ww:
                        acc[oy, ox] += xi[iy, ix][src] * w[0, r, s] if dw else w[:, r, s, :] @ xi[iy, ix]
    if len(o.inputs) > 2:
        acc += model.tensors[o.inputs[2]].data.astype(np.int64)
    sws = Q.scales_of(tw)
    return Q._conv_out(acc, tx.scale, sws[::-1] if reverse else sws, ty.scale, Q.zp_of(ty), o.opts.get("act", 0), ty.dtype)[None]


def _rejected(real, right, wrong, name):
    """The right reading passes; the wrong one is rejected OFF the band. Returns the count of such elements."""
    real.check(right, label=("right reading", name))
    _, off, _ = real.judge(wrong)
    assert off > 0, "the real reference cannot tell the wrong reading '%s' from the right one: the case is too weak" % name
    return off


def test_eight_wrong_readings_are_rejected():
    rng = np.random.default_rng(8)
    counts = {}

    def conv_reading(name, dt, switch, **case):
        m, x = C.conv_case(dt, rng, n=1, **case)
        real = R.real(m, 0, {m.inputs[0]: x})
        right = _conv_copy(m, x)
        assert np.array_equal(right, restated(Q.run_model, m, x))
        counts[name] = _rejected(real, right, _conv_copy(m, x, **{switch: True}), name)

    conv_reading("1 SAME padding, odd pixel in front", "u8", "front", h=8, w=8, ci=4, co=9, stride=(2, 2))
    conv_reading("2 depthwise output channel m Ci + ic", "u8", "swapped", h=9, w=7, ci=4, depthwise=True, dm=2)
    conv_reading("3 weights read as OIHW", "i8", "oihw", h=9, w=7, ci=4, co=9)
    conv_reading("4 per-channel scales reversed", "i8pc", "reverse", h=9, w=7, ci=4, co=9)

    for name, mode, wrong_mode in (("5 half_pixel_centers ignored", "half_pixel", (False, False)), ("6 align_corners scale H / Ho", "align", (False, False))):
        off = 0
        for dt, fn in (("u8", O.resize_bilinear_u8), ("i8", Q.resize_bilinear_i8)):
            h, w, ho, wo = (5, 7, 7, 11) if dt == "u8" else C.RESIZE_I8[mode][0]
            m, x = C.resize_case(dt, rng, h, w, ho, wo, mode, n=1)
            real = R.real(m, 0, {m.inputs[0]: x})
            off += _rejected(real, fn(x, ho, wo, *C.MODES[mode]), fn(x, ho, wo, *wrong_mode), name)
        counts[name] = off

    name = "7 ADD with sa and sb exchanged"
    m, x = C.add_case("u8", C.ADD_SCALES[0], n=1)
    (sa, sb, so), (za, zb, zo) = C.ADD_SCALES[0], C.ADD_ZPS["u8"]
    b = m.tensors[1].data
    counts[name] = _rejected(R.real(m, 0, {0: x}), O.add_u8(x, za, sa, b, zb, sb, zo, so, 0), O.add_u8(x, za, sb, b, zb, sa, zo, so, 0), name)

    name = "8 PAD filling with 0, not the zero point"
    off = 0
    for dt in ("u8", "i8"):
        m, x = C.pad_case(dt, rng, n=1)
        pads = [(int(a), int(b)) for a, b in m.tensors[1].data]
        off += _rejected(R.real(m, 0, {0: x}), np.pad(x, pads, constant_values=x.dtype.type(m.tensors[2].zp)), np.pad(x, pads, constant_values=0), name)
    counts[name] = off
    assert len(counts) == 8
    for name, off in counts.items():
        print("wrong reading %s: rejected off the band at %d elements" % (name, off))


# ------------------------------------------------------------------ the rule itself, and independence
def test_the_rule_on_hand_made_values():
    """check: off the band the nearest integer exactly; inside it floor or ceil; the clamp applied to both; the share returned."""
    t = np.array([1.2, 1.5, 1.49, -3.5, 300.0, -300.0, 2.5004])
    assert R.check(np.array([11, 12, 11, 7, 255, 0, 13]), t, 0.001, 10, 0, 255) == pytest.approx(3 / 7)
    assert R.check(np.array([11, 11, 12, 6, 255, 0, 13]), t, 0.011, 10, 0, 255) == pytest.approx(4 / 7)
    assert R.judge(np.array([12, 12, 11, 7, 255, 0, 12]), t, 0.001, 10, 0, 255)[1:] == (1, 0)       # 1.2 -> 12 is off the band; 2.5004 -> 12 in it
    assert R.judge(np.array([11, 13, 11, 7, 255, 0, 13]), t, 0.001, 10, 0, 255)[1:] == (0, 1)       # a tie two codes away is wrong inside the band
    assert R.judge(np.array([11, 12, 11, 7, 254, 0, 13]), t, 0.001, 10, 0, 255)[1:] == (1, 0)       # the clamp is exact
    with pytest.raises(AssertionError):
        R.check(np.array([12, 12, 11, 7, 255, 0, 13]), t, 0.001, 10, 0, 255)
    assert [R.right_shift(v) for v in (1.0, 0.5, 0.49, 2.0 ** -5, 0.03, 3.0)] == [0, 0, 1, 4, 5, 0]


def test_the_real_reference_is_independent():
    """In a fresh interpreter, importing tfl_real_ref and running a convolution through it loads neither restatement, nor the
    accumulators of tfl_cases, nor the product; and its text names none of them."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; import tfl_real_ref as R; "
            "R.conv_real(np.zeros((1, 3, 3, 1)), 0, np.ones((1, 1, 1, 1)), 0, None, (1, 1), (1, 1), 0); "
            "bad = sorted(m for m in sys.modules if m.split('.')[0] in ('tfl_oracle', 'tfl_q_ref', 'tfl_cases', 'tfl_q_cases', 'yolact_amd', 'oracle')); "
            "print('LOADED', bad)") % here
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "LOADED []" in out.stdout, (out.stdout, out.stderr[-2000:])
    text = open(os.path.join(here, "tfl_real_ref.py")).read()
    for word in ("tfl_oracle", "tfl_q_ref", "conv_acc", "yolact_amd"):
        assert word not in text, word
