"""-m gpu: the device's own bytes against the value-level reference tests/tfl_real_ref.py (float64 arithmetic of what each operator
means; no restatement takes part in any comparison here). Every kernel family alone, named through yh_tfl_op_info, on the geometries
that carry the meaning, with one and two images per invoke; then whole graphs teacher-forced: every operator's own output tensor
against the real result on the executor's own input tensors, so one-code differences cannot accumulate. The rule, the band and the
5 % cap: tests/tfl_real_ref.py; the cases: tests/tfl_real_cases.py; the same cases against the restatements: tests/test_tfl_real_ref.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfl_builder as B
import tfl_builder_q as BQ
import tfl_models as M
import tfl_real_cases as C
from tfl_models_q import int8_twin

pytestmark = pytest.mark.gpu

# the geometries that carry the meaning, on 9 x 7 (and SAME under stride 2 on 8 x 8, where the padding is odd: one pixel, behind)
GEOS = (dict(h=9, w=7, stride=(2, 2)), dict(h=9, w=7, dil=(2, 2)), dict(h=8, w=8, stride=(2, 2)))

# family: (tfl_dot, Ci, depthwise, depth multiplier, the quantisations the family has a form for)
CONV_FAMILIES = {
    "conv_i8_direct": (3, 64, False, 1, ("u8", "i8pc")),
    "conv_i8_lds": (2, 64, False, 1, ("u8", "i8pc")),
    "conv_dot4": (1, 16, False, 1, ("u8",)),
    "conv_dot1": (1, 20, False, 1, ("u8",)),
    "conv_px8": (1, 3, False, 1, ("u8", "i8pc")),
    "conv_scalar": (0, 3, False, 1, ("u8", "i8pc")),
    "dw_c4": (3, 8, True, 1, ("u8", "i8pc")),
    "dw_scalar": (3, 4, True, 2, ("u8", "i8pc")),
}


def _tune(dot, **more):
    t = dict(more)
    if dot != 3:
        t["tfl_dot"] = dot          # (3 is the default: that plan runs with no field set)
    return t or None


@pytest.mark.parametrize("family", sorted(CONV_FAMILIES))
def test_every_convolution_family_means_what_float64_says(built, family):
    """3 x 3, SAME: stride 2 and dilation 2 on 9 x 7, stride 2 on 8 x 8; Co = 9 and 17 (the ragged channel tile; depthwise: Ci dm);
    bias, RELU6 / RELU / none in turn; uint8 and int8 per channel where the family has the form; one and two images."""
    dot, ci, dw, dm, types = CONV_FAMILIES[family]
    rng = np.random.default_rng(sorted(CONV_FAMILIES).index(family))
    act = 0
    for dt in types:
        for geo in GEOS:
            for co in ((9, 17) if not dw else (ci * dm,)):
                act = (act + 1) % 3
                m, x = C.conv_case(dt, rng, ci=ci, co=co, act=(3, 1, 0)[act], depthwise=dw, dm=dm, **geo)
                if dt == "i8pc":
                    assert len(set(C.conv_right_shifts(m))) > 1
                share = C.device_check(m, x, {0: family}, _tune(dot), label=(family, dt, geo, co))
                print("%s %s %s Co %d: band share %.4f" % (family, dt, geo, m.tensors[1].shape[3 if dw else 0], share))


def test_add_family_on_all_pairs(built):
    for dt in ("u8", "i8"):
        for scales, act in ((C.ADD_SCALES[0], 0), (C.ADD_SCALES[1], 3)):
            m, x = C.add_case(dt, scales, act=act)
            print("add %s %s act %d: band share %.4f" % (dt, scales, act, C.device_check(m, x, {0: "add"}, label=("add", dt, scales))))


def test_requant_lut_quantize_dequantize_families(built):
    """QUANTIZE in the four type directions, RELU, RELU6 (requant) and TANH (lut) on all 256 codes; QUANTIZE from float32 and
    DEQUANTIZE in both types."""
    for ps in (C.UNARY_SETS[0], C.UNARY_SETS[2]):
        for code, pairs in (("QUANTIZE", (("u8", "u8"), ("u8", "i8"), ("i8", "u8"), ("i8", "i8"))), ("RELU", (("u8", "u8"), ("i8", "i8"))),
                            ("RELU6", (("u8", "u8"), ("i8", "i8")))):
            for di, do in pairs:
                m, x = C.unary_case(code, di, do, ps)
                print("requant %s %s -> %s %s: band share %.4f" % (code, di, do, ps, C.device_check(m, x, {0: "requant"}, label=(code, di, do, ps))))
    for dt in ("u8", "i8"):
        m, x = C.tanh_case(dt)
        print("lut TANH %s: band share %.4f" % (dt, C.device_check(m, x, {0: "lut"}, label=("tanh", dt))))
        for ps in C.UNARY_SETS[:2]:
            m, x = C.unary_case("QUANTIZE", "f32", dt, ps)
            print("quantize_f32 -> %s: band share %.4f" % (dt, C.device_check(m, x, {0: "quantize_f32"}, label=("quantize_f32", dt, ps))))
            m, x = C.unary_case("DEQUANTIZE", dt, "f32", ps)
            C.device_check(m, x, {0: "dequantize"}, label=("dequantize", dt, ps))
            print("dequantize %s: every value within one float32 rounding" % dt)


def test_pad_concat_resize_families(built):
    rng = np.random.default_rng(6)
    for dt in ("u8", "i8"):
        m, x = C.pad_case(dt, rng)
        assert C.device_check(m, x, {0: "pad"}, label=("pad", dt)) == 0.0
        m, x = C.concat_case(dt, rng, False)
        assert C.device_check(m, x, {0: "concat"}, label=("concat", dt)) == 0.0
        print("pad, concat %s: equal" % dt)
    m, x = C.concat_case("u8", rng, True)
    print("concat u8 with rescaling: band share %.4f" % C.device_check(m, x, {0: "concat"}, label=("concat rescale",)))
    for mode in sorted(C.MODES):
        for dt, sizes in (("u8", C.RESIZE_U8), ("i8", C.RESIZE_I8[mode])):
            for h, w, ho, wo in sizes:
                m, x = C.resize_case(dt, rng, h, w, ho, wo, mode)
                share = C.device_check(m, x, {0: "resize"}, label=("resize", dt, mode, h, w))
                print("resize %s %s %dx%d -> %dx%d: band share %.4f" % (dt, mode, h, w, ho, wo, share))


# ------------------------------------------------------------------ whole graphs, teacher-forced
GRAPH_SEED = 3


def _graph(which):
    m = M.mobilenet_like(np.random.default_rng(GRAPH_SEED), S=64, C=6)
    if which == "i8pc":
        m = int8_twin(m, np.random.default_rng(GRAPH_SEED + 1))
    C.tame_right_shifts(m)       # re-scaled for the cap: no convolution keeps a right shift below 6
    return m, (BQ.serialize(m) if which == "i8pc" else bytes(B.serialize(m)))


def _teacher_forced_on_device(which, nb):
    import yolact_amd as ya
    model, blob = _graph(which)
    x = np.random.default_rng(GRAPH_SEED + 2).integers(0, 256, (nb, 64, 64, 3), dtype=np.uint8)
    eng = ya.TfliteEngine(blob, tune=dict(tfl_fuse=0), max_images=max(nb, 2))      # tfl_fuse = 0: every tensor exists
    try:
        eng.set_batch(nb)
        eng.set_input(x)
        eng.invoke()
        read = C.engine_reader(eng, model, nb)
        assert np.array_equal(read(model.inputs[0]), x)
        shares = C.teacher_forced(model, read, (which, nb))
        names = {k: eng.op_info(k)["family"] for k in shares}
    finally:
        eng.close()
    assert len(shares) == len(model.ops)
    for k, (code, s) in shares.items():
        print("%s nb %d op %2d %-18s %-14s band share %.4f" % (which, nb, k, code, names[k], s))
    print("%s nb %d: %d of %d operators checked; by kind (count, largest band share): %s" % (which, nb, len(shares), len(model.ops), C.by_kind(shares)))
    return shares


@pytest.mark.parametrize("which", ("u8", "i8pc"))
def test_whole_graph_every_operator_on_the_executors_own_tensors(built, which):
    """mobilenet_like(S = 64, C = 6) and its int8 / per-channel twin, two images, tfl_fuse = 0: every operator of the plan at its real
    shapes and scales, its own output tensor against the real result on its own input tensors."""
    _teacher_forced_on_device(which, 2)


def test_whole_graph_through_the_batch_plan_five_images(built):
    """The same walk with max_images = 5 and five images (uint8): image b's tensors through the batch plan, the heads the detection
    tail reads among them."""
    shares = _teacher_forced_on_device("u8", 5)
    assert {"CONV_2D", "DEPTHWISE_CONV_2D", "ADD", "PAD", "RESIZE_BILINEAR", "RELU", "TANH", "QUANTIZE", "RESHAPE", "CONCATENATION"} == {c for c, _ in shares.values()}
