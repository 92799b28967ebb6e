"""-m gpu: the TFLite executor at more than two images per invoke (yh_tfl_create_batch, DESIGN.md §11 "TFLite classify batch"). Every
kernel form of the executor is integer-exact, so image i of an invoke of nb images must be the numpy oracle (oracle/tfl_oracle.py)
on image i alone, byte for byte, for every nb: single convolutions whose pixel tiles straddle image boundaries, random graphs with
folded operators (their per-image operand index), grouped convolutions (their tables for a new image count are built at its first
invoke) and the 40-op MobileNetV2-shaped graph, eager and as a captured graph. Every comparison is array_equal."""
import numpy as np
import pytest

import tfl_batch_cases as T
import tfl_builder as B
import tfl_cases as TC
import tfl_models as M

pytestmark = pytest.mark.gpu

CASES = T.conv_cases()


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%dx%d_ci%d_co%d_k%d_s%d_p%d_a%d" % c for c in CASES])
def test_single_conv_at_three_and_five_images(built, i):
    """One CONV_2D, 3 and 5 images on a handle with max_images = 5, under the default tfl_dot = 3 (Ci = 4 .. 160: the register-fed
    int8 kernel, one 16 x 16 tile per wave; yh_tfl_op_info must say so) and, as the checker, under tfl_dot = 0 (one lane per element)."""
    import yolact_amd as ya
    model, x = T.conv_case_model(i, CASES[i])
    wants = T.oracle_images(model, x)
    blob = bytes(B.serialize(model))
    h, w, ci, co, k, stride, padding, act = CASES[i]
    for tune, family in ((dict(tfl_dot=3), TC.expected_conv_family(k, k, ci, 3)), (dict(tfl_dot=0), TC.expected_conv_family(k, k, ci, 0))):
        assert (family == "conv_i8_direct") == (tune["tfl_dot"] == 3)
        eng = ya.TfliteEngine(blob, tune=tune, max_images=5)
        try:
            for nb in (3, 5):
                eng.set_batch(nb)
                eng.set_input(x[:nb])
                eng.invoke()
                info = eng.op_info(0)
                assert info["family"] == family and not info["grouped"] and not info["folded"], (tune, nb, info)
                T.check_outputs(eng, model, wants, nb, label=(CASES[i], tune, nb))
        finally:
            eng.close()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_graphs_at_three_images_every_surviving_tensor(built, seed):
    """random_dag at nb = 3: the folded operators' per-image index (apply_post takes the image: a folded ADD reads its other operand
    at image x bytes-per-image), in-place CONCATENATION parts and grouped convolutions whose tables for three images are built at this
    invoke. Fused + grouped, and everything off; every tensor the plan still writes, of every image, against the oracle on that
    image alone; then a replay."""
    import yolact_amd as ya
    rng = np.random.default_rng(4000 + seed)
    model = M.random_dag(rng, n_ops=36, hw=(9, 7))
    blob = bytes(B.serialize(model))
    x = rng.integers(0, 256, (3, 9, 7, 16), dtype=np.uint8)
    wants = T.oracle_images(model, x)
    written = sorted({o for op in model.ops for o in op.outputs})
    for tune in (dict(tfl_fuse=1, tfl_group=1), dict(tfl_fuse=0, tfl_group=0, tfl_dot=0)):
        eng = ya.TfliteEngine(blob, tune=tune, max_images=3)
        try:
            eng.set_batch(3)
            eng.set_input(x)
            eng.invoke()
            first = T.check_outputs(eng, model, wants, 3, label=(seed, tune))
            gone = sum(0 if T.check_tensor(eng, model, t, wants, 3, label=(seed, tune)) else 1 for t in written)
            assert gone == 0 or tune["tfl_fuse"], (seed, tune, gone)               # (one launch per operator: every tensor is written)
            eng.invoke()                                                      # replay: the same bytes again
            for a, b in zip(first, T.check_outputs(eng, model, wants, 3, label=(seed, tune, "replay"))):
                assert np.array_equal(a, b)
        finally:
            eng.close()


@pytest.mark.parametrize("producer", ["conv", "dw"])
def test_in_place_concatenation_part_at_an_unaligned_byte_per_image(built, producer):
    """A producer that writes straight into a CONCATENATION part which starts at byte 3 of an image of 123 bytes: at images 0, 1, 2 the
    part starts at bytes 3, 126, 249 - address mod 4 = 3, 2, 1 - so the packed-dword store is never legal and every image differs."""
    import yolact_amd as ya
    rng = np.random.default_rng(77)
    model, y = TC.unaligned_concat_model(1, 3, producer, rng)
    per_image = int(np.prod(model.tensors[model.outputs[0]].shape))
    starts = [b * per_image + 3 for b in range(3)]
    assert [s % 4 for s in starts] == [3, 2, 1]                                # an unaligned part is among the cases: all three are
    ci = model.tensors[model.inputs[0]].shape[3]
    x = rng.integers(0, 256, (3, 3, 5, ci), dtype=np.uint8)
    wants = T.oracle_images(model, x)
    eng = ya.TfliteEngine(bytes(B.serialize(model)), max_images=3)
    try:
        eng.set_batch(3)
        eng.set_input(x)
        eng.invoke()
        T.check_outputs(eng, model, wants, 3, label=producer)
        assert not T.check_tensor(eng, model, y, wants, 3)                     # the producer's own tensor is folded: it wrote in place
        eng.invoke()
        T.check_outputs(eng, model, wants, 3, label=(producer, "replay"))
    finally:
        eng.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_mobilenet_like_at_six_images(built, graph):
    """mobilenet_like(S = 64, C = 6) at nb = 6 on one handle (max_images = 6), eager and as a captured graph: output 4 and every fifth
    written tensor per image; then one image on the same handle; then two images after six - the group tables built at the first
    invoke of six must not disturb those of two built at create."""
    import yolact_amd as ya
    rng = np.random.default_rng(7)
    model = M.mobilenet_like(rng, S=64, C=6)
    x = rng.integers(0, 256, (6, 64, 64, 3), dtype=np.uint8)
    wants = T.oracle_images(model, x)
    written = sorted({o for op in model.ops for o in op.outputs})
    eng = ya.TfliteEngine(bytes(B.serialize(model)), tune=dict(tfl_graph=graph), max_images=6)
    try:
        eng.set_batch(2); eng.set_input(x[:2]); eng.invoke()
        two = [eng.output(k) for k in range(5)]
        for nb in (6, 6, 1, 2):                                                # (six twice: the capture, then its replay)
            eng.set_batch(nb)
            eng.set_input(x[:nb])
            eng.invoke()
            outs = T.check_outputs(eng, model, wants, nb, label=(graph, nb))
            assert outs[4].reshape(nb, -1).shape[1] == 64 * 6
            for t in written[::5]:
                T.check_tensor(eng, model, t, wants, nb, label=(graph, nb))
        for a, b in zip(two, outs):
            assert np.array_equal(a, b)
    finally:
        eng.close()


def test_limits(built):
    import yolact_amd as ya
    EINVAL = ya.capi.EINVAL
    blob = bytes(B.serialize(M.single_op("RELU", np.random.default_rng(0))))
    for bad in (0, -1, 513):
        with pytest.raises(ya.YhError) as e:
            ya.TfliteEngine(blob, max_images=bad)
        assert e.value.code == EINVAL and "max_images" in str(e.value)
    eng = ya.TfliteEngine(blob, max_images=5)
    assert T.code(lambda: eng.set_batch(6)) == EINVAL and T.code(lambda: eng.set_batch(0)) == EINVAL
    eng.set_batch(5)
    x = np.random.default_rng(1).integers(0, 256, (5, 4, 4, 16), dtype=np.uint8)
    assert T.code(lambda: eng.set_input(x[:4])) == EINVAL                      # the input carries set_batch images
    eng.set_input(x)
    eng.invoke()
    assert eng.output(0).shape == (5, 1, 4, 4, 16)
    eng.close()
    default = ya.TfliteEngine(blob)
    assert T.code(lambda: default.set_batch(3)) == EINVAL                      # a default handle still holds two images
    default.set_batch(2)
    default.close()
    one = ya.TfliteEngine(blob, max_images=1)
    assert T.code(lambda: one.set_batch(2)) == EINVAL
    one.set_input(x[:1]); one.invoke()
    relu = M.single_op("RELU", np.random.default_rng(0))
    assert np.array_equal(one.output(0).reshape(-1), T.oracle_images(relu, x[:1])[0][relu.outputs[0]].reshape(-1))
    one.close()
    # a model with an operator along the image axis keeps one image per invoke, whatever max_images
    import refpath_cases as R
    axis0 = ya.TfliteEngine(bytes(B.serialize(R.painter(image_axis=True))), max_images=4)
    assert T.code(lambda: axis0.set_batch(2)) == EINVAL
    axis0.close()
