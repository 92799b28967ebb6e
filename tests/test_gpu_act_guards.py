"""-m gpu: a step of n frames on a handle made for n + 1 stays inside its n images - in every activation allocation, in the E4M3
twins of an fp8 handle, and in front of the 256 zero bytes (the zero pixel every padded tap reads first among them) behind each - and
nothing that lies in image n can reach a result. yh_debug_act_paint fills images n .. max_batch - 1 of every allocation with 0xFF
(NaN as f16 and as E4M3); yh_debug_act_check wants every one of those bytes back, and the trailers zero (Bounds).

The whole-network comparisons tolerate 3 % of absmax, and a store into a neighbour's rows that a later layer overwrites leaves no
trace in them; the fusions that exist only in the engine's plans - the FPN upsample in the lateral's epilogue, the projection shortcut
inside a block's last conv, the prototype conv in an epilogue, the bottleneck chains - have no other bounds test. The handles are
those of the fusion tests of tests/test_gpu_net.py, one frame larger; every comparison is bit equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THRESH = 0.005   # (as tests/test_gpu_net.py: the seeded weights give no candidate above the default at these sizes)
CONFIGS = [(128, 2, 50, -1, "f16"), (145, 1, 101, -1, "f16"), (224, 3, 50, 4, "f16"), (160, 2, 50, 4, "fp8")]


def _record(eng, n):
    heads = [eng.output(i) for i in range(4)]
    assert all(a.shape[0] == n for a in heads)
    return heads, [eng.detections(f) for f in range(n)]


def _same(a, b):
    for x, y in zip(a[0], b[0]):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    for (da, ma), (db, mb) in zip(a[1], b[1]):
        assert da == db and np.array_equal(ma, mb)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("S,n,backbone,plan_cus,precision", CONFIGS)
def test_a_step_of_n_frames_stays_inside_its_n_images(built, S, n, backbone, plan_cus, precision, use_graph):
    ya = built
    fp8 = precision == "fp8"
    eng = ya.Engine(input_size=S, backbone=backbone, max_batch=n + 1, use_graph=use_graph, conf_thresh=THRESH, tune=dict(plan_cus=plan_cus),
                    precision=ya.PRECISION_FP8 if fp8 else ya.PRECISION_F16)
    eng.load_weights(eng.generate_weights(1))
    img = np.random.default_rng(S + n).integers(0, 256, (n + 1, S, S, 3), dtype=np.uint8)
    eng.set_input(img[:n])
    if fp8:
        eng.fp8_calibrate()
    eng.evaluate()
    first = _record(eng, n)
    assert np.isfinite(first[0][3]).all() and np.abs(first[0][3]).max() > 0.1
    # the same step over painted images n ..: nothing of them changes, nothing of them is read into a result
    eng.act_paint(n)
    eng.set_input(img[:n])
    eng.evaluate()
    eng.act_check(n)
    _same(_record(eng, n), first)
    # a full step leaves real data in image n; painted over, the step of n frames again
    eng.set_input(img)
    eng.evaluate()
    eng.act_paint(n)
    eng.set_input(img[:n])
    eng.evaluate()
    eng.act_check(n)
    _same(_record(eng, n), first)
    # the plans under test were the ones taken (the profiler lists the plan of the current batch size, and runs it once more)
    names = [p["name"] for p in eng.profile(with_tail=False, reps=1)]
    assert not any(nm.startswith(("bilinear_f16:up", "bilinear2x_f16:up")) for nm in names)          # FPN upsample in the lateral's epilogue
    assert not any(nm.endswith("b0_d") for nm in names)                                              # projection shortcut inside the last conv
    assert any(nm.startswith("bneck_chain_f16") for nm in names)                                     # bottleneck chains
    if plan_cus == 4:
        assert any(nm.endswith(":proto3+proto") and "[+1x1]" in nm for nm in names)                  # prototype conv in an epilogue
        assert any(nm.startswith("conv_igemm_fp8") for nm in names) == fp8
    eng.act_check(n)
    eng.close()


def test_the_check_sees_one_changed_byte_and_the_calls_refuse_bad_arguments(built):
    ya = built
    eng = ya.Engine(input_size=64, max_batch=3, use_graph=False)
    for call in (eng.act_paint, eng.act_check):
        with pytest.raises(ya.YhError) as ei:
            call(1)                                        # no weights yet
        assert ei.value.code == ya.capi.ESTATE
    eng.load_weights(eng.generate_weights(1))
    for call in (eng.act_paint, eng.act_check):
        for bad in (0, 3, -1):
            with pytest.raises(ya.YhError) as ei:
                call(bad)
            assert ei.value.code == ya.capi.EINVAL, bad
    # painted from image 1 on, a step of TWO frames must be reported: it writes image 1 of every tensor it makes
    img = np.random.default_rng(1).integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    eng.act_paint(1)
    eng.act_check(1)
    eng.set_input(img)
    eng.invoke()
    eng.act_check(2)                                       # (image 2 is still painted)
    with pytest.raises(ya.YhError) as ei:
        eng.act_check(1)
    assert ei.value.code == ya.capi.EOVERFLOW and "image 1 row 0 byte" in str(ei.value), str(ei.value)
    assert 1 <= len(ei.value.offenders) <= 9 and all(": image 1 row " in ln for ln in ei.value.offenders), ei.value.offenders
    eng.close()
    one = ya.Engine(input_size=64, max_batch=1, use_graph=False)
    one.load_weights(one.generate_weights(1))
    with pytest.raises(ya.YhError) as ei:
        one.act_paint(1)                                   # a handle of one image has no image to paint
    assert ei.value.code == ya.capi.EINVAL
    one.close()
