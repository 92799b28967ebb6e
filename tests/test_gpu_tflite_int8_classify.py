"""-m gpu: Yolact::classify (yolact.rs:192-234) with an int8 / per-channel .tflite in the middle - the twin of mobilenet_like(S = 64)
with a uint8 input behind a QUANTIZE and output 4 behind a QUANTIZE to uint8 - on a 96 x 64 frame: the single call against the
refpath oracle fed with tests/tfl_q_ref.py's output 4, the batch of three against three single calls (host frames and a device
pointer), and the refusal of a model whose output 4 is int8."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfl_batch_cases as TB
import tfl_builder_q as BQ
import tfl_models as M
import tfl_q_cases as Q
import tfl_q_ref as R

pytestmark = pytest.mark.gpu

S, C, W, H = 64, 6, 96, 64


def _twin(**kw):
    rng = np.random.default_rng(11)
    return Q.int8_twin(M.mobilenet_like(rng, S=S, C=C), rng, **kw)


def _frames(n):
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint32)
    return ((rgb[..., 0] << 24) | (rgb[..., 1] << 16) | (rgb[..., 2] << 8)).astype(np.uint32)


def test_classify_frame_through_an_int8_model(built, oracle):
    import yolact_amd as ya
    model = _twin()
    o4 = model.tensors[model.outputs[4]]
    assert o4.dtype == "u8" and model.tensors[model.inputs[0]].dtype == "u8"
    eng = ya.TfliteEngine(BQ.serialize(model))
    frame0 = _frames(1)[0].reshape(-1)
    tiles = oracle.classify_pre(frame0, W, H, S)
    cells = np.stack([oracle.dequant_u8(R.run_model(model, {model.inputs[0]: tiles[t:t + 1]})[model.outputs[4]].reshape(-1), R.f32(o4.scale), R.zp_of(o4))
                      .reshape(S // 8 * (S // 8), C) for t in range(2)])
    for mode in (ya.COMPAT_SANE, ya.COMPAT_STRICT):
        rc, want = oracle.classify_post(cells, S, C, mode, W, H)
        frame = frame0.copy()
        if rc:
            with pytest.raises(ya.YhError) as e:
                eng.classify_frame(frame, W, H, mode)
            assert e.value.code == ya.EDIVERGE and np.array_equal(frame, frame0)
        else:
            eng.classify_frame(frame, W, H, mode)
            assert np.array_equal(frame, want)
    eng.close()


def test_classify_batch_of_three_equals_three_single_calls(built):
    import yolact_amd as ya
    blob = BQ.serialize(_twin())
    frames = _frames(3)
    single = ya.TfliteEngine(blob)
    want = frames.copy()
    for b in range(3):
        f = want[b].reshape(-1)
        single.classify_frame(f, W, H, ya.COMPAT_SANE)
    single.close()
    assert not np.array_equal(want, frames)
    eng = ya.TfliteEngine(blob, max_images=6)
    got, div = eng.classify_batch(frames_u32=frames.copy(), width=W, height=H, mode=ya.COMPAT_SANE)
    assert np.array_equal(got, want) and not div.any()
    src = TB.DeviceCopy(frames)
    try:
        got, div = eng.classify_batch(frames_dev_ptr=src.ptr, n=3, width=W, height=H, mode=ya.COMPAT_SANE)
        assert np.array_equal(got, want) and not div.any()
    finally:
        src.close()
    eng.close()


def test_an_int8_output_4_is_refused_by_classify(built):
    import yolact_amd as ya
    model = _twin(quant_output=None)
    assert model.tensors[model.outputs[4]].dtype == "i8"
    eng = ya.TfliteEngine(BQ.serialize(model), max_images=2)
    frame = _frames(1)[0].reshape(-1)
    with pytest.raises(ya.YhError) as e:
        eng.classify_frame(frame, W, H, ya.COMPAT_SANE)
    assert e.value.code == ya.capi.EINVAL and "output 4 is int8" in str(e.value) and "uint8 or float32" in str(e.value)
    with pytest.raises(ya.YhError) as e:
        eng.classify_batch(frames_u32=_frames(1), width=W, height=H, mode=ya.COMPAT_SANE)
    assert "output 4 is int8" in str(e.value)
    eng.close()
