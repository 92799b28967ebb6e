"""-m gpu: the TFLite classify batch (yh_tfl_classify_batch_u32, DESIGN.md §11 "TFLite classify batch"): n camera frames through ONE
uint8 invoke of 2n images, on device. The executor is integer-exact in every kernel form, so the batch promises more than the
engine's: frame b of the batch is yh_tfl_classify_frame_u32 on frame b alone AND the oracle chain classify_pre -> tfl_oracle per
tile -> dequant_u8 -> classify_post, bit for bit, for every n. Model: mobilenet_like(S = 64, C = 6); frames: the two golden
photographs and a seeded noise frame, at 160 x 120 and 97 x 61. Every comparison is array_equal."""
import time

import numpy as np
import pytest

import refpath_cases as R
import tfl_batch_cases as T
import tfl_builder as B
import tfl_models as M

pytestmark = pytest.mark.gpu

S, NC = 64, 6
SIZES = [(160, 120), (97, 61)]


@pytest.fixture(scope="module")
def model():
    return M.mobilenet_like(np.random.default_rng(11), S=S, C=NC)


@pytest.fixture(scope="module")
def eng(built, model):
    import yolact_amd as ya
    e = ya.TfliteEngine(bytes(B.serialize(model)), max_images=6)
    yield e
    e.close()


def _frames(oracle, golden_dir, w, h):
    noise = np.random.default_rng(11).integers(0, 2 ** 32, w * h, dtype=np.uint64).astype(np.uint32) | np.uint32(1)
    f = np.stack([oracle.pack_rgb(R.frame_rgb("frc_balls", w, h, golden_dir)), oracle.pack_rgb(R.frame_rgb("red_robot", w, h, golden_dir)),
                  noise]).reshape(3, h, w)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def cases(oracle, golden_dir, model):
    """Per size: the frames uint32 [3][h][w] and, per mode and frame, the oracle's (diverges, frame): computed once, shared, read only."""
    import tfl_oracle as O
    import yolact_amd as ya
    out = {}
    for w, h in SIZES:
        frames = _frames(oracle, golden_dir, w, h)
        cells = []
        for f in frames:
            tiles = oracle.classify_pre(f.reshape(-1), w, h, S)
            q = [O.run_model(model, {model.inputs[0]: tiles[t:t + 1]})[model.outputs[4]] for t in range(2)]
            cells.append(np.stack([oracle.dequant_u8(v.reshape(-1), 0.0078125, 128).reshape(S // 8 * (S // 8), NC) for v in q]))
        want = {}
        for mode in (ya.COMPAT_SANE, ya.COMPAT_STRICT):
            res = [oracle.classify_post(c, S, NC, mode, w, h) for c in cells]
            for _, fr in res:
                fr.setflags(write=False)
            want[mode] = res
        out[(w, h)] = (frames, want)
    return out


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("strict", [False, True])
def test_batch_of_three_equals_single_calls_and_the_oracle(eng, cases, w, h, strict):
    import yolact_amd as ya
    mode = ya.COMPAT_STRICT if strict else ya.COMPAT_SANE
    frames, want = cases[(w, h)]
    flags = [1 if rc else 0 for rc, _ in want[mode]]
    singles = []
    for b in range(3):                                                           # frame b alone through the single call
        f = frames[b].copy().reshape(-1)
        if flags[b]:
            assert T.code(lambda: eng.classify_frame(f, w, h, mode)) == ya.EDIVERGE and np.array_equal(f, frames[b].reshape(-1))
        else:
            eng.classify_frame(f, w, h, mode)
            assert np.array_equal(f, want[mode][b][1]), b
        singles.append(f.reshape(h, w))
    out = np.full((3, h, w), 0xDEADBEEF, np.uint32)
    if any(flags):
        with pytest.raises(ya.YhError) as e:
            eng.classify_batch(frames_u32=frames, width=w, height=h, mode=mode, out=out)
        assert e.value.code == ya.EDIVERGE and e.value.diverged.tolist() == flags
        assert (out == 0xDEADBEEF).all() and not eng.classify_batch_device_frames()
        return
    res, div = eng.classify_batch(frames_u32=frames, width=w, height=h, mode=mode, out=out)
    assert res is out and not div.any() and eng.classify_batch_device_frames()
    for b in range(3):
        assert np.array_equal(out[b], singles[b]), b
        assert np.array_equal(out[b].reshape(-1), want[mode][b][1]), b
    assert np.array_equal(T.device_u32(eng.classify_batch_device_frames(), out.size).reshape(out.shape), out)


def test_strict_divergence_marks_exactly_the_diverging_frames(built, oracle):
    """The painter (refpath_cases: output 4 is what the frame shows) at 128 x 64: frame 1 shows a vertical pair of balls, on which the
    reference's flood fill does not terminate. STRICT: EDIVERGE, flags [0, 1, 0], out untouched, no batch left; SANE: fine."""
    import yolact_amd as ya
    model = R.painter()
    bad = R.paint_tiles("c_vertical_pair")
    other = [R.paint_other(), R.paint_other()]
    frames = np.stack([R.painted_frame(other), R.painted_frame(bad), R.painted_frame(other)]).reshape(3, 64, 128)
    want = []
    for f in frames:
        cells, _ = R.painter_cells(oracle, model, oracle.classify_pre(f.reshape(-1), 128, 64, R.PAINT_S))
        want.append({m: oracle.classify_post(cells, R.PAINT_S, R.PAINT_C, m, 128, 64) for m in (ya.COMPAT_SANE, ya.COMPAT_STRICT)})
    assert [1 if w[ya.COMPAT_STRICT][0] else 0 for w in want] == [0, 1, 0]
    eng = ya.TfliteEngine(bytes(B.serialize(model)), max_images=6)
    try:
        eng.classify_batch(frames_u32=frames[::2], width=128, height=64, mode=ya.COMPAT_STRICT)      # a batch to lose
        assert eng.classify_batch_device_frames()
        out = np.full((3, 64, 128), 0xDEADBEEF, np.uint32)
        with pytest.raises(ya.YhError) as e:
            eng.classify_batch(frames_u32=frames, width=128, height=64, mode=ya.COMPAT_STRICT, out=out)
        assert e.value.code == ya.EDIVERGE and e.value.diverged.tolist() == [0, 1, 0]
        assert (out == 0xDEADBEEF).all() and not eng.classify_batch_device_frames()
        got, div = eng.classify_batch(frames_u32=frames, width=128, height=64, mode=ya.COMPAT_SANE)
        assert not div.any()
        for b in range(3):
            rc, fr = want[b][ya.COMPAT_SANE]
            assert rc == 0 and np.array_equal(got[b].reshape(-1), fr), b
    finally:
        eng.close()


def test_batch_of_one_in_place_and_no_read_back(eng, cases):
    import yolact_amd as ya
    w, h = SIZES[0]
    frames, want = cases[(w, h)]
    for b in (0, 2):
        f = frames[b].copy().reshape(-1)
        eng.classify_frame(f, w, h, ya.COMPAT_SANE)
        out, div = eng.classify_batch(frames_u32=frames[b:b + 1], width=w, height=h, mode=ya.COMPAT_SANE)
        assert np.array_equal(out[0].reshape(-1), f) and not div.any(), b
    buf = frames.copy()                                                          # in place: out is the input
    res, div = eng.classify_batch(frames_u32=buf, width=w, height=h, mode=ya.COMPAT_SANE, out=buf)
    assert res is buf and not div.any()
    for b in range(3):
        assert np.array_equal(buf[b].reshape(-1), want[ya.COMPAT_SANE][b][1]), b
    res, div = eng.classify_batch(frames_u32=frames[::-1].copy(), width=w, height=h, mode=ya.COMPAT_SANE, read=False)
    assert res is None and not div.any()
    dev = T.device_u32(eng.classify_batch_device_frames(), 3 * w * h).reshape(3, h, w)
    assert np.array_equal(dev, buf[::-1])


def test_device_input_and_the_yolact_mirror(eng, cases, model, tmp_path):
    import yolact_amd as ya
    from yolact_amd.yolact import Yolact
    w, h = SIZES[1]
    frames, want = cases[(w, h)]
    src = T.DeviceCopy(frames)
    try:
        got, div = eng.classify_batch(frames_dev_ptr=src.ptr, n=3, width=w, height=h, mode=ya.COMPAT_SANE)
        assert not div.any()
        for b in range(3):
            assert np.array_equal(got[b].reshape(-1), want[ya.COMPAT_SANE][b][1]), b
        assert np.array_equal(T.device_u32(src.ptr, frames.size).reshape(frames.shape), frames)      # the source is read only
        res, _ = eng.classify_batch(frames_dev_ptr=src.ptr, n=2, width=w, height=h, mode=ya.COMPAT_SANE, read=False)
        assert res is None
        assert np.array_equal(T.device_u32(eng.classify_batch_device_frames(), 2 * w * h).reshape(2, h, w), got[:2])
    finally:
        src.close()
    path = tmp_path / "model.tflite"
    path.write_bytes(bytes(B.serialize(model)))
    y = Yolact.init(model_path=str(path), compat_mode=ya.COMPAT_SANE, max_batch=6)
    buf = frames.copy().reshape(3, h * w)
    div = y.classify_batch(buf, w, h)
    assert not div.any() and np.array_equal(buf.reshape(3, h, w), got)
    one = frames[1].copy().reshape(-1)
    y.classify(one, w, h)
    assert np.array_equal(one, got[1].reshape(-1))
    y.interpreter.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_device_frames_feed_the_scene_batch(eng, cases):
    import yolact_amd as ya
    w, h = SIZES[0]
    frames, _ = cases[(w, h)]
    out, _ = eng.classify_batch(frames_u32=frames, width=w, height=h, mode=ya.COMPAT_SANE)
    ptr = eng.classify_batch_device_frames()
    assert np.array_equal(T.device_u32(ptr, out.size).reshape(out.shape), out)
    depths = np.random.default_rng(3).integers(200, 4000, (3, h, w)).astype(np.uint16)
    a, s = ya.SceneBatch(w, h, 3), ya.SceneBatch(w, h, 3)
    try:
        a.stage_frames(0, depths, frames_dev_ptr=ptr)
        s.stage_frames(0, depths, frames_u32=out)
        a.append(3, ya.COMPAT_SANE); s.append(3, ya.COMPAT_SANE)
        for b in range(3):
            ra, rs = a.read(b), s.read(b)
            assert ra.keys() == rs.keys() and all(np.array_equal(_bits(ra[k]), _bits(rs[k])) for k in ra), b
    finally:
        a.close(); s.close()


def test_refusals_leave_the_previous_batch(eng, cases):
    import yolact_amd as ya
    EINVAL = ya.capi.EINVAL
    w, h = SIZES[0]
    frames, _ = cases[(w, h)]
    want, _ = eng.classify_batch(frames_u32=frames[:2], width=w, height=h, mode=ya.COMPAT_SANE)
    ptr = eng.classify_batch_device_frames()
    four = np.zeros((4, h, w), np.uint32)
    sentinel = np.full((4, h, w), 0xDEADBEEF, np.uint32)
    for call in (lambda: eng.classify_batch(frames_u32=four, width=w, height=h, mode=ya.COMPAT_SANE, out=sentinel),             # 8 images > 6
                 lambda: eng.classify_batch(frames_u32=four, n=0, width=w, height=h, mode=ya.COMPAT_SANE, read=False),
                 lambda: eng.classify_batch(frames_u32=four, n=-1, width=w, height=h, mode=ya.COMPAT_SANE, read=False),
                 lambda: eng.classify_batch(frames_u32=four[:1], width=w, height=h, mode=7, read=False),
                 lambda: eng.classify_batch(frames_u32=four[:1], n=1, width=0, height=h, mode=ya.COMPAT_SANE, read=False),
                 lambda: eng.classify_batch(frames_u32=four[:1], n=1, width=w, height=-3, mode=ya.COMPAT_SANE, read=False)):
        assert T.code(call) == EINVAL
        assert eng.classify_batch_device_frames() == ptr
    assert (sentinel == 0xDEADBEEF).all()
    assert np.array_equal(T.device_u32(ptr, 2 * w * h).reshape(2, h, w), want)


def test_models_the_batch_refuses(built):
    """Fewer than five outputs; an operator along the image axis (the message names the single call). Nothing is left behind."""
    import yolact_amd as ya
    f = np.zeros((1, 64, 128), np.uint32)
    short = M.mobilenet_like(np.random.default_rng(11), S=S, C=NC)
    short.outputs = short.outputs[:4]
    axis0 = R.painter(image_axis=True)
    for m, word in ((short, "fewer outputs"), (axis0, "yh_tfl_classify_frame_u32")):
        e = ya.TfliteEngine(bytes(B.serialize(m)), max_images=4)
        with pytest.raises(ya.YhError) as err:
            e.classify_batch(frames_u32=f, width=128, height=64, mode=ya.COMPAT_SANE)
        assert err.value.code == ya.capi.EINVAL and word in str(err.value), str(err.value)
        assert not e.classify_batch_device_frames()
        e.close()
    default = ya.TfliteEngine(bytes(B.serialize(R.painter())))                   # max_images = 2: one frame fits, two do not
    out, _ = default.classify_batch(frames_u32=f, width=128, height=64, mode=ya.COMPAT_SANE)
    ptr = default.classify_batch_device_frames()
    assert ptr and T.code(lambda: default.classify_batch(frames_u32=np.zeros((2, 64, 128), np.uint32), width=128, height=64, mode=ya.COMPAT_SANE)) == ya.capi.EINVAL
    assert default.classify_batch_device_frames() == ptr
    default.close()


def test_single_call_on_a_handle_with_room_for_one_image(built, model, cases):
    """max_images = 1: the single call has no second image to put its second tile in and runs the tiles one after the other - the
    bytes of a default handle (both tiles in one invoke) and of the oracle; the batch, which needs two images per frame, is refused."""
    import yolact_amd as ya
    blob = bytes(B.serialize(model))
    one, two = ya.TfliteEngine(blob, max_images=1), ya.TfliteEngine(blob)
    try:
        for (w, h) in SIZES:
            frames, want = cases[(w, h)]
            for b in range(3):
                fa, fb = frames[b].copy().reshape(-1), frames[b].copy().reshape(-1)
                one.classify_frame(fa, w, h, ya.COMPAT_SANE)
                two.classify_frame(fb, w, h, ya.COMPAT_SANE)
                assert np.array_equal(fa, fb) and np.array_equal(fa, want[ya.COMPAT_SANE][b][1]), (w, h, b)
        w, h = SIZES[0]
        assert T.code(lambda: one.classify_batch(frames_u32=cases[(w, h)][0][:1], width=w, height=h, mode=ya.COMPAT_SANE)) == ya.capi.EINVAL
        assert not one.classify_batch_device_frames()
        x = np.random.default_rng(5).integers(0, 256, (1, S, S, 3), dtype=np.uint8)      # and the handle still invokes at one image
        for e in (one, two):
            e.set_input(x); e.invoke()
        assert np.array_equal(one.output(4), two.output(4))
    finally:
        one.close(); two.close()


def test_batch_and_single_call_do_not_disturb_each_other(eng, cases):
    import yolact_amd as ya
    w, h = SIZES[0]
    frames, want = cases[(w, h)]
    eng.set_batch(1)
    a, _ = eng.classify_batch(frames_u32=frames[:2], width=w, height=h, mode=ya.COMPAT_SANE)
    pa = eng.classify_batch_device_frames()
    f = frames[2].copy().reshape(-1)
    eng.classify_frame(f, w, h, ya.COMPAT_SANE)                                  # a single call between two batches
    assert np.array_equal(f, want[ya.COMPAT_SANE][2][1])
    assert eng.classify_batch_device_frames() == pa and np.array_equal(T.device_u32(pa, a.size).reshape(a.shape), a)
    b, _ = eng.classify_batch(frames_u32=frames[1:3], width=w, height=h, mode=ya.COMPAT_SANE)
    g = frames[0].copy().reshape(-1)
    eng.classify_frame(g, w, h, ya.COMPAT_SANE)                                  # a single call after a batch
    assert np.array_equal(g, want[ya.COMPAT_SANE][0][1])
    assert np.array_equal(T.device_u32(eng.classify_batch_device_frames(), b.size).reshape(b.shape), b)
    # the caller's set_batch(1) still holds: the input takes one image, not six
    x = np.random.default_rng(5).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    assert T.code(lambda: eng.set_input(x)) == ya.capi.EINVAL
    eng.set_input(x[:1]); eng.invoke()
    assert eng.output(4).shape == (1, (S // 8) ** 2, NC)


def test_a_batch_of_four_is_not_slower_than_four_single_frames(built):
    """A condition, not a measurement (tools/time_tflite.py --batch measures): in this process, on one handle of the full-size
    stand-in (max_images = 8), after warm-up, the median of 10 classify_batch calls on 4 frames of 640 x 480 (host in, host out) is
    below 4 x the median of 10 classify_frame calls. No margin."""
    import yolact_amd as ya
    W, H = 640, 480
    eng = ya.TfliteEngine(bytes(B.serialize(M.mobilenetv2_yolact(np.random.default_rng(31)))), max_images=8)
    four = np.random.default_rng(12).integers(0, 2 ** 32, (4, H, W), dtype=np.uint64).astype(np.uint32)
    out = np.empty_like(four)
    one = four[0].copy().reshape(-1)

    def batch():
        eng.classify_batch(frames_u32=four, width=W, height=H, mode=ya.COMPAT_SANE, out=out)

    def single():
        eng.classify_frame(one, W, H, ya.COMPAT_SANE)

    def clock(fn):
        one[:] = four[0].reshape(-1)                                             # (the single call works in place: refilled outside the clock)
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

    try:
        for _ in range(3):
            batch(); clock(single)
        assert np.array_equal(out[0].reshape(-1), one)
        tb = sorted(clock(batch) for _ in range(10))
        ts = sorted(clock(single) for _ in range(10))
    finally:
        eng.close()
    mb, ms = (tb[4] + tb[5]) / 2, 4 * (ts[4] + ts[5]) / 2
    print(f"tflite classify of 4 frames 640x480: batch {mb:.3f} ms, 4 x single {ms:.3f} ms, ratio {mb / ms:.3f}")
    assert mb < ms
