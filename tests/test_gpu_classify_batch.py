"""The classify batch (yh_classify_batch_u32, DESIGN.md §11 "Classify batch") on the device: n camera frames through one network step
of 2n tiles. The engine's launch plan depends on the batch size, so output 4 of a step of 2n is not compared with steps of 2; what
is exact is everything around the network: tiles 2b, 2b + 1 are the oracle's classify_pre of frame b (shown through set_input + invoke
at the same batch size, hence the same plan), frame b is the oracle's classify_post of the engine's own output 4 for those tiles,
and with n = 1 the call equals classify_frame. Every comparison is array_equal. One engine for the module: input 224, max_batch 8,
graph, seeded weights; SANE unless said. The kernels' edge shapes are in tests/test_gpu_classify_batch_edges.py."""
import ctypes as C
import time

import numpy as np
import pytest

import refpath_cases as R

pytestmark = pytest.mark.gpu

W, H, S, NCH = 640, 480, 224, 81


def _device_u32(ptr, n):
    """n uint32 from device memory."""
    path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), "libamdhip64.so")
    hip = C.CDLL(path)
    out = np.zeros(n, np.uint32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0   # hipMemcpyDeviceToHost
    return out


def _code(fn):
    from yolact_amd import capi
    try:
        fn()
    except capi.YhError as e:
        return e.code
    return 0


@pytest.fixture(scope="module")
def eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=S, max_batch=8, use_graph=True)
    e.load_weights(e.generate_weights(seed=1))
    yield e
    e.close()


@pytest.fixture(scope="module")
def frames(oracle, golden_dir):
    """uint32 [3][H][W]: the two golden photographs and a seeded noise frame (low byte set: it must be ignored)."""
    noise = np.random.default_rng(11).integers(0, 2 ** 32, W * H, dtype=np.uint64).astype(np.uint32) | np.uint32(1)
    f = np.stack([oracle.pack_rgb(R.frame_rgb("frc_balls", W, H, golden_dir)), oracle.pack_rgb(R.frame_rgb("red_robot", W, H, golden_dir)),
                  noise]).reshape(3, H, W)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def batch3(eng, frames):
    """The batch of three, run once: (frames out, diverged, output 4 of the step, the device pointer)."""
    import yolact_amd as ya
    out, div = eng.classify_batch(frames_u32=frames, width=W, height=H, mode=ya.COMPAT_SANE)
    cells = eng.output(4)
    ptr = eng.classify_batch_device_frames()
    dev = _device_u32(ptr, out.size).reshape(out.shape)
    for a in (out, cells, dev):
        a.setflags(write=False)
    return out, div, cells, ptr, dev


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def test_batch_of_three(eng, oracle, frames, batch3):
    import yolact_amd as ya
    out, div, cells, ptr, dev = batch3
    assert out.shape == (3, H, W) and cells.shape == (6, 28, 28, NCH) and not div.any() and ptr
    # the post half: the oracle on the engine's own output 4
    for b in range(3):
        rc, want = oracle.classify_post(cells[2 * b:2 * b + 2], S, NCH, ya.COMPAT_SANE, W, H)
        assert rc == 0 and np.array_equal(out[b].reshape(-1), want), b
    # the device copy, raw and through the scene batch (the class images never on the host) against the same frames from the host
    assert np.array_equal(dev, out)
    depths = np.random.default_rng(3).integers(200, 4000, (3, H, W)).astype(np.uint16)
    a, s = ya.SceneBatch(W, H, 3), ya.SceneBatch(W, H, 3)
    a.stage_frames(0, depths, frames_dev_ptr=ptr)
    s.stage_frames(0, depths, frames_u32=out)
    a.append(3, ya.COMPAT_SANE); s.append(3, ya.COMPAT_SANE)
    for b in range(3):
        ra, rs = a.read(b), s.read(b)
        assert ra.keys() == rs.keys() and all(np.array_equal(_bits(ra[k]), _bits(rs[k])) for k in ra), b
    a.close(); s.close()
    # the pre half: the oracle's tiles through a step of the same size (the same plan) give the same output 4
    eng.set_input(np.concatenate([oracle.classify_pre(f, W, H, S) for f in frames]))
    eng.invoke()
    assert np.array_equal(eng.output(4), cells)
    assert np.array_equal(_device_u32(eng.classify_batch_device_frames(), out.size).reshape(out.shape), out)   # invoke leaves the batch


def test_batch_of_one_is_classify_frame(eng, frames):
    import yolact_amd as ya
    for b in (0, 2):
        f = frames[b].copy()
        eng.classify_frame(f.reshape(-1), W, H, ya.COMPAT_SANE)
        c1 = eng.output(4)
        out, div = eng.classify_batch(frames_u32=frames[b:b + 1], width=W, height=H, mode=ya.COMPAT_SANE)
        assert np.array_equal(out[0], f) and np.array_equal(eng.output(4), c1) and not div.any(), b


def test_in_place_and_the_yolact_mirror(eng, frames, batch3):
    import yolact_amd as ya
    from yolact_amd.yolact import Yolact
    buf = frames.copy().reshape(3, H * W)
    div = Yolact(eng, ya.COMPAT_SANE).classify_batch(buf, W, H)
    assert np.array_equal(buf.reshape(3, H, W), batch3[0]) and not div.any()


DEVICE_INPUT = r"""
import ctypes as C, sys
import torch                      # first: the library then shares torch's HIP runtime, and a tensor's pointer is one it knows
import numpy as np
sys.path[:0] = [%(pkg)r]
import yolact_amd as ya
if not torch.cuda.is_available():
    sys.exit(77)
W, H, n = 640, 480, 3
frames = np.random.default_rng(11).integers(0, 2 ** 32, (n, H, W), dtype=np.uint64).astype(np.uint32)
eng = ya.Engine(input_size=224, max_batch=8, use_graph=True)
eng.load_weights(eng.generate_weights(seed=1))
want, _ = eng.classify_batch(frames_u32=frames, width=W, height=H, mode=ya.COMPAT_SANE)
t = torch.from_numpy(frames.view(np.int32).copy()).cuda()
torch.cuda.synchronize()
got, div = eng.classify_batch(frames_dev_ptr=t.data_ptr(), n=n, width=W, height=H, mode=ya.COMPAT_SANE)
assert np.array_equal(got, want) and want.any() and not div.any()
assert np.array_equal(t.cpu().numpy().view(np.uint32), frames)                   # the source is read only
eng.classify_batch(frames_u32=frames[::-1].copy(), width=W, height=H, mode=ya.COMPAT_SANE, out=False)   # another batch in between
got, div = eng.classify_batch(frames_dev_ptr=t.data_ptr(), n=n, width=W, height=H, mode=ya.COMPAT_SANE, out=False)
ptr = eng.classify_batch_device_frames()
assert got is None and not div.any() and ptr
back = torch.empty((n, H, W), dtype=torch.int32, device="cuda")
hip = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln))
assert hip.hipMemcpy(C.c_void_p(back.data_ptr()), C.c_void_p(ptr), C.c_size_t(want.nbytes), 3) == 0   # hipMemcpyDeviceToDevice
assert np.array_equal(back.cpu().numpy().view(np.uint32), want)
eng.close()
print("device input ok")
"""


def test_device_input(built):
    """frames_dev_ptr at a torch ROCm tensor gives what host input gives, and with out=False nothing comes back but the pointer is
    valid. In a child process, because torch has to be imported before the library is loaded for the two to share one HIP runtime
    (and this process must not load a second one for the tests after it). Skipped if torch sees no device."""
    import os
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tiny-object-detection_amd")
    r = subprocess.run([sys.executable, "-c", DEVICE_INPUT % dict(pkg=pkg)], capture_output=True, text=True, timeout=120)
    if r.returncode == 77:
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and "device input ok" in r.stdout, r.stdout + r.stderr


def test_refusals_leave_the_previous_batch(eng, frames):
    import yolact_amd as ya
    EINVAL = ya.capi.EINVAL
    want, _ = eng.classify_batch(frames_u32=frames[:2], width=W, height=H, mode=ya.COMPAT_SANE)
    ptr = eng.classify_batch_device_frames()
    five = np.zeros((5, H, W), np.uint32)
    sentinel = np.full((5, H, W), 0xDEADBEEF, np.uint32)
    for call in (lambda: eng.classify_batch(frames_u32=five, width=W, height=H, mode=ya.COMPAT_SANE, out=sentinel),          # 10 tiles > 8
                 lambda: eng.classify_batch(frames_u32=five, n=0, width=W, height=H, mode=ya.COMPAT_SANE, out=False),
                 lambda: eng.classify_batch(frames_u32=five, n=-1, width=W, height=H, mode=ya.COMPAT_SANE, out=False),
                 lambda: eng.classify_batch(frames_u32=five[:1], width=W, height=H, mode=7, out=False),
                 lambda: eng.classify_batch(frames_u32=five[:1], n=1, width=0, height=H, mode=ya.COMPAT_SANE, out=False),
                 lambda: eng.classify_batch(frames_u32=five[:1], n=1, width=W, height=-3, mode=ya.COMPAT_SANE, out=False)):
        assert _code(call) == EINVAL
        assert eng.classify_batch_device_frames() == ptr
    assert (sentinel == 0xDEADBEEF).all()
    assert np.array_equal(_device_u32(ptr, 2 * W * H).reshape(2, H, W), want)


def test_batch_and_single_frame_do_not_disturb_each_other(eng, frames):
    import yolact_amd as ya
    a, _ = eng.classify_batch(frames_u32=frames[:2], width=W, height=H, mode=ya.COMPAT_SANE)
    pa = eng.classify_batch_device_frames()
    f = frames[2].copy()
    eng.classify_frame(f.reshape(-1), W, H, ya.COMPAT_SANE)
    assert eng.classify_batch_device_frames() == pa and np.array_equal(_device_u32(pa, a.size).reshape(a.shape), a)
    single = _device_u32(eng.classify_device_frame(), W * H).reshape(H, W)
    assert np.array_equal(single, f)
    b, _ = eng.classify_batch(frames_u32=frames[1:3], width=W, height=H, mode=ya.COMPAT_SANE)
    assert np.array_equal(_device_u32(eng.classify_device_frame(), W * H).reshape(H, W), f)
    assert np.array_equal(_device_u32(eng.classify_batch_device_frames(), b.size).reshape(b.shape), b)


def test_no_weights_is_a_state_error(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=64, max_batch=2, use_graph=False)
    assert _code(lambda: e.classify_batch(frames_u32=np.zeros((1, 4, 4), np.uint32), width=4, height=4, mode=ya.COMPAT_SANE)) == ya.capi.ESTATE
    assert not e.classify_batch_device_frames()
    e.close()


def _strict_cells(diverging):
    """Cells [6][784][81] of three frames; frame 1's first tile holds a vertical pair of balls (the reference's flood fill does not
    terminate on it) if `diverging`, else every tile a terminating pattern."""
    g = S // 8
    calm = [R.c_two_apart(g), R.c_diagonal(g), R.c_wrap_miss(g), R.c_first_last(g), R.b_corners(g), R.c_two_apart(g)]
    cl = [c["classes"].copy() for c in calm]
    for k in (1, 4):                                                             # robots of both colours beside the balls
        free = np.nonzero(cl[k] == 0)[0]
        cl[k][free[::5]] = 1
        cl[k][free[2::7]] = 2
    if diverging:
        cl[2] = R.c_vertical_pair(g)["classes"]
    assert [bool(R.linear_pairs(c, g)) for c in cl] == [False, False, bool(diverging), False, False, False]
    return np.stack([R.paint(c, NCH) for c in cl])


def test_strict_one_frame_diverges(eng, oracle):
    import yolact_amd as ya
    cells = _strict_cells(True)
    eng.op_classify_post_batch(_strict_cells(False), W, H, ya.COMPAT_STRICT)     # a batch to lose
    assert eng.classify_batch_device_frames()
    out = np.full((3, H, W), 0xDEADBEEF, np.uint32)
    with pytest.raises(ya.YhError) as e:
        eng.op_classify_post_batch(cells, W, H, ya.COMPAT_STRICT, out=out)
    assert e.value.code == ya.EDIVERGE and e.value.diverged.tolist() == [0, 1, 0]
    assert (out == 0xDEADBEEF).all() and not eng.classify_batch_device_frames()
    for b in range(3):
        assert oracle.classify_post(cells[2 * b:2 * b + 2], S, NCH, ya.COMPAT_STRICT, W, H)[0] == (1 if b == 1 else 0)
    got, div = eng.op_classify_post_batch(cells, W, H, ya.COMPAT_SANE)           # the same cells are fine in SANE
    assert not div.any()
    for b in range(3):
        rc, want = oracle.classify_post(cells[2 * b:2 * b + 2], S, NCH, ya.COMPAT_SANE, W, H)
        assert rc == 0 and np.array_equal(got[b].reshape(-1), want), b


def test_strict_terminating_batch(eng, oracle):
    import yolact_amd as ya
    cells = _strict_cells(False)
    got, div = eng.op_classify_post_batch(cells, W, H, ya.COMPAT_STRICT)
    assert not div.any() and eng.classify_batch_device_frames()
    for b in range(3):
        rc, want = oracle.classify_post(cells[2 * b:2 * b + 2], S, NCH, ya.COMPAT_STRICT, W, H)
        assert rc == 0 and np.array_equal(got[b].reshape(-1), want) and want.any(), b
        assert (oracle.consumer_low16(got[b]) == 0).all()


@pytest.mark.parametrize("w,h", [(W, H), (449, 223), (97, 61)])
def test_sane_ids_saturate(eng, oracle, w, h):
    """Grid 28 holds what the small engines of the edge file cannot: a checkerboard of 392 one-cell components (ids 0 .. 126, then
    127) beside robots and background (id byte 0xFF), through the batch's post kernel at three sizes, four frames."""
    import yolact_amd as ya
    g = S // 8
    tiles = []
    for t in range(8):
        cl = np.roll(R.checker(g).reshape(g, g), t, axis=1).reshape(-1).copy()
        free = np.nonzero(cl == 0)[0]
        cl[free[t::3]] = 1 + t % 2
        tiles.append(R.paint(cl, NCH))
    cells = np.stack(tiles)
    got, div = eng.op_classify_post_batch(cells, w, h, ya.COMPAT_SANE)
    assert not div.any()
    for b in range(4):
        rc, want = oracle.classify_post(cells[2 * b:2 * b + 2], S, NCH, ya.COMPAT_SANE, w, h)
        assert rc == 0 and np.array_equal(got[b].reshape(-1), want), b
    if (w, h) == (W, H):
        ids = (got >> 16) & 0xFF
        assert set(range(128)) | {0xFF} <= set(np.unique(ids).tolist())


def test_a_batch_of_four_is_not_slower_than_four_single_frames(eng, frames):
    """A condition, not a measurement (tools/time_classify.py --batch measures): in this process, on this engine, after warm-up, the
    median of 10 classify_batch calls on 4 frames (host in, host out) is below 4 x the median of 10 classify_frame calls. No margin."""
    import yolact_amd as ya
    four = np.concatenate([frames, frames[:1]])
    out = np.empty_like(four)
    one = frames[0].copy().reshape(-1)

    def batch():
        eng.classify_batch(frames_u32=four, width=W, height=H, mode=ya.COMPAT_SANE, out=out)

    def single():
        one[:] = frames[0].reshape(-1)
        eng.classify_frame(one, W, H, ya.COMPAT_SANE)

    def clock(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

    for _ in range(3):
        batch(); single()
    tb = sorted(clock(batch) for _ in range(10))
    ts = sorted(clock(single) for _ in range(10))
    mb, ms = (tb[4] + tb[5]) / 2, 4 * (ts[4] + ts[5]) / 2
    print(f"classify of 4 frames 640x480: batch {mb:.3f} ms, 4 x single {ms:.3f} ms, ratio {mb / ms:.3f}")
    assert mb < ms
