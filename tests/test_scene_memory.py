"""The scene memory (DESIGN.md §11 "Scene memory"): yh_scene_append_memory carries the height map and the balls of a yh_scene from
frame to frame by the robot's motion. CPU part: the numpy restatement (tests/scene_memory_ref.py) pinned to the oracle's connection
fields and to known answers worked out by hand; the binding's surface. GPU part (-m gpu): every output of the library against
the restatement, bit for bit, with the frame's stamps and balls taken from the oracle."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import scene_memory_ref as R
from test_scene import _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
Q = 65536


def shift(dx, dy):
    """(gather, carry) of a map that moved by (dx, dy) pixels"""
    return (Q, 0, -dx * Q, 0, Q, -dy * Q), (Q, 0, dx * Q, 0, Q, dy * Q)


def turn90(px, py):
    """the exact quarter turn about (px, py): carry (x, y) -> (px - (y - py), py + (x - px))"""
    return (0, Q, (px - py) * Q, -Q, 0, (px + py) * Q), (0, -Q, (px + py) * Q, Q, 0, (py - px) * Q)


IDENT = (R.IDENTITY, R.IDENTITY)


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------------

def test_restated_fields_equal_the_oracle(oracle):
    for H, W, seed in ((37, 53, 1), (3, 3, 2), (8, 8, 3), (100, 9, 4)):
        depth, ci = _frame(np.random.default_rng(seed), H, W)
        want = oracle.scene(depth, ci, mode=1)
        world, conn0, conn1 = R.fields(want["map"])
        for name, got in (("world", world), ("conn0", conn0), ("conn1", conn1)):
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), (name, H, W)
    assert want["map"].max() > 0


def test_carry_fade_fuse_known_answers():
    H, W = 5, 7
    M = np.arange(1, H * W + 1, dtype=np.uint32).reshape(H, W) * 10
    Z = np.zeros_like(M)
    assert np.array_equal(R.fuse(Z, M, R.IDENTITY, 256), M)                       # identity, no fading
    assert np.array_equal(R.fuse(Z, M, R.IDENTITY, 128), M // 2) and not R.fuse(Z, M, R.IDENTITY, 0).any()
    N = Z.copy(); N[2, 3] = 1000; N[0, 0] = 1
    F = R.fuse(N, M, R.IDENTITY, 256)
    assert F[2, 3] == 1000 and F[0, 0] == 10 and F[4, 6] == 350                   # max with the stamps
    g, _ = shift(3, -2)                                                           # what was at (x, y) is now at (x + 3, y - 2)
    F = R.fuse(Z, M, g, 256)
    assert np.array_equal(F[:H - 2, 3:], M[2:, :W - 3]) and not F[H - 2:].any() and not F[:, :3].any()
    g, c = turn90(3, 2)
    F = R.fuse(Z, M, g, 256)
    for y in range(H):
        for x in range(W):
            cx, cy = R.affine(c, x, y)
            assert (cx, cy) == (3 - (y - 2), 2 + (x - 3))
            if 0 <= cx < W and 0 <= cy < H:
                assert F[cy, cx] == M[y, x] and R.affine(g, cx, cy) == (x, y)
    assert int((F > 0).sum()) == sum(0 <= 3 - (y - 2) < W and 0 <= 2 + (x - 3) < H for y in range(H) for x in range(W))
    # floor, not truncation: half a pixel to the left of pixel 0 rounds to -1 (outside), a quarter rounds to 0
    assert R.affine((Q, 0, -Q // 2 - 1, 0, Q, 0), 0, 0) == (-1, 0) and R.affine((Q, 0, -Q // 4, 0, Q, 0), 0, 0) == (0, 0)
    assert R.affine((Q, 0, -3 * Q // 2, 0, Q, -3 * Q // 2 - 1), 0, 0) == (-1, -2)      # -1.5 -> -1 (round half up), just below -> -2
    F = R.fuse(Z, M, (Q // 2, 0, -Q // 2 - 1, 0, Q, 0), 256)                      # sx = floor(x / 2 - 0.5 - eps + 0.5): -1, 0, 0, 1, 1, ..
    assert not F[:, 0].any() and np.array_equal(F[:, 1:], M[:, [0, 0, 1, 1, 2, 2]])
    # the 64-bit path: coefficients at the ends of int32 neither wrap nor index
    ext = (I32_MAX, I32_MIN, 0, I32_MIN, I32_MAX, 0)
    assert R.affine(ext, 5, 5) == (0, 0) and R.affine(ext, 6, 5) == (32768, -32768) and R.affine(ext, 8191, 0)[0] == (I32_MAX * 8191 + 32768) >> 16
    F = R.fuse(Z, M, ext, 256)
    assert all(F[i, i] == M[0, 0] for i in range(H)) and int((F > 0).sum()) == H
    # keep = 255 takes ceil(v / 256) off a value per frame, so it reaches 0 and no fixed point: 300 -> 298 -> .. -> 256 in 22 steps
    # of two, then 256 steps of one
    for v0, want in ((200, 200), (300, 278)):
        steps, m = 0, np.full((1, 1), v0, np.uint32)
        while m[0, 0]:
            m = R.fuse(np.zeros((1, 1), np.uint32), m, R.IDENTITY, 255)
            steps += 1
        assert steps == want


def test_ball_rules_every_branch():
    W, H = 40, 30
    fb = np.zeros((100, 4), np.float32)
    fb[7] = (12.75, 20.5, 9, 0); fb[99] = (3.0, 4.0, 2, 0)
    B, out = R.balls_step(np.zeros((100, 4), np.int32), fb, R.IDENTITY, 3, W, H)                    # seen
    assert B[7].tolist() == [12, 20, 9, 0] and B[99].tolist() == [3, 4, 2, 0] and np.array_equal(out, fb) and int((B[:, 2] > 0).sum()) == 2
    none = np.zeros((100, 4), np.float32)
    _, c = shift(30, 0)
    B1, out = R.balls_step(B, none, c, 3, W, H)                                                     # carried out of the frame: kept, not shown
    assert B1[7].tolist() == [42, 20, 9, 1] and not out[7].any() and B1[99].tolist() == [33, 4, 2, 1] and out[99].tolist() == [33, 4, 2, 0]
    _, c = shift(-30, 0)
    B2, out = R.balls_step(B1, none, c, 3, W, H)                                                    # carried back in: shown with its age so far
    assert B2[7].tolist() == [12, 20, 9, 2] and out[7].tolist() == [12, 20, 9, 1]
    B3, out = R.balls_step(B2, none, R.IDENTITY, 3, W, H)                                           # age + 1 == max_age: still kept
    assert B3[7].tolist() == [12, 20, 9, 3] and out[7].tolist() == [12, 20, 9, 2]
    B4, out = R.balls_step(B3, none, R.IDENTITY, 3, W, H)                                           # aged out
    assert not B4.any() and not out.any()
    fb2 = none.copy(); fb2[7] = (1.0, 2.0, 4, 0)
    B5, out = R.balls_step(B2, fb2, R.IDENTITY, 3, W, H)                                            # seen again: the frame wins, age 0
    assert B5[7].tolist() == [1, 2, 4, 0] and out[7].tolist() == [1, 2, 4, 0] and B5[99, 3] == 3
    B6, out = R.balls_step(B, none, R.IDENTITY, 0, W, H)                                            # max_age 0 remembers nothing
    assert not B6.any() and not out.any()
    # the 2^20 limit, on 64-bit values: x' = 16384 x is 2^20 for x = 64 (cleared) and 2^20 - 16384 for x = 63 (kept, outside the frame)
    Bx = np.zeros((100, 4), np.int32)
    Bx[7] = (64, 4, 9, 0); Bx[99] = (63, 4, 2, 0)
    for sign in (1, -1):
        B7, out = R.balls_step(Bx, none, (sign * (1 << 30), 0, 0, 0, Q, 0), 3, W, H)
        assert not B7[7].any() and B7[99].tolist() == [sign * 63 * 16384, 4, 2, 1] and not out.any()
    B8, out = R.balls_step(B, none, (I32_MIN, I32_MIN, I32_MIN, I32_MAX, I32_MAX, I32_MAX), 3, W, H)
    assert not B8[7].any() and B8[99].tolist() == [-262144, 262144, 2, 1] and not out.any()     # x' = -2^31 * 33 / 2^16 for id 7: past the limit


def test_scene_motion():
    from yolact_amd import scene_motion
    assert scene_motion() == (list(R.IDENTITY), list(R.IDENTITY))
    g, c = scene_motion(3, -2)
    assert (tuple(g), tuple(c)) == shift(3, -2)
    g, c = scene_motion(0, 0, math.pi / 2, pivot=(3, 2))
    assert (tuple(g), tuple(c)) == turn90(3, 2)
    g, c = scene_motion(0, 0, math.pi / 2)
    assert (tuple(g), tuple(c)) == turn90(400, 479)                              # the default pivot: START_NODE of a 640 x 480 frame
    assert scene_motion(0, 0, math.pi / 2, size=(64, 32)) == tuple(list(m) for m in turn90(40, 31))
    rng = np.random.default_rng(5)
    for _ in range(50):
        g, c = scene_motion(rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(-math.pi, math.pi), pivot=(int(rng.integers(0, 640)), int(rng.integers(0, 480))))
        assert all(I32_MIN <= v <= I32_MAX for v in g + c)
        for _ in range(20):
            x, y = int(rng.integers(0, 640)), int(rng.integers(0, 480))
            bx, by = R.affine(c, *R.affine(g, x, y))
            assert abs(bx - x) <= 1 and abs(by - y) <= 1


def test_surface(built):
    from yolact_amd import capi
    L = capi.load_library()
    pub = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read()
    protos = dict((s[0], s) for s in capi.SYMBOLS)
    _i, _vp = capi.C.c_int32, capi.C.c_void_p
    assert protos["yh_scene_append_memory"][1:] == (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i])
    assert protos["yh_scene_memory_read"][1:] == (_i, [_vp, _vp, _vp]) and protos["yh_scene_memory_reset"][1:] == (_i, [_vp])
    assert protos["yh_scene_memory_time"][1:] == (_i, [_vp, _i, capi.C.POINTER(capi.C.c_float)])
    for name in ("yh_scene_append_memory", "yh_scene_memory_read", "yh_scene_memory_reset"):
        assert hasattr(L, name) and re.search(r"\bint %s\(yh_scene\* h" % name, pub), name
    assert hasattr(L, "yh_scene_memory_time") and "yh_scene_memory_time" not in pub and re.search(r"\bint yh_scene_memory_time\(yh_scene\* h, int32_t reps, float\* ms_per_frame\);", dbg)
    assert re.search(r"int yh_scene_append_memory\(yh_scene\* h, const uint16_t\* depth_host, const uint32_t\* frame, int32_t frame_on_device,\s*"
                     r"const int32_t\* gather_q16 /\* \[6\] \*/, const int32_t\* carry_q16 /\* \[6\] \*/, int32_t keep, int32_t ball_max_age\);", pub)
    assert "yh_instance_track" in pub[pub.index("---- scene memory"):pub.index("int yh_scene_append_memory")]   # ids mean something only as track ids
    sig = inspect.signature(capi.Scene.append_memory)
    assert list(sig.parameters) == ["self", "depth", "frame_u32", "frame_dev_ptr", "cls_id", "motion", "keep", "ball_max_age"]
    assert [sig.parameters[k].default for k in ("frame_u32", "frame_dev_ptr", "cls_id", "motion", "keep", "ball_max_age")] == [None, None, None, None, 224, 30]
    assert list(inspect.signature(capi.Scene.read_memory).parameters) == ["self"] and list(inspect.signature(capi.Scene.memory_reset).parameters) == ["self"]
    assert inspect.signature(capi.Scene.memory_time).parameters["reps"].default == 20
    assert list(inspect.signature(capi.scene_motion).parameters)[:4] == ["dx", "dy", "dtheta", "pivot"]
    cfg = capi.Config()
    L.yh_default_config(cfg)
    assert cfg.abi_version == 4


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

_ORACLE = {}


def _stamps(oracle, H, W, seed, balls=True):
    """(depth, class image, the oracle's SANE frame) of _frame(seed), computed once"""
    key = (H, W, seed, balls)
    if key not in _ORACLE:
        depth, ci = _frame(np.random.default_rng(seed), H, W, balls)
        _ORACLE[key] = (depth, ci, oracle.scene(depth, ci, mode=1))
    return _ORACLE[key]


def _same(got, want, what):
    for k in ("map", "balls", "world", "conn1", "conn0"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k,) + tuple(what)


def _same_memory(sc, ref, what):
    mem = sc.read_memory()
    assert np.array_equal(mem["map"], ref.M) and np.array_equal(mem["balls"], ref.B), what


def _motions(H, W):
    px, py = (W * 5) // 8, H - 1
    out_of_frame = ((Q, 0, 2 * W * Q, 0, Q, 0), (Q, 0, -2 * W * Q, 0, Q, 0))
    rotation = ((65209, 6543, -40000, -6543, 65209, 90000), (65209, -6543, 48785, 6543, 65209, -85560))
    sheared = ((Q // 2, Q // 4, 0, 0, Q // 2, Q), (2 * Q, -Q, 2 * Q, 0, 2 * Q, -2 * Q))
    return {
        "identity": [IDENT, IDENT, IDENT],
        "shift": [IDENT, shift(3, -2), shift(3, -2)],
        "turn90": [IDENT, turn90(px, py), turn90(px // 2, py // 2)],
        # about 0.1 rad (cos, sin = 65209, 6543 in q16) and a translation, gather and carry written out
        "rotation": [IDENT, rotation, rotation],
        # not rigid: gather halves and shears, carry doubles and shears back
        "affine": [IDENT, sheared, sheared],
        "outside": [IDENT, out_of_frame, out_of_frame],
        # a shift that brings remembered heights to the pixel (0, 0) the extreme gather reads on its diagonal, then int32's ends
        "int32_ends": [IDENT, shift(-min(W, H) // 2, -min(W, H) // 2), ((I32_MAX, I32_MIN, 0, I32_MIN, I32_MAX, 0), (I32_MIN, I32_MAX, I32_MIN, I32_MAX, I32_MIN, I32_MAX)),
                       ((I32_MAX, I32_MAX, I32_MAX, I32_MIN, I32_MIN, I32_MIN), (I32_MAX, I32_MAX, I32_MAX, I32_MAX, I32_MAX, I32_MAX))],
    }


def _run_sequence(built, oracle, H, W, name):
    import yolact_amd as ya
    sc, ref = ya.Scene(W, H), R.Memory(W, H)
    for t, (g, c) in enumerate(_motions(H, W)[name]):
        depth, ci, o = _stamps(oracle, H, W, 10 * H + W + t, balls=t != 1)    # the second frame has no ball: those of the first are remembered
        keep = (256, 224, 200, 255)[t]
        sc.append_memory(depth, cls_id=ci, motion=(g, c), keep=keep, ball_max_age=5)
        want = ref.append(o["map"], o["balls"], g, c, keep, 5)
        _same(sc.read(), want, (name, H, W, t))
        _same_memory(sc, ref, (name, H, W, t))
    sc.close()
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["identity", "shift", "turn90", "rotation", "affine", "outside", "int32_ends"])
@pytest.mark.parametrize("H,W", [(8, 8), (3, 3), (37, 53), (100, 9)])
def test_memory_sequences_match_the_restatement(built, oracle, H, W, name):
    ref = _run_sequence(built, oracle, H, W, name)
    if name in ("identity", "shift", "rotation") and H >= 37:
        # the sequence did carry something: the memory holds more than the last frame's own stamps
        assert (ref.M > _stamps(oracle, H, W, 10 * H + W + 2)[2]["map"]).any()


@pytest.mark.gpu
def test_memory_sequence_at_the_camera_size(built, oracle):
    _run_sequence(built, oracle, 480, 640, "rotation")


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (37, 53)])
def test_empty_memory_or_nothing_kept_is_a_plain_append(built, oracle, H, W):
    import yolact_amd as ya
    d0, c0, _ = _stamps(oracle, H, W, 1)
    d1, c1, _ = _stamps(oracle, H, W, 2)
    mem, plain = ya.Scene(W, H), ya.Scene(W, H)
    mem.append_memory(d0, cls_id=c0, motion=shift(1, 1), keep=256, ball_max_age=255)       # empty memory
    plain.append_classified(d0, frame_u32=ya.SceneBatch.pack(c0), mode=ya.COMPAT_SANE)
    _same(mem.read(), plain.read(), ("empty", H, W))
    mem.append_memory(d1, cls_id=c1, motion=IDENT, keep=0, ball_max_age=0)                 # a full memory, nothing of it kept
    plain.append_classified(d1, frame_u32=ya.SceneBatch.pack(c1), mode=ya.COMPAT_SANE)
    _same(mem.read(), plain.read(), ("keep 0", H, W))
    assert plain.read()["map"].max() > 0
    mem.close(); plain.close()


@pytest.mark.gpu
def test_the_same_frame_twice_changes_nothing(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    d0, c0, _ = _stamps(oracle, H, W, 1)
    d1, c1, _ = _stamps(oracle, H, W, 2)
    sc = ya.Scene(W, H)
    sc.append_memory(d0, cls_id=c0, keep=256)
    sc.append_memory(d1, cls_id=c1, keep=256)
    first, mem = sc.read(), sc.read_memory()
    sc.append_memory(d1, cls_id=c1, keep=256)
    _same(sc.read(), first, ("twice",))
    again = sc.read_memory()
    assert np.array_equal(again["map"], mem["map"]) and np.array_equal(again["balls"], mem["balls"])
    sc.close()


def _ball_frame(rng, H, W, ids):
    depth = rng.integers(200, 4000, (H, W)).astype(np.uint16)
    ci = np.zeros((H, W, 2), np.uint8)
    for n, k in enumerate(ids):
        ci[4 + 5 * n:8 + 5 * n, 6 + 3 * n:11 + 3 * n] = (3, k)
    return depth, ci


@pytest.mark.gpu
def test_a_ball_is_seen_remembered_carried_out_and_back_and_aged_out(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    rng = np.random.default_rng(11)
    sc, ref = ya.Scene(W, H), R.Memory(W, H)
    seen, unseen = _ball_frame(rng, H, W, (7, 99, 100, 150)), _ball_frame(rng, H, W, ())
    steps = [(seen, IDENT), (unseen, IDENT), (unseen, shift(100, 0)), (unseen, shift(-100, 0)), (unseen, IDENT), (unseen, IDENT), (seen, IDENT)]
    rows = []
    for t, ((depth, ci), (g, c)) in enumerate(steps):
        o = oracle.scene(depth, ci, mode=1)
        sc.append_memory(depth, cls_id=ci, motion=(g, c), keep=200, ball_max_age=4)
        want = ref.append(o["map"], o["balls"], g, c, 200, 4)
        got = sc.read()
        _same(got, want, ("balls", t))
        _same_memory(sc, ref, ("balls", t))
        rows.append((got["balls"].copy(), sc.read_memory()["balls"].copy()))
    for k in (7, 99):
        (b0, m0), (b1, m1), (b2, m2), (b3, m3), (b4, m4), (b5, m5), (b6, m6) = ((b[k], m[k]) for b, m in rows)
        assert b0[2] > 0 and m0.tolist() == [int(b0[0]), int(b0[1]), int(b0[2]), 0]                              # seen
        assert b1.tolist() == [m0[0], m0[1], m0[2], 0] and m1.tolist() == [m0[0], m0[1], m0[2], 1]               # remembered where it was
        assert not b2.any() and m2.tolist() == [m0[0] + 100, m0[1], m0[2], 2]                                    # behind the robot: kept, not shown
        assert b3.tolist() == [m0[0], m0[1], m0[2], 2] and m3[3] == 3                                            # back
        assert b4[3] == 3 and m4[3] == 4 and not b5.any() and not m5.any()                                       # the last frame it is kept, then gone
        assert np.array_equal(b6, b0) and np.array_equal(m6, m0)
    assert int((rows[0][1][:, 2] > 0).sum()) == 2 and int((rows[0][0][:, 2] > 0).sum()) == 2                     # ids 100 and 150: ignored
    sc.close()


class _DeviceFrame:
    """A packed frame in device memory of its own (the HIP runtime the library has loaded, through ctypes)."""

    def __init__(self, frame):
        import ctypes as C
        path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), "libamdhip64.so")
        self.hip, self.ptr = C.CDLL(path), C.c_void_p()
        frame = np.ascontiguousarray(frame, np.uint32)
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(frame.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, frame.ctypes.data_as(C.c_void_p), C.c_size_t(frame.nbytes), 1) == 0   # hipMemcpyHostToDevice

    def free(self):
        assert self.hip.hipFree(self.ptr) == 0


@pytest.mark.gpu
def test_frame_from_a_device_pointer_and_from_the_host(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    host, dev, ref = ya.Scene(W, H), ya.Scene(W, H), R.Memory(W, H)
    for t in range(2):
        depth, ci, o = _stamps(oracle, H, W, 20 + t)
        frame = ya.SceneBatch.pack(ci)
        on_dev = _DeviceFrame(frame)
        host.append_memory(depth, frame_u32=frame, motion=shift(2, 1))
        dev.append_memory(depth, frame_dev_ptr=on_dev.ptr.value, motion=shift(2, 1))
        want = ref.append(o["map"], o["balls"], *shift(2, 1))
        _same(host.read(), want, ("host", t))
        _same(dev.read(), want, ("device", t))
        _same_memory(dev, ref, ("device", t))
        assert dev.memory_time(2) > 0                                            # the replay reads the device frame again: still valid
        _same(dev.read(), want, ("device, replayed", t))
        on_dev.free()
    host.close(); dev.close()


@pytest.mark.gpu
def test_planners_run_on_the_fused_frame_and_a_remembered_ball(built, oracle):
    import yolact_amd as ya
    H, W = 33, 65
    start = ((W * 5) // 8, H - 1)
    d0, c0, _ = _stamps(oracle, H, W, 31)
    d1, c1, o1 = _stamps(oracle, H, W, 32, balls=False)
    sc, other = ya.Scene(W, H), ya.Scene(W, H)
    sc.append_memory(d0, cls_id=c0)
    sc.append_memory(d1, cls_id=c1, motion=shift(2, -1), keep=240)
    f = sc.read()
    assert not o1["balls"].any() and (f["balls"][:, 2] > 0).sum() >= 1 and (f["map"] > o1["map"]).any()          # balls only remembered, map fused
    remembered = [(int(b[0]), int(b[1])) for b in f["balls"] if b[2] > 0]
    assert sc.read_memory()["balls"][5, 3] == 1 and all(0 <= x < W and 0 <= y < H for x, y in remembered)
    other.set_fields(f["map"], f["conn0"], f["conn1"])
    same = lambda a, b, what: [np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}") for k in a] and None
    for targets in (remembered, None):
        for conn in (4, 8):
            sc.plan(targets, n_targets=3, start=start, connectivity=conn)
            other.plan(remembered[:3], start=start, connectivity=conn)
            same(sc.read_plan(), other.read_plan(), f"plan {conn} {targets}")
        sc.plan_turn(targets, n_targets=3, start=start, heading=6, turn_price=2.0)
        other.plan_turn(remembered[:3], start=start, heading=6, turn_price=2.0)
        same(sc.read_turn(), other.read_turn(), f"turn {targets}")
    sc.plan_tour(remembered, start=start, connectivity=8)
    other.plan_tour(remembered, start=start, connectivity=8)
    same(sc.read_tour(fields=True), other.read_tour(fields=True), "tour")
    sc.close(); other.close()


@pytest.mark.gpu
def test_plain_appends_fields_and_reset_leave_or_empty_the_memory(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    sc, ref = ya.Scene(W, H), R.Memory(W, H)
    zero = sc.read_memory()
    assert not zero["map"].any() and not zero["balls"].any() and zero["balls"].shape == (100, 4)                 # before any memory append
    sc.memory_reset()
    d0, c0, o0 = _stamps(oracle, H, W, 41)
    d1, c1, o1 = _stamps(oracle, H, W, 42)
    d2, c2, o2 = _stamps(oracle, H, W, 43, balls=False)
    sc.append_memory(d0, cls_id=c0, keep=250)
    ref.append(o0["map"], o0["balls"], keep=250)
    sc.append(d1, c1, ya.COMPAT_SANE)
    _same(sc.read(), o1, ("plain append after a memory append",))
    _same_memory(sc, ref, "append")
    sc.append_classified(d1, frame_u32=ya.SceneBatch.pack(c1), mode=ya.COMPAT_STRICT)
    f = sc.read()
    sc.set_fields(o1["map"], o1["conn0"], o1["conn1"])
    sc.plan([(5, 5)], start=(1, 1))
    _same_memory(sc, ref, "append_classified, set_fields, plan")
    sc.append_memory(d2, cls_id=c2, motion=shift(1, 0), keep=250)                                                # the chain goes on from frame 0
    want = ref.append(o2["map"], o2["balls"], *shift(1, 0), keep=250)
    _same(sc.read(), want, ("after plain appends",))
    _same_memory(sc, ref, "chain")
    assert ref.M.max() > 0 and (ref.B[:, 2] > 0).any() and f["map"].max() > 0
    ms = sc.memory_time(3)                                                                                       # the replay commits nothing
    assert ms > 0
    _same_memory(sc, ref, "memory_time")
    _same(sc.read(), want, ("memory_time",))
    sc.memory_reset()
    ref.reset()
    _same_memory(sc, ref, "reset")
    with pytest.raises(ya.YhError) as e:
        sc.memory_time(1)
    assert e.value.code == ya.capi.ESTATE
    sc.append_memory(d1, cls_id=c1, motion=shift(1, 0))
    _same(sc.read(), o1, ("after reset",))
    sc.close()


@pytest.mark.gpu
def test_refusals_touch_nothing_and_scene_time_names_the_memory_hook(built, oracle):
    import ctypes as C
    import yolact_amd as ya
    from yolact_amd.capi import _p
    H, W = 37, 53
    start = ((W * 5) // 8, H - 1)
    d0, c0, _ = _stamps(oracle, H, W, 51)
    d1, c1, _ = _stamps(oracle, H, W, 52)
    sc = ya.Scene(W, H)
    sc.append_memory(d0, cls_id=c0)
    sc.plan(None, start=start)
    before, mem, plan = sc.read(), sc.read_memory(), sc.read_plan()
    for kw in (dict(keep=-1), dict(keep=257), dict(ball_max_age=-1), dict(ball_max_age=256)):
        with pytest.raises(ya.YhError) as e:
            sc.append_memory(d1, cls_id=c1, motion=shift(1, 1), **kw)
        assert e.value.code == ya.capi.EINVAL, kw
    frame, g = ya.SceneBatch.pack(c1), np.array(R.IDENTITY, np.int32)
    full = [sc.h, _p(d1), _p(frame), 0, _p(g), _p(g), 224, 30]
    for hole in (0, 1, 2, 4, 5):
        args = list(full)
        args[hole] = None
        assert sc.L.yh_scene_append_memory(*args) == ya.capi.EINVAL, hole
    assert sc.L.yh_scene_memory_read(None, None, None) == ya.capi.EINVAL and sc.L.yh_scene_memory_reset(None) == ya.capi.EINVAL
    ms = C.c_float()
    assert sc.L.yh_scene_memory_time(sc.h, 0, C.byref(ms)) == ya.capi.EINVAL and sc.L.yh_scene_memory_time(sc.h, 1, None) == ya.capi.EINVAL
    _same(sc.read(), before, ("refused",))
    after = sc.read_memory()
    assert np.array_equal(after["map"], mem["map"]) and np.array_equal(after["balls"], mem["balls"])
    again = sc.read_plan()                                                                                       # not a new frame: the plan is still readable
    assert all(np.array_equal(again[k], plan[k]) for k in plan)
    with pytest.raises(ya.YhError) as e:
        sc.time(2)
    assert e.value.code == ya.capi.ESTATE and "yh_scene_memory_time" in str(e.value)
    sc.append_memory(d1, cls_id=c1)                                                                              # a new frame: the plan is of an earlier one
    with pytest.raises(ya.YhError) as e:
        sc.read_plan()
    assert e.value.code == ya.capi.ESTATE
    sc.append(d1, c1, ya.COMPAT_SANE)                                                                            # yh_scene_time is what it was for plain frames
    assert sc.time(2) > 0
    sc.close()


@pytest.mark.gpu
def test_memory_append_costs_no_more_than_a_plain_append(built):
    """At 640 x 480, on the terrain-only and the robots + balls frame of tools/time_scene.py, in this process: yh_scene_memory_time
    against yh_scene_time, alternated, one warm-up each, the median of five runs of 30 frames.
    Ceiling 1.016, from profiles/scene_memory_timings.txt (2026-10-19): the largest ratio of the two tables, 0.982, plus the largest
    run-to-run spread of the plain append in those runs, 0.4 %, plus the 3 % by which the pool's boxes differ (the two figures of a
    ratio come from one box, but how the fuse launch and the three it replaces share a box's clocks need not be the same on another)."""
    import yolact_amd as ya
    H, W = 480, 640
    depth = np.random.default_rng(0).integers(200, 4000, (H, W)).astype(np.uint16)
    plain, mem = ya.Scene(W, H), ya.Scene(W, H)
    motion = ya.scene_motion(3.0, -2.0, 0.05)
    for name, robots in (("terrain only", False), ("robots + balls", True)):
        ci = np.zeros((H, W, 2), np.uint8)
        if robots:
            ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
        plain.append(depth, ci, ya.COMPAT_SANE)
        mem.append_memory(depth, cls_id=ci, motion=motion)
        mem.append_memory(depth, cls_id=ci, motion=motion)                       # replayed: this frame fused into a filled memory
        plain.time(30); mem.memory_time(30)
        tp, tm = [], []
        for _ in range(5):
            tp.append(plain.time(30)); tm.append(mem.memory_time(30))
        ratio = float(np.median(tm) / np.median(tp))
        print(f"scene 640x480, {name}: plain {np.median(tp):.4f} ms, memory {np.median(tm):.4f} ms, ratio {ratio:.3f}")
        assert ratio <= 1.016, (name, tp, tm)
    plain.close(); mem.close()
