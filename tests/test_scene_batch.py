"""The scene batch (yh_scene_batch, DESIGN.md §11 "Scene batch"): N frames appended and planned in one set of launches. The
definition is the single handle's: frame b of a batch equals, bit for bit, what a Scene gives when it is fed that frame alone -
every comparison here is array_equal (floats through their u32 view), against a Scene in the same process and, at the small sizes,
against the oracle and the planner's restatement (tests/path_ref.py). CPU part: the surface. GPU part (-m gpu): the equality, the
life cycle, every refusal, and a floor on time (a batch of eight must beat eight single frames)."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

import path_ref as R
from test_scene import _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ("yh_scene_batch_create", "yh_scene_batch_destroy", "yh_scene_batch_last_error", "yh_scene_batch_stage", "yh_scene_batch_append",
          "yh_scene_batch_read", "yh_scene_batch_plan", "yh_scene_batch_plan_read")
DEBUG = ("yh_scene_batch_time", "yh_scene_batch_plan_time", "yh_scene_batch_set_fields")
SP_BATCH = 16   # csrc/scene_path_dev.h: rounds enqueued per host read of the counters


# ---------------------------------------------------------------- CPU

def test_batch_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0] for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read(), flags=re.S)
    assert "typedef struct yh_scene_batch yh_scene_batch;" in pub
    for name in PUBLIC:
        assert re.search(r"\b%s\s*\(" % name, pub) and name in bound, name
    for name in DEBUG:
        assert re.search(r"\b%s\s*\(" % name, dbg) and not re.search(r"\b%s\s*\(" % name, pub) and name in bound, name
    assert "#define YH_ABI_VERSION 4" in pub


def test_scene_batch_class_has_the_methods():
    import yolact_amd as ya
    from yolact_amd import capi
    assert ya.SceneBatch is capi.SceneBatch
    for m in ("stage", "append", "read", "plan", "read_plan", "time", "plan_time", "set_fields", "close"):
        assert callable(getattr(capi.SceneBatch, m)), m


def test_packing_of_a_class_id_image():
    """class << 24 | id << 16 | id << 8 | class: STRICT reads class = bits 7-0, id = bits 15-8, SANE class = bits 31-24, id = bits 23-16."""
    from yolact_amd import capi
    rng = np.random.default_rng(5)
    ci = rng.integers(0, 256, (7, 9, 2), dtype=np.uint8)
    got = capi.SceneBatch.pack(ci)
    c, i = ci[..., 0].astype(np.uint32), ci[..., 1].astype(np.uint32)
    assert got.dtype == np.uint32 and got.shape == (7, 9) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, c << 24 | i << 16 | i << 8 | c)
    assert np.array_equal(got & 255, c) and np.array_equal((got >> 8) & 255, i) and np.array_equal(got >> 24, c) and np.array_equal((got >> 16) & 255, i)


# ---------------------------------------------------------------- GPU

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _frames(H, W, n, seed, balls=None):
    """n frames of test_scene._frame, a different seed per slot; balls[b] False: that frame has none."""
    return [_frame(np.random.default_rng(seed + 17 * b), H, W, balls=True if balls is None else balls[b]) for b in range(n)]


def _single(sc, depth, ci, mode):
    from yolact_amd import capi
    sc.append_classified(depth, frame_u32=capi.SceneBatch.pack(ci), mode=mode)
    return sc.read()


def _code(fn):
    from yolact_amd import capi
    try:
        fn()
    except capi.YhError as e:
        return e.code
    return 0


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,n,max_frames", [(8, 8, 2, 2), (37, 53, 3, 4), (100, 9, 2, 2), (480, 640, 2, 3)])
@pytest.mark.parametrize("mode", [0, 1])
def test_append_equals_the_single_handle_and_the_oracle(built, oracle, H, W, n, max_frames, mode):
    import yolact_amd as ya
    frames = _frames(H, W, n, 1000 * H + W + mode, balls=[b != 1 for b in range(n)])
    sb, sc = ya.SceneBatch(W, H, max_frames), ya.Scene(W, H)
    for b, (depth, ci) in enumerate(frames):
        sb.stage(b, depth, cls_id=ci)
    sb.append(n, mode)
    want = [_single(sc, d, ci, mode) for d, ci in frames]
    got = [sb.read(b) for b in range(n)]
    for b in range(n):
        assert _same(got[b], want[b]), (b, H, W, mode)
        if H < 480:
            ora = oracle.scene(*frames[b], mode)
            assert all(np.array_equal(_bits(got[b][k]), _bits(ora[k])) for k in ("map", "balls", "world", "conn1", "conn0")), (b, H, W, mode)
    assert got[0]["map"].max() > 0 and not got[1]["balls"].any() and (H < 100 or got[0]["balls"][5, 2] > 0)
    assert not np.array_equal(got[0]["balls"], got[1]["balls"]) and (H < 30 or not np.array_equal(got[0]["map"], got[1]["map"]))
    assert _code(lambda: sb.read(n)) == ya.capi.EINVAL
    # slot 1 restaged, slot 0 untouched: the new frame 1, the same frame 0 - state is reset per frame
    depth, ci = _frame(np.random.default_rng(7 + H), H, W)
    sb.stage(1, depth, frame_u32=ya.SceneBatch.pack(ci))
    sb.append(n, mode)
    assert _same(sb.read(0), want[0]) and _same(sb.read(1), _single(sc, depth, ci, mode))
    assert n < 3 or _same(sb.read(2), want[2])
    sb.close(); sc.close()


@pytest.mark.gpu
def test_device_frames_are_staged_before_the_next_instance_frame_overwrites_them(built):
    """Two noise frames evaluated, every class mapped to a ball or a robot: the instance frame of detection frame 0 is staged from the
    device, then yh_instance_frame paints detection frame 1 over it and that is staged. Both frames of the batch equal a Scene fed the
    host copies."""
    import yolact_amd as ya
    H, W = 480, 640
    eng = ya.Engine(input_size=550, backbone=50, max_batch=2, use_graph=False)
    eng.load_weights(eng.generate_weights(seed=1))
    eng.set_input(np.random.default_rng(5).integers(0, 256, (2, 550, 550, 3), dtype=np.uint8))
    eng.evaluate()
    cm = (np.arange(80) % 3 + 1).astype(np.uint8)
    sb, sc = ya.SceneBatch(W, H, 2), ya.Scene(W, H)
    depths = [_frame(np.random.default_rng(40 + b), H, W)[0] for b in range(2)]
    host = []
    for b in range(2):
        host.append(eng.instance_frame(b, W, H, class_map=cm).copy())
        sb.stage(b, depths[b], frame_dev_ptr=eng.instance_device_frame())
    assert host[0].any() and not np.array_equal(host[0], host[1])
    sb.append(2, ya.COMPAT_SANE)
    for b in range(2):
        sc.append_classified(depths[b], frame_u32=host[b], mode=ya.COMPAT_SANE)
        assert _same(sb.read(b), sc.read()), b
    sb.close(); sc.close(); eng.close()


def _single_plan(sc, targets, n_targets, start, conn):
    """Scene.plan + read_plan, or the error code of a refused plan."""
    import yolact_amd as ya
    try:
        sc.plan(targets=targets, n_targets=n_targets, start=start, connectivity=conn)
    except ya.YhError as e:
        return e.code
    return sc.read_plan()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,n", [(33, 65, 3), (96, 128, 4)])
@pytest.mark.parametrize("conn", [4, 8])
def test_plan_equals_the_single_handle(built, H, W, n, conn):
    import yolact_amd as ya
    frames = _frames(H, W, n, 100 * H + W, balls=[b != 1 for b in range(n)])
    frames[2][1][H // 8:H // 8 + 6, W // 8:W // 8 + 7] = 0           # frame 2 keeps one ball only (id 0): the frames' seed lists are ragged
    sb, sc = ya.SceneBatch(W, H, n), ya.Scene(W, H)
    for b, (depth, ci) in enumerate(frames):
        sb.stage(b, depth, cls_id=ci)
    sb.append(n, ya.COMPAT_SANE)
    fields = [_single(sc, d, ci, ya.COMPAT_SANE) for d, ci in frames]
    assert all(_same(sb.read(b), fields[b]) for b in range(n))
    # explicit targets: different per frame, frame 1 with a duplicated target, frame 0 starting on its own target
    targets = [[(3 + 5 * b, 4 + 3 * b), (W - 2 - b, H - 3 - 2 * b)] for b in range(n)]
    targets[1][1] = targets[1][0]
    starts = [targets[0][1]] + [(W // 2 + b, H - 1 - b) for b in range(1, n)]
    assert sb.plan(targets=targets, starts=starts, connectivity=conn) == [ya.capi.OK] * n
    for b in range(n):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        want, got = _single_plan(sc, targets[b], 0, starts[b], conn), sb.read_plan(b)
        assert _same(got, want), (b, conn)
        assert len(got["path"]) == (1 if b == 0 else len(want["path"])) and len(got["path"]) >= 1
        if (H, W, conn) == (33, 65, 4):
            f = fields[b]
            d = R.dijkstra(f["map"], f["conn0"], f["conn1"], targets[b])
            assert np.array_equal(_bits(got["cost"]), _bits(d)), b
            path, dirs = R.walk(d, R.successors(d, f["map"], f["conn0"], f["conn1"], targets[b]), starts[b])
            assert np.array_equal(got["path"], path) and np.array_equal(_bits(got["directions"]), _bits(dirs)), b
    # NULL targets: each frame's own balls; frame 1 has none - YH_ESTATE, no plan, the others are planned
    for n_targets in (3, 1):
        status = sb.plan(targets=None, n_targets=n_targets, starts=starts, connectivity=conn)
        assert status == [ya.capi.ESTATE if b == 1 else ya.capi.OK for b in range(n)]
        for b in range(n):
            sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
            want = _single_plan(sc, None, n_targets, starts[b], conn)
            if b == 1:
                assert want == ya.capi.ESTATE and _code(lambda: sb.read_plan(1)) == ya.capi.ESTATE
                continue
            got = sb.read_plan(b)
            assert _same(got, want), (b, conn, n_targets)
            want_targets = R.ball_targets(fields[b]["balls"], n_targets, W, H)
            assert len(want_targets) == (1 if b == 2 or n_targets == 1 else 2)
            assert sorted(map(tuple, np.argwhere(got["next"] == -1)[:, ::-1].tolist())) == sorted(set(want_targets))
    sb.close(); sc.close()


@pytest.mark.gpu
def test_frames_that_converge_at_different_rounds(built):
    """A flat map, the serpentine and a random field side by side: the serpentine takes more than SP_BATCH rounds, so the host loop
    goes round again while the other two frames have long converged. rounds counts the launches in which some tile of some frame
    ran: frames do not touch each other, so it is the largest of the frames' own counts - asserted as: at least the largest of the
    three single plans' and less than SP_BATCH above it (a frame's own count may differ between two runs of the asynchronous solver)."""
    import yolact_amd as ya
    S = 96
    serp, s_start, s_target = R.serpentine(S, S)
    maps = [np.zeros((S, S), np.uint32), serp, np.random.default_rng(3).integers(0, 40, (S, S)).astype(np.uint32)]
    targets, starts = [[(5, 7)], [s_target], [(50, 30)]], [(90, 80), s_start, (2, 93)]
    sb, sc = ya.SceneBatch(S, S, 4), ya.Scene(S, S)
    want, rounds = [], []
    for b in range(3):
        sc.set_fields(maps[b], *R.sane_connections(maps[b]))
        sc.plan(targets=targets[b], start=starts[b])
        want.append(sc.read_plan())
        rounds.append(sc.plan_time(1)["rounds"])
        sb.set_fields(b, maps[b], *R.sane_connections(maps[b]))
    print(f"single plans at {S}x{S}: rounds {rounds}")
    assert rounds[1] > SP_BATCH and rounds[0] < SP_BATCH and rounds[2] < SP_BATCH
    assert sb.plan(targets=targets, starts=starts) == [0, 0, 0]
    for b in range(3):
        assert _same(sb.read_plan(b), want[b]), b
    stats = sb.plan_time(1)
    print(f"batch of 3: {stats}")
    assert 0 <= stats["rounds"] - max(rounds) < SP_BATCH and stats["tile_runs"] >= stats["rounds"]
    for b in range(3):
        assert _same(sb.read_plan(b), want[b]), b
    # a frame below n without fields: refused
    sb2 = ya.SceneBatch(S, S, 3)
    sb2.set_fields(1, maps[1], *R.sane_connections(maps[1]))
    assert _code(lambda: sb2.plan(targets=[[(1, 1)], [(1, 1)]], starts=[(0, 0), (0, 0)])) == ya.capi.ESTATE
    sb.close(); sb2.close(); sc.close()


@pytest.mark.gpu
def test_life_cycle_and_refusals(built):
    import yolact_amd as ya
    from yolact_amd import capi
    from yolact_amd.capi import _p
    H, W = 40, 48
    frames = _frames(H, W, 2, 77)
    sc = ya.Scene(W, H)
    before = _single(sc, *frames[0], ya.COMPAT_SANE)
    sc.plan(targets=[(3, 3)], start=(40, 30))
    before_plan = sc.read_plan()
    for bad in (0, 257):
        with pytest.raises(ya.YhError) as e:
            ya.SceneBatch(W, H, bad)
        assert e.value.code == capi.EINVAL
    sb = ya.SceneBatch(W, H, 2)
    L, h = sb.L, sb.h
    starts = np.array([[40, 30], [10, 35]], np.int32)                       # (frame 0: the single plan above, its target given twice)
    tg = np.array([[[3, 3], [3, 3]], [[44, 2], [20, 9]]], np.int32)
    plan = lambda t=tg, s=starts, conn=4, k=2: L.yh_scene_batch_plan(h, None if t is None else _p(t), k, None if s is None else _p(s), conn, None)
    assert plan() == capi.ESTATE                                            # before any append
    assert _code(lambda: sb.read(0)) == capi.ESTATE and _code(lambda: sb.read_plan(0)) == capi.ESTATE
    assert _code(lambda: sb.stage(-1, frames[0][0], cls_id=frames[0][1])) == capi.EINVAL
    assert _code(lambda: sb.stage(2, frames[0][0], cls_id=frames[0][1])) == capi.EINVAL
    sb.stage(0, frames[0][0], cls_id=frames[0][1])
    assert _code(lambda: sb.append(2, ya.COMPAT_SANE)) == capi.ESTATE and b"slot 1" in L.yh_scene_batch_last_error(h)
    sb.stage(1, frames[1][0], cls_id=frames[1][1])
    assert _code(lambda: sb.append(0, ya.COMPAT_SANE)) == capi.EINVAL and _code(lambda: sb.append(3, ya.COMPAT_SANE)) == capi.EINVAL
    assert _code(lambda: sb.append(2, 2)) == capi.EINVAL
    assert _code(lambda: sb.read(0)) == capi.ESTATE                         # the refused appends ran nothing
    sb.append(2, ya.COMPAT_STRICT)
    assert plan() == capi.ESTATE and b"STRICT" in L.yh_scene_batch_last_error(h)
    sb.append(2, ya.COMPAT_SANE)
    fields = [sb.read(b) for b in range(2)]
    assert _same(fields[0], before)
    assert plan() == capi.OK
    p0, p1 = sb.read_plan(0), sb.read_plan(1)
    assert _same(p0, before_plan)
    bad = tg.copy(); bad[1, 1] = (W, 2)                                     # a target outside the frame, in frame 1 only
    assert plan(t=bad) == capi.EINVAL and b"frame 1" in L.yh_scene_batch_last_error(h)
    assert plan(conn=6) == capi.EINVAL and plan(s=None) == capi.EINVAL and plan(k=0) == capi.EINVAL
    out = starts.copy(); out[1] = (3, H)
    assert plan(s=out) == capi.EINVAL
    assert _same(sb.read_plan(0), p0) and _same(sb.read_plan(1), p1)         # the refusals touched nothing
    assert all(_same(sb.read(b), fields[b]) for b in range(2))
    n = ctypes.c_int32(-1)
    path = np.zeros((1, 2), np.int32)
    assert len(p1["path"]) > 1
    assert L.yh_scene_batch_plan_read(h, 1, None, None, _p(path), None, 1, ctypes.byref(n)) == capi.EOVERFLOW and n.value == len(p1["path"])
    assert _code(lambda: sb.read_plan(2)) == capi.EINVAL
    sb.append(1, ya.COMPAT_SANE)                                            # a newer append: the plan is gone
    assert _code(lambda: sb.read_plan(0)) == capi.ESTATE and _code(lambda: sb.read(1)) == capi.EINVAL
    assert _code(lambda: sb.plan_time(1)) == capi.ESTATE
    assert _same(sb.read(0), before)
    # the single handle, used before the batch, gives afterwards what it gave
    assert _same(sc.read(), before) and _same(sc.read_plan(), before_plan)
    assert _same(_single(sc, *frames[0], ya.COMPAT_SANE), before)
    sc.plan(targets=[(3, 3)], start=(40, 30))
    assert _same(sc.read_plan(), before_plan)
    sb.close(); sc.close()


def _camera_frame(seed):
    """The camera-like frame of tools/time_path.py (robots + two balls), its depth from `seed`."""
    H, W = 480, 640
    depth = np.random.default_rng(seed).integers(200, 4000, (H, W)).astype(np.uint16)
    ci = np.zeros((H, W, 2), np.uint8)
    ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
    return depth, ci


@pytest.mark.gpu
def test_a_batch_of_eight_beats_eight_single_frames(built):
    """640 x 480, n = 8, camera-like frames, connectivity 4: stage + append + plan of the batch against the same eight frames through one
    Scene, append + plan each, in this process; median of five, alternated, one warm-up each. The assertion is batch < eight singles:
    a ratio of 1 or more would mean the feature has no purpose."""
    import yolact_amd as ya
    n = 8
    frames = [_camera_frame(b) for b in range(n)]
    packed = [ya.SceneBatch.pack(ci) for _, ci in frames]
    sb, sc = ya.SceneBatch(640, 480, n), ya.Scene(640, 480)

    def batch():                                                            # (staging is part of bringing eight frames in: it is timed)
        for b in range(n):
            sb.stage(b, frames[b][0], frame_u32=packed[b])
        sb.append(n, ya.COMPAT_SANE)
        assert sb.plan() == [0] * n

    def singles():
        for b in range(n):
            sc.append_classified(frames[b][0], frame_u32=packed[b], mode=ya.COMPAT_SANE)
            sc.plan()

    def clock(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

    batch(); singles()                                                      # warm-up: buffers, code objects
    assert _same(sb.read_plan(n - 1, fields=False), sc.read_plan(fields=False))
    tb, ts = [], []
    for _ in range(5):
        tb.append(clock(batch)); ts.append(clock(singles))
    mb, ms = sorted(tb)[2], sorted(ts)[2]
    print(f"append + plan of {n} frames: batch {mb:.3f} ms, {n} singles {ms:.3f} ms, ratio {mb / ms:.3f}")
    assert mb < ms
    sb.close(); sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plan4", "plan8", "turn", "turn_tour"])
def test_a_scene_is_the_batch_of_one(built, kind):
    """One driver plans for both handles, so a Scene and a SceneBatch of one frame given the same fields return the same arrays AND
    the same solver counters - the same numbers, not merely within SP_BATCH of each other. 40 x 36: 2 x 2 tiles of 32 x 32, ragged on
    both axes; one target on the corner pixel of tile (0, 0), the other across both borders in tile (1, 1). Each kind stays pinned to
    its restatement (path_ref, path8_ref through path_ref's conn = 8, turn_ref, turn_tour_ref). (The counters are those of two runs
    of the asynchronous solver: should they ever differ by a round, the cause is the border race DESIGN.md §11 "Scene batch"
    describes, not the driver.)"""
    import yolact_amd as ya
    from test_scene_batch_turn import _check_turn
    from test_scene_path8 import _check_plan, _random_fields
    from test_scene_turn_tour import _check
    W, H, tau = 40, 36, 2.0
    f = _random_fields(np.random.default_rng(4036), H, W)
    targets, start, heading = [(31, 31), (32, 33)], (2, 34), 6
    sc, sb = ya.Scene(W, H), ya.SceneBatch(W, H, 1)
    sc.set_fields(*f)
    sb.set_fields(0, *f)
    if kind in ("plan4", "plan8"):
        conn = int(kind[-1])
        sc.plan(targets=targets, start=start, connectivity=conn)
        assert sb.plan(targets=[targets], starts=[start], connectivity=conn) == [ya.capi.OK]
        one, got, t_one, t_got = sc.read_plan(), sb.read_plan(0), sc.plan_time(1), sb.plan_time(1)
        _check_plan(got, f, targets, start, conn=conn)
    elif kind == "turn":
        sc.plan_turn(targets=targets, start=start, heading=heading, turn_price=tau)
        assert sb.plan_turn(targets=[targets], starts=[start], headings=[heading], turn_price=tau) == [ya.capi.OK]
        one, got, t_one, t_got = sc.read_turn(), sb.read_turn(0), sc.turn_time(1), sb.turn_time(1)
        _check_turn(got, f, targets, start, heading, tau)
    else:
        sc.plan_turn_tour(targets=targets, start=start, heading=heading, turn_price=tau)
        assert sb.plan_turn_tour(targets=[targets], starts=[start], headings=[heading], turn_price=tau) == [ya.capi.OK]
        one, got, t_one, t_got = sc.read_turn_tour(), sb.read_turn_tour(0), sc.turn_tour_time(1), sb.turn_tour_time(1)
        _check(got, f, targets, start, heading, tau)
    assert one.keys() == got.keys()
    for k in one:
        a, b = np.asarray(one[k]), np.asarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), k
    print(f"{kind}: scene {t_one}, batch of one {t_got}")
    assert t_one["rounds"] == t_got["rounds"] and t_one["tile_runs"] == t_got["tile_runs"]
    sb.close(); sc.close()
