"""The scene batch's turn-aware plan (yh_scene_batch_plan_turn, DESIGN.md §11 "Scene batch: turns"): yh_scene_plan_turn for every
frame of a batch in shared solver rounds. The definition is the single handle's: frame b equals, bit for bit, what Scene.plan_turn
gives on that frame alone - cost [8][H][W], act, route, turns, directions, route length. Every comparison is array_equal (floats
through their u32 view), against a Scene in the same process and, at the small sizes, against the restatement (tests/turn_ref.py).
There is no tolerance anywhere. CPU part: the surface. GPU part (-m gpu): the equality with ragged seed lists, tile borders and
corners inside a batch, frames that converge at different rounds, the full size, independence from the batch's plain plan, the life
cycle with every refusal, and a floor on time (a batched turn plan of eight frames must beat eight single ones)."""
import ctypes
import inspect
import os
import re
import time

import numpy as np
import pytest

import path8_ref as P
import path_ref as R
import tour_ref as T
import turn_ref as U
from test_scene_batch import SP_BATCH, _camera_frame, _code, _frames, _same, _single
from test_scene_path8 import _bits, _fields_scene, _random_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- CPU

def test_batch_turn_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0]: s for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read(), flags=re.S)
    for name, text, other, nargs in (("yh_scene_batch_plan_turn", pub, dbg, 7), ("yh_scene_batch_turn_read", pub, dbg, 9),
                                     ("yh_scene_batch_turn_time", dbg, pub, 5)):
        assert re.search(r"\b%s\s*\(" % name, text) and not re.search(r"\b%s\s*\(" % name, other) and name in bound, name
        assert len(bound[name][2]) == nargs, name
    assert "#define YH_ABI_VERSION 4" in pub
    for m in ("plan_turn", "read_turn", "turn_time"):
        assert callable(getattr(capi.SceneBatch, m)), m
    sig = inspect.signature(capi.SceneBatch.plan_turn).parameters
    assert sig["headings"].default == 6 and "turn_price" in sig


def test_size_guards_on_the_cpu():
    assert R.size_ok(3, 2894) and not U.size_ok(3, 2894)                           # between the two guards


# ---------------------------------------------------------------- GPU

def _check_turn(got, f, targets, start, heading, tau):
    """cost, act, path, turns and directions of a turn plan against the restatement on the fields f = (map, conn0, conn1)."""
    want = U.dijkstra(*f, targets, tau)
    assert np.array_equal(_bits(got["cost"]), _bits(want))
    act = U.actions(want, *f, targets, tau)
    assert np.array_equal(got["act"], act)
    path, dirs, turns = U.walk(want, act, start, heading)
    assert np.array_equal(got["path"], path) and np.array_equal(got["turns"], turns)
    assert np.array_equal(_bits(got["directions"]), _bits(dirs))
    assert (np.abs(got["turns"]) <= 4).all()
    return want


def _single_turn(sc, targets, n_targets, start, heading, tau):
    """Scene.plan_turn + read_turn, or the error code of a refused plan."""
    import yolact_amd as ya
    try:
        sc.plan_turn(targets=targets, n_targets=n_targets, start=start, heading=heading, turn_price=tau)
    except ya.YhError as e:
        return e.code
    return sc.read_turn()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,n", [(33, 65, 3), (96, 128, 4)])
def test_turn_plan_equals_the_single_handle_and_the_restatement(built, H, W, n):
    """Frame 1 has no balls, frame 2 one ball: the seed lists are ragged. n >= 3 is what tells a frame stride of W H from 8 W H."""
    import yolact_amd as ya
    tau = 2.0
    frames = _frames(H, W, n, 100 * H + W, balls=[b != 1 for b in range(n)])
    frames[2][1][H // 8:H // 8 + 6, W // 8:W // 8 + 7] = 0           # frame 2 keeps one ball only (id 0)
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
    headings = [6, 0, 3, 5][:n]
    assert sb.plan_turn(targets=targets, starts=starts, headings=headings, turn_price=tau) == [ya.capi.OK] * n
    for b in range(n):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        want, got = _single_turn(sc, targets[b], 0, starts[b], headings[b], tau), sb.read_turn(b)
        assert _same(got, want), b
        assert got["cost"].shape == (8, H, W) and got["act"].shape == (8, H, W)
        if b == 0:
            assert len(got["path"]) == 1 and got["turns"].shape == (0,) and got["directions"].shape == (0, 2)
        else:
            assert len(got["path"]) > 1 and len(got["turns"]) == len(got["directions"]) == len(got["path"]) - 1
        if (H, W) == (33, 65):
            f = fields[b]
            _check_turn(got, (f["map"], f["conn0"], f["conn1"]), targets[b], starts[b], headings[b], tau)
    # NULL targets: each frame's own balls; frame 1 has none - YH_ESTATE, no plan, the others are planned
    for n_targets in (3, 1):
        status = sb.plan_turn(targets=None, n_targets=n_targets, starts=starts, headings=headings, turn_price=tau)
        assert status == [ya.capi.ESTATE if b == 1 else ya.capi.OK for b in range(n)]
        for b in range(n):
            sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
            want = _single_turn(sc, None, n_targets, starts[b], headings[b], tau)
            if b == 1:
                assert want == ya.capi.ESTATE and _code(lambda: sb.read_turn(1)) == ya.capi.ESTATE
                continue
            got = sb.read_turn(b)
            assert _same(got, want), (b, n_targets)
            want_targets = sorted(set(R.ball_targets(fields[b]["balls"], n_targets, W, H)))
            assert len(want_targets) == (1 if b == 2 or n_targets == 1 else 2)
            zeros = np.argwhere(got["cost"] == 0)
            assert len(zeros) == 8 * len(want_targets)
            assert sorted(set((int(x), int(y)) for _, y, x in zeros)) == want_targets
            assert all((got["cost"][:, y, x] == 0).all() and (got["act"][:, y, x] == 255).all() for x, y in want_targets)
            assert (got["act"] == 255).sum() == 8 * len(want_targets)
    sb.close(); sc.close()


@pytest.mark.gpu
def test_tile_borders_and_corners_inside_a_batch(built):
    """64 x 64, three constructed frames in one call with one price: the late corner (the cheap way into the diagonal tile is through
    one corner cell that settles late), targets on both sides of a tile corner, and a flat diagonal across it. A corner wake-up that
    lands in another frame's flags, or a missed one, shows here."""
    import yolact_amd as ya
    S, tau = 64, 1.0
    fs = [P.late_corner(), _random_fields(np.random.default_rng(64), S, S, 30), T.flat_fields(S, S)]
    targets = [[(0, 0), (0, 0)], [(31, 31), (32, 32)], [(63, 63), (63, 63)]]
    starts, headings = [(63, 63), (5, 60), (0, 0)], [6, 6, 6]
    sb = ya.SceneBatch(S, S, 3)
    for b, f in enumerate(fs):
        sb.set_fields(b, *f)
    assert sb.plan_turn(targets=targets, starts=starts, headings=headings, turn_price=tau) == [0, 0, 0]
    got = [sb.read_turn(b) for b in range(3)]
    for b in range(3):
        assert np.isfinite(got[b]["cost"]).all()
        _check_turn(got[b], fs[b], targets[b], starts[b], headings[b], tau)
    assert got[2]["turns"][0] == 3 and (got[2]["turns"][1:] == 0).all() and len(got[2]["path"]) == S
    sb.close()


@pytest.mark.gpu
def test_frames_that_converge_at_different_rounds(built):
    """A flat map, the serpentine and a random field side by side: the serpentine takes more than SP_BATCH rounds, so the host loop
    goes round again while the other two frames have long converged. The batch takes the rounds of its slowest frame: at least the
    largest of the three single plans' and less than SP_BATCH above it (a frame's own count may differ between two runs of the
    asynchronous solver)."""
    import yolact_amd as ya
    S, tau = 96, 2.0
    serp, s_start, s_target = R.serpentine(S, S)
    maps = [np.zeros((S, S), np.uint32), serp, np.random.default_rng(3).integers(0, 40, (S, S)).astype(np.uint32)]
    targets, starts, headings = [[(5, 7)], [s_target], [(50, 30)]], [(90, 80), s_start, (2, 93)], [6, 0, 2]
    sb, sc = ya.SceneBatch(S, S, 4), ya.Scene(S, S)
    want, rounds = [], []
    for b in range(3):
        sc.set_fields(maps[b], *R.sane_connections(maps[b]))
        sc.plan_turn(targets=targets[b], start=starts[b], heading=headings[b], turn_price=tau)
        want.append(sc.read_turn())
        rounds.append(sc.turn_time(1)["rounds"])
        sb.set_fields(b, maps[b], *R.sane_connections(maps[b]))
    print(f"single turn plans at {S}x{S}: rounds {rounds}")
    assert rounds[1] > SP_BATCH and rounds[0] < SP_BATCH and rounds[2] < SP_BATCH
    assert sb.plan_turn(targets=targets, starts=starts, headings=headings, turn_price=tau) == [0, 0, 0]
    for b in range(3):
        assert _same(sb.read_turn(b), want[b]), b
    stats = sb.turn_time(1)
    print(f"batch of 3: {stats}")
    assert 0 <= stats["rounds"] - max(rounds) < SP_BATCH and stats["tile_runs"] >= stats["rounds"]
    for b in range(3):
        assert _same(sb.read_turn(b), want[b]), b
    sb.close(); sc.close()


@pytest.mark.gpu
def test_full_size(built):
    """640 x 480, two of three slots, camera-like frames with different depth seeds, each frame's own balls."""
    import yolact_amd as ya
    H, W, tau = 480, 640, 2.0
    frames = [_camera_frame(20 + b) for b in range(2)]
    sb, sc = ya.SceneBatch(W, H, 3), ya.Scene(W, H)
    for b, (depth, ci) in enumerate(frames):
        sb.stage(b, depth, cls_id=ci)
    sb.append(2, ya.COMPAT_SANE)
    assert sb.plan_turn(turn_price=tau) == [0, 0]
    got = [sb.read_turn(b) for b in range(2)]
    for b in range(2):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        sc.plan_turn(turn_price=tau)
        assert _same(got[b], sc.read_turn()), b
    assert not np.array_equal(_bits(got[0]["cost"]), _bits(got[1]["cost"]))
    r = sb.read(1)
    tg = R.ball_targets(r["balls"], 3, W, H)
    assert len(tg) == 2
    d = got[1]["cost"]
    assert np.isfinite(d).all() and (d == 0).sum() == 8 * len(tg)
    assert U.equation_residual(d, r["map"], r["conn0"], r["conn1"], tg, tau) == 0
    assert (got[1]["act"] != 3).all()
    assert tuple(got[1]["path"][0]) == (400, 479) and tuple(got[1]["path"][-1]) in tg
    sb.close(); sc.close()


@pytest.mark.gpu
def test_plan_and_turn_plan_do_not_disturb_each_other(built):
    import yolact_amd as ya
    H, W, n = 40, 48, 2
    frames = _frames(H, W, n, 31)
    targets, starts = [[(3, 3)], [(44, 2)]], [(40, 30), (10, 35)]
    sc = ya.Scene(W, H)
    _single(sc, *frames[0], ya.COMPAT_SANE)
    sc.plan_turn(targets=targets[0], start=starts[0], heading=1, turn_price=3.0)
    before = sc.read_turn()
    sb = ya.SceneBatch(W, H, n)
    for b, (depth, ci) in enumerate(frames):
        sb.stage(b, depth, cls_id=ci)
    sb.append(n, ya.COMPAT_SANE)
    sb.plan(targets=targets, starts=starts, connectivity=8)
    p8 = [sb.read_plan(b) for b in range(n)]
    assert _code(lambda: sb.read_turn(0)) == ya.capi.ESTATE and _code(lambda: sb.turn_time(1)) == ya.capi.ESTATE   # no turn plan yet
    assert sb.plan_turn(targets=targets, starts=starts, headings=[1, 4], turn_price=3.0) == [0, 0]
    t = [sb.read_turn(b) for b in range(n)]
    assert _same(t[0], before)
    assert all(_same(sb.read_plan(b), p8[b]) for b in range(n))
    stats = sb.turn_time(1)
    assert stats["rounds"] >= 1 and stats["tile_runs"] >= stats["rounds"]
    assert all(_same(sb.read_plan(b), p8[b]) for b in range(n)) and all(_same(sb.read_turn(b), t[b]) for b in range(n))
    sb.plan(targets=targets, starts=starts, connectivity=4)
    sb.plan_time(1)
    assert all(_same(sb.read_turn(b), t[b]) for b in range(n))
    assert not _same(sb.read_plan(0), p8[0])
    # the single handle, used before the batch, gives afterwards what it gave
    assert _same(sc.read_turn(), before)
    sc.plan_turn(targets=targets[0], start=starts[0], heading=1, turn_price=3.0)
    assert _same(sc.read_turn(), before)
    sb.close(); sc.close()


@pytest.mark.gpu
def test_life_cycle_and_refusals(built):
    import yolact_amd as ya
    from yolact_amd import capi
    from yolact_amd.capi import _p
    H, W = 40, 48
    frames = _frames(H, W, 2, 77)
    sb = ya.SceneBatch(W, H, 2)
    L, h = sb.L, sb.h
    starts = np.array([[40, 30], [10, 35]], np.int32)
    heads = np.array([6, 2], np.int32)
    tg = np.array([[[3, 3], [3, 3]], [[44, 2], [20, 9]]], np.int32)
    plan = lambda t=tg, s=starts, hd=heads, k=2, price=2.0: L.yh_scene_batch_plan_turn(
        h, None if t is None else _p(t), k, None if s is None else _p(s), None if hd is None else _p(hd), price, None)
    assert plan() == capi.ESTATE                                            # before any append
    assert _code(lambda: sb.read_turn(0)) == capi.ESTATE and _code(lambda: sb.turn_time(1)) == capi.ESTATE
    for b in range(2):
        sb.stage(b, frames[b][0], cls_id=frames[b][1])
    sb.append(2, ya.COMPAT_STRICT)
    assert plan() == capi.ESTATE and b"STRICT" in L.yh_scene_batch_last_error(h)
    sb.append(2, ya.COMPAT_SANE)
    assert plan() == capi.OK
    t = [sb.read_turn(b) for b in range(2)]
    sc = ya.Scene(W, H)
    _single(sc, *frames[1], ya.COMPAT_SANE)
    sc.plan_turn(targets=tg[1], start=(10, 35), heading=2, turn_price=2.0)
    assert _same(t[1], sc.read_turn())
    untouched = lambda: all(_same(sb.read_turn(b), t[b]) for b in range(2))
    bad = heads.copy(); bad[1] = 8                                          # a heading of 8, in frame 1 only
    assert plan(hd=bad) == capi.EINVAL and b"frame 1" in L.yh_scene_batch_last_error(h) and untouched()
    assert plan(hd=None) == capi.EINVAL and untouched()
    assert plan(s=None) == capi.EINVAL and untouched()
    assert plan(k=0) == capi.EINVAL and untouched()
    for price in (float("nan"), 0.5, 2048.0):
        assert plan(price=price) == capi.EINVAL and b"turn price" in L.yh_scene_batch_last_error(h) and untouched()
    out = tg.copy(); out[1, 1] = (W, 2)                                     # a target outside the frame, in frame 1 only
    assert plan(t=out) == capi.EINVAL and b"frame 1" in L.yh_scene_batch_last_error(h) and untouched()
    n = ctypes.c_int32(-1)
    path = np.zeros((1, 2), np.int32)
    assert len(t[1]["path"]) > 1
    assert L.yh_scene_batch_turn_read(h, 1, None, None, _p(path), None, None, 1, ctypes.byref(n)) == capi.EOVERFLOW and n.value == len(t[1]["path"])
    assert not path.any()
    assert _code(lambda: sb.read_turn(2)) == capi.EINVAL
    sb.append(1, ya.COMPAT_SANE)                                            # a newer append: the turn plan is gone
    assert _code(lambda: sb.read_turn(0)) == capi.ESTATE and _code(lambda: sb.turn_time(1)) == capi.ESTATE
    sb.close(); sc.close()
    # between the planner's guard and the turn planner's: an 8-connected plan runs, a turn plan is refused
    H, W = 2894, 3
    sb = ya.SceneBatch(W, H, 1)
    sb.set_fields(0, *T.flat_fields(H, W))
    assert sb.plan(targets=[[(1, 0)]], starts=[(1, 5)], connectivity=8) == [0]
    assert len(sb.read_plan(0, fields=False)["path"]) == 6
    assert _code(lambda: sb.plan_turn(targets=[[(1, 0)]], starts=[(1, 5)])) == capi.EINVAL
    assert b"8 * 1024" in sb.L.yh_scene_batch_last_error(sb.h)
    sb.close()


@pytest.mark.gpu
def test_a_batched_turn_plan_of_eight_beats_eight_single_ones(built):
    """640 x 480, n = 8, camera-like frames: SceneBatch.plan_turn against eight Scene.append_classified + plan_turn. A Scene holds
    one frame, so bringing each frame in is part of planning eight frames through it; the batch's side therefore carries the same
    work for the same frames (stage + append), as test_scene_batch's floor does. Median of five, alternated in one process, one
    warm-up each. The assertion is batch < eight singles: a ratio of 1 or more would mean the feature has no purpose."""
    import yolact_amd as ya
    n = 8
    frames = [_camera_frame(b) for b in range(n)]
    packed = [ya.SceneBatch.pack(ci) for _, ci in frames]
    sb, sc = ya.SceneBatch(640, 480, n), ya.Scene(640, 480)

    def batch():
        for b in range(n):
            sb.stage(b, frames[b][0], frame_u32=packed[b])
        sb.append(n, ya.COMPAT_SANE)
        assert sb.plan_turn() == [0] * n

    def singles():
        for b in range(n):
            sc.append_classified(frames[b][0], frame_u32=packed[b], mode=ya.COMPAT_SANE)
            sc.plan_turn()

    def clock(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

    batch(); singles()                                                      # warm-up: buffers, code objects
    assert _same(sb.read_turn(n - 1, fields=False), sc.read_turn(fields=False))
    tb, ts = [], []
    for _ in range(5):
        tb.append(clock(batch)); ts.append(clock(singles))
    mb, ms = sorted(tb)[2], sorted(ts)[2]
    print(f"bring in + turn plan of {n} frames: batch {mb:.3f} ms, {n} singles {ms:.3f} ms, ratio {mb / ms:.3f}")
    assert mb < ms
    sb.close(); sc.close()
