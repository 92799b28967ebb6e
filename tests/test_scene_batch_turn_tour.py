"""The scene batch's turn-aware tour (yh_scene_batch_plan_turn_tour, DESIGN.md §11 "Scene batch: turn tours"): yh_scene_plan_turn_tour
for every frame of a batch in shared solver rounds. The definition is the single handle's: frame b equals, bit for bit, what
Scene.plan_turn_tour gives on that frame alone - targets, order, leg table, total, the K cost and action fields, the label, the joined
route with its turns, directions and leg ends. Every comparison is on bit patterns (array_equal, floats through their u32 view),
against a Scene in the same process and, at the small sizes, against the restatement (tests/turn_tour_ref.py). There is no tolerance
anywhere. CPU part: the surface. GPU part (-m gpu): the strides with a ragged K (field z = b Kmax + f, not b K_b + f), tile borders
and corners inside a batch, frames that converge at different rounds, K = 6 beside K = 1, the full size, the staged pipeline,
independence from the batch's other two planners, the life cycle with every refusal, and a floor on time (a batched turn tour of eight
frames must beat eight single ones)."""
import ctypes
import inspect
import os
import re
import time

import numpy as np
import pytest

import path_ref as R
import tour_ref as T
import turn_ref as U
from test_scene import _frame
from test_scene_batch import SP_BATCH, _camera_frame, _code, _frames
from test_scene_path8 import _bits, _fields_scene, _random_fields, _same
from test_scene_turn_tour import _check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- CPU

def test_batch_turn_tour_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0]: s for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read(), flags=re.S)
    for name, text, other, nargs in (("yh_scene_batch_plan_turn_tour", pub, dbg, 7), ("yh_scene_batch_turn_tour_read", pub, dbg, 18),
                                     ("yh_scene_batch_turn_tour_time", dbg, pub, 5)):
        assert re.search(r"\b%s\s*\(" % name, text) and not re.search(r"\b%s\s*\(" % name, other) and name in bound, name
        assert len(bound[name][2]) == nargs, name
    # the batched read takes the frame, then exactly the single read's arguments
    assert bound["yh_scene_batch_turn_tour_read"][2][2:] == bound["yh_scene_turn_tour_read"][2][1:]
    assert "#define YH_ABI_VERSION 4" in pub and "#define YH_TOUR_MAX 6" in pub


def test_scene_batch_has_the_turn_tour_methods_with_their_defaults():
    from yolact_amd import capi
    for m in ("plan_turn_tour", "read_turn_tour", "turn_tour_time"):
        assert callable(getattr(capi.SceneBatch, m)), m
    sig = inspect.signature(capi.SceneBatch.plan_turn_tour).parameters
    assert list(sig)[1:] == ["targets", "n_targets", "starts", "headings", "turn_price"]
    assert sig["targets"].default is None and sig["n_targets"].default == 3 and sig["starts"].default is None
    assert sig["headings"].default == 6 and sig["turn_price"].default == 2.0
    sig = inspect.signature(capi.SceneBatch.read_turn_tour).parameters
    assert list(sig)[1:] == ["b", "fields"] and sig["fields"].default is True
    assert inspect.signature(capi.SceneBatch.turn_tour_time).parameters["reps"].default == 20


# ---------------------------------------------------------------- GPU

def _single_tour(sc, targets, n_targets, start, heading, tau, fields=True):
    """Scene.plan_turn_tour + read_turn_tour, or the error code of a refused call."""
    import yolact_amd as ya
    try:
        sc.plan_turn_tour(targets=targets, n_targets=n_targets, start=start, heading=heading, turn_price=tau)
    except ya.YhError as e:
        return e.code
    return sc.read_turn_tour(fields=fields)


def _ball_frame(H, W, seed, balls):
    """test_scene._frame without its balls, then one pixel per ball: balls = [(id, column, row, depth)]. A ball's target is
    (its column, a row that follows from its depth), so balls in different columns are different targets and two balls of one
    depth on neighbouring rows of one column fall on one pixel."""
    depth, ci = _frame(np.random.default_rng(seed), H, W, balls=False)
    for k, x, y, d in balls:
        ci[y, x] = (3, k)
        depth[y, x] = d
    return depth, ci


def _append(sb, frames, mode):
    """Stages and appends the frames; returns every frame's fields as the batch reads them back."""
    for b, (depth, ci) in enumerate(frames):
        sb.stage(b, depth, cls_id=ci)
    sb.append(len(frames), mode)
    return [sb.read(b) for b in range(len(frames))]


@pytest.mark.gpu
def test_strides_with_explicit_targets_against_the_single_handle_and_the_restatement(built):
    """33 x 65 (one pixel past a tile border both ways), n = 3, Kmax = 3, fields through set_fields: every frame against
    Scene.plan_turn_tour on that frame alone and against turn_tour_ref. Frame 1 starts on one of its targets (the junction rule: a leg
    of one node adds nothing and passes the heading on)."""
    import yolact_amd as ya
    H, W, n, tau = 33, 65, 3, 2.0
    fs = [_random_fields(np.random.default_rng(900 + b), H, W) for b in range(n)]
    targets = [[(64, 32), (3, 3), (32, 31)], [(10, 30), (60, 2), (31, 16)], [(0, 0), (33, 32), (64, 0)]]
    starts, headings = [(10, 30), (10, 30), (40, 20)], [6, 0, 3]
    sb = ya.SceneBatch(W, H, n)
    for b, f in enumerate(fs):
        sb.set_fields(b, *f)
    assert sb.plan_turn_tour(targets=targets, starts=starts, headings=headings, turn_price=tau) == [ya.capi.OK] * n
    got = [sb.read_turn_tour(b) for b in range(n)]
    for b in range(n):
        sc = _fields_scene(fs[b])
        want = _single_tour(sc, targets[b], 0, starts[b], headings[b], tau)
        assert _same(got[b], want), b
        _check(got[b], fs[b], targets[b], starts[b], headings[b], tau)
        short = sb.read_turn_tour(b, fields=False)
        assert set(short) == set(got[b]) - {"cost", "act", "label"} and all(np.array_equal(short[k], got[b][k]) for k in short)
        sc.close()
    # frame 1's start is its target 0: the leg there costs nothing, adds no node and passes the heading on
    assert got[1]["legs"][0, 0] == 0 and got[1]["arrive"][0, 0] == headings[1]
    assert got[1]["order"][0] == 0 and got[1]["leg_ends"][0] == 0 and got[1]["leg_headings"][0] == headings[1]
    assert not np.array_equal(_bits(got[0]["cost"]), _bits(got[2]["cost"]))
    sb.close()


RAGGED = [   # per frame: [(id, column, row, depth)] - 3, 0, 1 and 2 usable balls (frame 3: three balls, two of them on one pixel)
    [(5, 20, 30, 2000), (9, 100, 60, 1500), (40, 64, 10, 3000)],
    [],
    [(7, 90, 50, 2500)],
    [(1, 40, 20, 2000), (2, 40, 21, 2000), (3, 110, 70, 1000)],
]


@pytest.mark.gpu
def test_ragged_k_with_the_frames_own_balls(built):
    """96 x 128, n = 4, NULL targets, n_targets = 3: K_b = 3, 0, 1, 2. Frame 1 has no ball (YH_ESTATE, no tour, its read refused),
    frame 2 a single one - K_b < Kmax in the middle of the batch is what tells field z = b Kmax + f from b K_b + f and a stride of
    8 W H from W H -, frame 3 two balls on one pixel. Headings 6, 0, 3, 5."""
    import yolact_amd as ya
    H, W, n, tau = 96, 128, 4, 2.0
    frames = [_ball_frame(H, W, 300 + b, RAGGED[b]) for b in range(n)]
    sb, sc = ya.SceneBatch(W, H, n), ya.Scene(W, H)
    fields = _append(sb, frames, ya.COMPAT_SANE)
    raw = [R.ball_targets(f["balls"], 3, W, H) for f in fields]
    want_targets = [T.distinct(t) for t in raw]
    assert [len(t) for t in raw] == [3, 0, 1, 3] and [len(t) for t in want_targets] == [3, 0, 1, 2]
    starts, headings = [(64, 95), (5, 5), (120, 3), (0, 90)], [6, 0, 3, 5]
    status = sb.plan_turn_tour(targets=None, n_targets=3, starts=starts, headings=headings, turn_price=tau)
    assert status == [ya.capi.OK, ya.capi.ESTATE, ya.capi.OK, ya.capi.OK]
    for b in range(n):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        want = _single_tour(sc, None, 3, starts[b], headings[b], tau)
        if b == 1:
            assert want == ya.capi.ESTATE and _code(lambda: sb.read_turn_tour(1)) == ya.capi.ESTATE
            assert b"frame 1" in sb.L.yh_scene_batch_last_error(sb.h)
            continue
        got = sb.read_turn_tour(b)
        assert _same(got, want), b
        K = len(want_targets[b])
        assert got["targets"].tolist() == [list(t) for t in want_targets[b]] and got["cost"].shape == (K, 8, H, W) and got["legs"].shape == (1 + 8 * K, K)
        assert sorted(got["order"].tolist()) == list(range(K)) and np.isfinite(got["cost"]).all()
        for f, (x, y) in enumerate(want_targets[b]):
            assert (got["cost"][f] == 0).sum() == 8 and (got["cost"][f][:, y, x] == 0).all()
            assert (got["act"][f] == 255).sum() == 8 and (got["act"][f][:, y, x] == 255).all() and (got["act"][f] != 3).all()
        assert np.array_equal(got["label"], np.argmin(got["cost"], axis=0))
        assert tuple(got["path"][0]) == starts[b] and got["path"][got["leg_ends"]].tolist() == [list(want_targets[b][o]) for o in got["order"]]
    # fewer balls asked for than some frames have: Kmax = 1, every planned frame has K_b = 1
    assert sb.plan_turn_tour(targets=None, n_targets=1, starts=starts, headings=headings, turn_price=tau) == status
    for b in (0, 2, 3):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        assert _same(sb.read_turn_tour(b), _single_tour(sc, None, 1, starts[b], headings[b], tau)), b
    sb.close(); sc.close()


@pytest.mark.gpu
def test_tile_borders_and_corners_inside_a_batch(built):
    """96 x 128, n = 3, K = 4: targets at x = 0 and 31 mod 32, y = 31 mod 32 and at corners of four tiles, placed differently per
    frame - round 0's flags per field z, and the wake-ups across borders and corners, must land in that field's flags."""
    import yolact_amd as ya
    H, W, n, tau = 96, 128, 3, 2.0
    fs = [_random_fields(np.random.default_rng(H * 1000 + W + b), H, W) for b in range(n)]
    targets = [[(32, 10), (95, 70), (50, 63), (31, 32)], [(0, 31), (127, 95), (64, 64), (63, 63)], [(96, 0), (31, 31), (32, 32), (100, 95)]]
    starts, headings = [(64, 95), (64, 0), (5, 50)], [6, 2, 7]
    sb = ya.SceneBatch(W, H, n)
    for b, f in enumerate(fs):
        sb.set_fields(b, *f)
    assert sb.plan_turn_tour(targets=targets, starts=starts, headings=headings, turn_price=tau) == [0] * n
    for b in range(n):
        sc = _fields_scene(fs[b])
        got = sb.read_turn_tour(b)
        assert _same(got, _single_tour(sc, targets[b], 0, starts[b], headings[b], tau)), b
        assert np.isfinite(got["cost"]).all()
        if b == 1:
            for f, t in enumerate(targets[b]):
                assert U.equation_residual(got["cost"][f], *fs[b], [t], tau) == 0, f
        sc.close()
    sb.close()


@pytest.mark.gpu
def test_frames_that_converge_at_different_rounds(built):
    """A flat map, the serpentine and a random field at 96 x 96, K = 2 each, in one call: the serpentine's fields take more than
    SP_BATCH rounds, so the host loop goes round again while the other frames' fields have long converged. Every frame equals its
    single tour; the batch takes the rounds of its slowest field: at most the slowest single tour's plus one batch of SP_BATCH."""
    import yolact_amd as ya
    S, tau = 96, 2.0
    serp, s_start, s_target = R.serpentine(S, S)
    maps = [np.zeros((S, S), np.uint32), serp, np.random.default_rng(3).integers(0, 40, (S, S)).astype(np.uint32)]
    targets, starts, headings = [[(5, 7), (80, 20)], [s_target, (48, 44)], [(50, 30), (3, 90)]], [(90, 80), s_start, (2, 93)], [6, 0, 2]
    assert all(serp[y, x] == 0 for x, y in targets[1] + [s_start])
    sb, sc = ya.SceneBatch(S, S, 4), ya.Scene(S, S)
    want, rounds = [], []
    for b in range(3):
        f = (maps[b],) + R.sane_connections(maps[b])
        sc.set_fields(*f)
        want.append(_single_tour(sc, targets[b], 0, starts[b], headings[b], tau))
        rounds.append(sc.turn_tour_time(1)["rounds"])
        sb.set_fields(b, *f)
    print(f"single turn tours at {S}x{S}: rounds {rounds}")
    assert rounds[1] > SP_BATCH and rounds[0] < SP_BATCH and rounds[2] < SP_BATCH
    assert sb.plan_turn_tour(targets=targets, starts=starts, headings=headings, turn_price=tau) == [0, 0, 0]
    for b in range(3):
        assert _same(sb.read_turn_tour(b), want[b]), b
    stats = sb.turn_tour_time(1)
    print(f"batch of 3: {stats}")
    assert 1 <= stats["rounds"] <= max(rounds) + SP_BATCH and stats["tile_runs"] >= stats["rounds"]
    for b in range(3):
        assert _same(sb.read_turn_tour(b), want[b]), b                          # the replay left the same bits
    sb.close(); sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (37, 53)])
def test_six_targets_beside_one(built, H, W):
    """n = 2, NULL targets, n_targets = 6: frame 0 has six balls, frame 1 one - five of frame 1's six fields have no seed."""
    import yolact_amd as ya
    cols = [0, 1, 3, 4, 6, 7] if W == 8 else [2, 11, 20, 29, 40, 52]
    six = [(k, x, (3 * k) % H, 1200 + 400 * k) for k, x in enumerate(cols)]
    frames = [_ball_frame(H, W, 60, six), _ball_frame(H, W, 61, [(0, cols[2], H // 2, 2000)])]
    sb, sc = ya.SceneBatch(W, H, 2), ya.Scene(W, H)
    fields = _append(sb, frames, ya.COMPAT_SANE)
    assert [len(T.distinct(R.ball_targets(f["balls"], 6, W, H))) for f in fields] == [6, 1]
    starts, headings = [(W - 1, H - 1), (0, 0)], [6, 1]
    assert sb.plan_turn_tour(targets=None, n_targets=6, starts=starts, headings=headings, turn_price=3.0) == [0, 0]
    for b in range(2):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        got = sb.read_turn_tour(b)
        assert _same(got, _single_tour(sc, None, 6, starts[b], headings[b], 3.0)), b
        assert len(got["targets"]) == (6, 1)[b] and got["legs"].shape == ((49, 6), (9, 1))[b]
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
    assert sb.plan_turn_tour(turn_price=tau) == [0, 0]
    got = [sb.read_turn_tour(b) for b in range(2)]
    for b in range(2):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        sc.plan_turn_tour(turn_price=tau)
        assert _same(got[b], sc.read_turn_tour()), b
    assert not np.array_equal(_bits(got[0]["cost"]), _bits(got[1]["cost"]))
    tg = T.distinct(R.ball_targets(sb.read(1)["balls"], 3, W, H))
    assert len(tg) == 2 and got[1]["targets"].tolist() == [list(t) for t in tg]
    assert np.isfinite(got[1]["cost"]).all() and (got[1]["act"] != 3).all()
    assert tuple(got[1]["path"][0]) == (400, 479) and tuple(got[1]["path"][-1]) == tg[got[1]["order"][-1]]
    sb.close(); sc.close()


@pytest.mark.gpu
def test_staged_frames_to_turn_tours(built):
    """The step's pipeline without the engine: stage_frames (one copy for all slots) -> append(SANE) -> plan_turn_tour; frame b
    equals Scene.append_classified -> plan_turn_tour on that frame."""
    import yolact_amd as ya
    H, W, n = 40, 48, 3
    frames = _frames(H, W, n, 515)
    depths = np.stack([d for d, _ in frames])
    packed = np.stack([ya.SceneBatch.pack(ci) for _, ci in frames])
    sb, sc = ya.SceneBatch(W, H, n), ya.Scene(W, H)
    sb.stage_frames(0, depths, frames_u32=packed)
    sb.append(n, ya.COMPAT_SANE)
    starts, headings = [(40, 30), (10, 35), (24, 39)], [6, 2, 4]
    assert sb.plan_turn_tour(n_targets=2, starts=starts, headings=headings, turn_price=1.5) == [0] * n
    for b in range(n):
        sc.append_classified(depths[b], frame_u32=packed[b], mode=ya.COMPAT_SANE)
        assert _same(sb.read_turn_tour(b), _single_tour(sc, None, 2, starts[b], headings[b], 1.5)), b
    sb.close(); sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["plan, turn, tour", "tour, turn, plan"])
def test_the_batchs_three_planners_do_not_disturb_one_another(built, order):
    import yolact_amd as ya
    H, W, n = 40, 48, 2
    frames = _frames(H, W, n, 31)
    targets, starts = [[(3, 3), (30, 20)], [(44, 2), (8, 30)]], [(40, 30), (10, 35)]
    sb = ya.SceneBatch(W, H, n)
    for b, (depth, ci) in enumerate(frames):
        sb.stage(b, depth, cls_id=ci)
    sb.append(n, ya.COMPAT_SANE)
    assert _code(lambda: sb.read_turn_tour(0)) == ya.capi.ESTATE and _code(lambda: sb.turn_tour_time(1)) == ya.capi.ESTATE   # none yet
    run = {"plan": lambda: sb.plan(targets=targets, starts=starts, connectivity=8),
           "turn": lambda: sb.plan_turn(targets=targets, starts=starts, headings=[1, 4], turn_price=3.0),
           "tour": lambda: sb.plan_turn_tour(targets=targets, starts=starts, headings=[1, 4], turn_price=3.0)}
    read = {"plan": sb.read_plan, "turn": sb.read_turn, "tour": sb.read_turn_tour}
    replay = {"plan": sb.plan_time, "turn": sb.turn_time, "tour": sb.turn_tour_time}
    seen = {}
    for kind in order.split(", "):
        assert run[kind]() == [0, 0]
        seen[kind] = [read[kind](b) for b in range(n)]
        replay[kind](2)
        for k in seen:                                                         # what was there before, and this one after its replay
            assert all(_same(read[k](b), seen[k][b]) for b in range(n)), (kind, k)
    for kind in order.split(", "):
        stats = replay[kind](1)
        assert stats["rounds"] >= 1 and stats["tile_runs"] >= stats["rounds"]
        for k in seen:
            assert all(_same(read[k](b), seen[k][b]) for b in range(n)), (kind, k)
    # the same tour as the single handle's, whatever ran beside it
    sc = ya.Scene(W, H)
    sc.append_classified(frames[1][0], frame_u32=ya.SceneBatch.pack(frames[1][1]), mode=ya.COMPAT_SANE)
    assert _same(seen["tour"][1], _single_tour(sc, targets[1], 0, starts[1], 4, 3.0))
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
    err = lambda: L.yh_scene_batch_last_error(h)
    starts = np.array([[40, 30], [10, 35]], np.int32)
    heads = np.array([6, 2], np.int32)
    tg = np.array([[[3, 3], [30, 20]], [[44, 2], [20, 9]]], np.int32)
    plan = lambda t=tg, s=starts, hd=heads, k=2, price=2.0: L.yh_scene_batch_plan_turn_tour(
        h, None if t is None else _p(t), k, None if s is None else _p(s), None if hd is None else _p(hd), price, None)
    assert plan() == capi.ESTATE                                            # before any append
    assert _code(lambda: sb.read_turn_tour(0)) == capi.ESTATE and _code(lambda: sb.turn_tour_time(1)) == capi.ESTATE
    for b in range(2):
        sb.stage(b, frames[b][0], cls_id=frames[b][1])
    sb.append(2, ya.COMPAT_STRICT)
    assert plan() == capi.ESTATE and b"STRICT" in err()
    sb.append(2, ya.COMPAT_SANE)
    assert plan() == capi.OK
    t = [sb.read_turn_tour(b) for b in range(2)]
    sc = ya.Scene(W, H)
    sc.append_classified(frames[1][0], frame_u32=ya.SceneBatch.pack(frames[1][1]), mode=ya.COMPAT_SANE)
    assert _same(t[1], _single_tour(sc, tg[1], 0, (10, 35), 2, 2.0))
    untouched = lambda: all(_same(sb.read_turn_tour(b), t[b]) for b in range(2))
    assert plan(s=None) == capi.EINVAL and untouched()
    assert plan(hd=None) == capi.EINVAL and untouched()
    for v in (8, -1):                                                       # a heading outside 0 .. 7, in frame 1 only
        bad = heads.copy(); bad[1] = v
        assert plan(hd=bad) == capi.EINVAL and b"frame 1" in err() and untouched()
    for price in (float("nan"), float("inf"), 0.5, 2048.0):
        assert plan(price=price) == capi.EINVAL and b"turn price" in err() and untouched()
    out = tg.copy(); out[1, 1] = (W, 2)                                     # a target outside the frame, in frame 1 only
    assert plan(t=out) == capi.EINVAL and b"frame 1" in err() and untouched()
    off = starts.copy(); off[1] = (3, H)                                    # a start outside the frame, in frame 1 only
    assert plan(s=off) == capi.EINVAL and b"frame 1" in err() and untouched()
    assert plan(k=0) == capi.EINVAL and untouched()
    seven = np.zeros((2, 7, 2), np.int32); seven[:, :, 0] = np.arange(7)
    assert plan(t=seven, k=7) == capi.EINVAL and b"YH_TOUR_MAX" in err() and untouched()
    assert plan(t=None, k=7) == capi.EINVAL and b"YH_TOUR_MAX" in err() and untouched()
    dup = tg.copy(); dup[1, 1] = dup[1, 0]                                  # two equal targets, in frame 1 only
    assert plan(t=dup) == capi.EINVAL and b"frame 1" in err() and b"duplicate" in err() and untouched()
    # path_capacity too small: YH_EOVERFLOW with the needed length, nothing written - for each of path_xy, directions and turns
    n = len(t[1]["path"])
    assert n > 2
    for which in range(3):
        cnt, k = ctypes.c_int32(-1), ctypes.c_int32(-1)
        small = np.full(2 * (n - 1), -7, np.int32)
        ptr = [None, None, None]
        ptr[which] = small.ctypes.data_as(ctypes.c_void_p)
        rc = L.yh_scene_batch_turn_tour_read(h, 1, ctypes.byref(k), None, None, None, None, None, None, None, None, None, ptr[0], ptr[1], ptr[2], None, n - 1, ctypes.byref(cnt))
        assert rc == capi.EOVERFLOW and cnt.value == n and (small == -7).all() and k.value == -1 and b"path_capacity" in err()
    assert _code(lambda: sb.read_turn_tour(2)) == capi.EINVAL and _code(lambda: sb.read_turn_tour(-1)) == capi.EINVAL
    assert untouched()
    assert plan() == capi.OK and untouched()                                # twice on one append: the same bits
    # n_targets grows from 2 to 4 on one handle: the buffers are reallocated, the old result is gone, the new one is right
    tg4 = np.array([[[3, 3], [30, 20], [45, 38], [0, 39]], [[44, 2], [20, 9], [47, 0], [5, 5]]], np.int32)
    assert plan(t=tg4, k=4) == capi.OK
    for b in range(2):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        got = sb.read_turn_tour(b)
        assert got["cost"].shape == (4, 8, H, W) and not _same(got, t[b])
        assert _same(got, _single_tour(sc, tg4[b], 0, tuple(int(v) for v in starts[b]), int(heads[b]), 2.0)), b
    assert plan() == capi.OK and untouched()                                # and back to two, in the larger buffers
    sb.append(1, ya.COMPAT_SANE)                                            # a newer append: the turn tour is gone
    assert _code(lambda: sb.read_turn_tour(0)) == capi.ESTATE and _code(lambda: sb.turn_tour_time(1)) == capi.ESTATE
    sb.close(); sc.close()
    # uploaded fields: a frame given none, a frame whose diagonals no SANE frame gives, no frame with a ball
    f = _random_fields(np.random.default_rng(1), H, W, 30)
    sb = ya.SceneBatch(W, H, 2)
    sb.set_fields(1, *f)
    assert _code(lambda: sb.plan_turn_tour(targets=tg, starts=starts, headings=heads)) == capi.ESTATE
    assert b"frame 0" in sb.L.yh_scene_batch_last_error(sb.h) and b"no fields" in sb.L.yh_scene_batch_last_error(sb.h)
    sb.set_fields(0, *f)
    assert sb.plan_turn_tour(targets=tg, starts=starts, headings=heads) == [0, 0]
    c0 = f[1].copy(); c0[5, 6, 3] = 0.5
    sb.set_fields(1, f[0], c0, f[2])
    assert _code(lambda: sb.plan_turn_tour(targets=tg, starts=starts, headings=heads)) == capi.ESTATE
    assert b"frame 1" in sb.L.yh_scene_batch_last_error(sb.h) and b"4-connected" in sb.L.yh_scene_batch_last_error(sb.h)
    assert _code(lambda: sb.read_turn_tour(0)) == capi.ESTATE               # set_fields counts as a newer frame
    sb.set_fields(1, *f)
    assert _code(lambda: sb.plan_turn_tour(targets=None, starts=starts, headings=heads)) == capi.ESTATE   # uploaded fields have no balls
    assert b"no frame of the batch" in sb.L.yh_scene_batch_last_error(sb.h)
    sb.close(); sb.close()
    # between the planner's guard and the turn planner's: an 8-connected plan runs, a turn tour is refused
    H, W = 2894, 3
    assert R.size_ok(W, H) and not U.size_ok(W, H)
    sb = ya.SceneBatch(W, H, 1)
    sb.set_fields(0, *T.flat_fields(H, W))
    assert sb.plan(targets=[[(1, 0)]], starts=[(1, 5)], connectivity=8) == [0]
    assert _code(lambda: sb.plan_turn_tour(targets=[[(1, 0)]], starts=[(1, 5)])) == capi.EINVAL
    assert b"8 * 1024" in sb.L.yh_scene_batch_last_error(sb.h)
    assert _code(lambda: sb.read_turn_tour(0)) == capi.ESTATE
    sb.close()
    # destroy after a turn tour only, and starts=None away from 640 x 480
    sb = ya.SceneBatch(12, 9, 1)
    sb.set_fields(0, *T.flat_fields(9, 12))
    with pytest.raises(ValueError):
        sb.plan_turn_tour(targets=[[(1, 1)]])
    assert sb.plan_turn_tour(targets=[[(3, 3)]], starts=[(3, 3)], headings=2, turn_price=1.0) == [0]
    got = sb.read_turn_tour(0)
    assert got["path"].tolist() == [[3, 3]] and got["directions"].shape == (0, 2) and got["turns"].shape == (0,) and got["leg_headings"].tolist() == [2]
    sb.close()


@pytest.mark.gpu
def test_a_batched_turn_tour_of_eight_beats_eight_single_ones(built):
    """640 x 480, n = 8, camera-like frames, each frame's own balls: stage x 8 + append + plan_turn_tour of the batch against eight
    Scene.append_classified + plan_turn_tour, all in this process. A Scene holds one frame, so bringing each frame in is part of
    planning eight frames through it; the batch's side carries the same work for the same frames. Alternated, one warm-up each,
    median of five. The assertion is batch < eight singles: a ratio of 1 or more would mean the feature has no purpose - that is the
    whole condition, no ratio is fixed in advance. The two medians and the ratio are printed."""
    import yolact_amd as ya
    n = 8
    frames = [_camera_frame(b) for b in range(n)]
    packed = [ya.SceneBatch.pack(ci) for _, ci in frames]
    sb, sc = ya.SceneBatch(640, 480, n), ya.Scene(640, 480)

    def batch():
        for b in range(n):
            sb.stage(b, frames[b][0], frame_u32=packed[b])
        sb.append(n, ya.COMPAT_SANE)
        assert sb.plan_turn_tour() == [0] * n

    def singles():
        for b in range(n):
            sc.append_classified(frames[b][0], frame_u32=packed[b], mode=ya.COMPAT_SANE)
            sc.plan_turn_tour()

    def clock(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

    batch(); singles()                                                      # warm-up: buffers, code objects
    assert _same(sb.read_turn_tour(n - 1, fields=False), sc.read_turn_tour(fields=False))
    tb, ts = [], []
    for _ in range(5):
        tb.append(clock(batch)); ts.append(clock(singles))
    mb, ms = sorted(tb)[2], sorted(ts)[2]
    print(f"bring in + turn tour of {n} frames: batch {mb:.3f} ms, {n} singles {ms:.3f} ms, ratio {mb / ms:.3f}")
    assert mb < ms
    sb.close(); sc.close()
