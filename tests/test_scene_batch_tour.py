"""The scene batch's tour (yh_scene_batch_plan_tour, DESIGN.md §11 "Scene batch: tours"): yh_scene_plan_tour_conn for every frame of a
batch in shared solver rounds, on the one driver that also serves the single handle. The definition is the single handle's: frame b
equals, bit for bit, what Scene.plan_tour gives on that frame alone - targets, order, leg matrix, total, the K cost and successor
fields, the label, the joined route with its directions and leg ends. Every comparison is on bit patterns (array_equal, floats
through their u32 view), against a Scene in the same process and against the restatement (tests/tour_ref.py). There is no tolerance
anywhere. CPU part: the surface. GPU part (-m gpu): a scene as the batch of one, frame bases that are no multiple of a wave, a
ragged K (field z = b Kmax + f, not b K_b + f), a maze beside easy frames, round 0's flags per field and frame, successive calls on
one handle, independence from the batch's other three planners, every refusal, the chain from the engine's instance batch, and a
floor on time (a batched tour of eight frames must beat eight single ones)."""
import ctypes
import inspect
import os
import re
import time

import numpy as np
import pytest

import instance_ref as I
import path_ref as R
import tour_ref as T
from test_instance_batch import evaluated  # noqa: F401  (the fixture: seeded weights, three frames evaluated, the class map)
from test_scene import _frame
from test_scene_batch import SP_BATCH, _bits, _camera_frame, _code, _frames
from test_scene_path8 import _fields_scene, _random_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"targets", "order", "legs", "total", "path", "directions", "leg_ends"}


def _same(a, b):
    """The same keys, shapes, dtypes and bits."""
    return a.keys() == b.keys() and all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype
                                        and np.array_equal(_bits(np.asarray(a[k])), _bits(np.asarray(b[k]))) for k in a)


# ---------------------------------------------------------------- CPU

def test_batch_tour_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0]: s for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read(), flags=re.S)
    for name, text, other, nargs in (("yh_scene_batch_plan_tour", pub, dbg, 6), ("yh_scene_batch_tour_read", pub, dbg, 15),
                                     ("yh_scene_batch_tour_time", dbg, pub, 5)):
        assert re.search(r"\b%s\s*\(" % name, text) and not re.search(r"\b%s\s*\(" % name, other) and name in bound, name
        assert len(bound[name][2]) == nargs, name
    # the batched read takes the frame, then exactly the single read's arguments; the batched plan those of yh_scene_batch_plan
    assert bound["yh_scene_batch_tour_read"][2][2:] == bound["yh_scene_tour_read"][2][1:]
    assert bound["yh_scene_batch_plan_tour"][2] == bound["yh_scene_batch_plan"][2]
    assert "#define YH_ABI_VERSION 4" in pub and "#define YH_TOUR_MAX 6" in pub


def test_library_exports_the_batch_tour_symbols(built):
    from yolact_amd import capi
    L = capi.load_library()
    for name in ("yh_scene_batch_plan_tour", "yh_scene_batch_tour_read", "yh_scene_batch_tour_time"):
        assert hasattr(L, name), name


def test_scene_batch_has_the_tour_methods_with_their_defaults():
    from yolact_amd import capi
    for m in ("plan_tour", "read_tour", "tour_time"):
        assert callable(getattr(capi.SceneBatch, m)), m
    sig = inspect.signature(capi.SceneBatch.plan_tour).parameters
    assert list(sig)[1:] == ["targets", "n_targets", "starts", "connectivity"]
    assert sig["targets"].default is None and sig["n_targets"].default == 3 and sig["starts"].default is None and sig["connectivity"].default == 4
    sig = inspect.signature(capi.SceneBatch.read_tour).parameters
    assert list(sig)[1:] == ["b", "fields"] and sig["fields"].default is False
    assert inspect.signature(capi.SceneBatch.tour_time).parameters["reps"].default == 20
    # Scene's methods keep their signatures
    sig = inspect.signature(capi.Scene.plan_tour).parameters
    assert list(sig)[1:] == ["targets", "n_targets", "start", "connectivity"] and sig["n_targets"].default == 3 and sig["connectivity"].default == 4
    assert list(inspect.signature(capi.Scene.read_tour).parameters)[1:] == ["fields"] and inspect.signature(capi.Scene.read_tour).parameters["fields"].default is False


# ---------------------------------------------------------------- GPU

def _single_tour(sc, targets, n_targets, start, conn, fields=True):
    """Scene.plan_tour + read_tour, or the error code of a refused call."""
    import yolact_amd as ya
    try:
        sc.plan_tour(targets=targets, n_targets=n_targets, start=start, connectivity=conn)
    except ya.YhError as e:
        return e.code
    return sc.read_tour(fields=fields)


def _ref(f, targets, start, conn):
    """tour_ref's tour as read_tour(fields=True) returns it."""
    want = T.tour(*f, targets, start, conn)
    want["total"] = np.float32(want["total"])
    return want


def _ball_frame(H, W, seed, balls):
    """test_scene._frame without its balls, then one pixel per ball: balls = [(id, column, row, depth)]. A ball's target is
    (its column, a row that follows from its depth), so balls in different columns are different targets and two balls of one
    depth on neighbouring rows of one column fall on one pixel."""
    depth, ci = _frame(np.random.default_rng(seed), H, W, balls=False)
    for k, x, y, d in balls:
        ci[y, x] = (3, k)
        depth[y, x] = d
    return depth, ci


def _fields_batch(fs, max_frames=None):
    import yolact_amd as ya
    H, W = fs[0][0].shape
    sb = ya.SceneBatch(W, H, max_frames or len(fs))
    for b, f in enumerate(fs):
        sb.set_fields(b, *f)
    return sb


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [4, 8])
def test_a_scene_is_the_batch_of_one(built, conn):
    """40 x 36: 2 x 2 tiles of 32 x 32, ragged on both axes; one target on the corner pixel of tile (0, 0), the other across both
    borders in tile (1, 1). One driver serves both handles: the same keys, shapes, dtypes and bits, the same solver counters, and both
    equal to tour_ref."""
    import yolact_amd as ya
    W, H = 40, 36
    f = _random_fields(np.random.default_rng(4036), H, W)
    targets, start = [(31, 31), (32, 33)], (2, 34)
    sc, sb = _fields_scene(f), _fields_batch([f])
    sc.plan_tour(targets=targets, start=start, connectivity=conn)
    assert sb.plan_tour(targets=[targets], starts=[start], connectivity=conn) == [ya.capi.OK]
    one, got, t_one, t_got = sc.read_tour(fields=True), sb.read_tour(0, fields=True), sc.tour_time(1), sb.tour_time(1)
    assert _same(one, got) and set(got) == KEYS | {"cost", "next", "label"}
    want = _ref(f, targets, start, conn)
    assert _same(got, want), [k for k in want if not np.array_equal(_bits(np.asarray(got[k])), _bits(np.asarray(want[k])))]
    print(f"conn {conn}: scene {t_one}, batch of one {t_got}")
    assert t_one["rounds"] == t_got["rounds"] and t_one["tile_runs"] == t_got["tile_runs"]
    assert _same(sc.read_tour(fields=True), one) and _same(sb.read_tour(0, fields=True), got)   # the replays left the same bits
    sb.close(); sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [4, 8])
def test_frame_bases_that_are_not_aligned(built, conn):
    """7 x 3, n = 6, Kmax = 3: a frame is 21 pixels, less than a wave, and no field, label or route starts on a multiple of anything.
    Explicit targets; frame 4 starts on one of its targets. Every frame against a Scene fed that frame, and against tour_ref."""
    import yolact_amd as ya
    H, W, n = 3, 7, 6
    fs = [_random_fields(np.random.default_rng(70 + b), H, W, 9) for b in range(n)]
    targets = [[(0, 0), (6, 2), (3, 1)], [(6, 0), (0, 2), (1, 1)], [(3, 0), (3, 2), (5, 1)], [(2, 2), (4, 0), (0, 1)], [(1, 0), (5, 2), (6, 1)], [(4, 1), (2, 1), (3, 1)]]
    starts = [(3, 2), (3, 1), (0, 0), (6, 2), (1, 0), (0, 2)]
    sb = _fields_batch(fs)
    assert sb.plan_tour(targets=targets, starts=starts, connectivity=conn) == [ya.capi.OK] * n
    got = [sb.read_tour(b, fields=True) for b in range(n)]
    for b in range(n):
        sc = _fields_scene(fs[b])
        assert _same(got[b], _single_tour(sc, targets[b], 0, starts[b], conn)), b
        assert _same(got[b], _ref(fs[b], targets[b], starts[b], conn)), b
        short = sb.read_tour(b)
        assert set(short) == KEYS and all(np.array_equal(short[k], got[b][k]) for k in short)
        sc.close()
    assert got[4]["legs"][0, 0] == 0 and got[4]["order"][0] == 0 and got[4]["leg_ends"][0] == 0
    sb.close()


# per frame: [(id, column, row, depth)] as fractions of the frame - 3, 1, 0 and 2 usable balls, three balls two of them on one
# pixel, and 3
def _ragged(H, W):
    x = lambda v: int(v * (W - 1))
    y = lambda v: int(v * (H - 1))
    return [
        [(5, x(0.2), y(0.4), 2000), (9, x(0.8), y(0.7), 1500), (40, x(0.5), y(0.1), 3000)],
        [(7, x(0.7), y(0.6), 2500)],
        [],
        [(1, x(0.3), y(0.3), 2000), (3, x(0.9), y(0.8), 1000)],
        [(1, x(0.3), y(0.3), 2000), (2, x(0.3), y(0.3) + 1, 2000), (3, x(0.9), y(0.8), 1000)],
        [(2, x(0.1), y(0.9), 1200), (4, x(0.6), y(0.2), 2600), (8, x(0.95), y(0.5), 1800)],
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(17, 33), (33, 65)])
def test_ragged_k_with_the_frames_own_balls(built, H, W):
    """Appended frames (33 x 17: one pixel past a tile border; 65 x 33: 3 x 2 tiles, the last partial both ways), NULL targets,
    n_targets = 3: K_b = 3, 1, 0, 2, 2 (two of three balls on one pixel), 3. K_b < Kmax in the middle of the batch is what tells field
    z = b Kmax + f from b K_b + f. Frame 2 has no ball: YH_ESTATE, no tour, its read refused."""
    import yolact_amd as ya
    n = 6
    frames = [_ball_frame(H, W, 300 + b, balls) for b, balls in enumerate(_ragged(H, W))]
    sb, sc = ya.SceneBatch(W, H, n), ya.Scene(W, H)
    for b, (depth, ci) in enumerate(frames):
        sb.stage(b, depth, cls_id=ci)
    sb.append(n, ya.COMPAT_SANE)
    fields = [sb.read(b) for b in range(n)]
    raw = [R.ball_targets(f["balls"], 3, W, H) for f in fields]
    want_targets = [T.distinct(t) for t in raw]
    assert [len(t) for t in raw] == [3, 1, 0, 2, 3, 3] and [len(t) for t in want_targets] == [3, 1, 0, 2, 2, 3]
    starts = [(W // 2, H - 1), (1, 1), (W - 2, 1), (0, H - 2), (W - 1, 0), (W // 3, H // 2)]
    for conn in (4, 8):
        status = sb.plan_tour(targets=None, n_targets=3, starts=starts, connectivity=conn)
        assert status == [ya.capi.OK, ya.capi.OK, ya.capi.ESTATE, ya.capi.OK, ya.capi.OK, ya.capi.OK]
        for b in range(n):
            sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
            want = _single_tour(sc, None, 3, starts[b], conn)
            if b == 2:
                assert want == ya.capi.ESTATE and _code(lambda: sb.read_tour(2)) == ya.capi.ESTATE
                assert b"frame 2" in sb.L.yh_scene_batch_last_error(sb.h)
                continue
            got = sb.read_tour(b, fields=True)
            assert _same(got, want), (conn, b)
            K = len(want_targets[b])
            assert got["targets"].tolist() == [list(t) for t in want_targets[b]] and got["cost"].shape == (K, H, W) and got["legs"].shape == (K + 1, K)
            f = (fields[b]["map"], fields[b]["conn0"], fields[b]["conn1"])
            assert _same(got, _ref(f, want_targets[b], starts[b], conn)), (conn, b)
    # fewer balls asked for than some frames have: Kmax = 1, every planned frame has K_b = 1
    assert sb.plan_tour(targets=None, n_targets=1, starts=starts) == status
    for b in (0, 4, 5):
        sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
        assert _same(sb.read_tour(b, fields=True), _single_tour(sc, None, 1, starts[b], 4)), b
    sb.close(); sc.close()


@pytest.mark.gpu
def test_a_maze_beside_easy_frames(built):
    """A flat map, the serpentine and another flat map at 96 x 96, K = 2 each, in one call: the serpentine's fields take more than
    SP_BATCH rounds, so the host loop goes round again - and tour_legs writes every frame's matrix again - while the other frames'
    fields have long converged. Every frame equals its single tour; the batch's rounds are within SP_BATCH of the maze's alone."""
    import yolact_amd as ya
    S = 96
    serp, s_start, s_target = R.serpentine(S, S)
    maps = [np.zeros((S, S), np.uint32), serp, np.zeros((S, S), np.uint32)]
    targets, starts = [[(5, 7), (80, 20)], [s_target, (48, 44)], [(50, 30), (3, 90)]], [(90, 80), s_start, (2, 93)]
    assert all(serp[y, x] == 0 for x, y in targets[1] + [s_start])
    fs = [(m,) + R.sane_connections(m) for m in maps]
    sb, sc = _fields_batch(fs, 4), ya.Scene(S, S)
    want, rounds = [], []
    for b in range(3):
        sc.set_fields(*fs[b])
        want.append(_single_tour(sc, targets[b], 0, starts[b], 4))
        rounds.append(sc.tour_time(1)["rounds"])
    print(f"single tours at {S}x{S}: rounds {rounds}")
    assert rounds[1] > SP_BATCH and rounds[0] < SP_BATCH and rounds[2] < SP_BATCH
    assert sb.plan_tour(targets=targets, starts=starts) == [0, 0, 0]
    for b in range(3):
        assert _same(sb.read_tour(b, fields=True), want[b]), b
    stats = sb.tour_time(1)
    print(f"batch of 3: {stats}")
    assert abs(stats["rounds"] - rounds[1]) <= SP_BATCH and stats["tile_runs"] >= stats["rounds"]
    for b in range(3):
        assert _same(sb.read_tour(b, fields=True), want[b]), b                  # the replay left the same bits
    sb.close(); sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,targets,starts", [
    (64, 64, [[(31, 31), (32, 32), (0, 32), (63, 31)], [(32, 31), (31, 32), (63, 32), (0, 31)], [(0, 0), (63, 63), (32, 0), (31, 63)]], [(5, 60), (60, 5), (33, 33)]),
    (3, 64, [[(31, 1), (32, 1)], [(32, 0), (31, 2)], [(0, 1), (63, 1)]], [(63, 2), (0, 0), (32, 2)]),
    (64, 3, [[(1, 31), (1, 32)], [(0, 32), (2, 31)], [(1, 0), (1, 63)]], [(0, 0), (2, 63), (1, 33)]),
])
def test_round_zero_flags_per_field_and_frame(built, H, W, targets, starts):
    """Each field has ONE target: on a tile's last row / column, on its first, in a corner of four tiles - in different tiles per
    frame. Round 0 must wake field z's tiles across those borders (no field may lean on another field's or another frame's flags)."""
    import yolact_amd as ya
    n = 3
    fs = [_random_fields(np.random.default_rng(H + W + b), H, W, 30) for b in range(n)]
    sb = _fields_batch(fs)
    for conn in (4, 8):
        assert sb.plan_tour(targets=targets, starts=starts, connectivity=conn) == [0] * n
        for b in range(n):
            got = sb.read_tour(b, fields=True)
            assert np.isfinite(got["cost"]).all()
            assert _same(got, _ref(fs[b], targets[b], starts[b], conn)), (conn, b)
    sc = _fields_scene(fs[2])
    assert _same(sb.read_tour(2, fields=True), _single_tour(sc, targets[2], 0, starts[2], 8))
    sb.close(); sc.close()


@pytest.mark.gpu
def test_succession_on_one_handle(built):
    """n = 5 then n = 2 (frames 2 .. 4 are outside the last append), n_targets 2 then 4 (the buffers grow: the earlier tour is gone
    until planned again), connectivity 4 then 8, and a new append makes the tour unreadable."""
    import yolact_amd as ya
    from yolact_amd import capi
    H, W = 40, 48
    frames = _frames(H, W, 5, 123)
    sb, sc = ya.SceneBatch(W, H, 5), ya.Scene(W, H)
    tg2 = [[(3, 3), (30, 20)], [(44, 2), (20, 9)], [(1, 38), (47, 39)], [(31, 31), (32, 32)], [(10, 10), (11, 10)]]
    tg4 = [t + [(45, 38), (0, 39)] for t in tg2]
    starts = [(40, 30), (10, 35), (24, 0), (0, 0), (47, 20)]

    def append(n):
        for b in range(n):
            sb.stage(b, frames[b][0], cls_id=frames[b][1])
        sb.append(n, ya.COMPAT_SANE)

    def check(n, tg, conn):
        for b in range(n):
            sc.append_classified(frames[b][0], frame_u32=ya.SceneBatch.pack(frames[b][1]), mode=ya.COMPAT_SANE)
            assert _same(sb.read_tour(b, fields=True), _single_tour(sc, tg[b], 0, starts[b], conn)), (n, conn, b)

    append(5)
    assert sb.plan_tour(targets=tg2, starts=starts) == [0] * 5
    check(5, tg2, 4)
    append(2)
    assert _code(lambda: sb.read_tour(0)) == capi.ESTATE                    # a newer append: the tour is gone
    assert sb.plan_tour(targets=tg2[:2], starts=starts[:2]) == [0, 0]
    check(2, tg2, 4)
    for b in (2, 3, 4):
        assert _code(lambda: sb.read_tour(b)) == capi.EINVAL, b
    two = [sb.read_tour(b, fields=True) for b in range(2)]
    assert sb.plan_tour(targets=tg4[:2], starts=starts[:2]) == [0, 0]       # the buffers grow
    check(2, tg4, 4)
    assert sb.read_tour(0, fields=True)["cost"].shape == (4, H, W) and not _same(sb.read_tour(0, fields=True), two[0])
    assert sb.plan_tour(targets=tg2[:2], starts=starts[:2]) == [0, 0]       # and back to two, in the larger buffers
    assert all(_same(sb.read_tour(b, fields=True), two[b]) for b in range(2))
    assert sb.plan_tour(targets=tg2[:2], starts=starts[:2], connectivity=8) == [0, 0]
    check(2, tg2, 8)
    assert not _same(sb.read_tour(1, fields=True), two[1])
    assert sb.tour_time(2)["rounds"] >= 1                                    # the replay has the last call's connectivity
    check(2, tg2, 8)
    append(5)
    assert _code(lambda: sb.read_tour(0)) == capi.ESTATE and _code(lambda: sb.tour_time(1)) == capi.ESTATE
    sb.close(); sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["plan, tour, turn, turn_tour", "turn_tour, turn, tour, plan", "tour, plan, turn_tour, turn"])
def test_the_batchs_four_planners_do_not_disturb_one_another(built, order):
    import yolact_amd as ya
    H, W, n = 40, 48, 2
    frames = _frames(H, W, n, 31)
    targets, starts = [[(3, 3), (30, 20)], [(44, 2), (8, 30)]], [(40, 30), (10, 35)]
    sb = ya.SceneBatch(W, H, n)
    for b, (depth, ci) in enumerate(frames):
        sb.stage(b, depth, cls_id=ci)
    sb.append(n, ya.COMPAT_SANE)
    assert _code(lambda: sb.read_tour(0)) == ya.capi.ESTATE and _code(lambda: sb.tour_time(1)) == ya.capi.ESTATE   # none yet
    run = {"plan": lambda: sb.plan(targets=targets, starts=starts, connectivity=8),
           "tour": lambda: sb.plan_tour(targets=targets, starts=starts, connectivity=8),
           "turn": lambda: sb.plan_turn(targets=targets, starts=starts, headings=[1, 4], turn_price=3.0),
           "turn_tour": lambda: sb.plan_turn_tour(targets=targets, starts=starts, headings=[1, 4], turn_price=3.0)}
    read = {"plan": sb.read_plan, "tour": lambda b: sb.read_tour(b, fields=True), "turn": sb.read_turn, "turn_tour": sb.read_turn_tour}
    replay = {"plan": sb.plan_time, "tour": sb.tour_time, "turn": sb.turn_time, "turn_tour": sb.turn_tour_time}
    seen = {}
    for kind in order.split(", "):
        assert run[kind]() == [0, 0]
        seen[kind] = [read[kind](b) for b in range(n)]
        replay[kind](2)
        for k in seen:                                                         # what was there before, and this one after its replay
            assert all(_same(read[k](b), seen[k][b]) for b in range(n)), (kind, k)
    # the same tour as the single handle's, whatever ran beside it
    sc = ya.Scene(W, H)
    sc.append_classified(frames[1][0], frame_u32=ya.SceneBatch.pack(frames[1][1]), mode=ya.COMPAT_SANE)
    assert _same(seen["tour"][1], _single_tour(sc, targets[1], 0, starts[1], 8))
    sb.close(); sc.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_previous_tour_readable(built):
    import yolact_amd as ya
    from yolact_amd import capi
    from yolact_amd.capi import _p
    H, W = 40, 48
    frames = _frames(H, W, 2, 77)
    sb = ya.SceneBatch(W, H, 2)
    L, h = sb.L, sb.h
    err = lambda: L.yh_scene_batch_last_error(h)
    starts = np.array([[40, 30], [10, 35]], np.int32)
    tg = np.array([[[3, 3], [30, 20]], [[44, 2], [20, 9]]], np.int32)
    plan = lambda t=tg, s=starts, k=2, conn=4: L.yh_scene_batch_plan_tour(h, None if t is None else _p(t), k, None if s is None else _p(s), conn, None)
    assert plan() == capi.ESTATE                                            # before any append
    assert _code(lambda: sb.read_tour(0)) == capi.ESTATE and _code(lambda: sb.tour_time(1)) == capi.ESTATE
    for b in range(2):
        sb.stage(b, frames[b][0], cls_id=frames[b][1])
    sb.append(2, ya.COMPAT_STRICT)
    assert plan() == capi.ESTATE and b"STRICT" in err()
    sb.append(2, ya.COMPAT_SANE)
    assert plan() == capi.OK
    t = [sb.read_tour(b, fields=True) for b in range(2)]
    sc = ya.Scene(W, H)
    sc.append_classified(frames[1][0], frame_u32=ya.SceneBatch.pack(frames[1][1]), mode=ya.COMPAT_SANE)
    assert _same(t[1], _single_tour(sc, tg[1], 0, (10, 35), 4))
    untouched = lambda: all(_same(sb.read_tour(b, fields=True), t[b]) for b in range(2))
    assert plan(s=None) == capi.EINVAL and untouched()
    for conn in (0, 5, 6, 16):
        assert plan(conn=conn) == capi.EINVAL and b"4 or 8" in err() and untouched()
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
    # path_capacity too small: YH_EOVERFLOW with the needed length, nothing written - for each of path_xy and directions
    n = len(t[1]["path"])
    assert n > 2
    for which in range(2):
        cnt, k = ctypes.c_int32(-1), ctypes.c_int32(-1)
        small = np.full(2 * (n - 1), -7, np.int32)
        ptr = [None, None]
        ptr[which] = small.ctypes.data_as(ctypes.c_void_p)
        rc = L.yh_scene_batch_tour_read(h, 1, ctypes.byref(k), None, None, None, None, None, None, None, ptr[0], ptr[1], None, n - 1, ctypes.byref(cnt))
        assert rc == capi.EOVERFLOW and cnt.value == n and (small == -7).all() and k.value == -1 and b"path_capacity" in err()
    assert _code(lambda: sb.read_tour(2)) == capi.EINVAL and _code(lambda: sb.read_tour(-1)) == capi.EINVAL
    assert untouched()
    assert plan() == capi.OK and untouched()                                # twice on one append: the same bits
    sb.close(); sc.close()
    # uploaded fields: a frame given none, a frame whose diagonals no SANE frame gives (connectivity 8 only), no frame with a ball
    f = _random_fields(np.random.default_rng(1), H, W, 30)
    sb = ya.SceneBatch(W, H, 2)
    sb.set_fields(1, *f)
    assert _code(lambda: sb.plan_tour(targets=tg, starts=starts)) == capi.ESTATE
    assert b"frame 0" in sb.L.yh_scene_batch_last_error(sb.h) and b"no fields" in sb.L.yh_scene_batch_last_error(sb.h)
    sb.set_fields(0, *f)
    c0 = f[1].copy(); c0[5, 6, 3] = 0.5
    sb.set_fields(1, f[0], c0, f[2])
    assert sb.plan_tour(targets=tg, starts=starts, connectivity=4) == [0, 0]
    t = [sb.read_tour(b, fields=True) for b in range(2)]
    assert _code(lambda: sb.plan_tour(targets=tg, starts=starts, connectivity=8)) == capi.ESTATE
    assert b"frame 1" in sb.L.yh_scene_batch_last_error(sb.h) and b"4-connected" in sb.L.yh_scene_batch_last_error(sb.h)
    assert all(_same(sb.read_tour(b, fields=True), t[b]) for b in range(2))
    assert _code(lambda: sb.plan_tour(targets=None, starts=starts)) == capi.ESTATE   # uploaded fields have no balls
    assert b"no frame of the batch" in sb.L.yh_scene_batch_last_error(sb.h)
    assert all(_same(sb.read_tour(b, fields=True), t[b]) for b in range(2))
    sb.close(); sb.close()
    # the planner's size guard
    H, W = 2895, 3
    assert not R.size_ok(W, H)
    sb = ya.SceneBatch(W, H, 1)
    sb.set_fields(0, *T.flat_fields(H, W))
    assert _code(lambda: sb.plan_tour(targets=[[(1, 0)]], starts=[(1, 5)])) == capi.EINVAL
    assert b"too large" in sb.L.yh_scene_batch_last_error(sb.h)
    sb.close()
    # starts=None away from 640 x 480, a start on the only target, and destroy with a tour live
    sb = ya.SceneBatch(12, 9, 1)
    sb.set_fields(0, *T.flat_fields(9, 12))
    with pytest.raises(ValueError):
        sb.plan_tour(targets=[[(1, 1)]])
    assert sb.plan_tour(targets=[[(3, 3)]], starts=[(3, 3)]) == [0]
    got = sb.read_tour(0)
    assert got["path"].tolist() == [[3, 3]] and got["directions"].shape == (0, 2) and got["leg_ends"].tolist() == [0]
    sb.close()


@pytest.mark.gpu
def test_the_chain_from_the_instance_batch_stays_on_the_device(evaluated):
    """Engine.instance_batch(read=False) -> stage_frames(frames_dev_ptr) -> append(SANE) -> plan_tour(), the class images never on
    the host: every read_tour(b) has the bits of a scene batch fed instance_ref's frames from the host."""
    import yolact_amd as ya
    eng, cm = evaluated["eng"], evaluated["cm"]
    W, H, n = 64, 48, 3
    depths = np.stack([_frame(np.random.default_rng(40 + b), H, W)[0] for b in range(n)])
    a, s = ya.SceneBatch(W, H, n), ya.SceneBatch(W, H, n)
    assert eng.instance_batch(0, n, W, H, class_map=cm, read=False) is None
    a.stage_frames(0, depths, frames_dev_ptr=eng.instance_batch_device_frames())
    host = []
    for b in range(n):
        dets, masks = eng.detections(b)
        host.append(I.instance_frame(masks, [d["class_id"] for d in dets], [d["score"] for d in dets], W, H, class_map=cm)[0])
    s.stage_frames(0, depths, frames_u32=np.stack(host))
    a.append(n, ya.COMPAT_SANE); s.append(n, ya.COMPAT_SANE)
    starts = [(40, 47), (5, 5), (60, 20)]
    sa, ss = a.plan_tour(starts=starts), s.plan_tour(starts=starts)          # NULL targets: each frame's own balls
    assert sa == ss and ya.capi.OK in sa
    for b in range(n):
        if sa[b] == ya.capi.OK:
            assert _same(a.read_tour(b, fields=True), s.read_tour(b, fields=True)), b
        else:
            assert _code(lambda: a.read_tour(b)) == ya.capi.ESTATE
    a.close(); s.close()


def _camera_frame3(seed):
    """test_scene_batch._camera_frame with a third ball."""
    depth, ci = _camera_frame(seed)
    ci[300:315, 100:125] = (3, 6)
    return depth, ci


@pytest.mark.gpu
def test_a_batched_tour_of_eight_beats_eight_single_ones(built):
    """640 x 480, n = 8, camera-like frames with three balls, n_targets = 3, on one append each side: plan_tour of the batch against
    eight Scene.plan_tour calls (a Scene holds one frame, so each of its frames is brought in before its tour; bringing frames in is
    timed on neither side). Alternated, one warm-up each, median of five. The assertion is batch < eight singles: a ratio of 1 or
    more would mean the batch has no purpose - that is the whole condition, no ratio is fixed in advance. The two medians and the
    ratio are printed."""
    import yolact_amd as ya
    n = 8
    frames = [_camera_frame3(b) for b in range(n)]
    packed = [ya.SceneBatch.pack(ci) for _, ci in frames]
    sb, scs = ya.SceneBatch(640, 480, n), [ya.Scene(640, 480) for _ in range(n)]
    for b in range(n):
        sb.stage(b, frames[b][0], frame_u32=packed[b])
        scs[b].append_classified(frames[b][0], frame_u32=packed[b], mode=ya.COMPAT_SANE)
    sb.append(n, ya.COMPAT_SANE)

    def batch():
        assert sb.plan_tour() == [0] * n

    def singles():
        for sc in scs:
            sc.plan_tour()

    def clock(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

    batch(); singles()                                                      # warm-up: buffers, code objects
    for b in (0, n - 1):
        got = sb.read_tour(b)
        assert _same(got, scs[b].read_tour()) and len(got["targets"]) == 3
    tb, ts = [], []
    for _ in range(5):
        tb.append(clock(batch)); ts.append(clock(singles))
    mb, ms = sorted(tb)[2], sorted(ts)[2]
    print(f"tour of {n} frames: batch {mb:.3f} ms, {n} singles {ms:.3f} ms, ratio {mb / ms:.3f}")
    assert mb < ms
    for sc in scs:
        sc.close()
    sb.close()
