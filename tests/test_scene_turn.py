"""The turn-aware planner (yh_scene_plan_turn / yh_scene_turn_read; DESIGN.md §11 "Turns"). CPU part: the restatement
(tests/turn_ref.py) against itself - a heap Dijkstra and Jacobi sweeps over (pixel, heading) bit for bit -, hand cases, the relation
to the 8-connected planner and what the turn price does to a route. GPU part (-m gpu): the HIP field, action field, route, turns and
directions bit-equal to the restatement on the engine's own scene fields and on constructed ones, the full frame through its
equations, every start heading, the prices, independence from plans and tours, every error, the life cycle and a floor on time.
Every comparison is on bit patterns; there is no tolerance anywhere."""
import inspect
import os
import re
import struct
import time

import numpy as np
import pytest

import path8_ref as P
import path_ref as R
import tour_ref as T
import turn_ref as U
from test_scene import _frame
from test_scene_path8 import _bits, _fields_scene, _raises, _random_fields, _same, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUGH = dict(H=40, W=56, seed=11, targets=[(5, 7), (50, 30)], start=(28, 39))     # the seeded rough field of the CPU cases


def _rough():
    return _random_fields(np.random.default_rng(ROUGH["seed"]), ROUGH["H"], ROUGH["W"])


# ---------------------------------------------------------------- CPU

@pytest.mark.parametrize("H,W,targets", [(40, 56, ROUGH["targets"]), (96, 128, [(5, 7), (120, 80)])])
@pytest.mark.parametrize("tau", [1.0, 4.0])
def test_dijkstra_equals_jacobi_bit_for_bit(H, W, targets, tau):
    f = _random_fields(np.random.default_rng(11), H, W)
    a = U.dijkstra(*f, targets, tau)
    b, sweeps = U.jacobi(*f, targets, tau)
    assert a.shape == (8, H, W) and a.dtype == np.float32
    assert np.array_equal(_bits(a), _bits(b)) and sweeps > 10
    assert U.equation_residual(a, *f, targets, tau) == 0
    assert np.isfinite(a).all() and (a == 0).sum() == 8 * len(targets)
    # d[h][v] <= fl(d[h +- 1][v] + tau) everywhere
    t = np.float32(tau)
    assert (a <= np.roll(a, 1, 0) + t).all() and (a <= np.roll(a, -1, 0) + t).all()
    worse = a.copy(); worse[3, 5, 5] += 1
    assert U.equation_residual(worse, *f, targets, tau) > 0


def test_flat_map_by_hand():
    """5 x 5, flat, unit edges, tau = 1, target (0, 2). From (4, 2): facing left it is four drives; every 45 degrees away from left
    costs one more, both ways round, 8 when facing right - where counter-clockwise wins the tie."""
    f = T.flat_fields(5, 5)
    tg = [(0, 2)]
    d = U.dijkstra(*f, tg, 1.0)
    assert np.array_equal(_bits(d), _bits(U.jacobi(*f, tg, 1.0)[0]))
    assert d[:, 2, 4].tolist() == [8, 7, 6, 5, 4, 5, 6, 7]
    assert d[4, 2].tolist() == [0, 1, 2, 3, 4]                                   # straight values along the row, facing left
    act = U.actions(d, *f, tg, 1.0)
    assert act[:, 2, 4].tolist() == [U.CCW, U.CW, U.CW, U.CW, U.DRIVE, U.CCW, U.CCW, U.CCW]
    assert d[6, 2, 4] == 6 and act[6, 2, 4] == U.CCW and act[5, 2, 4] == U.CCW    # facing up: two turns, then the four drives
    assert (act[:, 2, 0] == U.AT_TARGET).all() and (d[:, 2, 0] == 0).all()
    root2 = np.float32(np.sqrt(np.float32(2)))
    assert _bits(d[3, 1, 1]) == _bits(root2) and act[3, 1, 1] == U.DRIVE          # (1, 1) facing down-left: one diagonal
    path, dirs, turns = U.walk(d, act, (4, 2), 6)
    assert path.tolist() == [[4, 2], [3, 2], [2, 2], [1, 2], [0, 2]] and turns.tolist() == [-2, 0, 0, 0]
    assert np.array_equal(_bits(dirs), _bits(np.array([[1, R.ROT[2]], [1, R.ROT[0]], [1, R.ROT[0]], [1, R.ROT[0]]], np.float32)))


def test_drive_wins_its_tie_with_a_turn():
    """Flat 5 x 5, tau = 1, targets (0, 0) and (3, 1). At (0, 1) facing right: three drives to (3, 1) cost 3, and so does turning
    to up-right, where one more turn and one drive up reach (0, 0): the candidates tie bitwise and the action is the drive."""
    f = T.flat_fields(5, 5)
    tg = [(0, 0), (3, 1)]
    d = U.dijkstra(*f, tg, 1.0)
    drive, ccw, cw = U.candidates(d, *f, 1.0)
    assert d[0, 1, 0] == 3 and d[7, 1, 0] == 2 and d[6, 1, 0] == 1
    assert drive[0, 1, 0] == 3 and ccw[0, 1, 0] == 3 and cw[0, 1, 0] > 3
    assert U.actions(d, *f, tg, 1.0)[0, 1, 0] == U.DRIVE
    path, _, turns = U.walk(d, U.actions(d, *f, tg, 1.0), (0, 1), 0)
    assert path.tolist() == [[0, 1], [1, 1], [2, 1], [3, 1]] and turns.tolist() == [0, 0, 0]


def test_three_nodes_with_a_reversal():
    """A flat 4 x 3 frame's middle row: start (2, 1) facing right, the target (0, 1) directly behind. Both ways round tie at every
    step and counter-clockwise wins: turns = -4 and rot = 0 at the start, then one straight drive more."""
    f = T.flat_fields(3, 4)
    tg = [(0, 1)]
    d = U.dijkstra(*f, tg, 1.0)
    act = U.actions(d, *f, tg, 1.0)
    assert d[0, 1, 2] == 6 and act[0, 1, 2] == U.CCW
    path, dirs, turns = U.walk(d, act, (2, 1), 0)
    assert path.tolist() == [[2, 1], [1, 1], [0, 1]] and turns.tolist() == [-4, 0]
    assert np.array_equal(_bits(dirs), _bits(np.array([[1, 0], [1, np.pi]], np.float32)))
    path, dirs, turns = U.walk(d, act, (0, 1), 3)                                  # start on a target: one node, nothing else
    assert path.tolist() == [[0, 1]] and dirs.shape == (0, 2) and turns.shape == (0,)


def test_never_cheaper_than_the_eight_connected_plan():
    f, tg = _rough(), ROUGH["targets"]
    d8 = R.dijkstra(*f, tg, conn=8)
    for tau in (1.0, 4.0):
        d = U.dijkstra(*f, tg, tau)
        assert (d.min(0) >= d8).all() and (d.min(0) > d8).sum() > d8.size // 2


def test_turn_price_straightens_the_route():
    """The seeded rough field: the 8-connected route changes heading at most of its steps; with tau = 4 strictly fewer steps turn."""
    f, tg, start = _rough(), ROUGH["targets"], ROUGH["start"]
    d8 = R.dijkstra(*f, tg, conn=8)
    p8, _ = R.walk(d8, R.successors(d8, *f, tg, conn=8), start, conn=8)
    steps8, total8 = U.turning_steps(p8)
    seen = {}
    for tau in (1.0, 4.0):
        d = U.dijkstra(*f, tg, tau)
        path, dirs, turns = U.walk(d, U.actions(d, *f, tg, tau), start, 6)
        assert tuple(path[-1]) in tg and tuple(path[0]) == start and len(dirs) == len(turns) == len(path) - 1
        assert (np.abs(turns) <= 4).all()
        assert (np.abs(np.diff(path, axis=0)).max(1) == 1).all()
        assert np.array_equal(_bits(dirs[:, 1]), _bits(np.array([R.ROT[abs(int(t))] for t in turns], np.float32)))
        assert U.turning_steps(path) == (int((turns[1:] != 0).sum()), int(np.abs(turns[1:]).sum()))
        seen[tau] = int((turns != 0).sum())
        print(f"tau {tau}: {len(path)} nodes, {seen[tau]} steps with a turn, {int(np.abs(turns).sum())} x 45 degrees; 8-connected: {len(p8)} nodes, {steps8} / {total8}")
    assert seen[4.0] < steps8 and seen[4.0] <= seen[1.0]


def test_serialiser_takes_the_pairs_as_they_are():
    from yolact_amd import capi
    f, tg = _rough(), ROUGH["targets"]
    d = U.dijkstra(*f, tg, 4.0)
    _, dirs, _ = U.walk(d, U.actions(d, *f, tg, 4.0), ROUGH["start"], 6)
    blob = capi.serialize_path(dirs, 1700000000)
    assert len(blob) == 8 + 8 * len(dirs) and struct.unpack(">Q", blob[:8])[0] == 1700000000
    back = np.frombuffer(blob[8:], ">f4").astype(np.float32).reshape(-1, 2)
    assert np.array_equal(_bits(back), _bits(dirs))


def test_size_guard():
    assert U.size_ok(640, 480) and U.size_ok(1440, 1440) and not U.size_ok(2048, 2048)
    assert R.size_ok(3, 2894) and not U.size_ok(3, 2894)                           # between the two guards


def test_turn_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0]: s for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read(), flags=re.S)
    for name, text, nargs in (("yh_scene_plan_turn", pub, 7), ("yh_scene_turn_read", pub, 8), ("yh_scene_turn_time", dbg, 5)):
        assert re.search(r"\b%s\s*\(" % name, text) and name in bound, name
        assert len(bound[name][2]) == nargs
    assert "#define YH_ABI_VERSION 4" in pub
    sig = inspect.signature(capi.Scene.plan_turn).parameters
    assert sig["heading"].default == 6 and "turn_price" in sig and hasattr(capi.Scene, "turn_time")


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


def _scene_fields(sc):
    r = sc.read()
    return r["map"], r["conn0"], r["conn1"]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,targets,start", [
    (8, 8, [(7, 0)], (0, 7)),                      # one partial tile
    (33, 33, [(30, 2)], (1, 32)),                  # the corner tile is 1 x 1, ragged edges
    (37, 53, [(2, 3), (50, 30)], (26, 36)),        # a general small frame
    (100, 9, [(4, 50)], (0, 0)),                   # a thin frame
])
def test_field_bit_equal_to_the_restatement(built, H, W, targets, start):
    """The engine's own Scene.read() fields go through turn_ref's Dijkstra; field, actions and route must have the same bits."""
    sc = _scene(H, W, H * 1000 + W)
    f = _scene_fields(sc)
    sc.plan_turn(targets=targets, start=start, turn_price=2.0)
    want = _check_turn(sc.read_turn(), f, targets, start, 6, 2.0)
    print(f"{W}x{H}: max cost {want.max()}, {sc.turn_time(1)}")
    sc.close()


@pytest.mark.gpu
def test_targets_on_tile_corners(built):
    f = _random_fields(np.random.default_rng(64), 64, 64, 30)
    sc = _fields_scene(f)
    tg = [(31, 31), (32, 32)]
    sc.plan_turn(targets=tg, start=(5, 60), turn_price=2.0)
    got = sc.read_turn()
    assert np.isfinite(got["cost"]).all()
    _check_turn(got, f, tg, (5, 60), 6, 2.0)
    sc.close()


@pytest.mark.gpu
def test_late_corner_on_the_device(built):
    """path8_ref.late_corner(): the cheap way into the diagonal tile is through one corner cell that settles late - the diagonal
    wake-up, in eight layers."""
    f = P.late_corner()
    sc = _fields_scene(f)
    sc.plan_turn(targets=[(0, 0)], start=(63, 63), turn_price=1.0)
    _check_turn(sc.read_turn(), f, [(0, 0)], (63, 63), 6, 1.0)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,target,start,heading,first", [
    (3, 130, (129, 1), (0, 1), 4, -4),             # one heading layer carried across four tiles, after a reversal
    (130, 3, (1, 129), (1, 0), 6, -4),
    (70, 70, (69, 69), (0, 0), 6, 3),              # a diagonal layer across tile corners: up -> down-right is three steps clockwise
])
def test_flat_strips_and_the_diagonal(built, H, W, target, start, heading, first):
    f = T.flat_fields(H, W)
    sc = _fields_scene(f)
    sc.plan_turn(targets=[target], start=start, heading=heading, turn_price=3.0)
    got = sc.read_turn()
    _check_turn(got, f, [target], start, heading, 3.0)
    assert got["turns"][0] == first and (got["turns"][1:] == 0).all()
    assert len(got["path"]) == max(H, W) and _bits(got["directions"][0, 1]) == _bits(R.ROT[abs(first)])
    print(f"{W}x{H}: {sc.turn_time(1)}")
    sc.close()


@pytest.mark.gpu
def test_serpentine(built):
    H, W = 96, 128
    hmap, start, target = R.serpentine(H, W)
    f = (hmap,) + R.sane_connections(hmap)
    sc = _fields_scene(f)
    sc.plan_turn(targets=[target], start=start, heading=0, turn_price=2.0)
    got = sc.read_turn()
    _check_turn(got, f, [target], start, 0, 2.0)
    print(f"serpentine {W}x{H}: route of {len(got['path'])} nodes, {sc.turn_time(1)}")
    sc.close()


@pytest.mark.gpu
def test_full_frame_satisfies_its_equations_at_every_state(built):
    """640 x 480, ball targets: no +inf left and the defining equations hold bitwise at every state - by uniqueness that is the field."""
    H, W, tau = 480, 640, 2.0
    sc = _scene(H, W, 5)
    r = sc.read()
    f = (r["map"], r["conn0"], r["conn1"])
    sc.plan_turn(turn_price=tau)
    got = sc.read_turn()
    tg = R.ball_targets(r["balls"], 3, W, H)
    assert len(tg) == 2
    d = got["cost"]
    assert np.isfinite(d).all() and d.max() < 2 ** 24
    assert all((d[:, y, x] == 0).all() for x, y in tg) and (d == 0).sum() == 8 * len(tg)
    assert U.equation_residual(d, *f, tg, tau) == 0
    t = np.float32(tau)
    assert (d <= np.roll(d, 1, 0) + t).all() and (d <= np.roll(d, -1, 0) + t).all()
    sc.plan(connectivity=8)
    d8 = sc.read_plan()["cost"]
    assert (d.min(0) >= d8).all() and (d.min(0) > d8).any()
    act = U.actions(d, *f, tg, tau)
    assert np.array_equal(got["act"], act) and (act == U.AT_TARGET).sum() == 8 * len(tg) and (act != 3).all()
    path, dirs, turns = U.walk(d, act, (400, 479), 6)
    assert np.array_equal(got["path"], path) and np.array_equal(got["turns"], turns) and np.array_equal(_bits(got["directions"]), _bits(dirs))
    assert tuple(path[0]) == (400, 479) and tuple(path[-1]) in tg and (np.abs(turns) <= 4).all()
    hd = np.array([R._COMPASS[(int(a), int(b))] for a, b in np.diff(path, axis=0)])
    cost = d[np.append(hd, hd[-1]), path[:, 1], path[:, 0]]                          # along the walk, in the heading driven
    assert (np.diff(cost) < 0).all() and cost[-1] == 0
    print(f"route of {len(path)} nodes, {int((turns != 0).sum())} steps with a turn, {sc.turn_time(1)}")
    sc.close()


@pytest.mark.gpu
def test_every_start_heading_and_the_prices(built):
    H, W = 37, 53
    sc = _scene(H, W, H * 1000 + W)
    f = _scene_fields(sc)
    tg, start = [(2, 3), (50, 30)], (26, 36)
    want = {}
    for tau in (2.5, 1.0, 1024.0):
        d = want[tau] = U.dijkstra(*f, tg, tau)
        act = U.actions(d, *f, tg, tau)
        for heading in (range(8) if tau == 2.5 else (6,)):
            sc.plan_turn(targets=tg, start=start, heading=heading, turn_price=tau)
            got = sc.read_turn()
            assert np.array_equal(_bits(got["cost"]), _bits(d)) and np.array_equal(got["act"], act), (tau, heading)
            path, dirs, turns = U.walk(d, act, start, heading)
            assert np.array_equal(got["path"], path) and np.array_equal(got["turns"], turns), (tau, heading)
            assert np.array_equal(_bits(got["directions"]), _bits(dirs)), (tau, heading)
    assert not np.array_equal(want[1.0], want[2.5]) and (want[1024.0] >= want[2.5]).all()
    sc.close()


@pytest.mark.gpu
def test_plans_tour_and_turn_plan_do_not_disturb_one_another(built):
    sc = _scene(70, 90, 3)
    f = _scene_fields(sc)
    tg, start = [(5, 5), (80, 60)], (40, 69)
    sc.plan_turn(targets=tg, start=start, turn_price=2.0)
    t0 = sc.read_turn()
    _check_turn(t0, f, tg, start, 6, 2.0)
    sc.plan(targets=tg, start=start)
    p4 = sc.read_plan()
    assert _same(t0, sc.read_turn())
    sc.plan_tour(targets=tg, start=start, connectivity=8)
    tour = sc.read_tour(fields=True)
    assert _same(t0, sc.read_turn()) and _same(p4, sc.read_plan())
    sc.plan(targets=tg, start=start, connectivity=8)
    p8 = sc.read_plan()
    assert _same(t0, sc.read_turn()) and _same(tour, sc.read_tour(fields=True))
    sc.plan_turn(targets=tg[:1], start=start, heading=1, turn_price=5.0)           # another turn plan beside them
    t1 = sc.read_turn()
    _check_turn(t1, f, tg[:1], start, 1, 5.0)
    assert _same(p8, sc.read_plan()) and _same(tour, sc.read_tour(fields=True)) and not _same(t0, t1)
    assert np.array_equal(_bits(p8["cost"]), _bits(R.dijkstra(*f, tg, conn=8)))
    stats = sc.turn_time(3)                                                        # the replay has the plan's heading and price
    assert _same(t1, sc.read_turn()) and stats["rounds"] >= 1 and stats["tile_runs"] >= stats["rounds"]
    sc.plan_time(2); sc.tour_time(2)
    assert _same(t1, sc.read_turn()) and _same(p8, sc.read_plan()) and _same(tour, sc.read_tour(fields=True))
    sc.close()


@pytest.mark.gpu
def test_errors_leave_the_last_turn_plan_readable(built):
    import yolact_amd as ya
    from yolact_amd import capi
    H, W = 40, 70
    f = _random_fields(np.random.default_rng(1), H, W, 30)
    sc = _fields_scene(f)
    tg, start = [(3, 3)], (60, 30)
    _raises(capi.ESTATE, lambda: sc.read_turn(), "no turn plan")
    _raises(capi.ESTATE, lambda: sc.turn_time(1), "no turn plan")
    sc.plan_turn(targets=tg, start=start, turn_price=2.0)
    a = sc.read_turn()
    _check_turn(a, f, tg, start, 6, 2.0)
    for heading in (-1, 8, 64):
        _raises(capi.EINVAL, lambda: sc.plan_turn(targets=tg, start=start, heading=heading, turn_price=2.0), "heading")
    for price in (np.nan, np.inf, -np.inf, 0.5, 0.0, -2.0, 1024.5, 1e30):
        _raises(capi.EINVAL, lambda: sc.plan_turn(targets=tg, start=start, turn_price=price), "turn price")
    _raises(capi.EINVAL, lambda: sc.plan_turn(targets=None, n_targets=0, start=start), "n_targets")
    _raises(capi.EINVAL, lambda: sc.plan_turn(targets=tg, start=(W, 0)), "start")
    _raises(capi.EINVAL, lambda: sc.plan_turn(targets=[(0, H)], start=start), "target")
    _raises(capi.ESTATE, lambda: sc.plan_turn(targets=None, start=start), "no ball")   # uploaded fields have no balls
    assert _same(a, sc.read_turn())                                                 # every refusal touched nothing
    n = len(a["path"])
    cnt = capi.C.c_int32()
    small = np.zeros(n - 1, np.int32)
    for args in ((small.ctypes.data, None, None), (None, small.ctypes.data, None), (None, None, small.ctypes.data)):
        assert sc.L.yh_scene_turn_read(sc.h, None, None, args[0], args[1], args[2], n // 2 - 1, capi.C.byref(cnt)) == capi.EOVERFLOW
        assert cnt.value == n and not small.any()
    assert _same(a, sc.read_turn())
    # diagonals no SANE frame gives: refused, and why; it counts as a new frame, of which no turn plan exists
    c0 = f[1].copy(); c0[5, 6, 3] = 0.5
    sc.set_fields(f[0], c0, f[2])
    _raises(capi.ESTATE, lambda: sc.plan_turn(targets=tg, start=start), "length")
    _raises(capi.ESTATE, lambda: sc.read_turn(), "newer frame")
    _raises(capi.ESTATE, lambda: sc.turn_time(1), "newer frame")
    sc.set_fields(*f)
    sc.plan_turn(targets=tg, start=start, turn_price=2.0)
    assert _same(a, sc.read_turn())
    sc.close()
    # frames: none, STRICT, SANE, and an append since the plan
    depth, ci = _frame(np.random.default_rng(2), H, W)
    sc = ya.Scene(W, H)
    _raises(capi.ESTATE, lambda: sc.plan_turn(targets=tg, start=start), "no frame")
    sc.append(depth, ci, ya.COMPAT_STRICT)
    _raises(capi.ESTATE, lambda: sc.plan_turn(targets=tg, start=start), "STRICT")
    sc.append(depth, ci, ya.COMPAT_SANE)
    sc.plan_turn(targets=tg, start=start, turn_price=2.0)
    b = sc.read_turn()
    _check_turn(b, _scene_fields(sc), tg, start, 6, 2.0)
    sc.append(depth, ci, ya.COMPAT_STRICT)
    _raises(capi.ESTATE, lambda: sc.plan_turn(targets=tg, start=start), "STRICT")
    _raises(capi.ESTATE, lambda: sc.read_turn(), "newer frame")
    sc.append(depth, ci, ya.COMPAT_SANE)
    _raises(capi.ESTATE, lambda: sc.read_turn(), "newer frame")
    sc.plan_turn(targets=tg, start=start, turn_price=2.0)
    assert _same(b, sc.read_turn())
    sc.close()


@pytest.mark.gpu
def test_size_guard_and_life_cycle(built):
    import yolact_amd as ya
    from yolact_amd import capi
    # between the planner's guard and the turn planner's: an 8-connected plan runs, a turn plan is refused
    H, W = 2894, 3
    sc = _fields_scene(T.flat_fields(H, W))
    _raises(capi.EINVAL, lambda: sc.plan_turn(targets=[(1, 0)], start=(1, 5)), "8 * 1024")
    sc.plan(targets=[(1, 0)], start=(1, 5), connectivity=8)
    assert len(sc.read_plan(fields=False)["path"]) == 6
    sc.close()
    # destroy after a turn plan only; start on a target; two handles side by side; a closed one is gone
    f = T.flat_fields(9, 12)
    a, b = _fields_scene(f), _fields_scene(f)
    a.plan_turn(targets=[(3, 3)], start=(3, 3), heading=2, turn_price=1.0)
    got = a.read_turn()
    assert got["path"].tolist() == [[3, 3]] and got["directions"].shape == (0, 2) and got["turns"].shape == (0,)
    b.plan_turn(targets=[(0, 0)], start=(11, 8), heading=0, turn_price=1.0)
    a.close()
    _check_turn(b.read_turn(), f, [(0, 0)], (11, 8), 0, 1.0)
    b.close(); b.close()


@pytest.mark.gpu
def test_turn_plan_beats_the_cpu_restatement(built):
    """A floor that catches a broken work list, not a target (tools/time_path.py --turn-price measures): at 96 x 128 a turn plan
    must beat turn_ref's numpy Jacobi solve of the same field, timed here on the same box."""
    H, W, tau = 96, 128, 2.0
    sc = _scene(H, W, 13)
    f = _scene_fields(sc)
    tg, start = [(5, 7), (120, 80)], (64, 95)
    sc.plan_turn(targets=tg, start=start, turn_price=tau)          # warm-up: buffers, code objects
    t0 = time.perf_counter()
    sc.plan_turn(targets=tg, start=start, turn_price=tau)
    gpu_s = time.perf_counter() - t0
    got = sc.read_turn()
    t0 = time.perf_counter()
    want, sweeps = U.jacobi(*f, tg, tau)
    cpu_s = time.perf_counter() - t0
    stats = sc.turn_time(10)
    print(f"turn plan 128x96: host wall {gpu_s * 1e3:.3f} ms, {stats}; numpy Jacobi {cpu_s:.3f} s in {sweeps} sweeps")
    assert np.array_equal(_bits(got["cost"]), _bits(want))
    assert gpu_s < cpu_s and stats["ms_per_plan"] * 1e-3 < cpu_s
    sc.close()
