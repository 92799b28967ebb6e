"""The turn-aware tour (yh_scene_plan_turn_tour / yh_scene_turn_tour_read; DESIGN.md §11 "Turn tour"): one turn-plan field per ball
solved in the same launches, the leg table with arrival headings, the visiting order of least total with every leg starting in the
heading the leg before arrived with, the joined route. CPU part: the restatement (tests/turn_tour_ref.py) against hand results,
against turn_ref and against the pixel tour; the ABI surface. GPU part (-m gpu): every output bit-equal to the restatement on
constructed fields, the full frame against the shipped Scene.plan_turn, the maze, independence from the other three planners, the
life cycle and every refusal, and a floor on time. Every comparison is on bit patterns; there is no tolerance anywhere."""
import ctypes as C
import functools
import inspect
import os
import re
import struct

import numpy as np
import pytest

import path_ref as R
import tour_ref as T
import turn_ref as U
import turn_tour_ref as X
from test_scene import _frame
from test_scene_path8 import _bits, _fields_scene, _raises, _random_fields, _same, _scene
from test_scene_turn import ROUGH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP = dict(targets=[(7, 0), (14, 0)], start=(10, 0), heading=0, tau=4.0)              # the issue's 1 x 20 strip
ROUGH4 = dict(targets=[(5, 7), (50, 30), (30, 3), (12, 35)], start=ROUGH["start"], heading=6)


def _f32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------- CPU

def test_strip_by_hand_headings_change_the_order():
    """Flat 1 x 20 strip, targets (7, 0) and (14, 0), start (10, 0) facing right, tau = 4. The pixel tour goes left first (3 + 7 = 10
    against 4 + 7 = 11). With headings carried, left first is a reversal, three drives, a reversal, seven drives: 16 + 3 + 16 + 7 = 42;
    right first is four drives, a reversal, seven drives: 4 + 16 + 7 = 27."""
    f = T.flat_fields(1, 20)
    t = X.turn_tour(*f, STRIP["targets"], STRIP["start"], STRIP["heading"], STRIP["tau"])
    assert X.tour_total(t["legs"], t["arrive"], (0, 1))[0] == 42 and X.tour_total(t["legs"], t["arrive"], (1, 0))[0] == 27
    assert tuple(t["order"]) == (1, 0) and t["total"] == 27 and t["total"].dtype == np.float32
    assert tuple(T.tour(*f, STRIP["targets"], STRIP["start"])["order"]) == (0, 1)              # the pixel tour
    assert t["path"][:, 0].tolist() == list(range(10, 15)) + list(range(13, 6, -1)) and t["leg_ends"].tolist() == [4, 11]
    turns = np.zeros(11, np.int32); turns[4] = -4                                              # the reversal at the junction, node 4
    assert np.array_equal(t["turns"], turns) and t["leg_headings"].tolist() == [0, 4]
    assert np.array_equal(_f32(t["directions"]), _f32([[1, R.ROT[abs(k)]] for k in turns]))
    assert t["legs"].shape == (17, 2) and t["arrive"].shape == (17, 2) and t["arrive"].dtype == np.uint8
    assert t["legs"][0].tolist() == [19, 4] and t["arrive"][0].tolist() == [4, 0]
    # row 1 + 8 a + h: from (t_a, h); on its own target 0 and the row's heading, else the strip's length and up to four turns
    for h in range(8):
        k = min(h, 8 - h)
        assert t["legs"][X.row_of(0, h)].tolist() == [0, 7 + 4 * k] and t["arrive"][X.row_of(0, h)].tolist() == [h, 0]
        assert t["legs"][X.row_of(1, h)].tolist() == [7 + 4 * (4 - k), 0] and t["arrive"][X.row_of(1, h)].tolist() == [4, h]
    assert t["label"].shape == (8, 1, 20) and t["label"][0, 0].tolist() == [0] * 8 + [1] * 12   # facing right: 7 is passed, 14 lies ahead
    assert t["label"][4, 0].tolist() == [0] * 14 + [1] * 6


def test_tie_goes_to_the_lexicographically_smallest_order():
    """Start (10, 0) facing up, targets (7, 0) and (13, 0), tau = 4: either way two turns, three drives, a reversal, six drives."""
    f = T.flat_fields(1, 20)
    for targets in ([(7, 0), (13, 0)], [(13, 0), (7, 0)]):
        t = X.turn_tour(*f, targets, (10, 0), 6, 4.0)
        assert X.tour_total(t["legs"], t["arrive"], (0, 1))[0] == 33 and X.tour_total(t["legs"], t["arrive"], (1, 0))[0] == 33
        assert tuple(t["order"]) == (0, 1) and t["total"] == 33 and tuple(t["path"][3]) == targets[0]
        assert abs(int(t["turns"][0])) == 2 and t["turns"][3] == -4 and t["leg_ends"].tolist() == [3, 9]


def test_start_on_a_target_adds_no_node_and_carries_the_heading():
    f = T.flat_fields(1, 20)
    t = X.turn_tour(*f, [(10, 0), (13, 0)], (10, 0), 4, 4.0)
    assert tuple(t["order"]) == (0, 1) and t["total"] == 19 and t["leg_ends"].tolist() == [0, 3] and t["leg_headings"].tolist() == [4, 0]
    assert t["path"][:, 0].tolist() == [10, 11, 12, 13] and t["turns"].tolist() == [-4, 0, 0]   # the start heading, turned at node 0
    assert np.array_equal(_f32(t["directions"]), _f32([[1, 0], [1, np.pi], [1, np.pi]]))
    t = X.turn_tour(*f, [(10, 0)], (10, 0), 3, 4.0)
    assert t["path"].tolist() == [[10, 0]] and t["directions"].shape == (0, 2) and t["turns"].shape == (0,)
    assert t["leg_ends"].tolist() == [0] and t["leg_headings"].tolist() == [3] and t["total"] == 0


@functools.lru_cache(maxsize=None)
def _rough4(tau):
    f = _random_fields(np.random.default_rng(ROUGH["seed"]), ROUGH["H"], ROUGH["W"])
    return f, X.turn_tour(*f, ROUGH4["targets"], ROUGH4["start"], ROUGH4["heading"], tau)


@pytest.mark.parametrize("tau", [1.0, 4.0])
def test_rough_field_min_legs_and_labels(tau):
    f, t = _rough4(tau)
    tg, K = ROUGH4["targets"], 4
    assert np.array_equal(_bits(np.minimum.reduce(t["cost"])), _bits(U.dijkstra(*f, tg, tau)))    # the multi-target turn plan's field
    lab = np.zeros(t["label"].shape, np.uint8)
    best = t["cost"][0].copy()
    for b in range(1, K):
        lab[t["cost"][b] < best] = b
        best = np.minimum(best, t["cost"][b])
    assert np.array_equal(t["label"], lab) and all((t["label"][:, y, x] == b).all() for b, (x, y) in enumerate(tg))
    for b, (x, y) in enumerate(tg):                                                               # field b: 0 and 255 at t_b only
        assert (t["cost"][b] == 0).sum() == 8 and (t["cost"][b][:, y, x] == 0).all()
        assert (t["act"][b] == U.AT_TARGET).sum() == 8 and (t["act"][b][:, y, x] == U.AT_TARGET).all() and (t["act"][b] != 3).all()
    # each leg is turn_ref.walk from the carried state; the total is the f32 sum of the legs' start costs, left to right
    pos, g, at, total = ROUGH4["start"], ROUGH4["heading"], 0, np.float32(0)
    for j, b in enumerate(t["order"]):
        path, dirs, turns = U.walk(t["cost"][b], t["act"][b], pos, g)
        n = len(path) - 1
        assert np.array_equal(t["path"][at:at + n + 1], path) and np.array_equal(t["turns"][at:at + n], turns)
        assert np.array_equal(_bits(t["directions"][at:at + n]), _bits(dirs))
        total = np.float32(total + t["cost"][b][g, pos[1], pos[0]])
        at, g, pos = at + n, (g + int(turns.sum())) % 8, tg[b]
        assert t["leg_ends"][j] == at and t["leg_headings"][j] == g and tuple(t["path"][at]) == pos
    assert _bits(total) == _bits(t["total"]) and len(t["path"]) == at + 1 and (np.abs(t["turns"]) <= 4).all()
    totals = {o: X.tour_total(t["legs"], t["arrive"], o)[0] for o in __import__("itertools").permutations(range(K))}
    assert min(totals.values()) == t["total"] and [o for o in sorted(totals) if totals[o] == t["total"]][0] == tuple(t["order"])
    assert (np.diag(t["legs"][1::8]) == 0).all() and t["legs"][0].tolist() == [float(t["cost"][b][6, 39, 28]) for b in range(K)]
    print(f"tau {tau}: order {t['order'].tolist()}, total {t['total']}, route of {len(t['path'])} nodes, arrival headings {t['leg_headings'].tolist()}")


def test_turn_tour_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0]: s for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read(), flags=re.S)
    for name, text, nargs in (("yh_scene_plan_turn_tour", pub, 7), ("yh_scene_turn_tour_read", pub, 17), ("yh_scene_turn_tour_time", dbg, 5)):
        assert re.search(r"\b%s\s*\(" % name, text) and name in bound, name
        assert len(bound[name][2]) == nargs
    assert not re.search(r"\byh_scene_turn_tour_time\s*\(", pub)
    assert "#define YH_ABI_VERSION 4" in pub and "#define YH_TOUR_MAX 6" in pub and capi.TOUR_MAX == X.TOUR_MAX == 6
    sig = inspect.signature(capi.Scene.plan_turn_tour).parameters
    assert sig["heading"].default == 6 and sig["turn_price"].default == 2.0 and sig["n_targets"].default == 3
    assert inspect.signature(capi.Scene.read_turn_tour).parameters["fields"].default is True and callable(capi.Scene.turn_tour_time)


# ---------------------------------------------------------------- GPU

FIELDS = ("cost", "act", "label")


def _check(got, f, targets, start, heading, tau, want=None):
    """Everything read_turn_tour() returns against turn_tour_ref on the fields f = (map, conn0, conn1); returns want."""
    from yolact_amd import capi
    want = want if want is not None else X.turn_tour(*f, targets, start, heading, tau)
    K = len(targets)
    assert got["targets"].tolist() == [list(t) for t in targets] and got["cost"].shape == (K, 8) + f[0].shape
    for b, t in enumerate(targets):
        assert np.array_equal(_bits(got["cost"][b]), _bits(want["cost"][b])), f"field {b}"
        assert U.equation_residual(got["cost"][b], *f, [t], tau) == 0, f"field {b}"           # (does not rest on the Dijkstra)
        assert np.array_equal(got["act"][b], want["act"][b]), f"field {b}"
    assert got["label"].dtype == np.uint8 and np.array_equal(got["label"], want["label"])
    assert np.array_equal(_bits(got["legs"]), _bits(want["legs"])) and np.array_equal(got["arrive"], want["arrive"])
    assert got["order"].tolist() == want["order"].tolist() and _f32(got["total"]) == _f32(want["total"])
    assert np.array_equal(got["path"], want["path"]) and np.array_equal(got["turns"], want["turns"])
    assert np.array_equal(_bits(got["directions"]), _bits(want["directions"]))
    assert got["leg_ends"].tolist() == want["leg_ends"].tolist() and got["leg_headings"].tolist() == want["leg_headings"].tolist()
    assert (np.abs(got["turns"]) <= 4).all() and got["path"][got["leg_ends"]].tolist() == [list(targets[o]) for o in got["order"]]
    wire = capi.serialize_path(got["directions"], 1700000000)
    assert struct.unpack(">Q", wire[:8])[0] == 1700000000
    assert np.array_equal(_bits(np.frombuffer(wire[8:], ">f4").astype(np.float32).reshape(-1, 2)), _bits(got["directions"]))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,targets,start,heading", [
    (8, 8, [(7, 0), (0, 0), (3, 4), (4, 3), (7, 7), (0, 6)], (0, 7), 6),                   # one tile, smaller than a tile; K = 6
    (37, 53, [(2, 3), (50, 30)], (26, 36), 1),                                              # ragged tiles
    (100, 9, [(4, 50)], (0, 0), 2),                                                         # K = 1
    (33, 65, [(64, 32), (3, 3), (32, 31)], (10, 30), 6),                                    # one pixel past a tile border
    # targets on x = 0 and x = 31 mod 32, on y = 31 mod 32, and at the corner of four tiles (y = 0 mod 32 too): round 0's flags per field
    (96, 128, [(32, 10), (95, 70), (50, 63), (31, 32)], (64, 95), 6),
])
def test_fields_tables_order_and_route_equal_the_restatement(built, H, W, targets, start, heading):
    f = _random_fields(np.random.default_rng(H * 1000 + W), H, W)
    sc = _fields_scene(f)
    sc.plan_turn_tour(targets=targets, start=start, heading=heading, turn_price=2.0)
    got = sc.read_turn_tour()
    _check(got, f, targets, start, heading, 2.0)
    assert np.isfinite(got["cost"]).all()
    short = sc.read_turn_tour(fields=False)
    assert set(short) == set(got) - set(FIELDS) and all(np.array_equal(short[k], got[k]) for k in short)
    print(f"{W}x{H}: K = {len(targets)}, order {got['order'].tolist()}, total {got['total']}, route of {len(got['path'])} nodes, {sc.turn_tour_time(1)}")
    sc.close()


def _strip_scene():
    """A scene is at least 3 rows high, so the 1 x 20 strip is row 1 of a 3 x 20 frame between two walls of height 400 (a step onto
    a wall costs more than 800, the whole strip with two reversals 51): on the strip everything is as derived by hand."""
    hmap = np.full((3, 20), 400, np.uint32)
    hmap[1] = 0
    f = (hmap,) + R.sane_connections(hmap)
    return _fields_scene(f), f


@pytest.mark.gpu
@pytest.mark.parametrize("targets,start,heading,order,total,turns_at,leg_headings", [
    (STRIP["targets"], STRIP["start"], 0, [1, 0], 27, {4: -4}, [0, 4]),                     # the issue's strip
    ([(7, 0), (13, 0)], (10, 0), 2, [0, 1], 33, {0: 2, 3: -4}, [4, 0]),                     # the tie (facing down: the wall is no way)
    ([(10, 0), (13, 0)], (10, 0), 4, [0, 1], 19, {0: -4}, [4, 0]),                          # a start on a target
])
def test_hand_cases_on_the_device(built, targets, start, heading, order, total, turns_at, leg_headings):
    row = lambda pts: [(x, 1) for x, _ in pts]
    sc, f = _strip_scene()
    sc.plan_turn_tour(targets=row(targets), start=(start[0], 1), heading=heading, turn_price=4.0)
    got = sc.read_turn_tour()
    _check(got, f, row(targets), (start[0], 1), heading, 4.0)
    assert got["order"].tolist() == order and got["total"] == total and got["leg_headings"].tolist() == leg_headings
    assert (got["path"][:, 1] == 1).all() and len(got["path"]) == total - 4 * sum(abs(v) for v in turns_at.values()) + 1
    assert {i: int(v) for i, v in enumerate(got["turns"]) if v} == turns_at
    strip = X.turn_tour(*T.flat_fields(1, 20), targets, start, heading, 4.0)                  # the 1 x 20 strip itself, on the CPU
    assert np.array_equal(got["legs"], strip["legs"]) and np.array_equal(got["arrive"], strip["arrive"])
    assert np.array_equal(got["path"][:, 0], strip["path"][:, 0]) and np.array_equal(got["turns"], strip["turns"])
    assert np.array_equal(_bits(got["directions"]), _bits(strip["directions"])) and got["leg_ends"].tolist() == strip["leg_ends"].tolist()
    sc.close()


@pytest.mark.gpu
def test_full_frame_against_the_shipped_turn_plan(built):
    """640 x 480, the camera-like frame, K = 3: every cost field and every leg against Scene.plan_turn with that single target and
    the carried state, the total against the f32 sum of those plans' start costs, the minimum against the multi-target plan."""
    import yolact_amd as ya
    H, W, tau = 480, 640, 2.0
    sc = ya.Scene(W, H)
    sc.append(*T.camera_like_frame(H, W), ya.COMPAT_SANE)
    targets, start, heading = [(70, 67), (515, 410), (320, 40)], (400, 479), 6
    sc.plan_turn_tour(targets=targets, start=start, heading=heading, turn_price=tau)
    got = sc.read_turn_tour()
    assert sorted(got["order"].tolist()) == [0, 1, 2] and np.isfinite(got["cost"]).all()
    pos, g, at, total = start, heading, 0, np.float32(0)
    for j, b in enumerate(got["order"]):
        sc.plan_turn(targets=[targets[b]], start=pos, heading=g, turn_price=tau)
        one = sc.read_turn()
        assert np.array_equal(_bits(got["cost"][b]), _bits(one["cost"])) and np.array_equal(got["act"][b], one["act"]), f"field {b}"
        n = len(one["path"]) - 1
        assert np.array_equal(got["path"][at:at + n + 1], one["path"]) and np.array_equal(got["turns"][at:at + n], one["turns"]), f"leg {j}"
        assert np.array_equal(_bits(got["directions"][at:at + n]), _bits(one["directions"])), f"leg {j}"
        assert _bits(got["legs"][0 if j == 0 else X.row_of(got["order"][j - 1], g), b]) == _bits(one["cost"][g, pos[1], pos[0]])
        total = np.float32(total + one["cost"][g, pos[1], pos[0]])
        at, g, pos = at + n, (g + int(one["turns"].sum())) % 8, targets[b]
        assert got["leg_ends"][j] == at and got["leg_headings"][j] == g and tuple(got["path"][at]) == pos
    assert _f32(total) == _f32(got["total"]) and len(got["path"]) == at + 1
    legs, arrive = X.leg_tables(got["cost"], got["act"], targets, start, heading)                 # the tables from the device's fields
    assert np.array_equal(_bits(got["legs"]), _bits(legs)) and np.array_equal(got["arrive"], arrive)
    assert X.best_order(legs, arrive)[0] == tuple(got["order"])
    assert np.array_equal(got["label"], np.argmin(got["cost"], axis=0))
    sc.plan_turn(targets=targets, start=start, heading=heading, turn_price=tau)
    assert np.array_equal(_bits(np.minimum.reduce(got["cost"])), _bits(sc.read_turn()["cost"]))
    assert _same(got, sc.read_turn_tour())
    print(f"order {got['order'].tolist()}, total {got['total']}, route of {len(got['path'])} nodes, {sc.turn_tour_time(1)}")
    sc.close()


@pytest.mark.gpu
def test_maze_three_fields_in_the_rounds_of_the_slowest(built):
    """The serpentine corridor, targets at both ends and in the middle: the fields relax in the same launches, so the turn tour's
    rounds stay at or below those of the slowest single-target turn plan plus one batch of 16."""
    H, W, tau = 96, 128, 2.0
    hmap, end0, end1 = R.serpentine(H, W)
    targets, start = [end0, end1, (64, 44)], (30, 20)
    assert all(hmap[y, x] == 0 for x, y in targets + [start])
    f = (hmap,) + R.sane_connections(hmap)
    sc = _fields_scene(f)
    single = []
    for t in targets:
        sc.plan_turn(targets=[t], start=start, heading=0, turn_price=tau)
        single.append(sc.turn_time(1))
    sc.plan_turn_tour(targets=targets, start=start, heading=0, turn_price=tau)
    stats = sc.turn_tour_time(1)
    print(f"maze turn tour: {stats}; single-target turn plans: {single}")
    got = sc.read_turn_tour()
    _check(got, f, targets, start, 0, tau)
    assert stats["rounds"] <= max(s["rounds"] for s in single) + 16
    assert (hmap[got["path"][:, 1], got["path"][:, 0]] == 0).all()                # the route never leaves the corridor
    sc.close()


@pytest.mark.gpu
def test_the_four_planners_do_not_disturb_one_another(built):
    sc = _scene(70, 90, 3)
    r = sc.read()
    f = (r["map"], r["conn0"], r["conn1"])
    tg, start = [(5, 5), (80, 60), (40, 10)], (40, 69)
    sc.plan_turn_tour(targets=tg, start=start, turn_price=2.0)
    a = sc.read_turn_tour()
    _check(a, f, tg, start, 6, 2.0)
    sc.plan(targets=tg, start=start, connectivity=8)
    plan = sc.read_plan()
    sc.plan_tour(targets=tg, start=start, connectivity=8)
    tour = sc.read_tour(fields=True)
    sc.plan_turn(targets=tg, start=start, turn_price=2.0)
    turn = sc.read_turn()
    assert _same(a, sc.read_turn_tour())
    sc.plan_turn_tour(targets=tg[:2], start=start, heading=1, turn_price=5.0)      # another turn tour beside them
    b = sc.read_turn_tour()
    _check(b, f, tg[:2], start, 1, 5.0)
    assert _same(plan, sc.read_plan()) and _same(tour, sc.read_tour(fields=True)) and _same(turn, sc.read_turn()) and not _same(a, b)
    stats = sc.turn_tour_time(3)                                                   # the replay has the tour's heading and price
    assert _same(b, sc.read_turn_tour()) and stats["rounds"] >= 1 and stats["tile_runs"] >= stats["rounds"]
    sc.plan_time(2); sc.tour_time(2); sc.turn_time(2)
    assert _same(b, sc.read_turn_tour()) and _same(plan, sc.read_plan()) and _same(tour, sc.read_tour(fields=True)) and _same(turn, sc.read_turn())
    sc.close()


@pytest.mark.gpu
def test_refusals_leave_the_last_turn_tour_readable(built):
    import yolact_amd as ya
    from yolact_amd import capi
    H, W = 40, 70
    f = _random_fields(np.random.default_rng(1), H, W, 30)
    sc = _fields_scene(f)
    tg, start = [(3, 3), (60, 8)], (60, 30)
    _raises(capi.ESTATE, lambda: sc.read_turn_tour(), "no turn tour")
    _raises(capi.ESTATE, lambda: sc.turn_tour_time(1), "no turn tour")
    sc.plan_turn_tour(targets=tg, start=start, turn_price=2.0)
    a = sc.read_turn_tour()
    _check(a, f, tg, start, 6, 2.0)
    for heading in (-1, 8, 64):
        _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=tg, start=start, heading=heading), "heading")
    for price in (np.nan, np.inf, -np.inf, 0.5, 0.0, -2.0, 1024.5, 1e30):
        _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=tg, start=start, turn_price=price), "turn price")
    _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=None, n_targets=0, start=start), "n_targets")
    _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=None, n_targets=7, start=start), "YH_TOUR_MAX")
    _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=[(k, k) for k in range(7)], start=start), "YH_TOUR_MAX")
    _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=[(5, 5), (9, 9), (5, 5)], start=start), "duplicate")
    _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=tg, start=(W, 0)), "start")
    _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=[(0, H)], start=start), "target")
    _raises(capi.ESTATE, lambda: sc.plan_turn_tour(targets=None, start=start), "no ball")          # uploaded fields have no balls
    assert _same(a, sc.read_turn_tour())                                                           # every refusal touched nothing
    # path_capacity too small: YH_EOVERFLOW with the needed length, nothing written
    n = len(a["path"])
    for which in range(3):
        cnt, k = C.c_int32(-1), C.c_int32(-1)
        small = np.full(2 * (n - 1), -7, np.int32)
        ptr = [None, None, None]
        ptr[which] = small.ctypes.data_as(C.c_void_p)
        rc = sc.L.yh_scene_turn_tour_read(sc.h, C.byref(k), None, None, None, None, None, None, None, None, None, ptr[0], ptr[1], ptr[2], None, n - 1, C.byref(cnt))
        assert rc == capi.EOVERFLOW and cnt.value == n and (small == -7).all() and k.value == -1
        assert b"path_capacity" in sc.L.yh_scene_last_error(sc.h)
    assert _same(a, sc.read_turn_tour())
    sc.plan_turn_tour(targets=tg, start=start, turn_price=2.0)                                     # twice on one frame: the same bits
    assert _same(a, sc.read_turn_tour())
    # diagonals no SANE frame gives: refused, and why; it counts as a new frame, of which no turn tour exists
    c0 = f[1].copy(); c0[5, 6, 3] = 0.5
    sc.set_fields(f[0], c0, f[2])
    _raises(capi.ESTATE, lambda: sc.plan_turn_tour(targets=tg, start=start), "length")
    _raises(capi.ESTATE, lambda: sc.read_turn_tour(), "newer frame")
    _raises(capi.ESTATE, lambda: sc.turn_tour_time(1), "newer frame")
    sc.set_fields(*f)
    for K in (1, 2, 6, 3):                                                                         # the buffers grow with K and stay
        t = [(3 + 11 * k, 3 + 5 * k) for k in range(K)]
        sc.plan_turn_tour(targets=t, start=start, turn_price=2.0)
        got = sc.read_turn_tour()
        assert got["cost"].shape == (K, 8, H, W) and sorted(got["order"].tolist()) == list(range(K)) and got["legs"].shape == (1 + 8 * K, K)
        assert all((got["cost"][b][:, y, x] == 0).all() and (got["cost"][b] == 0).sum() == 8 for b, (x, y) in enumerate(t))
    sc.plan_turn_tour(targets=tg, start=start, turn_price=2.0)
    assert _same(a, sc.read_turn_tour())
    sc.close()
    # frames: none, STRICT, SANE, and an append since the turn tour
    depth, ci = _frame(np.random.default_rng(2), H, W)
    sc = ya.Scene(W, H)
    _raises(capi.ESTATE, lambda: sc.plan_turn_tour(targets=tg, start=start), "no frame")
    sc.append(depth, ci, ya.COMPAT_STRICT)
    _raises(capi.ESTATE, lambda: sc.plan_turn_tour(targets=tg, start=start), "STRICT")
    sc.append(depth, ci, ya.COMPAT_SANE)
    sc.plan_turn_tour(targets=tg, start=start, turn_price=2.0)
    b = sc.read_turn_tour()
    r = sc.read()
    _check(b, (r["map"], r["conn0"], r["conn1"]), tg, start, 6, 2.0)
    sc.append(depth, ci, ya.COMPAT_SANE)
    _raises(capi.ESTATE, lambda: sc.read_turn_tour(), "newer frame")
    _raises(capi.ESTATE, lambda: sc.turn_tour_time(1), "newer frame")
    sc.plan_turn_tour(targets=tg, start=start, turn_price=2.0)
    assert _same(b, sc.read_turn_tour())
    sc.close()
    s2 = ya.Scene(64, 48)
    with pytest.raises(ValueError):
        s2.plan_turn_tour(targets=[(1, 1)])
    s2.close()


@pytest.mark.gpu
def test_size_guard_and_life_cycle(built):
    from yolact_amd import capi
    # between the planner's guard and the turn planner's: an 8-connected tour runs, a turn tour is refused
    H, W = 2894, 3
    sc = _fields_scene(T.flat_fields(H, W))
    _raises(capi.EINVAL, lambda: sc.plan_turn_tour(targets=[(1, 0)], start=(1, 5)), "8 * 1024")
    _raises(capi.ESTATE, lambda: sc.read_turn_tour(), "no turn tour")
    sc.plan_tour(targets=[(1, 0)], start=(1, 5), connectivity=8)
    assert len(sc.read_tour()["path"]) == 6
    sc.close()
    # destroy after a turn tour only; two handles side by side; a closed one is gone
    f = T.flat_fields(9, 12)
    a, b = _fields_scene(f), _fields_scene(f)
    a.plan_turn_tour(targets=[(3, 3)], start=(3, 3), heading=2, turn_price=1.0)
    got = a.read_turn_tour()
    assert got["path"].tolist() == [[3, 3]] and got["directions"].shape == (0, 2) and got["turns"].shape == (0,) and got["leg_headings"].tolist() == [2]
    b.plan_turn_tour(targets=[(0, 0), (11, 0)], start=(11, 8), heading=0, turn_price=1.0)
    a.close()
    _check(b.read_turn_tour(), f, [(0, 0), (11, 0)], (11, 8), 0, 1.0)
    b.close(); b.close()


@pytest.mark.gpu
def test_balls_on_one_pixel_are_one_target(built):
    """A ball whose truncated mean equals an earlier ball's is dropped: targets are distinct pixels."""
    import yolact_amd as ya
    H, W = 48, 64
    depth = np.full((H, W), 2000, np.uint16)
    ci = np.zeros((H, W, 2), np.uint8)
    ci[12:14, 20:22] = (3, 1); ci[14:16, 20:22] = (3, 2); ci[30:32, 40:42] = (3, 7)   # balls 1 and 2: means (20.5, 29.0) both
    sc = ya.Scene(W, H)
    sc.append(depth, ci, ya.COMPAT_SANE)
    r = sc.read()
    assert R.ball_targets(r["balls"], 3, W, H) == [(20, 29), (20, 29), (40, 36)]
    sc.plan_turn_tour(start=(0, 0))
    got = sc.read_turn_tour()
    assert got["targets"].tolist() == [[20, 29], [40, 36]]
    _check(got, (r["map"], r["conn0"], r["conn1"]), [(20, 29), (40, 36)], (0, 0), 6, 2.0)
    sc.plan_turn_tour(n_targets=2, start=(0, 0))                                  # the first TWO balls: one pixel, one target
    assert sc.read_turn_tour(fields=False)["targets"].tolist() == [[20, 29]]
    sc.close()


@pytest.mark.gpu
def test_classify_scene_turn_tour_chain_stays_on_the_device(built):
    """classify -> append_classified(frame_dev_ptr=...) -> turn tour to the frame's balls: the class image never visits the host."""
    import yolact_amd as ya
    from test_scene_tour import _weights_that_see_balls
    H, W = 480, 640
    rng = np.random.default_rng(3)
    depth, _ = _frame(rng, H, W)
    eng = ya.Engine(input_size=224, backbone=50, max_batch=2, use_graph=True)
    eng.load_weights(_weights_that_see_balls(eng.generate_weights(1)))
    y = ya.Yolact(eng, ya.COMPAT_SANE)
    cam = (rng.integers(0, 256, (H, W, 3), dtype=np.uint32) * np.array([1 << 24, 1 << 16, 1 << 8], np.uint32)).sum(-1).astype(np.uint32).reshape(-1)
    y.classify(cam)
    sc = ya.Scene(W, H)
    sc.append_classified(depth, frame_dev_ptr=eng.classify_device_frame(), mode=ya.COMPAT_SANE)
    r = sc.read()
    f = (r["map"], r["conn0"], r["conn1"])
    tg = T.distinct(R.ball_targets(r["balls"], 3, W, H))
    assert len(tg) >= 2                                                           # the turn tour has an order to choose
    sc.plan_turn_tour(n_targets=3)
    got = sc.read_turn_tour()
    assert got["targets"].tolist() == [list(t) for t in tg]
    for b, t in enumerate(tg):
        assert U.equation_residual(got["cost"][b], *f, [t], 2.0) == 0 and np.isfinite(got["cost"][b]).all()
    assert got["path"][0].tolist() == [400, 479] and tuple(got["path"][-1]) == tg[got["order"][-1]]
    assert got["path"][got["leg_ends"]].tolist() == [list(tg[o]) for o in got["order"]]
    assert len(ya.serialize_path(got["directions"], 1700000000)) == 8 + 8 * len(got["directions"])
    sc.close(); eng.close()


@pytest.mark.gpu
def test_turn_tour_beats_one_turn_plan_per_target(built):
    """A condition, not a measurement: on the camera-like 640 x 480 frame with three explicit targets the median of three turn tours
    must take less than the three single-target turn plans one after the other, timed here on the same box with the shipped
    turn_time - and those are only the first of the calls a host would need. The figures are printed (tools/time_tour.py
    --turn-price measures them)."""
    import yolact_amd as ya
    H, W = 480, 640
    sc = ya.Scene(W, H)
    sc.append(*T.camera_like_frame(H, W), ya.COMPAT_SANE)
    targets, start = [(70, 67), (515, 410), (320, 40)], (400, 479)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    single = []
    for t in targets:
        sc.plan_turn(targets=[t], start=start, turn_price=2.0)                    # (warm-up too)
        single.append(med([sc.turn_time(5)["ms_per_plan"] for _ in range(3)]))
    sc.plan_turn_tour(targets=targets, start=start, turn_price=2.0)
    runs = [sc.turn_tour_time(5) for _ in range(3)]
    tour = med([r["ms_per_tour"] for r in runs])
    print(f"turn tour of 3 on the camera-like frame: {tour:.3f} ms ({runs[0]['rounds']} rounds, {runs[0]['tile_runs']} tile runs); "
          f"single-target turn plans {[round(s, 3) for s in single]} ms, sum {sum(single):.3f}")
    assert tour < sum(single)
    sc.close()
