"""The planner and the tour on the 8-connected grid (yh_scene_plan_conn / yh_scene_plan_tour_conn with connectivity 8; DESIGN.md
§11 "Diagonals"). CPU part: the restatement (tests/path_ref.py with conn=8, tests/path8_ref.py) against itself - two solvers bit for
bit -, closed forms, hand cases for every rotation constant, and the tile-round emulation that shows what a solver without the corner rule gets wrong.
GPU part (-m gpu): the HIP solver's fields bit-equal to the restatement on the engine's own scene fields and on constructed ones
(the late corner among them), successors, routes, the tour, the life cycle and every error."""
import os
import re
import time

import numpy as np
import pytest

import path8_ref as P
import path_ref as R
import tour_ref as T
from test_scene import _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI, PI34, PI2, PI4 = (np.float32(np.pi), np.float32(3 * np.pi / 4), np.float32(np.pi / 2), np.float32(np.pi / 4))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _random_fields(rng, H, W, hmax=40):
    hmap = rng.integers(0, hmax, (H, W)).astype(np.uint32)
    return (hmap,) + R.sane_connections(hmap)


def _route_fields(H, W, route, other=100.0):
    """Flat H x W fields in which the edges along `route` (pixels (x, y), each a neighbour of the one before) have length 1 and every
    other edge `other`: with fewer than `other` steps the cheapest way from route[0] to route[-1] is the route itself."""
    edges = [np.full((H, W), other, np.float32) for _ in range(4)]                 # right, down, down-right, down-left
    which = {(1, 0): 0, (0, 1): 1, (1, 1): 2, (-1, 1): 3}
    for p, q in zip(route[:-1], route[1:]):
        if (q[1], q[0]) < (p[1], p[0]):                                            # the edge belongs to its upper (then left) end
            p, q = q, p
        edges[which[(q[0] - p[0], q[1] - p[1])]][p[1], p[0]] = 1
    return P.fields_from_edges(*edges)


STAIRS = [(0, 0), (1, 0), (2, 1), (2, 2), (3, 2), (4, 3), (3, 4), (3, 5), (4, 5), (5, 5)]
# headings E, SE, S, E, SE, SW, S, E, E: 45, 45, 90, 45, 90, 45, 90, 0 degrees between them
STAIRS_ROT = [0, PI34, PI34, PI2, PI34, PI2, PI34, PI2, PI]


# ---------------------------------------------------------------- CPU

def test_dijkstra8_equals_jacobi8_bit_for_bit():
    rng = np.random.default_rng(11)
    H, W = 40, 56
    f = _random_fields(rng, H, W)
    targets = [(5, 7), (50, 30)]
    a = R.dijkstra(*f, targets, conn=8)
    b, sweeps = R.jacobi(*f, targets, conn=8)
    assert np.array_equal(_bits(a), _bits(b)) and sweeps > 10
    assert R.equation_residual(a, *f, targets, conn=8) == 0
    c0, c1 = f[1], f[2]
    assert (c0[1:, :-1, 1] >= 1).all() and (c0[:-1, :-1, 3] >= 1).all()                       # every SANE diagonal is >= 1
    assert np.array_equal(c0[1:, :-1, 1], c1[:-1, 1:, 1]) and np.array_equal(c0[:-1, :-1, 3], c1[1:, 1:, 3])   # and symmetric
    d4 = R.dijkstra(*f, targets)                                                                # every 4-path is an 8-path
    assert (a <= d4).all() and (a < d4).sum() > H * W // 2
    assert R.equation_residual(d4, *f, targets, conn=8) > 0 and R.equation_residual(a, *f, targets) > 0


def test_flat_map_diagonal_sums_and_the_tie_that_prefers_the_straight_move():
    f = T.flat_fields(5, 5)
    d = R.dijkstra(*f, [(0, 0)], conn=8)
    assert np.array_equal(_bits(d), _bits(R.jacobi(*f, [(0, 0)], conn=8)[0]))
    s = np.float32(0)
    for k in range(1, 5):
        s = np.float32(s + np.float32(np.sqrt(np.float32(2))))
        assert _bits(d[k, k]) == _bits(s)
    root2 = np.float32(np.sqrt(np.float32(2)))
    assert _bits(d[1, 2]) == _bits(np.float32(root2 + np.float32(1)))                          # d(2, 1): x = 2, y = 1
    cands = R.candidates(d, *f, conn=8)
    assert _bits(cands[0][1, 2]) == _bits(d[1, 2]) and _bits(cands[4][1, 2]) == _bits(d[1, 2])  # left and up-left tie ...
    nxt = R.successors(d, *f, [(0, 0)], conn=8)
    assert nxt[1, 2] == 1 * 5 + 1                                                              # ... and left wins
    assert nxt[0, 0] == -1 and nxt[3, 3] == 2 * 5 + 2


def test_three_nodes_by_hand_turn_by_135_degrees():
    """(0,0) - (1,0) = 1, down-left from (1,0) to (0,1) = 1, (0,0) - (0,1) = 100, (0,0) - (1,1) = 100: the way from (0,0) to (0,1)
    goes east, then south-west: three 45-degree steps between the headings, rot_1 = float32(pi / 4)."""
    f = _route_fields(3, 3, [(0, 0), (1, 0), (0, 1)])
    assert f[2][0, 0, 0] == 100 and f[1][0, 0, 3] == 100 and f[1][0, 0, 2] == 1 and f[2][0, 1, 1] == 1
    d = R.dijkstra(*f, [(0, 1)], conn=8)
    assert d[0, 0] == 2 and d[0, 1] == 1
    nxt = R.successors(d, *f, [(0, 1)], conn=8)
    path, dirs = R.walk(d, nxt, (0, 0), conn=8)
    assert path.tolist() == [[0, 0], [1, 0], [0, 1]]
    assert np.array_equal(_bits(dirs), _bits(np.array([[1, 0], [1, PI4]], np.float32)))
    assert float(PI4) == 0.7853981852531433


def test_staircase_route_has_three_quarter_and_half_turns():
    f = _route_fields(6, 6, STAIRS)
    d = R.dijkstra(*f, [STAIRS[-1]], conn=8)
    path, dirs = R.walk(d, R.successors(d, *f, [STAIRS[-1]], conn=8), STAIRS[0], conn=8)
    assert path.tolist() == [list(p) for p in STAIRS]
    assert np.array_equal(_bits(dirs[:, 1]), _bits(np.array(STAIRS_ROT, np.float32))) and (dirs[:, 0] == 1).all()
    assert [float(r) for r in R.ROT] == [float(PI), float(PI34), float(PI2), float(PI4), 0.0]
    assert R.rotation((0, 0), (1, 0), (0, 0)) == 0 and R.rotation((0, 0), (1, 1), (2, 2)) == PI   # a reversal; straight on a diagonal


def test_walk8_on_a_four_connected_route_is_path_refs_walk():
    """The rotation table on a route without diagonals, against the 4-connected rule written out: pi where the route goes straight
    on, pi / 2 where it turns, 0 at step 0; the magnitudes are the cost differences."""
    f = _random_fields(np.random.default_rng(2), 20, 30)
    d = R.dijkstra(*f, [(3, 4)])
    nxt = R.successors(d, *f, [(3, 4)])
    path, dirs = R.walk(d, nxt, (28, 17), conn=8)
    assert tuple(path[0]) == (28, 17) and tuple(path[-1]) == (3, 4) and (np.abs(np.diff(path, axis=0)).sum(1) == 1).all()
    assert np.array_equal(path[1:, 1] * 30 + path[1:, 0], nxt[path[:-1, 1], path[:-1, 0]])      # the walk follows next
    straight = (path[:-2] + path[2:] == 2 * path[1:-1]).all(1)
    assert straight.any() and not straight.all()
    want = np.concatenate([[np.float32(0)], np.where(straight, PI, PI2)]).astype(np.float32)
    assert np.array_equal(_bits(dirs[:, 1]), _bits(want))
    cost = d[path[:, 1], path[:, 0]]
    assert np.array_equal(_bits(dirs[:, 0]), _bits(cost[:-1] - cost[1:]))
    four = R.walk(d, nxt, (28, 17))                                                             # and the default is the same walk
    assert np.array_equal(four[0], path) and np.array_equal(_bits(four[1]), _bits(dirs))


def test_late_corner_needs_the_corner_rule():
    """The constructed fields of path8_ref.late_corner: the tile emulation with the corner rule equals the Dijkstra in 5 rounds;
    without it it stops after 4 with the whole diagonal tile wrong but finite - so the GPU case on these fields catches a solver
    that lacks the rule. A random field does not: without the rule the emulation still gets it right."""
    f = P.late_corner()
    want = R.dijkstra(*f, [(0, 0)], conn=8)
    assert want[31, 31] == 48.5 and want[32, 32] == 50.0
    d, rounds = P.tile_rounds(*f, [(0, 0)])
    assert np.array_equal(_bits(d), _bits(want)) and rounds == 5
    d, rounds = P.tile_rounds(*f, [(0, 0)], corner_flags=False)
    wrong = d != want
    assert rounds == 4 and wrong.sum() == 1024 and wrong[32:, 32:].all() and d[32, 32] == 5047.5 and np.isfinite(d).all()
    g = _random_fields(np.random.default_rng(11), 40, 56)
    d, _ = P.tile_rounds(*g, [(5, 7), (50, 30)], corner_flags=False)
    assert np.array_equal(_bits(d), _bits(R.dijkstra(*g, [(5, 7), (50, 30)], conn=8)))


def test_conn_symbols_are_declared_and_bound():
    import inspect
    from yolact_amd import capi
    bound = {s[0]: s for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    for name in ("yh_scene_plan_conn", "yh_scene_plan_tour_conn"):
        assert re.search(r"\b%s\s*\(" % name, pub) and name in bound, name
        assert len(bound[name][2]) == len(bound[name[:-5]][2]) + 1
    assert "#define YH_ABI_VERSION 4" in pub
    for m in ("plan", "plan_tour"):
        assert inspect.signature(getattr(capi.Scene, m)).parameters["connectivity"].default == 4


# ---------------------------------------------------------------- GPU

def _scene(H, W, seed):
    import yolact_amd as ya
    depth, ci = _frame(np.random.default_rng(seed), H, W)
    sc = ya.Scene(W, H)
    sc.append(depth, ci, ya.COMPAT_SANE)
    return sc


def _fields_scene(f):
    import yolact_amd as ya
    H, W = f[0].shape
    sc = ya.Scene(W, H)
    sc.set_fields(*f)
    return sc


def _raises(code, fn, word=None):
    import yolact_amd as ya
    with pytest.raises(ya.YhError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert word is None or word in str(e.value), str(e.value)


def _same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def _check_plan(got, f, targets, start, conn=8):
    """cost, next, path and directions of a plan (8-connected unless said) against the restatement on the fields f = (map, conn0, conn1)."""
    want = R.dijkstra(*f, targets, conn=conn)
    assert np.array_equal(_bits(got["cost"]), _bits(want))
    nxt = R.successors(want, *f, targets, conn=conn)
    assert np.array_equal(got["next"], nxt)
    path, dirs = R.walk(want, nxt, start, conn=conn)
    assert np.array_equal(got["path"], path) and np.array_equal(_bits(got["directions"]), _bits(dirs))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,targets,start", [
    (37, 53, [(2, 3), (50, 30)], (26, 36)),        # ragged 2 x 2 tiles
    (8, 8, [(7, 0)], (0, 7)),
    (100, 9, [(4, 50)], (0, 0)),
    (33, 33, [(30, 2)], (1, 32)),                  # the corner tile is 1 x 1
])
def test_cost_field_bit_equal_to_dijkstra8(built, H, W, targets, start):
    """The engine's own Scene.read() fields go through path_ref's Dijkstra; the device field must have the same bits."""
    sc = _scene(H, W, H * 1000 + W)
    f = sc.read()
    sc.plan(targets=targets, start=start, connectivity=8)
    got = sc.read_plan()
    want = _check_plan(got, (f["map"], f["conn0"], f["conn1"]), targets, start)
    print(f"{W}x{H}: max cost {want.max()}, {sc.plan_time(1)}")
    sc.close()


@pytest.mark.gpu
def test_full_frame_satisfies_its_equations_at_every_pixel(built):
    """640 x 480, ball targets: no +inf left and the defining equations hold bitwise everywhere - by uniqueness that is the field."""
    H, W = 480, 640
    sc = _scene(H, W, 5)
    f = sc.read()
    sc.plan(connectivity=8)
    got = sc.read_plan()
    tg = R.ball_targets(f["balls"], 3, W, H)
    assert len(tg) == 2
    d = got["cost"]
    assert np.isfinite(d).all() and d.max() < 2 ** 24
    assert all(d[y, x] == 0 for x, y in tg) and (d == 0).sum() == len(tg)
    assert R.equation_residual(d, f["map"], f["conn0"], f["conn1"], tg, conn=8) == 0
    # the route: next is the first of the eight achieving equality, costs strictly decrease, directions are walk8's
    nxt = R.successors(d, f["map"], f["conn0"], f["conn1"], tg, conn=8)
    assert np.array_equal(got["next"], nxt) and (nxt == -1).sum() == len(tg)
    path, dirs = R.walk(d, nxt, (400, 479), conn=8)
    assert np.array_equal(got["path"], path) and np.array_equal(_bits(got["directions"]), _bits(dirs))
    cost = d[path[:, 1], path[:, 0]]
    assert (np.diff(cost) < 0).all() and cost[-1] == 0 and tuple(path[-1]) in tg
    steps = np.abs(np.diff(path, axis=0))
    assert (steps.max(1) == 1).all() and (steps.sum(1) == 2).any()                  # neighbours, some of them diagonal
    assert set(np.unique(_bits(dirs[1:, 1]))) <= {int(r.view(np.uint32)) for r in R.ROT[:4]}
    print(f"route of {len(path)} nodes, {sc.plan_time(1)}")
    sc.close()


@pytest.mark.gpu
def test_late_corner_on_the_device(built):
    """The fields on which a tile solver without the corner rule leaves the diagonal tile wrong but finite
    (test_late_corner_needs_the_corner_rule): bit-equal to the Dijkstra."""
    f = P.late_corner()
    sc = _fields_scene(f)
    sc.plan(targets=[(0, 0)], start=(63, 63), connectivity=8)
    got = sc.read_plan()
    want = _check_plan(got, f, [(0, 0)], (63, 63))
    assert got["cost"][31, 31] == 48.5 and got["cost"][32, 32] == 50.0 and want[32, 32] == 50.0
    stats = sc.plan_time(1)
    print(f"late corner: {stats}")
    assert stats["rounds"] >= 4
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("targets", [[(31, 31)], [(32, 32)], [(32, 31)], [(31, 32)], [(31, 31), (32, 32), (0, 32), (63, 31)]])
def test_targets_on_tile_corners(built, targets):
    """A target's drop from +inf to 0 on a corner cell of a tile is a lowered corner like any other: 64 x 64, four tiles."""
    f = _random_fields(np.random.default_rng(64), 64, 64, 30)
    sc = _fields_scene(f)
    sc.plan(targets=targets, start=(5, 60), connectivity=8)
    got = sc.read_plan()
    assert np.isfinite(got["cost"]).all()
    _check_plan(got, f, targets, (5, 60))
    sc.close()


@pytest.mark.gpu
def test_hand_routes_on_the_device(built):
    """The three-node case (pi / 4) and the staircase (3 pi / 4, pi / 2, pi) through yh_scene_set_fields."""
    f = _route_fields(3, 3, [(0, 0), (1, 0), (0, 1)])
    sc = _fields_scene(f)
    sc.plan(targets=[(0, 1)], start=(0, 0), connectivity=8)
    got = sc.read_plan()
    _check_plan(got, f, [(0, 1)], (0, 0))
    assert got["path"].tolist() == [[0, 0], [1, 0], [0, 1]]
    assert np.array_equal(_bits(got["directions"]), _bits(np.array([[1, 0], [1, PI4]], np.float32)))
    sc.plan(targets=[(0, 1)], start=(0, 0))                                         # 4-connected: straight down the edge of 100
    assert sc.read_plan()["path"].tolist() == [[0, 0], [0, 1]]
    sc.close()
    f = _route_fields(6, 6, STAIRS)
    sc = _fields_scene(f)
    sc.plan(targets=[STAIRS[-1]], start=STAIRS[0], connectivity=8)
    got = sc.read_plan()
    _check_plan(got, f, [STAIRS[-1]], STAIRS[0])
    assert got["path"].tolist() == [list(p) for p in STAIRS]
    assert np.array_equal(_bits(got["directions"][:, 1]), _bits(np.array(STAIRS_ROT, np.float32)))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,targets,start", [
    (37, 53, [(2, 3), (50, 30), (26, 10)], (26, 36)),
    (8, 8, [(7, 0), (0, 0), (3, 4), (4, 3), (7, 7), (0, 6)], (0, 7)),
])
def test_tour_on_the_eight_connected_grid(built, H, W, targets, start):
    sc = _scene(H, W, H * 1000 + W)
    r = sc.read()
    f = (r["map"], r["conn0"], r["conn1"])
    sc.plan_tour(targets=targets, start=start, connectivity=8)
    got = sc.read_tour(fields=True)
    want = T.tour(*f, targets, start, conn=8)
    K = len(targets)
    assert got["targets"].tolist() == [list(t) for t in targets]
    for b in range(K):
        assert np.array_equal(_bits(got["cost"][b]), _bits(want["cost"][b])), f"field {b}"
        assert np.array_equal(got["next"][b], want["next"][b]), f"field {b}"
    sc.plan(targets=targets, start=start, connectivity=8)                          # the shipped planner with the same targets
    assert np.array_equal(_bits(np.minimum.reduce(got["cost"])), _bits(sc.read_plan()["cost"]))
    assert np.array_equal(got["label"], want["label"])
    assert np.array_equal(_bits(got["legs"]), _bits(want["legs"])) and (np.diag(got["legs"][1:]) == 0).all()
    assert got["order"].tolist() == want["order"].tolist() and _bits(got["total"]) == _bits(want["total"])
    assert np.array_equal(got["path"], want["path"]) and got["leg_ends"].tolist() == want["leg_ends"].tolist()
    assert np.array_equal(_bits(got["directions"]), _bits(want["directions"]))
    stats = sc.tour_time(1)
    assert _same(got, sc.read_tour(fields=True))                                   # the replay has the tour's connectivity
    print(f"{W}x{H}: K = {K}, order {want['order'].tolist()}, total {want['total']}, route of {len(want['path'])} nodes, {stats}")
    sc.close()


@pytest.mark.gpu
def test_default_is_four_and_eight_is_never_dearer(built):
    sc = _scene(37, 53, 7)
    tg, start = [(2, 3), (50, 30)], (26, 36)
    sc.plan(targets=tg, start=start)
    a = sc.read_plan()
    sc.plan(targets=tg, start=start, connectivity=4)
    assert _same(a, sc.read_plan())
    t = np.array(tg, np.int32)                                                     # and the entry point without the argument
    assert sc.L.yh_scene_plan(sc.h, t.ctypes.data, len(tg), start[0], start[1]) == 0
    assert _same(a, sc.read_plan())
    sc.plan(targets=tg, start=start, connectivity=8)
    b = sc.read_plan()
    assert (b["cost"] <= a["cost"]).all() and (b["cost"] < a["cost"]).any()
    sc.plan_tour(targets=tg, start=start)
    t = sc.read_tour(fields=True)
    sc.plan_tour(targets=tg, start=start, connectivity=4)
    assert _same(t, sc.read_tour(fields=True))
    sc.close()


@pytest.mark.gpu
def test_four_eight_and_tour_do_not_disturb_one_another(built):
    """Each entry point keeps its last result only; nothing else of one call shows in another's result."""
    sc = _scene(70, 90, 3)
    tg, start = [(5, 5), (80, 60)], (40, 69)
    sc.plan(targets=tg, start=start)
    p4 = sc.read_plan()
    sc.plan_tour(targets=tg, start=start, connectivity=8)
    assert _same(p4, sc.read_plan())                                               # 4-plan -> 8-tour -> read_plan unchanged
    t8 = sc.read_tour(fields=True)
    sc.plan(targets=tg, start=start, connectivity=8)
    p8 = sc.read_plan()
    assert _same(t8, sc.read_tour(fields=True)) and not _same(p4, p8)
    assert np.array_equal(_bits(p8["cost"]), _bits(np.minimum.reduce(t8["cost"])))
    sc.plan_tour(targets=tg, start=start)                                          # a 4-tour after the 8-tour, beside the 8-plan
    t4 = sc.read_tour(fields=True)
    assert _same(p8, sc.read_plan())
    sc.plan_time(2)                                                                # the replay has the plan's connectivity
    assert _same(p8, sc.read_plan()) and _same(t4, sc.read_tour(fields=True))
    sc.plan(targets=tg, start=start)                                               # and 4 after 8 is what it was before any 8
    assert _same(p4, sc.read_plan())
    assert np.array_equal(_bits(p4["cost"]), _bits(np.minimum.reduce(t4["cost"])))
    sc.close()


@pytest.mark.gpu
def test_one_solver_state_serves_kinds_connectivities_and_field_counts(built):
    """Plans and tours share the solver's buffers (edge terms, tile flags [2][F][ntiles], counters, read-back block): on ONE handle a
    tour of 6 fields, a plan, a tour of 2 (the flag array's layout shrinks), a plan to a tile corner, both replays, a tour of 5 (it
    grows again), connectivities mixed. 64 x 64: 2 x 2 tiles; two targets of the first tour face each other across the tile border
    x = 31 | 32. After every step the run just made equals the restatement bit for bit and the other kind's last result reads back
    byte for byte what it was."""
    f = _random_fields(np.random.default_rng(6464), 64, 64, 30)
    sc = _fields_scene(f)
    start = (5, 60)
    last, wants = {}, {}

    def check(kind, targets, conn):
        """the last run of `kind` against the restatement; the other kind's last result unchanged"""
        got = sc.read_tour(fields=True) if kind == "tour" else sc.read_plan()
        if kind == "plan":
            _check_plan(got, f, targets, start, conn)
        else:
            key = (tuple(targets), conn)
            want = wants[key] = wants.get(key) or T.tour(*f, targets, start, conn=conn)
            assert got["targets"].tolist() == want["targets"].tolist()
            assert np.array_equal(_bits(got["cost"]), _bits(want["cost"])) and np.array_equal(got["next"], want["next"])
            assert np.array_equal(got["label"], want["label"]) and np.array_equal(_bits(got["legs"]), _bits(want["legs"]))
            assert got["order"].tolist() == want["order"].tolist() and _bits(got["total"]) == _bits(want["total"])
            assert np.array_equal(got["path"], want["path"]) and got["leg_ends"].tolist() == want["leg_ends"].tolist()
            assert np.array_equal(_bits(got["directions"]), _bits(want["directions"]))
        last[kind] = got
        other = "plan" if kind == "tour" else "tour"
        if other in last:
            assert _same(last[other], sc.read_tour(fields=True) if other == "tour" else sc.read_plan()), f"{kind} disturbed the last {other}"

    tour6 = [(31, 20), (32, 20), (3, 3), (60, 5), (10, 50), (55, 58)]
    sc.plan_tour(targets=tour6, start=start, connectivity=8)
    check("tour", tour6, 8)
    plan3 = [(0, 0), (63, 63), (20, 33)]
    sc.plan(targets=plan3, start=start, connectivity=4)
    check("plan", plan3, 4)
    tour2 = [(40, 10), (7, 32)]
    sc.plan_tour(targets=tour2, start=start, connectivity=4)
    check("tour", tour2, 4)
    sc.plan(targets=[(31, 31)], start=start, connectivity=8)
    check("plan", [(31, 31)], 8)
    stats = [sc.tour_time(2)]
    check("tour", tour2, 4)
    stats.append(sc.plan_time(2))
    check("plan", [(31, 31)], 8)
    assert stats[0]["rounds"] >= 1 and stats[1]["rounds"] >= 1
    tour5 = [(32, 32), (31, 0), (0, 31), (63, 32), (16, 16)]
    sc.plan_tour(targets=tour5, start=start, connectivity=8)
    check("tour", tour5, 8)
    print(f"replays: {stats}")
    sc.close()


@pytest.mark.gpu
def test_errors(built):
    import yolact_amd as ya
    from yolact_amd import capi
    H, W = 40, 70
    f = _random_fields(np.random.default_rng(1), H, W, 30)
    sc = _fields_scene(f)
    tg, start = [(3, 3)], (60, 30)
    sc.plan(targets=tg, start=start, connectivity=8)
    a = sc.read_plan()
    sc.plan_tour(targets=tg, start=start, connectivity=8)
    t = sc.read_tour(fields=True)
    for c in (5, 0, -8, 6):
        _raises(capi.EINVAL, lambda: sc.plan(targets=tg, start=start, connectivity=c), "connectivity")
        _raises(capi.EINVAL, lambda: sc.plan_tour(targets=tg, start=start, connectivity=c), "connectivity")
    assert _same(a, sc.read_plan()) and _same(t, sc.read_tour(fields=True))         # the earlier results stay readable
    # diagonals no SANE frame gives: a 4-connected plan does not read them, an 8-connected one refuses them and says why
    for y, x, k, arr, v in ((5, 6, 3, 0, 0.5), (5, 6, 1, 1, np.inf), (7, 8, 3, 0, 9.0), (7, 8, 1, 0, 9.0), (7, 8, 3, 1, np.nan)):
        c = [f[1].copy(), f[2].copy()]
        c[arr][y, x, k] = v
        sc.set_fields(f[0], c[0], c[1])
        _raises(capi.ESTATE, lambda: sc.plan(targets=tg, start=start, connectivity=8), "length")
        _raises(capi.ESTATE, lambda: sc.plan_tour(targets=tg, start=start, connectivity=8), "length")
        _raises(capi.ESTATE, lambda: sc.read_plan(), "newer frame")                 # (refused: no plan of this frame exists)
        sc.plan(targets=tg, start=start)
        assert np.array_equal(_bits(sc.read_plan()["cost"]), _bits(R.dijkstra(*f, tg)))
        sc.plan_tour(targets=tg, start=start)
        assert tuple(sc.read_tour()["path"][-1]) == tg[0]
    sc.set_fields(*f)                                                              # sound fields again: 8 plans again
    sc.plan(targets=tg, start=start, connectivity=8)
    assert _same(a, sc.read_plan())
    # what set_fields refused before it still refuses, diagonals or not
    c0 = f[1].copy(); c0[5, 6, 2] = 0.5
    _raises(capi.EINVAL, lambda: sc.set_fields(f[0], c0, f[2]), "SANE")
    sc.close()
    # STRICT frames are refused as they are for 4; a SANE append after bad uploaded fields plans with 8 again
    depth, ci = _frame(np.random.default_rng(2), H, W)
    sc = ya.Scene(W, H)
    _raises(capi.ESTATE, lambda: sc.plan(targets=tg, start=start, connectivity=8), "no frame")
    sc.append(depth, ci, ya.COMPAT_STRICT)
    _raises(capi.ESTATE, lambda: sc.plan(targets=tg, start=start, connectivity=8), "STRICT")
    _raises(capi.ESTATE, lambda: sc.plan_tour(targets=tg, start=start, connectivity=8), "STRICT")
    c1 = f[2].copy(); c1[5, 6, 1] = 0.25
    sc.set_fields(f[0], f[1], c1)
    _raises(capi.ESTATE, lambda: sc.plan(targets=tg, start=start, connectivity=8), "length")
    sc.append(depth, ci, ya.COMPAT_SANE)
    sc.plan(targets=tg, start=start, connectivity=8)
    r = sc.read()
    assert np.array_equal(_bits(sc.read_plan()["cost"]), _bits(R.dijkstra(r["map"], r["conn0"], r["conn1"], tg, conn=8)))
    sc.close()


@pytest.mark.gpu
def test_plan8_beats_the_cpu_restatement(built):
    """As test_plan_beats_the_cpu_restatement: an 8-connected plan at 640 x 480 must beat path_ref's numpy Jacobi solve of the same
    field, timed here on the same box. A floor that catches a broken work list, not a target (tools/time_path.py measures)."""
    H, W = 480, 640
    sc = _scene(H, W, 13)
    f = sc.read()
    tg = R.ball_targets(f["balls"], 3, W, H)
    sc.plan(connectivity=8)                                       # warm-up: buffers, code objects
    t0 = time.perf_counter()
    sc.plan(connectivity=8)
    gpu_s = time.perf_counter() - t0
    got = sc.read_plan()
    t0 = time.perf_counter()
    want, sweeps = R.jacobi(f["map"], f["conn0"], f["conn1"], tg, conn=8)
    cpu_s = time.perf_counter() - t0
    stats = sc.plan_time(10)
    print(f"plan8 640x480: host wall {gpu_s * 1e3:.3f} ms, {stats}; numpy Jacobi {cpu_s:.2f} s in {sweeps} sweeps")
    assert np.array_equal(_bits(got["cost"]), _bits(want))
    assert gpu_s < cpu_s and stats["ms_per_plan"] * 1e-3 < cpu_s
    sc.close()
