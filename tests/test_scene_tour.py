"""The tour planner (yh_scene_plan_tour: one single-target cost field per ball solved in the same launches, the visiting order of
least total cost, the joined route; DESIGN.md §11 "Tour"). CPU part: the definition's restatement (tests/tour_ref.py) against hand
results and against path_ref; the ABI surface. GPU part (-m gpu): every field bit-equal to path_ref's Dijkstra and to its own
defining equations, the minimum over the fields bit-equal to the shipped planner's multi-source field, labels, leg matrix, order,
route, directions; round 0's flags per field; the maze; the life cycle and every error; a floor on time."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import path_ref as R
import tour_ref as T
from test_scene import _frame
from test_scene_path import _random_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- CPU

STRIP = dict(start=(10, 0), A=(13, 0), B=(6, 0), C=(30, 0))


def test_strip_by_hand_best_order_is_not_nearest_first():
    """Flat 1 x 40 strip, unit lengths, start x = 10, A at 13, B at 6, C at 30. By hand: ABC 3 + 7 + 24 = 34, ACB 3 + 17 + 24 = 44,
    BAC 4 + 7 + 17 = 28, BCA 4 + 24 + 17 = 45, CAB 20 + 17 + 7 = 44, CBA 20 + 24 + 7 = 51."""
    f = T.flat_fields(1, 40)
    t = T.tour(*f, [STRIP["A"], STRIP["B"], STRIP["C"]], STRIP["start"])
    totals = {o: float(T.tour_total(t["legs"], o)) for o in [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]}
    assert totals == {(0, 1, 2): 34, (0, 2, 1): 44, (1, 0, 2): 28, (1, 2, 0): 45, (2, 0, 1): 44, (2, 1, 0): 51}
    assert tuple(t["order"]) == (1, 0, 2) and t["total"] == 28
    assert T.nearest_first(t["legs"]) == (0, 1, 2) and T.tour_total(t["legs"], (0, 1, 2)) == 34
    assert t["path"][:, 0].tolist() == list(range(10, 5, -1)) + list(range(7, 31)) and t["leg_ends"].tolist() == [4, 11, 28]
    rot = np.full(28, R.PI, np.float32); rot[0] = 0; rot[4] = 0                   # the route reverses at B, node 4
    assert np.array_equal(_bits(t["directions"][:, 1]), _bits(rot)) and (t["directions"][:, 0] == 1).all()
    assert np.array_equal(t["legs"], np.array([[3, 4, 20], [0, 7, 17], [7, 0, 24], [17, 24, 0]], np.float32))


def test_tie_goes_to_the_lexicographically_smallest_order():
    f = T.flat_fields(1, 40)
    t = T.tour(*f, [(7, 0), (13, 0)], (10, 0))
    assert T.tour_total(t["legs"], (0, 1)) == 9 and T.tour_total(t["legs"], (1, 0)) == 9
    assert tuple(t["order"]) == (0, 1) and t["total"] == 9 and t["leg_ends"].tolist() == [3, 9]
    assert t["directions"][3, 1] == 0 and t["path"][3].tolist() == [7, 0]         # a reversal at A
    assert (np.delete(t["directions"][:, 1], [0, 3]) == R.PI).all()


def test_start_on_a_target_adds_no_node():
    f = T.flat_fields(1, 40)
    t = T.tour(*f, [(10, 0), (13, 0)], (10, 0))
    assert tuple(t["order"]) == (0, 1) and t["leg_ends"].tolist() == [0, 3] and t["path"][:, 0].tolist() == [10, 11, 12, 13]
    assert t["directions"][:, 1].tolist() == [0.0, float(R.PI), float(R.PI)]
    t = T.tour(*f, [(10, 0)], (10, 0))
    assert t["path"].tolist() == [[10, 0]] and t["directions"].shape == (0, 2) and t["leg_ends"].tolist() == [0] and t["total"] == 0


def test_seeded_field_min_of_fields_is_the_multi_source_field():
    f = _random_fields(np.random.default_rng(5), 96, 128)
    targets, start = [(5, 7), (100, 90), (64, 3), (20, 80)], (60, 95)
    t = T.tour(*f, targets, start)
    assert np.array_equal(_bits(np.minimum.reduce(t["cost"])), _bits(R.dijkstra(*f, targets)))
    assert tuple(t["order"]) == (1, 3, 0, 2) and tuple(t["order"]) != T.nearest_first(t["legs"])
    assert abs(float(t["total"]) - 4064.43) < 0.01 and abs(float(T.tour_total(t["legs"], T.nearest_first(t["legs"]))) - 4344.34) < 0.01
    assert t["legs"][2, 0] != t["legs"][1, 1] and abs(float(t["legs"][2, 0]) - float(t["legs"][1, 1])) < 0.01    # d_a[t_b] against d_b[t_a]
    lab = np.zeros(t["label"].shape, np.uint8)
    best = t["cost"][0].copy()
    for b in range(1, 4):
        lab[t["cost"][b] < best] = b
        best = np.minimum(best, t["cost"][b])
    assert np.array_equal(t["label"], lab) and all(t["label"][y, x] == b for b, (x, y) in enumerate(targets))
    for b in range(4):                                                            # field b: -1 at t_b only
        assert (t["next"][b] == -1).sum() == 1 and t["next"][b][targets[b][1], targets[b][0]] == -1
    assert tuple(t["path"][-1]) == targets[2] and t["path"][t["leg_ends"]].tolist() == [list(targets[o]) for o in t["order"]]


def test_tour_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0] for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read(), flags=re.S)
    for name in ("yh_scene_plan_tour", "yh_scene_tour_read"):
        assert re.search(r"\b%s\s*\(" % name, pub) and name in bound, name
    assert re.search(r"\byh_scene_tour_time\s*\(", dbg) and not re.search(r"\byh_scene_tour_time\s*\(", pub) and "yh_scene_tour_time" in bound
    assert "#define YH_ABI_VERSION 4" in pub and "#define YH_TOUR_MAX 6" in pub and capi.TOUR_MAX == T.TOUR_MAX == 6
    for m in ("plan_tour", "read_tour", "tour_time"):
        assert callable(getattr(capi.Scene, m))


# ---------------------------------------------------------------- GPU

def _scene(H, W, seed):
    import yolact_amd as ya
    rng = np.random.default_rng(seed)
    depth, ci = _frame(rng, H, W)
    sc = ya.Scene(W, H)
    sc.append(depth, ci, ya.COMPAT_SANE)
    return sc


def _fields_scene(hmap):
    import yolact_amd as ya
    H, W = hmap.shape
    f = (hmap,) + R.sane_connections(hmap)
    sc = ya.Scene(W, H)
    sc.set_fields(*f)
    return sc, f


def _check_tour(sc, f, targets, start, against_plan=True):
    """Everything read_tour(fields=True) returns against tour_ref on the fields f = (map, conn0, conn1); returns (got, want)."""
    from yolact_amd import capi
    got = sc.read_tour(fields=True)
    K = len(targets)
    assert got["targets"].tolist() == [list(t) for t in targets] and got["cost"].shape[0] == K
    want = T.tour(*f, targets, start)
    for b, t in enumerate(targets):
        assert np.array_equal(_bits(got["cost"][b]), _bits(want["cost"][b])), f"field {b}"
        assert R.equation_residual(got["cost"][b], *f, [t]) == 0, f"field {b}"        # (does not rest on the Dijkstra)
        assert np.array_equal(got["next"][b], R.successors(got["cost"][b], *f, [t])), f"field {b}"
    if against_plan:   # the shipped planner with the same targets, no CPU solver in between
        sc.plan(targets=targets, start=start)
        assert np.array_equal(_bits(np.minimum.reduce(got["cost"])), _bits(sc.read_plan()["cost"]))
    assert got["label"].dtype == np.uint8 and np.array_equal(got["label"], np.argmin(got["cost"], axis=0))
    legs = np.array([[got["cost"][b][y, x] for b in range(K)] for x, y in [start] + list(targets)], np.float32)
    assert np.array_equal(_bits(got["legs"]), _bits(legs)) and (np.diag(got["legs"][1:]) == 0).all()
    assert got["order"].tolist() == want["order"].tolist() and _bits(got["total"]) == _bits(want["total"])
    segs, at = [], start
    for b in got["order"]:                                                        # the joined path_ref.walk of each leg
        segs.append(R.walk(got["cost"][b], got["next"][b], at)[0][0 if not segs else 1:])
        at = targets[b]
    assert np.array_equal(got["path"], np.concatenate(segs)) and np.array_equal(got["path"], want["path"])
    assert np.array_equal(_bits(got["directions"]), _bits(want["directions"])) and got["leg_ends"].tolist() == want["leg_ends"].tolist()
    wire = capi.serialize_path(got["directions"], 1700000000)
    assert struct.unpack(">Q", wire[:8])[0] == 1700000000
    assert np.array_equal(_bits(np.frombuffer(wire[8:], ">f4").astype(np.float32).reshape(-1, 2)), _bits(got["directions"]))
    short = sc.read_tour()
    assert set(short) == {"targets", "order", "legs", "total", "path", "directions", "leg_ends"}
    assert all(np.array_equal(short[k], got[k]) for k in short)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,targets,start", [
    (480, 640, None, None),
    (480, 640, [(17, 400), (600, 30), (320, 240), (321, 240)], (400, 479)),
    (37, 53, [(2, 3), (50, 30)], (26, 36)),
    (8, 8, [(7, 0), (0, 0), (3, 4), (4, 3), (7, 7), (0, 6)], (0, 7)),
    (100, 9, [(4, 50)], (0, 0)),
])
def test_fields_order_and_route_equal_the_reference(built, H, W, targets, start):
    """The engine's own Scene.read() fields go through tour_ref; every output of the device tour must have the same bits."""
    sc = _scene(H, W, H * 1000 + W)
    f = sc.read()
    sc.plan_tour(targets=targets, start=start)
    tg = targets if targets is not None else T.distinct(R.ball_targets(f["balls"], 3, W, H))
    assert len(tg) >= (2 if targets is None else 1)
    got, _ = _check_tour(sc, (f["map"], f["conn0"], f["conn1"]), tg, start if start is not None else (400, 479))
    print(f"{W}x{H}: K = {len(tg)}, order {got['order'].tolist()}, total {got['total']}, route of {len(got['path'])} nodes, {sc.tour_time(1)}")
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("targets,order,total,reversal", [
    ([STRIP["A"], STRIP["B"], STRIP["C"]], [1, 0, 2], 28, 4),
    ([(7, 0), (13, 0)], [0, 1], 9, 3),
])
def test_hand_cases_on_the_device(built, targets, order, total, reversal):
    """The two hand-derived strips through yh_scene_set_fields: best order against nearest-first, the tie, the reversal's 0.0. A scene
    is at least 3 rows high, so the 1 x 40 strip is row 1 of a 3 x 40 frame between two walls of height 400 (a step onto a wall
    costs more than 800, the whole strip 39): on the strip the costs, the legs and the route are those derived by hand."""
    hmap = np.full((3, 40), 400, np.uint32)
    hmap[1] = 0
    row = lambda pts: [(x, 1) for x, _ in pts]
    sc, f = _fields_scene(hmap)
    sc.plan_tour(targets=row(targets), start=(10, 1))
    got, _ = _check_tour(sc, f, row(targets), (10, 1))
    assert got["order"].tolist() == order and got["total"] == total and (got["path"][:, 1] == 1).all()
    strip = T.tour(*T.flat_fields(1, 40), targets, (10, 0))                       # the 1 x 40 strip itself, on the CPU
    assert np.array_equal(got["legs"], strip["legs"]) and np.array_equal(got["path"][:, 0], strip["path"][:, 0])
    assert np.array_equal(_bits(got["directions"]), _bits(strip["directions"])) and got["leg_ends"].tolist() == strip["leg_ends"].tolist()
    rot = np.full(total, R.PI, np.float32); rot[0] = 0; rot[reversal] = 0
    assert np.array_equal(_bits(got["directions"][:, 1]), _bits(rot))
    sc.plan_tour(targets=[(10, 1), (13, 1)], start=(10, 1))                       # start on a target: that leg adds no node
    got, _ = _check_tour(sc, f, [(10, 1), (13, 1)], (10, 1))
    assert got["leg_ends"].tolist() == [0, 3] and len(got["path"]) == 4
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,targets,start", [
    (64, 64, [(31, 31), (32, 32), (0, 32), (63, 31)], (5, 60)),
    (3, 64, [(31, 1), (32, 1)], (63, 2)),
    (64, 3, [(1, 31), (1, 32)], (0, 0)),
])
def test_round_zero_flags_per_field(built, H, W, targets, start):
    """Each field has ONE target: on a tile's last row / column, on its first, in a corner of four tiles. Round 0 must wake that
    field's tiles across those borders (and no field may lean on another field's flags)."""
    sc, f = _fields_scene(np.random.default_rng(H + W).integers(0, 30, (H, W)).astype(np.uint32))
    sc.plan_tour(targets=targets, start=start)
    got, _ = _check_tour(sc, f, targets, start)
    assert np.isfinite(got["cost"]).all()
    sc.close()


@pytest.mark.gpu
def test_maze_three_fields_in_the_rounds_of_the_slowest(built):
    """The serpentine corridor at 480 x 640, targets at both ends and in the middle, start elsewhere in it. Fields equal to the
    Dijkstra; the fields relax in the same launches, so the tour's rounds stay at or below those of the slowest single-target
    plan plus one batch of 16."""
    H, W = 480, 640
    hmap, end0, end1 = R.serpentine(H, W)
    targets, start = [end0, end1, (320, 244)], (100, 84)
    assert all(hmap[y, x] == 0 for x, y in targets + [start])
    sc, f = _fields_scene(hmap)
    single = []
    for t in targets:
        sc.plan(targets=[t], start=start)
        single.append(sc.plan_time(1))
    sc.plan_tour(targets=targets, start=start)
    stats = sc.tour_time(1)
    print(f"maze tour: {stats}; single-target plans: {single}")
    got, _ = _check_tour(sc, f, targets, start, against_plan=False)
    assert stats["rounds"] <= max(s["rounds"] for s in single) + 16
    assert (hmap[got["path"][:, 1], got["path"][:, 0]] == 0).all()                # the route never leaves the corridor
    sc.close()


def _raises(code, fn, word=None):
    import yolact_amd as ya
    with pytest.raises(ya.YhError) as e:
        fn()
    assert e.value.code == code, (e.value.code, str(e.value))
    assert word is None or word in str(e.value), str(e.value)


def _same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.gpu
def test_tour_and_plan_do_not_disturb_each_other(built):
    sc = _scene(480, 640, 31)
    sc.plan(targets=[(50, 50)], start=(10, 470))
    plan = sc.read_plan()
    sc.plan_tour(targets=[(600, 30), (320, 240)], start=(400, 479))
    assert _same(plan, sc.read_plan())                                            # plan -> tour -> read_plan unchanged
    tour = sc.read_tour(fields=True)
    sc.plan(targets=[(7, 7), (300, 200)], start=(630, 10))
    sc.plan_time(2)
    assert _same(tour, sc.read_tour(fields=True))                                 # tour -> plan -> read_tour unchanged
    sc.close()


@pytest.mark.gpu
def test_tour_lifecycle_and_errors(built):
    import yolact_amd as ya
    from yolact_amd import capi
    H, W = 480, 640
    rng = np.random.default_rng(21)
    depth, ci = _frame(rng, H, W)
    sc = ya.Scene(W, H)
    _raises(capi.ESTATE, lambda: sc.plan_tour(), "no frame")
    _raises(capi.ESTATE, lambda: sc.read_tour(), "no tour")
    sc.append(depth, ci, ya.COMPAT_STRICT)
    _raises(capi.ESTATE, lambda: sc.plan_tour(), "STRICT")                        # a STRICT frame is refused
    sc.append(depth, ci, ya.COMPAT_SANE)
    _raises(capi.EINVAL, lambda: sc.plan_tour(n_targets=0), "n_targets")          # K = 0
    _raises(capi.EINVAL, lambda: sc.plan_tour(targets=np.zeros((0, 2), np.int32)), "n_targets")
    _raises(capi.EINVAL, lambda: sc.plan_tour(n_targets=7), "YH_TOUR_MAX")        # K = 7
    _raises(capi.EINVAL, lambda: sc.plan_tour(targets=[(k, k) for k in range(7)]), "YH_TOUR_MAX")
    _raises(capi.EINVAL, lambda: sc.plan_tour(targets=[(5, 5), (9, 9), (5, 5)]), "duplicate")
    _raises(capi.EINVAL, lambda: sc.plan_tour(targets=[(640, 0)]), "target")
    _raises(capi.EINVAL, lambda: sc.plan_tour(targets=[(5, 5), (3, -1)]), "target")
    _raises(capi.EINVAL, lambda: sc.plan_tour(targets=[(5, 5)], start=(0, 480)), "start")
    _raises(capi.ESTATE, lambda: sc.read_tour(), "no tour")                       # none of these left a tour behind
    _raises(capi.ESTATE, lambda: sc.tour_time(1), "no tour")
    # repeated tours with growing K; two tours on one frame give identical bits
    for K in (1, 3, 2, 6):
        tg = [(40 + 90 * k, 30 + 70 * k) for k in range(K)]
        sc.plan_tour(targets=tg)
        a = sc.read_tour(fields=True)
        assert a["cost"].shape == (K, H, W) and sorted(a["order"].tolist()) == list(range(K))
        assert all(a["cost"][b][y, x] == 0 and (a["cost"][b] == 0).sum() == 1 for b, (x, y) in enumerate(tg))
    sc.plan_tour(targets=tg)
    assert _same(a, sc.read_tour(fields=True))
    # a refused call leaves the previous tour readable
    _raises(capi.EINVAL, lambda: sc.plan_tour(targets=[(1, 1), (1, 1)]), "duplicate")
    _raises(capi.EINVAL, lambda: sc.plan_tour(n_targets=7))
    assert _same(a, sc.read_tour(fields=True))
    # path_capacity too small: YH_EOVERFLOW with the needed length, nothing written
    n, k = C.c_int32(-1), C.c_int32(-1)
    small = np.full((4, 2), -7, np.int32)
    rc = sc.L.yh_scene_tour_read(sc.h, C.byref(k), None, None, None, None, None, None, None, small.ctypes.data_as(C.c_void_p), None, None, 4, C.byref(n))
    assert rc == capi.EOVERFLOW and n.value == len(a["path"]) > 4 and (small == -7).all() and k.value == -1
    assert b"path_capacity" in sc.L.yh_scene_last_error(sc.h)
    # ball targets: the frame of test_scene.py has balls 0 and 5
    sc.plan_tour()
    f = sc.read()
    assert sc.read_tour()["targets"].tolist() == [list(t) for t in R.ball_targets(f["balls"], 3, W, H)]
    # a new frame makes the tour (and the plan) stale; without a usable ball there is nothing to tour
    sc.plan()
    depth2, ci2 = _frame(rng, H, W, balls=False)
    sc.append(depth2, ci2, ya.COMPAT_SANE)
    _raises(capi.ESTATE, lambda: sc.read_tour(), "newer frame")
    _raises(capi.ESTATE, lambda: sc.tour_time(1), "newer frame")
    _raises(capi.ESTATE, lambda: sc.read_plan(), "newer frame")
    _raises(capi.ESTATE, lambda: sc.plan_tour(), "ball")
    sc.plan_tour(targets=[(100, 100)])
    f2 = sc.read()
    assert np.array_equal(_bits(sc.read_tour(fields=True)["cost"][0]), _bits(R.dijkstra(f2["map"], f2["conn0"], f2["conn1"], [(100, 100)])))
    sc.close()                                                                    # destroy after a tour
    s2 = ya.Scene(64, 48)
    with pytest.raises(ValueError):
        s2.plan_tour(targets=[(1, 1)])
    s2.close()


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
    balls = sc.read()["balls"]
    assert R.ball_targets(balls, 3, W, H) == [(20, 29), (20, 29), (40, 36)]
    sc.plan_tour(start=(0, 0))
    assert sc.read_tour()["targets"].tolist() == [[20, 29], [40, 36]]
    sc.plan_tour(n_targets=2, start=(0, 0))                                       # the first TWO balls: one pixel, one target
    assert sc.read_tour()["targets"].tolist() == [[20, 29]]
    sc.close()


def _weights_that_see_balls(blob):
    """The seeded synthetic weights answer class 0 in every cell (their logit 0 is about 9.5 everywhere, and the gate
    yolact.rs:108-118 then never opens), so a frame classified with them has no ball. This copy silences logits 0..2 of anchor 0
    in the class head (the last record but one of the YHW1 blob, DESIGN.md §2: zero weights, bias -1), so a cell is a ball
    wherever the seeded logit 3 is positive, which it is in patches of the frame - and nowhere else in the network changes."""
    blob = blob.copy()
    n = int(blob[4:8].view(np.uint32)[0])
    off = 16
    for i in range(n):
        cout, cin, kh, kw = (int(v) for v in blob[off:off + 16].view(np.uint32))
        w0 = off + 16
        b0 = w0 + ((2 * cout * kh * kw * cin + 15) & ~15)
        off = b0 + ((4 * cout + 15) & ~15)
        if i == n - 2:
            assert cout == 3 * 81
            blob[w0:w0 + 2 * 3 * kh * kw * cin] = 0
            blob[b0:b0 + 12].view(np.float32)[:] = -1.0
    assert off == blob.size
    return blob


@pytest.mark.gpu
def test_classify_scene_tour_chain_stays_on_the_device(built):
    """classify -> append_classified(frame_dev_ptr=...) -> tour to the frame's balls: the class image never visits the host."""
    import yolact_amd as ya
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
    f = sc.read()
    tg = T.distinct(R.ball_targets(f["balls"], 3, W, H))
    print(f"classified frame: {int((f['balls'][:, 2] > 0).sum())} balls with pixels, targets {tg}")
    assert len(tg) >= 2                                                           # the tour has an order to choose
    sc.plan_tour(n_targets=3)
    got = sc.read_tour(fields=True)
    assert got["targets"].tolist() == [list(t) for t in tg]
    for b, t in enumerate(tg):
        assert np.array_equal(_bits(got["cost"][b]), _bits(R.dijkstra(f["map"], f["conn0"], f["conn1"], [t])))
    assert got["path"][0].tolist() == [400, 479] and tuple(got["path"][-1]) == tg[got["order"][-1]]
    assert len(ya.serialize_path(got["directions"], 1700000000)) == 8 + 8 * len(got["directions"])
    sc.close(); eng.close()


@pytest.mark.gpu
def test_tour_beats_one_plan_per_target(built):
    """A condition, not a measurement: on the camera-like 640 x 480 frame with three explicit targets the median tour must take
    less than the three single-target plans one after the other (medians taken here, on the same box) - batching that does not
    beat doing it one by one has no reason to exist. The numbers that matter are printed (tools/time_tour.py measures them)."""
    import yolact_amd as ya
    H, W = 480, 640
    depth, ci = T.camera_like_frame(H, W)
    sc = ya.Scene(W, H)
    sc.append(depth, ci, ya.COMPAT_SANE)
    targets, start = [(70, 67), (515, 410), (320, 40)], (400, 479)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    single = []
    for t in targets:
        sc.plan(targets=[t], start=start)                                         # (warm-up too)
        single.append(med([sc.plan_time(20)["ms_per_plan"] for _ in range(5)]))
    sc.plan_tour(targets=targets, start=start)
    runs = [sc.tour_time(20) for _ in range(5)]
    tour = med([r["ms_per_tour"] for r in runs])
    print(f"tour of 3 on the camera-like frame: {tour:.3f} ms ({runs[0]['rounds']} rounds, {runs[0]['tile_runs']} tile runs); "
          f"single-target plans {[round(s, 3) for s in single]} ms, sum {sum(single):.3f}")
    assert tour < sum(single)
    sc.close()
