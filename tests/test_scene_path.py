"""The path planner (yh_scene_plan: modify_path, src/path.rs:25-120, on the scene's device-resident fields; DESIGN.md §11 "Path
planner"). CPU part: the definition's restatement (tests/path_ref.py) against itself - two solvers, bit for bit -, closed forms and
a hand-derived case; the serialiser; the ABI surface. GPU part (-m gpu): the HIP solver's cost field bit-equal to the restatement on
the engine's own scene fields and on a constructed maze, the successor field, the route, the life cycle and every error.
PARITY UNPINNED against the reference: its modify_path indexes 224 x 224 arrays by x + y * 480 and panics."""
import os
import re
import struct
import time

import numpy as np
import pytest

import path_ref as R
from test_scene import _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_fields(rng, H, W, hmax=40):
    hmap = rng.integers(0, hmax, (H, W)).astype(np.uint32)
    return (hmap,) + R.sane_connections(hmap)


# ---------------------------------------------------------------- CPU

def test_dijkstra_equals_jacobi_bit_for_bit():
    rng = np.random.default_rng(11)
    H, W = 96, 128
    f = _random_fields(rng, H, W)
    targets = [(5, 7), (100, 90), (64, 3)]
    a = R.dijkstra(*f, targets)
    b, sweeps = R.jacobi(*f, targets)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and sweeps > 10
    assert R.equation_residual(a, *f, targets) == 0
    assert (f[1][:, :-1, 2] >= 1).all() and (f[2][:-1, :, 0] >= 1).all()          # every SANE length is >= 1
    assert np.array_equal(f[2][:, 1:, 2], f[1][:, :-1, 2]) and np.array_equal(f[1][1:, :, 0], f[2][:-1, :, 0])   # and symmetric


def test_flat_map_gives_the_manhattan_distance():
    H, W = 40, 56
    f = (np.zeros((H, W), np.uint32),) + R.sane_connections(np.zeros((H, W), np.uint32))
    targets = [(3, 4), (50, 30)]
    d = R.dijkstra(*f, targets)
    ys, xs = np.mgrid[0:H, 0:W]
    want = np.minimum.reduce([np.abs(xs - x) + np.abs(ys - y) for x, y in targets]).astype(np.float32)
    assert np.array_equal(d, want)
    assert np.array_equal(R.jacobi(*f, targets)[0], want)


def test_hand_derived_3x3_with_ties():
    """Unit lengths, one cell of height 3 at (x 1, y 0), the target in the middle. By hand: the four edge cells next to the target
    cost 1, except (1, 0) which pays its height step, 0 + 1 + 3 = 4 (through a corner it would be 2 + 1 + 3 = 6); corners cost 2.
    Corner (0, 2) can go right or up and corner (2, 2) left or up, all at cost 2: (left, right, up, down) decides - right / left."""
    hmap = np.zeros((3, 3), np.uint32)
    hmap[0, 1] = 3
    conn0 = np.full((3, 3, 4), -1, np.float32); conn1 = np.full((3, 3, 4), -1, np.float32)
    conn0[:, :-1, 2] = 1; conn1[:, 1:, 2] = 1; conn0[1:, :, 0] = 1; conn1[:-1, :, 0] = 1
    d = R.dijkstra(hmap, conn0, conn1, [(1, 1)])
    assert d.tolist() == [[2, 4, 2], [1, 0, 1], [2, 1, 2]]
    assert np.array_equal(R.jacobi(hmap, conn0, conn1, [(1, 1)])[0], d)
    nxt = R.successors(d, hmap, conn0, conn1, [(1, 1)])
    assert nxt.tolist() == [[3, 4, 5], [4, -1, 4], [7, 4, 7]]
    path, dirs = R.walk(d, nxt, (0, 2))
    assert path.tolist() == [[0, 2], [1, 2], [1, 1]]
    assert dirs.tolist() == [[1.0, 0.0], [1.0, float(np.float32(np.pi / 2))]]
    path, dirs = R.walk(d, nxt, (1, 1))
    assert path.tolist() == [[1, 1]] and dirs.shape == (0, 2)


def test_ball_targets_and_size_guard():
    balls = np.zeros((100, 4), np.float32)
    balls[2] = (10.9, 20.2, 5, 0); balls[4] = (700, 3, 1, 0); balls[7] = (1.5, 479.99, 9, 0); balls[9] = (5, 5, 2, 0)
    assert R.ball_targets(balls, 3, 640, 480) == [(10, 20), (1, 479)]          # ball 4 is taken and dropped, ball 9 is the fourth
    assert R.ball_targets(balls, 4, 640, 480) == [(10, 20), (1, 479), (5, 5)]
    assert R.size_ok(640, 480) and (640 + 480) * (2 * 480 + 1) == 1076320
    assert R.size_ok(1440, 1440) and not R.size_ok(2048, 2048)


def test_serialize_path_is_path_serialize_byte_for_byte():
    """path.rs:17-21: as_secs().to_be_bytes(), then m.to_be_bytes() ++ r.to_be_bytes() per pair."""
    from yolact_amd import capi
    got = capi.serialize_path(np.array([[1.0, 0.0], [2.5, np.pi]], np.float32), 0x0102030405)
    want = bytes([0, 0, 0, 1, 2, 3, 4, 5]) + bytes([0x3F, 0x80, 0, 0]) + bytes(4) + bytes([0x40, 0x20, 0, 0]) + bytes([0x40, 0x49, 0x0F, 0xDB])
    assert got == want
    assert capi.serialize_path(np.zeros((0, 2), np.float32), 7) == struct.pack(">Q", 7)


def test_planner_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0] for s in capi.SYMBOLS}
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read(), flags=re.S)
    for name in ("yh_scene_plan", "yh_scene_plan_read"):
        assert re.search(r"\b%s\s*\(" % name, pub) and name in bound, name
    for name in ("yh_scene_set_fields", "yh_scene_plan_time"):
        assert re.search(r"\b%s\s*\(" % name, dbg) and not re.search(r"\b%s\s*\(" % name, pub) and name in bound, name
    assert "#define YH_ABI_VERSION 4" in pub
    for m in ("plan", "read_plan", "set_fields", "plan_time"):
        assert callable(getattr(capi.Scene, m))


# ---------------------------------------------------------------- GPU

def _scene(H, W, seed):
    import yolact_amd as ya
    rng = np.random.default_rng(seed)
    depth, ci = _frame(rng, H, W)
    sc = ya.Scene(W, H)
    sc.append(depth, ci, ya.COMPAT_SANE)
    return sc, depth, ci


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,targets,start", [
    (480, 640, None, None),
    (480, 640, [(17, 400), (600, 30), (320, 240), (321, 240)], (400, 479)),
    (37, 53, [(2, 3), (50, 30)], (26, 36)),
    (8, 8, [(7, 0)], (0, 7)),
    (100, 9, [(4, 50)], (0, 0)),
])
def test_cost_field_bit_equal_to_the_reference(built, H, W, targets, start):
    """The engine's own Scene.read() fields go through path_ref's Dijkstra; the device field must have the same bits."""
    sc, _, _ = _scene(H, W, H * 1000 + W)
    f = sc.read()
    sc.plan(targets=targets, start=start)
    got = sc.read_plan()
    tg = targets if targets is not None else R.ball_targets(f["balls"], 3, W, H)
    assert len(tg) >= 1
    want = R.dijkstra(f["map"], f["conn0"], f["conn1"], tg)
    print(f"{W}x{H}: {len(tg)} targets, max cost {want.max()}, {sc.plan_time(1)}")
    assert np.array_equal(_bits(got["cost"]), _bits(want))
    nxt = R.successors(want, f["map"], f["conn0"], f["conn1"], tg)
    assert np.array_equal(got["next"], nxt)
    path, dirs = R.walk(want, nxt, start if start is not None else (400, 479))
    assert np.array_equal(got["path"], path) and np.array_equal(_bits(got["directions"]), _bits(dirs))
    sc.close()


@pytest.mark.gpu
def test_field_satisfies_its_defining_equations_at_every_pixel(built):
    """Proves the field without trusting the Dijkstra: 0 at the targets, elsewhere the minimum candidate, bitwise, everywhere."""
    H, W = 480, 640
    sc, _, _ = _scene(H, W, 5)
    f = sc.read()
    sc.plan()
    got = sc.read_plan()
    tg = R.ball_targets(f["balls"], 3, W, H)
    assert len(tg) == 2                                          # the frame of test_scene.py has balls 0 and 5
    assert np.isfinite(got["cost"]).all() and got["cost"].max() < 2 ** 24
    assert all(got["cost"][y, x] == 0 for x, y in tg) and (got["cost"] == 0).sum() == len(tg)
    assert R.equation_residual(got["cost"], f["map"], f["conn0"], f["conn1"], tg) == 0
    sc.close()


@pytest.mark.gpu
def test_next_and_route(built):
    """next is the first neighbour (left, right, up, down) achieving equality; the walk from the start reaches a target over
    strictly decreasing costs; directions are the f32 cost differences and the rotations {0, pi, pi/2} of the route's turns."""
    H, W = 480, 640
    sc, _, _ = _scene(H, W, 8)
    f = sc.read()
    sc.plan()
    got = sc.read_plan()
    d, nxt, path, dirs = got["cost"], got["next"], got["path"], got["directions"]
    tg = R.ball_targets(f["balls"], 3, W, H)
    cands = R.candidates(d, f["map"], f["conn0"], f["conn1"])
    idx = np.arange(H * W, dtype=np.int32).reshape(H, W)
    first = np.full((H, W), -1, np.int32)
    taken = np.zeros((H, W), bool)
    for c, off in zip(cands, (-1, 1, -W, W)):
        hit = (_bits(c) == _bits(d)) & ~taken
        first[hit] = idx[hit] + off
        taken |= hit
    for x, y in tg:
        first[y, x] = -1
    assert np.array_equal(nxt, first) and (nxt == -1).sum() == len(tg)
    assert path[0].tolist() == [400, 479] and tuple(path[-1]) in tg and len(path) > 100
    lin = path[:, 1] * W + path[:, 0]
    assert np.array_equal(nxt.flat[lin[:-1]], lin[1:])
    cost = d.flat[lin]
    assert (np.diff(cost) < 0).all() and cost[-1] == 0
    assert len(dirs) == len(path) - 1
    assert np.array_equal(_bits(dirs[:, 0]), _bits(cost[:-1] - cost[1:]))
    assert dirs[0, 1] == 0
    straight = (path[:-2] + path[2:] == 2 * path[1:-1]).all(1)
    assert np.array_equal(_bits(dirs[1:, 1]), _bits(np.where(straight, R.PI, R.HALF_PI).astype(np.float32)))
    assert (np.abs(np.diff(path, axis=0)).sum(1) == 1).all()
    # route only: the same route without the fields
    short = sc.read_plan(fields=False)
    assert set(short) == {"path", "directions"} and np.array_equal(short["path"], path) and np.array_equal(short["directions"], dirs)
    sc.close()


@pytest.mark.gpu
def test_constructed_maze(built):
    """A serpentine corridor between walls of height 400 at 480 x 640, one target at its far end: the geodesic crosses the frame 60
    times, so a solver whose round count were tied to tile adjacency would stop early. Bit-equal to the Dijkstra."""
    import yolact_amd as ya
    H, W = 480, 640
    hmap, start, target = R.serpentine(H, W)
    conn0, conn1 = R.sane_connections(hmap)
    sc = ya.Scene(W, H)
    sc.set_fields(hmap, conn0, conn1)
    sc.plan(targets=[target], start=start)
    got = sc.read_plan()
    want = R.dijkstra(hmap, conn0, conn1, [target])
    stats = sc.plan_time(3)
    print(f"maze {W}x{H}: route of {len(got['path'])} nodes, cost at start {want[start[1], start[0]]}, {stats}")
    assert np.array_equal(_bits(got["cost"]), _bits(want))
    assert want[start[1], start[0]] == (H // 8) * (W - 1) + (H // 8 - 1) * 8     # the corridor's length: flat, unit steps
    assert len(got["path"]) == int(want[start[1], start[0]]) + 1 and tuple(got["path"][-1]) == target
    assert (hmap[got["path"][:, 1], got["path"][:, 0]] == 0).all()               # the route never leaves the corridor
    assert stats["rounds"] > W // 8 and stats["tile_runs"] >= stats["rounds"]
    assert R.equation_residual(got["cost"], hmap, conn0, conn1, [target]) == 0
    sc.close()


def _tile_border_walls():
    """Target sets that cover a whole border between two of the solver's tiles (any tile edge that divides 32), so that the tile
    behind the wall sees nothing but targets move on that border: (H, W, targets, start)."""
    ring = [(x, y) for x in range(31, 65) for y in (31, 64)] + [(x, y) for y in range(32, 64) for x in (31, 64)]
    return [(3, 64, [(31, 0), (31, 1), (31, 2)], (63, 1)),                   # a wall on the left tile's last column
            (3, 64, [(32, 0), (32, 1), (32, 2)], (0, 1)),                    # ... on the right tile's first column
            (64, 3, [(0, 32), (1, 32), (2, 32)], (1, 0)),
            (33, 64, [(x, 31) for x in range(64)], (5, 32)),                 # a full row above a one-row band of tiles
            (96, 96, ring, (48, 48)),                                        # the middle tile enclosed by targets
            (96, 96, [(x, y) for x in range(32, 64) for y in range(32, 64)], (0, 0))]   # a tile made of targets


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(6))
def test_walls_of_targets_on_tile_borders(built, case):
    """A target's drop from +inf to 0 must wake the tile across the border it lies on: with a whole border segment made of targets
    nothing else on it moves. Constructed fields through set_fields; bit-equal to the Dijkstra, no +inf left, the walk arrives."""
    import yolact_amd as ya
    H, W, targets, start = _tile_border_walls()[case]
    hmap = np.random.default_rng(100 + case).integers(0, 30, (H, W)).astype(np.uint32)
    conn0, conn1 = R.sane_connections(hmap)
    sc = ya.Scene(W, H)
    sc.set_fields(hmap, conn0, conn1)
    sc.plan(targets=targets, start=start)
    got = sc.read_plan()
    want = R.dijkstra(hmap, conn0, conn1, targets)
    assert np.isfinite(got["cost"]).all()
    assert np.array_equal(_bits(got["cost"]), _bits(want))
    nxt = R.successors(want, hmap, conn0, conn1, targets)
    assert np.array_equal(got["next"], nxt)
    path, dirs = R.walk(want, nxt, start)
    assert np.array_equal(got["path"], path) and np.array_equal(_bits(got["directions"]), _bits(dirs))
    assert tuple(got["path"][-1]) in set(targets)
    sc.close()


@pytest.mark.gpu
def test_refused_calls_touch_nothing(built):
    """A plan refused with YH_EINVAL leaves the earlier plan of the frame readable; set_fields refuses fields no SANE frame gives
    (a length below 1, an edge whose two ends disagree) and uploads nothing."""
    import yolact_amd as ya
    from yolact_amd import capi
    H, W = 40, 70
    hmap = np.random.default_rng(1).integers(0, 30, (H, W)).astype(np.uint32)
    conn0, conn1 = R.sane_connections(hmap)
    sc = ya.Scene(W, H)
    sc.set_fields(hmap, conn0, conn1)
    sc.plan(targets=[(3, 3)], start=(60, 30))
    a = sc.read_plan()
    for bad in (lambda: sc.plan(targets=[(70, 0)], start=(0, 0)), lambda: sc.plan(targets=[(1, 1)], start=(0, 40))):
        with pytest.raises(ya.YhError) as e:
            bad()
        assert e.value.code == capi.EINVAL
    b = sc.read_plan()
    assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    for y, x, k, arr, v in ((5, 6, 2, 0, 0.5), (5, 6, 0, 1, np.inf), (7, 8, 2, 1, 9.0), (7, 8, 0, 0, 9.0)):
        c = [conn0.copy(), conn1.copy()]
        c[arr][y, x, k] = v
        with pytest.raises(ya.YhError) as e:
            sc.set_fields(hmap, c[0], c[1])
        assert e.value.code == capi.EINVAL and "SANE" in str(e.value)
    b = sc.read_plan()                                           # the refused uploads were no new frame
    assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    sc.close()


@pytest.mark.gpu
def test_lifecycle_and_errors(built):
    import yolact_amd as ya
    from yolact_amd import capi
    H, W = 480, 640
    rng = np.random.default_rng(21)
    depth, ci = _frame(rng, H, W)
    sc = ya.Scene(W, H)

    def raises(code, fn, word=None):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert word is None or word in str(e.value), str(e.value)

    raises(capi.ESTATE, lambda: sc.plan(), "no frame")                                    # plan before any append
    sc.append(depth, ci, ya.COMPAT_STRICT)
    raises(capi.ESTATE, lambda: sc.plan(), "STRICT")                                      # the last frame is STRICT
    sc.append(depth, ci, ya.COMPAT_SANE)
    raises(capi.ESTATE, lambda: sc.read_plan(), "no plan")                                # read before a plan
    raises(capi.EINVAL, lambda: sc.plan(targets=[(640, 0)]), "target")                    # target outside
    raises(capi.EINVAL, lambda: sc.plan(targets=[(5, 5), (3, -1)]), "target")
    raises(capi.EINVAL, lambda: sc.plan(start=(0, 480)), "start")                         # start outside
    raises(capi.EINVAL, lambda: sc.plan(n_targets=0), "n_targets")                        # n_targets < 1
    raises(capi.EINVAL, lambda: sc.plan(targets=np.zeros((0, 2), np.int32)), "n_targets")
    raises(capi.ESTATE, lambda: sc.read_plan(), "no plan")                                # none of these left a plan behind
    # two plans on one frame: identical bits
    sc.plan()
    a = sc.read_plan()
    sc.plan()
    b = sc.read_plan()
    assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    # path_capacity too small: YH_EOVERFLOW with the needed length, nothing written
    import ctypes as C
    n = C.c_int32(-1)
    small = np.full((4, 2), -7, np.int32)
    rc = sc.L.yh_scene_plan_read(sc.h, None, None, small.ctypes.data_as(C.c_void_p), None, 4, C.byref(n))
    assert rc == capi.EOVERFLOW and n.value == len(a["path"]) > 4 and (small == -7).all()
    assert b"path_capacity" in sc.L.yh_scene_last_error(sc.h)
    # no usable ball
    depth2, ci2 = _frame(rng, H, W, balls=False)
    sc.append(depth2, ci2, ya.COMPAT_SANE)
    raises(capi.ESTATE, lambda: sc.read_plan(), "newer frame")                            # a new append invalidates the plan
    raises(capi.ESTATE, lambda: sc.plan(), "ball")
    # a re-plan reflects the new frame
    sc.plan(targets=[(100, 100)])
    c = sc.read_plan()
    f2 = sc.read()
    assert np.array_equal(_bits(c["cost"]), _bits(R.dijkstra(f2["map"], f2["conn0"], f2["conn1"], [(100, 100)])))
    assert not np.array_equal(c["cost"], a["cost"])
    sc.close()
    # the size guard, at plan time
    big = ya.Scene(2048, 2048)
    big.append(np.full((2048, 2048), 1000, np.uint16), np.zeros((2048, 2048, 2), np.uint8), ya.COMPAT_SANE)
    raises(capi.EINVAL, lambda: big.plan(targets=[(1, 1)], start=(0, 0)), "2^24")
    big.close()
    # start=None names the reference's START_NODE, which exists at 640 x 480 only
    s2 = ya.Scene(64, 48)
    with pytest.raises(ValueError):
        s2.plan(targets=[(1, 1)])
    s2.close()


@pytest.mark.gpu
def test_classify_scene_plan_chain_stays_on_the_device(built):
    """classify -> append_classified(frame_dev_ptr=...) -> plan: the class image never visits the host."""
    import yolact_amd as ya
    H, W = 480, 640
    rng = np.random.default_rng(3)
    depth, _ = _frame(rng, H, W)
    y = ya.Yolact.init(seed=1, compat_mode=ya.COMPAT_SANE)
    cam = (rng.integers(0, 256, (H, W, 3), dtype=np.uint32) * np.array([1 << 24, 1 << 16, 1 << 8], np.uint32)).sum(-1).astype(np.uint32).reshape(-1)
    y.classify(cam)
    sc = ya.Scene(W, H)
    sc.append_classified(depth, frame_dev_ptr=y.interpreter.classify_device_frame(), mode=ya.COMPAT_SANE)
    tg = [(40, 60), (600, 400)]
    sc.plan(targets=tg)
    got, f = sc.read_plan(), sc.read()
    assert np.array_equal(_bits(got["cost"]), _bits(R.dijkstra(f["map"], f["conn0"], f["conn1"], tg)))
    assert tuple(got["path"][-1]) in tg and got["path"][0].tolist() == [400, 479]
    wire = ya.serialize_path(got["directions"], 1700000000)
    assert len(wire) == 8 + 8 * len(got["directions"])
    sc.close()


@pytest.mark.gpu
def test_plan_beats_the_cpu_restatement(built):
    """No earlier implementation exists and the reference's planner cannot execute, so the bound is relative: a plan at 640 x 480
    must beat path_ref's numpy Jacobi solve of the same field, timed here on the same box. A floor that catches a broken work list,
    not a target; the number that matters is printed (and measured properly by tools/time_path.py)."""
    H, W = 480, 640
    sc, _, _ = _scene(H, W, 13)
    f = sc.read()
    tg = R.ball_targets(f["balls"], 3, W, H)
    sc.plan()                                                     # warm-up: buffers, code objects
    t0 = time.perf_counter()
    sc.plan()
    gpu_s = time.perf_counter() - t0
    got = sc.read_plan()
    t0 = time.perf_counter()
    want, sweeps = R.jacobi(f["map"], f["conn0"], f["conn1"], tg)
    cpu_s = time.perf_counter() - t0
    stats = sc.plan_time(10)
    print(f"plan 640x480: host wall {gpu_s * 1e3:.3f} ms, {stats}; numpy Jacobi {cpu_s:.2f} s in {sweeps} sweeps")
    assert np.array_equal(_bits(got["cost"]), _bits(want))
    assert gpu_s < cpu_s and stats["ms_per_plan"] * 1e-3 < cpu_s
    sc.close()
