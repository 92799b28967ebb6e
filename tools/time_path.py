"""The path planner (yh_scene_plan: modify_path on the scene's device-resident fields) at 640x480: milliseconds per plan, solver
rounds and tile executions, for a camera-like frame (robots + balls, planned to its balls from the reference's START_NODE) and for
the serpentine maze of tests/path_ref.py (a geodesic that crosses the frame 60 times). Per case: one warm-up plan, then `sets`
repetitions of yh_scene_plan_time(reps) (device events around whole plans, the host's counter reads inside) and the host's own wall
clock around Scene.plan(); the scene back-end's time per frame beside it.
Usage: python tools/time_path.py [sets] [reps] [--connectivity 4|8] [--turn-price <tau>] [--lib <other libyolact_hip.so>]
--turn-price times the turn-aware plan (yh_scene_plan_turn, DESIGN.md §11 "Turns") with that price per 45 degrees instead, from the
same starts facing up (the serpentine's: facing right, along its corridor), and says how many steps of the route turn.
--lib times another build of the library (a build of the parent commit: `make -C tiny-object-detection_amd BUILD=build_old
LIBDIR=lib_old` in a checkout of it), to alternate with this one process by process on one box; a build without
yh_scene_plan_conn plans through yh_scene_plan (connectivity 4 only)."""
import ctypes, os, socket, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-object-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolact_amd import capi
import path_ref as R
args, conn, lib, tau = [], 4, None, None
it = iter(sys.argv[1:])
for a in it:
    if a == "--connectivity": conn = int(next(it))
    elif a == "--turn-price": tau = float(next(it))
    elif a == "--lib": lib = os.path.abspath(next(it))
    else: args.append(a)
sets = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 20
if lib:
    capi.lib_path = lambda: lib
has_conn = hasattr(ctypes.CDLL(capi.lib_path()), "yh_scene_plan_conn")
if not hasattr(ctypes.CDLL(capi.lib_path()), "yh_scene_plan_turn"):
    assert tau is None, "this build has no yh_scene_plan_turn"
    capi.SYMBOLS = [s for s in capi.SYMBOLS if "_turn" not in s[0]]
if not hasattr(ctypes.CDLL(capi.lib_path()), "yh_scene_batch_plan_turn"):
    capi.SYMBOLS = [s for s in capi.SYMBOLS if not s[0].startswith("yh_scene_batch_") or "turn" not in s[0]]
if not hasattr(ctypes.CDLL(capi.lib_path()), "yh_scene_batch_create"):
    capi.SYMBOLS = [s for s in capi.SYMBOLS if "_scene_batch_" not in s[0]]
if not has_conn:
    assert conn == 4, "this build has no yh_scene_plan_conn"
    capi.SYMBOLS = [s for s in capi.SYMBOLS if not s[0].endswith("_conn")]
import yolact_amd as ya
H, W = 480, 640
print(f"box {socket.gethostname()}, {ya.version()}, {os.path.relpath(capi.lib_path(), ROOT)}, " + (f"turn price {tau}" if tau else f"connectivity {conn}"))
sc = ya.Scene(W, H)


def plan_on(targets, start, heading=6):
    if tau:
        return sc.plan_turn(targets=targets, start=start, heading=heading, turn_price=tau)
    if has_conn:
        return sc.plan(targets=targets, start=start, connectivity=conn)
    t = None if targets is None else np.ascontiguousarray(targets, np.int32).reshape(-1, 2)
    sc._chk(sc.L.yh_scene_plan(sc.h, None if t is None else t.ctypes.data_as(ctypes.c_void_p), 3 if t is None else len(t), start[0], start[1]))


def report(name, plan):
    plan()                                                        # warm-up: buffers, code objects
    out = sc.read_turn(fields=False) if tau else sc.read_plan(fields=False)
    runs = [(sc.turn_time if tau else sc.plan_time)(reps) for _ in range(sets)]
    wall = []
    for _ in range(sets):
        t0 = time.perf_counter(); plan(); wall.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(r["ms_per_plan"] for r in runs)
    kind = f"turn price {tau}" if tau else f"{conn}-connected"
    turning = f" ({int((out['turns'] != 0).sum())} steps with a turn, {int(abs(out['turns']).sum())} x 45 degrees)" if tau else ""
    print(f"plan 640x480, {kind}, {name}: {ms[len(ms) // 2]:.3f} ms per plan (median of {sets} x {reps}; min {ms[0]:.3f}, max {ms[-1]:.3f}), "
          f"host wall per Scene.plan() {sorted(wall)[len(wall) // 2]:.3f} ms, {runs[0]['rounds']} rounds, {runs[0]['tile_runs']} tile runs, "
          f"route of {len(out['path'])} nodes{turning}")


rng = np.random.default_rng(0)
depth = rng.integers(200, 4000, (H, W)).astype(np.uint16)
ci = np.zeros((H, W, 2), np.uint8)
ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
sc.append(depth, ci, ya.COMPAT_SANE)
print(f"scene 640x480, robots + balls: {sc.time(30):.3f} ms per frame")
sc.append(depth, ci, ya.COMPAT_SANE)
report("camera-like frame, 2 balls", lambda: plan_on(None, (400, 479)))
hmap, start, target = R.serpentine(H, W)
sc.set_fields(hmap, *R.sane_connections(hmap))
report("serpentine maze, 1 target", lambda: plan_on([target], start, 0))
