"""The tour planner (yh_scene_plan_tour: K single-target cost fields relaxed in the same launches, best order, joined route) at
640x480, for K = 1, 2, 3, 6 on the camera-like frame of tools/time_path.py and on the serpentine maze of tests/path_ref.py:
milliseconds per tour, solver rounds and tile executions (median of `sets` x yh_scene_tour_time(reps); the maze with reps / 4),
and beside them what a host had to do before: K single-target yh_scene_plan calls one after the other (the sum of their medians by
yh_scene_plan_time; the read-backs and the stitching a host would add are NOT in it).
    python tools/time_tour.py [--connectivity 4|8] [sets = 5] [reps = 20]
    python tools/time_tour.py [--connectivity 4|8] --ab <other libyolact_hip.so> [passes = 2] [sets] [reps]
    python tools/time_tour.py --turn-price tau [sets] [reps]          (with --ab too)
--turn-price tau: the turn-aware tour instead (yh_scene_plan_turn_tour, DESIGN.md §11 "Turn tour"; start heading 6, the price tau
per 45 degrees; yh_scene_turn_tour_time), beside K single-target turn plans one after the other (yh_scene_turn_time) - the first
of the calls a host had to make before; the read-backs, the walks for the arrival headings and the stitching are NOT in it.
--connectivity 8: the tours and the single-target plans beside them on the 8-connected grid (DESIGN.md §11 "Diagonals").
--ab alternates this build and another one (a build of the parent commit: `make -C tiny-object-detection_amd BUILD=build_old
LIBDIR=lib_old` in a checkout of it) process by process on one box; the other build need not have the tour: it runs the
sequential plans only. A build without the _conn entry points runs with connectivity 4 only, through yh_scene_plan(_tour)."""
import json, os, socket, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-object-detection_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
H, W = 480, 640
KS = (1, 2, 3, 6)
CAMERA = dict(targets=[(70, 67), (515, 410), (320, 40), (600, 100), (30, 440), (250, 300)], start=(400, 479))
MAZE = dict(targets=[None, None, (320, 244), (500, 124), (100, 364), (600, 444)], start=(100, 84))   # [0], [1]: the corridor's ends


def median(xs):
    return sorted(xs)[len(xs) // 2]


def child(lib, sets, reps, conn, tau=0.0):
    """One process, one build: a JSON line per (case, K). tau: the turn price, 0 for the pixel tour."""
    from yolact_amd import capi
    import path_ref as R
    import tour_ref as T
    if lib:
        capi.lib_path = lambda: lib
    import ctypes
    has_tour = hasattr(ctypes.CDLL(capi.lib_path()), "yh_scene_plan_tour")
    if not has_tour:
        capi.SYMBOLS = [s for s in capi.SYMBOLS if "tour" not in s[0]]
    has_turn_tour = hasattr(ctypes.CDLL(capi.lib_path()), "yh_scene_plan_turn_tour")
    if not has_turn_tour:
        capi.SYMBOLS = [s for s in capi.SYMBOLS if "turn_tour" not in s[0]]
    has_conn = hasattr(ctypes.CDLL(capi.lib_path()), "yh_scene_plan_conn")
    if not has_conn:
        assert conn == 4, "this build has no yh_scene_plan_conn"
        capi.SYMBOLS = [s for s in capi.SYMBOLS if not s[0].endswith("_conn")]
    if lib:   # another build may lack entry points that came after it (the scene batch's tour): none of them is timed here
        capi.SYMBOLS = [s for s in capi.SYMBOLS if not s[0].startswith("yh_scene_batch_") or hasattr(ctypes.CDLL(lib), s[0])]
    import yolact_amd as ya
    sc = ya.Scene(W, H)

    if tau:   # the turn-aware entry points in place of the pixel ones: same cases, same rows
        has_tour = has_turn_tour
        sc.plan_time, sc.tour_time, sc.read_tour = sc.turn_time, (sc.turn_tour_time if has_turn_tour else None), lambda: sc.read_turn_tour(fields=False)

    def plan(entry, targets, start):   # Scene.plan / Scene.plan_tour, or on a build without connectivity the entry point it has
        if tau:
            return (sc.plan_turn_tour if entry == "yh_scene_plan_tour" else sc.plan_turn)(targets=targets, start=start, heading=6, turn_price=tau)
        if has_conn:
            return (sc.plan_tour if entry == "yh_scene_plan_tour" else sc.plan)(targets=targets, start=start, connectivity=conn)
        t = np.ascontiguousarray(targets, np.int32).reshape(-1, 2)
        sc._chk(getattr(sc.L, entry)(sc.h, t.ctypes.data_as(ctypes.c_void_p), len(t), start[0], start[1]))

    hmap, end0, end1 = R.serpentine(H, W)
    MAZE["targets"][:2] = [end0, end1]
    for name, case, r in (("camera", CAMERA, reps), ("maze", MAZE, max(1, reps // 4))):
        if name == "camera":
            sc.append(*T.camera_like_frame(H, W), ya.COMPAT_SANE)
        else:
            sc.set_fields(hmap, *R.sane_connections(hmap))
        single = []
        for t in case["targets"]:
            plan("yh_scene_plan", [t], case["start"])                             # warm-up: buffers, code objects
            runs = [sc.plan_time(r) for _ in range(sets)]
            single.append(dict(ms=median([x["ms_per_plan"] for x in runs]), rounds=runs[0]["rounds"], tile_runs=runs[0]["tile_runs"]))
        for K in KS:
            row = dict(box=socket.gethostname(), case=name, conn=conn, tau=tau, K=K, seq_ms=sum(s["ms"] for s in single[:K]), seq_rounds=[s["rounds"] for s in single[:K]],
                       seq_tile_runs=sum(s["tile_runs"] for s in single[:K]))
            if has_tour:
                plan("yh_scene_plan_tour", case["targets"][:K], case["start"])
                out = sc.read_tour()
                runs = [sc.tour_time(r) for _ in range(sets)]
                ms = sorted(x["ms_per_tour"] for x in runs)
                row.update(tour_ms=median(ms), tour_min=ms[0], tour_max=ms[-1], rounds=runs[0]["rounds"], tile_runs=runs[0]["tile_runs"],
                           order=out["order"].tolist(), route=len(out["path"]))
            print(json.dumps(row), flush=True)


def show(tag, row):
    tour = (f"{'turn ' if row.get('tau') else ''}tour {row['tour_ms']:.3f} ms ({row['tour_min']:.3f}-{row['tour_max']:.3f}), {row['rounds']} rounds, {row['tile_runs']} tile runs, "
            f"order {row['order']}, route of {row['route']} nodes | ") if "tour_ms" in row else ""
    kind = f"turn price {row['tau']:g}" if row.get("tau") else f"{row['conn']}-connected"
    print(f"{tag}{row['case']:6s} {kind} K={row['K']}: {tour}{row['K']} single-target {'turn ' if row.get('tau') else ''}plans one by one {row['seq_ms']:.3f} ms, rounds {row['seq_rounds']}, "
          f"{row['seq_tile_runs']} tile runs", flush=True)


def run_child(lib, sets, reps, conn, tau=0.0):
    out = subprocess.run([sys.executable, __file__, "--child", lib, str(sets), str(reps), str(conn), str(tau)], capture_output=True, text=True, check=True).stdout
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


if __name__ == "__main__":
    a = sys.argv[1:]
    conn = 4
    if "--connectivity" in a:
        i = a.index("--connectivity")
        conn = int(a[i + 1])
        del a[i:i + 2]
    tau = 0.0
    if "--turn-price" in a:
        i = a.index("--turn-price")
        tau, conn = float(a[i + 1]), 8
        del a[i:i + 2]
    if a and a[0] == "--child":
        child(a[1], int(a[2]), int(a[3]), int(a[4]), float(a[5]) if len(a) > 5 else 0.0)
    elif a and a[0] == "--ab":
        other = os.path.abspath(a[1])
        passes = int(a[2]) if len(a) > 2 else 2
        sets, reps = (int(a[3]) if len(a) > 3 else 5), (int(a[4]) if len(a) > 4 else 20)
        for r in range(passes):
            for tag, lib in (("this ", ""), ("other", other)):
                for row in run_child(lib, sets, reps, conn, tau):
                    show(f"pass {r} {tag} [{row['box']}] ", row)
    else:
        sets, reps = (int(a[0]) if a else 5), (int(a[1]) if len(a) > 1 else 20)
        for row in run_child("", sets, reps, conn, tau):
            show(f"[{row['box']}] ", row)
