"""The scene batch (yh_scene_batch, DESIGN.md §11 "Scene batch") against the single handle at 640x480, for n = 1, 2, 4, 8, 16, 64 frames:
the camera-like frame of tools/time_path.py (robots + two balls) with a different depth seed per slot. Per n: milliseconds PER FRAME of
the append (yh_scene_batch_time: device events round whole batches) and of the plan with connectivity 4 and 8 (yh_scene_batch_plan_time:
the host's counter reads inside, as for a caller), with the solver's rounds and tile runs; beside them the same frames through ONE
Scene handle, call after call (append, yh_scene_time, plan, yh_scene_plan_time per frame; the sums divided by n), and the host's wall
clock round stage + append + plan of the batch and round append + plan of the n single frames. Batch and single alternate set by set;
medians over the sets.
--turn-price P: the plan columns are the batched turn-aware plan instead (yh_scene_batch_plan_turn with price P per 45 degrees,
DESIGN.md §11 "Scene batch: turns"; yh_scene_batch_turn_time) beside the same frames through Scene.plan_turn (yh_scene_turn_time per
frame), every frame from the reference's START_NODE facing up; the host wall is then stage + append + turn plan.
--turn-tour (with --turn-price P): the batched turn-aware tour instead (yh_scene_batch_plan_turn_tour, DESIGN.md §11 "Scene batch: turn
tours"; yh_scene_batch_turn_tour_time) beside the same frames through Scene.plan_turn_tour (yh_scene_turn_tour_time per frame), to the
first K of tools/time_tour.py's six camera targets in every frame (--targets K, default 3); the host wall is then stage + append +
turn tour.
--tour [--connectivity 8]: the batched plain tour instead (yh_scene_batch_plan_tour, DESIGN.md §11 "Scene batch: tours";
yh_scene_batch_tour_time) beside the same frames through one Scene.plan_tour (yh_scene_tour_time per frame), to the first K of the same
camera targets (--targets K, default 3) on the 4- or 8-connected grid, for n = 1, 2, 8, 16, 64; the host wall is then stage + append + tour.
--memory: the memory append instead (yh_scene_batch_append_memory, DESIGN.md §11 "Scene batch: memory"; yh_scene_batch_memory_time),
no plans: ms per frame in two columns - a stream per frame (frames share every launch) and every frame on stream 0 (a chain of n fuse
launches) - beside the same frames through one Scene.append_memory (yh_scene_memory_time per frame), every memory filled before it is
timed; then, for n = 8 on the robots + balls frame of tools/time_scene.py in every slot, the two ratios and the run-to-run spread of
each side (what tests/test_scene_batch_memory.py derives its ceiling from).
--memory-search [--n-rot K --radius R]: the batched search append instead (yh_scene_batch_append_memory_search, DESIGN.md §11 "Scene
batch: registration"; yh_scene_batch_memory_search_time), no plans, over (n_rot, radius) = (1, 0), (1, 4), (5, 4), (9, 8) or the one
given: ms per frame of the whole append and, beside it, of its registration launches alone, in the same two columns, beside the same
frames through one Scene.append_memory_search (yh_scene_memory_search_time per frame); the candidates are tools/time_scene.py's prior
with bases 0.01 rad apart. Then, for n = 8 and (5, 4) on the robots + balls frame in every slot, alternated with the single handle, one
warm-up each, five runs of 30 replays: the two ratios and the single handle's spread (what tests/test_scene_batch_register.py derives
its ceiling from).
--memory-pyramid [--levels L --radius R --refine r --n-rot K]: the batched pyramid append instead (yh_scene_batch_append_memory_pyramid,
DESIGN.md §11 "Scene batch: pyramid registration"; yh_scene_batch_memory_pyramid_time), no plans, at (n_rot, levels, radius, refine) =
(5, 3, 8, 1) or the one given: the same columns as --memory-search, beside the same frames through one Scene.append_memory_pyramid
(yh_scene_memory_pyramid_time per frame). Then, for n = 8 and (5, 3, 8, 1) on the robots + balls frame in every slot, alternated with
the single handle, one warm-up each, five runs of 30 replays: the two ratios and the single handle's spread (what
tests/test_scene_batch_pyramid.py derives its ceiling from).
--memory-search-norm [--n-rot K --radius R] [--min-inside m], --memory-pyramid-norm [--levels L --radius R --refine r --n-rot K]
[--min-inside m]: the two normalised batched appends instead (yh_scene_batch_append_memory_search_norm, _pyramid_norm, DESIGN.md §11
"Scene batch: normalised registration", "Scene batch: normalised pyramid registration"; yh_scene_batch_memory_search_norm_time,
_pyramid_norm_time): the columns of --memory-search and --memory-pyramid, beside the same frames through one
Scene.append_memory_search_norm or _pyramid_norm (yh_scene_memory_search_norm_time, _pyramid_norm_time per frame), min_inside W H // 4
unless given; then the n = 8 run at (5, 4) or (5, 3, 8, 1) whose single-handle spread tests/test_scene_batch_register_norm.py and
tests/test_scene_batch_pyramid_norm.py derive their ceilings from.
--frames n,n,..: those batch sizes only.
--lib times another build of the library (a build of the parent commit: `make -C tiny-object-detection_amd BUILD=build_old
LIBDIR=lib_old` in a checkout of it), to alternate with this one process by process on one box.
Usage: python tools/time_scene_batch.py [sets] [reps] [--memory | --memory-search [--n-rot K --radius R] | --memory-pyramid [--levels L --radius R --refine r --n-rot K] | --memory-search-norm .. | --memory-pyramid-norm .. [--min-inside m] | --turn-price P [--turn-tour [--targets K]] | --tour [--connectivity 8] [--targets K]] [--frames n,n,..] [--lib <other libyolact_hip.so>]"""
import os, socket, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-object-detection_amd"))
from yolact_amd import capi
args, tau, tour, plain, conn_tour, K, sizes, lib, memory = [], None, False, False, 4, 3, None, None, False
search, n_rot_arg, radius_arg = False, None, None
pyramid, levels_arg, refine_arg = False, None, None
norm, min_inside = False, None
it = iter(sys.argv[1:])
for a in it:
    if a == "--turn-price": tau = float(next(it))
    elif a == "--turn-tour": tour = True
    elif a == "--tour": plain = True
    elif a == "--memory": memory = True
    elif a == "--memory-search": search = True
    elif a == "--memory-pyramid": pyramid = True
    elif a == "--memory-search-norm": search = norm = True
    elif a == "--memory-pyramid-norm": pyramid = norm = True
    elif a == "--min-inside": min_inside = int(next(it))
    elif a == "--levels": levels_arg = int(next(it))
    elif a == "--refine": refine_arg = int(next(it))
    elif a == "--n-rot": n_rot_arg = int(next(it))
    elif a == "--radius": radius_arg = int(next(it))
    elif a == "--connectivity": conn_tour = int(next(it))
    elif a == "--targets": K = int(next(it))
    elif a == "--frames": sizes = tuple(int(v) for v in next(it).split(","))
    elif a == "--lib": lib = os.path.abspath(next(it))
    else: args.append(a)
sets = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 20
if tour and not tau: sys.exit("--turn-tour needs --turn-price P")
if plain and tau: sys.exit("--tour is the plain tour: no --turn-price")
if memory and (plain or tau): sys.exit("--memory times the append alone: no --tour, no --turn-price")
if search and (memory or plain or tau): sys.exit("--memory-search times the search append alone: no --memory, no --tour, no --turn-price")
if pyramid and (search or memory or plain or tau): sys.exit("--memory-pyramid times the pyramid append alone: no --memory, no --memory-search, no --tour, no --turn-price")
if min_inside is not None and not norm: sys.exit("--min-inside goes with --memory-search-norm or --memory-pyramid-norm")
if pyramid:
    given = [v is not None for v in (n_rot_arg, levels_arg, radius_arg, refine_arg)]
    if any(given) and not all(given): sys.exit("--n-rot K, --levels L, --radius R and --refine r go together")
elif (n_rot_arg is None) != (radius_arg is None) or (n_rot_arg is not None and not search) or levels_arg is not None or refine_arg is not None:
    sys.exit("--n-rot K and --radius R go together, with --memory-search; --levels and --refine go with --memory-pyramid")
if sizes is None: sizes = (1, 2, 8, 16, 64) if plain else (1, 2, 4, 8, 16, 64)
own = tau or plain   # the plan columns are one kind of its own instead of the plan with connectivity 4 and 8
if lib:
    capi.lib_path = lambda: lib
import yolact_amd as ya
H, W = 480, 640
TARGETS = [(70, 67), (515, 410), (320, 40), (600, 100), (30, 440), (250, 300)][:K]   # tools/time_tour.py's camera targets
print(f"box {socket.gethostname()}, {ya.version()}, {os.path.relpath(capi.lib_path(), ROOT)}, {sets} sets x {reps} reps" + (", memory append" if memory else "") + (", search append" if search else "") + (", pyramid append" if pyramid else "") + (f", normalised, min_inside {min_inside if min_inside is not None else (W * H) // 4}" if norm else "") + (f", turn price {tau}" if tau else "") + (f", turn tour of {K} targets" if tour else "") + (f", tour of {K} targets, {conn_tour}-connected" if plain else ""))


def frame(seed):
    depth = np.random.default_rng(seed).integers(200, 4000, (H, W)).astype(np.uint16)
    ci = np.zeros((H, W, 2), np.uint8)
    ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
    return depth, ya.SceneBatch.pack(ci)


med = lambda v: sorted(v)[len(v) // 2]
sc = ya.Scene(W, H)


def memory_columns(frames, motion):
    """(single, a stream per frame, all on stream 0): lists over the sets of ms per frame for these frames, alternated set by set"""
    n = len(frames)
    sb = ya.SceneBatch(W, H, n)
    sb.stage_frames(0, np.stack([d for d, _ in frames]), frames_u32=np.stack([f for _, f in frames]))

    def single():
        sc.memory_reset()
        sc.append_memory(frames[-1][0], frame_u32=frames[-1][1], motion=motion)     # a filled memory: every timed frame fuses into one
        t = 0.0
        for d, f in frames:
            sc.append_memory(d, frame_u32=f, motion=motion)
            t += sc.memory_time(reps) / n
        return t

    def batch(streams):
        sb.memory_reset()
        for _ in range(2):                                                           # the replayed call fuses into filled memories
            sb.append_memory(n, motions=[motion] * n, streams=streams)
        return sb.memory_time(reps) / n

    cols = ([], [], [])
    single(); batch(list(range(n)) if n <= capi.SCENE_STREAMS_MAX else None); batch(None)   # warm-up: buffers, code objects
    for _ in range(sets):
        cols[0].append(single()); cols[1].append(batch(list(range(n)))); cols[2].append(batch(None))
    sb.close()
    return cols


if memory:
    motion = ya.scene_motion(3.0, -2.0, 0.05)           # tools/time_scene.py's: a small turn and a step
    print("memory append, ms per frame (median of the sets):")
    print(f"{'n':>4} {'single handle':>14} {'a stream per frame':>19} {'all on stream 0':>16}")
    for n in sizes:
        s, a, o = memory_columns([frame(b) for b in range(n)], motion)
        print(f"{n:4d} {med(s):14.4f} {med(a):19.4f} {med(o):16.4f}")
    s, a, o = memory_columns([frame(0)] * 8, motion)   # (slot 0's depth seed is that tool's)
    spread = lambda v: (max(v) - min(v)) / med(v)
    print(f"n = 8, the robots + balls frame of tools/time_scene.py in every slot, {sets} sets alternated:")
    print(f"  single handle          {med(s):.4f} ms per frame, spread (max - min) / median {100 * spread(s):.1f} %")
    print(f"  a stream per frame     {med(a):.4f} ms per frame, spread {100 * spread(a):.1f} %, ratio to the single handle {med(a) / med(s):.3f}")
    print(f"  all on stream 0        {med(o):.4f} ms per frame, spread {100 * spread(o):.1f} %, ratio to the single handle {med(o) / med(s):.3f}")
    sc.close()
    sys.exit(0)


def search_columns(frames, prior, cands, radius, runs, replays, pyr=None, norm=False):
    """(single, a stream per frame, all on stream 0): lists over the runs of (ms per frame, ms of the registration alone per frame)
    for these frames, alternated run by run, one warm-up each; every memory filled before it is timed. pyr = (levels, refine): the
    pyramid append instead of the search append; norm: the normalised form of either, at min_inside"""
    n = len(frames)
    motion = ya.scene_motion(*prior)
    sb = ya.SceneBatch(W, H, n)
    sb.stage_frames(0, np.stack([d for d, _ in frames]), frames_u32=np.stack([f for _, f in frames]))
    same = all(f is frames[0] for f in frames)

    def single():
        sc.memory_reset()
        sc.append_memory(frames[-1][0], frame_u32=frames[-1][1], motion=motion)
        t, r = 0.0, 0.0
        for d, f in (frames[:1] if same else frames):      # (the same frame in every slot: one replay stands for all)
            if pyr and norm:
                sc.append_memory_pyramid_norm(d, frame_u32=f, candidates=cands, levels=pyr[0], radius=radius, refine=pyr[1], min_inside=min_inside)
                a, b = sc.memory_pyramid_norm_time(replays)
            elif norm:
                sc.append_memory_search_norm(d, frame_u32=f, candidates=cands, radius=radius, min_inside=min_inside)
                a, b = sc.memory_search_norm_time(replays)
            elif pyr:
                sc.append_memory_pyramid(d, frame_u32=f, candidates=cands, levels=pyr[0], radius=radius, refine=pyr[1])
                a, b = sc.memory_pyramid_time(replays)
            else:
                sc.append_memory_search(d, frame_u32=f, candidates=cands, radius=radius)
                a, b = sc.memory_search_time(replays)
            t += a / (1 if same else n); r += b / (1 if same else n)
        return t, r

    def batch(streams):
        sb.memory_reset()
        sb.append_memory(n, motions=[motion] * n, streams=streams)
        if pyr and norm:
            sb.append_memory_pyramid_norm(n, candidates=[cands] * n, streams=streams, levels=pyr[0], radius=radius, refine=pyr[1], min_inside=min_inside)
            a, b = sb.memory_pyramid_norm_time(replays)
        elif norm:
            sb.append_memory_search_norm(n, candidates=[cands] * n, streams=streams, radius=radius, min_inside=min_inside)
            a, b = sb.memory_search_norm_time(replays)
        elif pyr:
            sb.append_memory_pyramid(n, candidates=[cands] * n, streams=streams, levels=pyr[0], radius=radius, refine=pyr[1])
            a, b = sb.memory_pyramid_time(replays)
        else:
            sb.append_memory_search(n, candidates=[cands] * n, streams=streams, radius=radius)
            a, b = sb.memory_search_time(replays)
        return a / n, b / n

    per_frame = list(range(n)) if n <= capi.SCENE_STREAMS_MAX else None
    cols = ([], [], [])
    single(); batch(per_frame); batch(None)
    for _ in range(runs):
        cols[0].append(single()); cols[1].append(batch(per_frame)); cols[2].append(batch(None))
    sb.close()
    return cols


if search:
    prior = (3.0, -2.0, 0.05)                             # tools/time_scene.py's: the prior is right, the search confirms it
    grids = ((n_rot_arg, radius_arg),) if n_rot_arg is not None else ((1, 0), (1, 4), (5, 4), (9, 8))
    print(("normalised " if norm else "") + "search append, ms per frame (median of the sets), the registration launches alone in brackets:")
    print(f"{'n':>4} {'n_rot':>5} {'R':>2} {'single handle':>18} {'a stream per frame':>20} {'all on one stream':>20}")
    for n in sizes:
        for n_rot, radius in grids:
            cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=(n_rot - 1) // 2)
            cols = search_columns([frame(b) for b in range(n)], prior, cands, radius, sets, reps, norm=norm)
            cell = lambda c: f"{med([v[0] for v in c]):.4f} ({med([v[1] for v in c]):.4f})"
            print(f"{n:4d} {n_rot:5d} {radius:2d} {cell(cols[0]):>18} {cell(cols[1]):>20} {cell(cols[2]):>20}" + ("   (n > 64 streams: both columns on one stream)" if n > capi.SCENE_STREAMS_MAX else ""))
    cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=2)
    s, a, o = search_columns([frame(0)] * 8, prior, cands, 4, 5, 30, norm=norm)
    ms = lambda c: [v[0] for v in c]
    spread = lambda v: (max(v) - min(v)) / med(v)
    print("n = 8, (n_rot, R) = (5, 4), the robots + balls frame of tools/time_scene.py in every slot, 5 runs of 30 replays alternated:")
    print(f"  single handle          {med(ms(s)):.4f} ms per frame, spread (max - min) / median {100 * spread(ms(s)):.2f} %")
    print(f"  a stream per frame     {med(ms(a)):.4f} ms per frame, spread {100 * spread(ms(a)):.2f} %, ratio to the single handle {med(ms(a)) / med(ms(s)):.3f}")
    print(f"  all on one stream      {med(ms(o)):.4f} ms per frame, spread {100 * spread(ms(o)):.2f} %, ratio to the single handle {med(ms(o)) / med(ms(s)):.3f}")
    sc.close()
    sys.exit(0)
if pyramid:
    prior = (3.0, -2.0, 0.05)                             # tools/time_scene.py's: the prior is right, the search confirms it
    n_rot, levels, radius, refine = (n_rot_arg, levels_arg, radius_arg, refine_arg) if n_rot_arg is not None else (5, 3, 8, 1)
    cell = lambda c: f"{med([v[0] for v in c]):.4f} ({med([v[1] for v in c]):.4f})"
    print(("normalised " if norm else "") + "pyramid append, ms per frame (median of the sets), the registration launches alone in brackets:")
    print(f"{'n':>4} {'n_rot':>5} {'L':>2} {'R':>2} {'r':>2} {'single handle':>18} {'a stream per frame':>20} {'all on one stream':>20}")
    cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=(n_rot - 1) // 2)
    for n in sizes:
        cols = search_columns([frame(b) for b in range(n)], prior, cands, radius, sets, reps, (levels, refine), norm)
        print(f"{n:4d} {n_rot:5d} {levels:2d} {radius:2d} {refine:2d} {cell(cols[0]):>18} {cell(cols[1]):>20} {cell(cols[2]):>20}")
    cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=2)
    s, a, o = search_columns([frame(0)] * 8, prior, cands, 8, 5, 30, (3, 1), norm)
    ms = lambda c: [v[0] for v in c]
    spread = lambda v: (max(v) - min(v)) / med(v)
    print("n = 8, (n_rot, L, R, r) = (5, 3, 8, 1), the robots + balls frame of tools/time_scene.py in every slot, 5 runs of 30 replays alternated:")
    print(f"  single handle          {med(ms(s)):.4f} ms per frame ({cell(s)}), spread (max - min) / median {100 * spread(ms(s)):.2f} %")
    print(f"  a stream per frame     {med(ms(a)):.4f} ms per frame ({cell(a)}), spread {100 * spread(ms(a)):.2f} %, ratio to the single handle {med(ms(a)) / med(ms(s)):.3f}")
    print(f"  all on one stream      {med(ms(o)):.4f} ms per frame ({cell(o)}), spread {100 * spread(ms(o)):.2f} %, ratio to the single handle {med(ms(o)) / med(ms(s)):.3f}")
    sc.close()
    sys.exit(0)
for n in sizes:
    frames = [frame(b) for b in range(n)]
    sb = ya.SceneBatch(W, H, n)
    kind = "tour" if plain else "turn tour" if tour else "turn plan"
    batch_turn = (lambda: sb.plan_turn_tour(targets=[TARGETS] * n, turn_price=tau)) if tour else (lambda: sb.plan_turn(turn_price=tau))
    single_turn = (lambda: sc.plan_turn_tour(targets=TARGETS, turn_price=tau)) if tour else (lambda: sc.plan_turn(turn_price=tau))
    if plain:
        batch_turn, single_turn = (lambda: sb.plan_tour(targets=[TARGETS] * n, connectivity=conn_tour)), (lambda: sc.plan_tour(targets=TARGETS, connectivity=conn_tour))

    def batch_set():
        t0 = time.perf_counter()
        for b in range(n):
            sb.stage(b, *frames[b])
        sb.append(n, ya.COMPAT_SANE)
        batch_turn() if own else sb.plan(connectivity=4)
        out = dict(wall=(time.perf_counter() - t0) * 1e3)
        out["append"] = sb.time(reps) / n
        if own:
            batch_turn()
            out["turn"] = sb.tour_time(reps) if plain else sb.turn_tour_time(reps) if tour else sb.turn_time(reps)
            return out
        for conn in (4, 8):
            sb.plan(connectivity=conn)
            out[conn] = sb.plan_time(reps)
        return out

    def single_set():
        t0 = time.perf_counter()
        for d, f in frames:
            sc.append_classified(d, frame_u32=f, mode=ya.COMPAT_SANE)
            single_turn() if own else sc.plan(connectivity=4)
        out = dict(wall=(time.perf_counter() - t0) * 1e3, append=0.0)
        out[4] = dict(ms=0.0, rounds=0, tile_runs=0); out[8] = dict(ms=0.0, rounds=0, tile_runs=0); out["turn"] = dict(ms=0.0, rounds=0, tile_runs=0)
        for d, f in frames:
            sc.append_classified(d, frame_u32=f, mode=ya.COMPAT_SANE)
            out["append"] += sc.time(reps) / n
            if own:
                single_turn()
                s = sc.tour_time(reps) if plain else sc.turn_tour_time(reps) if tour else sc.turn_time(reps)
                out["turn"]["ms"] += s["ms_per_tour" if tour or plain else "ms_per_plan"] / n
                out["turn"]["rounds"] = max(out["turn"]["rounds"], s["rounds"]); out["turn"]["tile_runs"] += s["tile_runs"]
                continue
            for conn in (4, 8):
                sc.plan(connectivity=conn)
                s = sc.plan_time(reps)
                out[conn]["ms"] += s["ms_per_plan"] / n
                out[conn]["rounds"] = max(out[conn]["rounds"], s["rounds"]); out[conn]["tile_runs"] += s["tile_runs"]
        return out

    batch_set(); single_set()                                     # warm-up: buffers, code objects
    B, S = [], []
    for _ in range(sets):
        B.append(batch_set()); S.append(single_set())
    print(f"n = {n}")
    print(f"  append, ms per frame:            batch {med([b['append'] for b in B]):.4f}   single {med([s['append'] for s in S]):.4f}")
    if own:
        print(f"  {kind}, {f'{conn_tour}-connected' if plain else f'price {tau}'}, ms per frame:  batch {med([b['turn']['ms_per_batch'] for b in B]) / n:.4f} ({B[0]['turn']['rounds']} rounds, {B[0]['turn']['tile_runs']} tile runs)"
              f"   single {med([s['turn']['ms'] for s in S]):.4f} (at most {S[0]['turn']['rounds']} rounds, {S[0]['turn']['tile_runs']} tile runs in all)")
    for conn in (() if own else (4, 8)):
        print(f"  plan {conn}-connected, ms per frame:  batch {med([b[conn]['ms_per_batch'] for b in B]) / n:.4f} ({B[0][conn]['rounds']} rounds, {B[0][conn]['tile_runs']} tile runs)"
              f"   single {med([s[conn]['ms'] for s in S]):.4f} (at most {S[0][conn]['rounds']} rounds, {S[0][conn]['tile_runs']} tile runs in all)")
    wb, ws = med([b["wall"] for b in B]), med([s["wall"] for s in S])
    print(f"  host wall, stage + append + {kind if own else 'plan (4-connected)'} of the n frames: batch {wb:.3f} ms   single {ws:.3f} ms   ratio {wb / ws:.3f}")
    sb.close()
