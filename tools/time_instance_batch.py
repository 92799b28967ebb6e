"""The instance batch (yh_instance_batch + yh_scene_batch_stage_frames, DESIGN.md §11 "Instance batch") against the single calls at
640x480, on the engine's own detections of noise frames (YOLACT-550 R50, seeded weights, a different frame per slot, every
foreground class mapped to an output class: class k -> 1 + k % 3), for n = 1, 2, 8, 16, 64 frames of one yh_evaluate. Per n:
milliseconds PER FRAME of the host's wall clock round instance_batch(read=False) + stage_frames from the device pointer, beside
n x (instance_frame(read=False) + stage from the device pointer), and the instance calls alone. A set is the mean of `reps`
back-to-back repetitions; batch and singles alternate set by set; median (min - max) over the sets. The oracle is not loaded.
Usage: python tools/time_instance_batch.py [sets = 5] [reps = 20] [--lib <other libyolact_hip.so>] [--track]
--lib times another build of the library (a build of the parent commit: `make -C tiny-object-detection_amd BUILD=build_old
LIBDIR=lib_old` in a checkout of it), to alternate with this one process by process on one box; a build without
yh_instance_batch times the single path only.
--track times the tracked batch instead (yh_instance_track_batch, DESIGN.md §11 "Instance track batch"): per n, milliseconds PER
FRAME of n instance_track(read=False) calls beside one instance_track_batch(read=False) of the same frames, once with all frames on
one stream (n rounds: the chain's worst case) and once with a stream per frame (one round). The frames stay on the device; batch
and singles alternate set by set; every set starts from trackers that hold the frames' own tracks (the warm-up made them)."""
import ctypes, os, socket, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-object-detection_amd"))
from yolact_amd import capi
args, lib, track = [], None, False
it = iter(sys.argv[1:])
for a in it:
    if a == "--lib": lib = os.path.abspath(next(it))
    elif a == "--track": track = True
    else: args.append(a)
sets = int(args[0]) if len(args) > 0 else 5
reps = int(args[1]) if len(args) > 1 else 20
if lib:
    capi.lib_path = lambda: lib
has_batch = hasattr(ctypes.CDLL(capi.lib_path()), "yh_instance_batch")
if not has_batch:
    capi.SYMBOLS = [s for s in capi.SYMBOLS if s[0] not in ("yh_instance_batch", "yh_instance_batch_device_frames", "yh_instance_batch_read",
                                                            "yh_scene_batch_stage_frames", "yh_op_instance_batch")]
import yolact_amd as ya
S, W, H = 550, 640, 480
print(f"box {socket.gethostname()}, {ya.version()}, {os.path.relpath(capi.lib_path(), ROOT)}, {sets} sets x {reps} reps", flush=True)
cm = (1 + np.arange(80) % 3).astype(np.uint8)


def timed(fn):
    """mean ms of `reps` back-to-back calls"""
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def row(v, n):
    v = sorted(x / n for x in v)
    return f"{v[len(v) // 2]:.4f} ({v[0]:.4f}-{v[-1]:.4f})"


for n in (1, 2, 8, 16, 64):
    eng = ya.Engine(input_size=S, backbone=50, max_batch=n, use_graph=False)
    eng.load_weights(eng.generate_weights(seed=1))
    eng.set_input(np.random.default_rng(5).integers(0, 256, (n, S, S, 3), dtype=np.uint8))
    eng.evaluate()
    nd = [len(eng.detections(b, want_masks=False)[0]) for b in range(n)]
    if track:
        each = list(range(n))

        def single_track():
            for b in range(n):
                eng.instance_track(b, W, H, class_map=cm, read=False)

        def batch_one_stream():
            eng.instance_track_batch(0, n, W, H, class_map=cm, read=False)

        def batch_n_streams():
            eng.instance_track_batch(0, n, W, H, class_map=cm, streams=each, read=False)

        single_track(); batch_one_stream(); batch_n_streams()         # warm-up: buffers, code objects, every stream's tracker
        T = dict(s=[], b1=[], bn=[])
        for _ in range(sets):
            T["b1"].append(timed(batch_one_stream)); T["s"].append(timed(single_track)); T["bn"].append(timed(batch_n_streams))
        med = lambda v: sorted(v)[len(v) // 2]
        print(f"n = {n} ({min(nd)}-{max(nd)} detections per frame), ms per frame, median (min-max) of the sets", flush=True)
        print(f"  singles          n x instance_track        {row(T['s'], n)}", flush=True)
        print(f"  batch, 1 stream  instance_track_batch R={n:<3} {row(T['b1'], n)}   ratio batch / singles {med(T['b1']) / med(T['s']):.3f}", flush=True)
        print(f"  batch, n streams instance_track_batch R=1   {row(T['bn'], n)}   ratio batch / singles {med(T['bn']) / med(T['s']):.3f}", flush=True)
        eng.close()
        continue
    depths = np.random.default_rng(1).integers(200, 4000, (n, H, W)).astype(np.uint16)
    sb = ya.SceneBatch(W, H, n)

    def batch_paint():
        eng.instance_batch(0, n, W, H, class_map=cm, read=False)

    def batch_both():
        batch_paint()
        sb.stage_frames(0, depths, frames_dev_ptr=eng.instance_batch_device_frames())

    def single_paint():
        for b in range(n):
            eng.instance_frame(b, W, H, class_map=cm, read=False)

    def single_both():
        for b in range(n):
            eng.instance_frame(b, W, H, class_map=cm, read=False)
            sb.stage(b, depths[b], frame_dev_ptr=eng.instance_device_frame())

    single_both()                                                 # warm-up: buffers, code objects
    if has_batch:
        batch_both()
    T = dict(bp=[], bb=[], sp=[], sb=[])
    for _ in range(sets):
        if has_batch:
            T["bp"].append(timed(batch_paint)); T["bb"].append(timed(batch_both))
        T["sp"].append(timed(single_paint)); T["sb"].append(timed(single_both))
    print(f"n = {n} ({min(nd)}-{max(nd)} detections per frame), ms per frame, median (min-max) of the sets", flush=True)
    print(f"  single  instance_frame {row(T['sp'], n)}   instance_frame + stage {row(T['sb'], n)}", flush=True)
    if has_batch:
        med = lambda v: sorted(v)[len(v) // 2]
        print(f"  batch   instance_batch {row(T['bp'], n)}   instance_batch + stage_frames {row(T['bb'], n)}   "
              f"ratio batch / singles {med(T['bb']) / med(T['sb']):.3f}", flush=True)
    sb.close(); eng.close()
