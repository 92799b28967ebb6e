"""Wall-clock latency of yh_instance_frame at 640x480 on the engine's own detections (YOLACT-550 R50, seeded weights): a noise
frame (about 100 detections) and tests/golden/frc_balls.png. Every foreground class is mapped to an output class (class k ->
1 + k % 3), so every detection is eligible: the most work the call can have for the frame. Milliseconds per call as the median of
`sets` x `reps` calls (each set: the mean of `reps` back-to-back calls), with the host copy of the frame (out_host) and without
(read=False: the frame stays on the device for yh_scene_append_classified; the 1 KB instance table comes back either way).
--track: a batch of two frames (the image and the image shifted by 8 pixels: the same objects, moved) and, beside
yh_instance_frame alternating between the two, yh_instance_track alternating between them, so that every tracked call has the
other frame's tracks to match (min_iou 0.3, max_age 2); the line also says how many tracks were matched, lost and born by the
last call.
    python tools/time_instance.py [sets = 5] [reps = 20] [--track]"""
import os, socket, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-object-detection_amd"))
import yolact_amd as ya

S, W, H = 550, 640, 480


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed(sets, reps, call):
    """(median, min, max) over `sets` of the mean ms of `reps` back-to-back calls call(k), k = 0, 1, 2, ..."""
    runs = []
    for _ in range(sets):
        t0 = time.perf_counter()
        for k in range(reps):
            call(k)
        runs.append((time.perf_counter() - t0) / reps * 1e3)
    return median(runs), min(runs), max(runs)


def main_track(sets, reps):
    from PIL import Image
    eng = ya.Engine(input_size=S, backbone=50, max_batch=2, use_graph=True)
    eng.load_weights(eng.generate_weights(seed=1))
    balls = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "frc_balls.png")).convert("RGB").resize((S, S), Image.BILINEAR))
    noise = np.random.default_rng(5).integers(0, 256, (S, S, 3), dtype=np.uint8)
    cm = (1 + np.arange(80) % 3).astype(np.uint8)
    for name, img in (("noise", noise), ("frc_balls", balls)):
        eng.set_input(np.ascontiguousarray(np.stack([img, np.roll(img, 8, axis=1)])))
        eng.evaluate()
        eng.track_reset()
        for b in (0, 1, 0, 1):                                                    # warm-up: buffers, code objects, the tracker filled
            eng.instance_frame(b, W, H, class_map=cm)
            eng.instance_track(b, W, H, class_map=cm)
        row = {}
        for read in (True, False):
            row["frame", read] = timed(sets, reps, lambda k: eng.instance_frame(k & 1, W, H, class_map=cm, read=read))
            row["track", read] = timed(sets, reps, lambda k: eng.instance_track(k & 1, W, H, class_map=cm, read=read))
        tr = eng.tracks()
        nd = [len(eng.detections(b, want_masks=False)[0]) for b in (0, 1)]
        f = lambda r: f"{r[0]:.3f} ms ({r[1]:.3f}-{r[2]:.3f})"
        print(f"[{socket.gethostname()}] instance track {W}x{H}, {name}: {nd[0]} / {nd[1]} detections, {len(tr)} tracks after the last call "
              f"({int((tr[:, 5] >= 0).sum())} seen, {int((tr[:, 3] > 0).sum())} lost) | with the host copy: tracked {f(row['track', True])}, "
              f"untracked {f(row['frame', True])} | without: tracked {f(row['track', False])}, untracked {f(row['frame', False])}", flush=True)
    eng.close()


def main(sets, reps):
    from PIL import Image
    eng = ya.Engine(input_size=S, backbone=50, max_batch=1, use_graph=True)
    eng.load_weights(eng.generate_weights(seed=1))
    balls = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "frc_balls.png")).convert("RGB").resize((S, S), Image.BILINEAR))[None]
    noise = np.random.default_rng(5).integers(0, 256, (1, S, S, 3), dtype=np.uint8)
    cm = (1 + np.arange(80) % 3).astype(np.uint8)
    for name, img in (("noise", noise), ("frc_balls", balls)):
        eng.set_input(np.ascontiguousarray(img))
        eng.evaluate()
        frame = eng.instance_frame(0, W, H, class_map=cm)                         # warm-up: buffers, code objects
        table = eng.instances()
        row = {}
        for read in (True, False):
            runs = []
            for _ in range(sets):
                t0 = time.perf_counter()
                for _ in range(reps):
                    eng.instance_frame(0, W, H, class_map=cm, read=read)
                runs.append((time.perf_counter() - t0) / reps * 1e3)
            row[read] = (median(runs), min(runs), max(runs))
        print(f"[{socket.gethostname()}] instance frame {W}x{H}, {name}: {len(eng.detections(0, want_masks=False)[0])} detections, {len(table)} eligible, "
              f"{np.count_nonzero(frame)} pixels painted | with the host copy {row[True][0]:.3f} ms ({row[True][1]:.3f}-{row[True][2]:.3f}), "
              f"without {row[False][0]:.3f} ms ({row[False][1]:.3f}-{row[False][2]:.3f})", flush=True)
    eng.close()


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x != "--track"]
    (main_track if "--track" in sys.argv[1:] else main)(int(a[0]) if a else 5, int(a[1]) if len(a) > 1 else 20)
