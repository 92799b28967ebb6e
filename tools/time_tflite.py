"""The reference's own model family on the GPU: a full-size synthetic MobileNetV2-FPN-YOLACT .tflite
(tests/tfl_models.mobilenetv2_yolact: the op census of data/FRC_model_edgetpu.log; the real
FRC_model.tflite is absent) through the uint8 executor: per-invoke latency (host input copy + graph
launch + sync) and classify() on a 640x480 frame. Parity of this model against the numpy oracle is
tests/test_gpu_tflite.py::test_full_size_mobilenetv2_yolact_graph (tools/ never load oracle/)."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("tiny-object-detection_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import yolact_amd as ya
import tfl_builder as B, tfl_models as M

ap = argparse.ArgumentParser()
ap.add_argument("--graph", type=int, default=-1, help="yh_tuning.tfl_graph: 1 = hipGraph replay of the plan, 0 = eager launches, -1 = library default")
ap.add_argument("--invokes", type=int, default=220)
ap.add_argument("--batch", action="store_true", help="the classify batch (yh_tfl_classify_batch_u32): ms per 640x480 frame for n = 1 .. 32 frames, three paths alternated in one process (profiles/tfl_classify_batch_timings.txt)")
ap.add_argument("--int8", action="store_true", help="the int8 / per-channel twin of the stand-in (tests/tfl_models_q.py) beside the uint8 stand-in, interleaved in one process: the invoke at 1, 2 and 16 images, or with --batch the classify batch at n = 4, 8, 32 (profiles/tfl_int8_timings.txt)")
ap.add_argument("--detect", action="store_true", help="the detection tail on the model's own heads (yh_tfl_evaluate): ms per image of invoke alone and of evaluate at 2, 16 and 64 images, uint8 heads beside float32 heads (DEQUANTIZE behind the four), interleaved in one process, and the tail's four launches timed by events (profiles/tfl_detect_timings.txt)")
ap.add_argument("--instance", action="store_true", help="the instance frames painted from the model's detections (yh_tfl_instance_frames): after a classify batch of n 640x480 frames and detect, ms per camera frame at n = 1, 4, 8, 32, left on the device and copied to the host, beside the engine's instance_batch at the same n (profiles/tfl_instance_timings.txt)")
a = ap.parse_args()
rng = np.random.default_rng(0)
model = M.mobilenetv2_yolact(rng)
buf = bytes(B.serialize(model))


def clock(fn):
    t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3


def batch_arm():
    """ms per frame of n frames, 640x480: classify_batch host in / host out; classify_batch from a device pointer with read=False;
    n single classify_frame calls. One handle (max_images = 64); per n the three paths alternate `rounds` times, medians reported."""
    import ctypes as C
    W, H, rounds = 640, 480, 15
    eng = ya.TfliteEngine(buf, max_images=64)
    hip = C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln))
    frames = rng.integers(0, 2 ** 32, (32, H, W), dtype=np.uint64).astype(np.uint32)
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(frames.nbytes)) == 0
    assert hip.hipMemcpy(dev, frames.ctypes.data_as(C.c_void_p), C.c_size_t(frames.nbytes), 1) == 0
    out, one = np.empty_like(frames), np.empty(W * H, np.uint32)
    print(f"tflite classify batch, {len(model.ops)}-op stand-in (S = 224), frames {W}x{H}, COMPAT_SANE; ms per frame, median of {rounds} alternated rounds (min .. max)")
    print(f"{'n':>3} {'batch host->host':>26} {'batch device->device':>26} {'n x classify_frame':>26} {'host/single':>12}")
    for n in (1, 2, 4, 8, 16, 32):
        def host(): eng.classify_batch(frames_u32=frames[:n], n=n, width=W, height=H, mode=ya.COMPAT_SANE, out=out[:n])
        def device(): eng.classify_batch(frames_dev_ptr=dev.value, n=n, width=W, height=H, mode=ya.COMPAT_SANE, read=False)
        def single():   # (the single call works in place: its buffer is refilled outside the clock, only the n calls are timed)
            total = 0.0
            for b in range(n):
                one[:] = frames[b].reshape(-1)
                total += clock(lambda: eng.classify_frame(one, W, H, ya.COMPAT_SANE))
            return total
        for _ in range(3):
            host(); device(); single()
        assert np.array_equal(out[n - 1].reshape(-1), one)      # (frame n - 1 of the batch is the single call's)
        t = np.array([[clock(host), clock(device), single()] for _ in range(rounds)]) / n
        med, lo, hi = np.median(t, 0), t.min(0), t.max(0)
        cols = [f"{med[k]:8.3f} ({lo[k]:6.3f} .. {hi[k]:6.3f})" for k in range(3)]
        print(f"{n:3d} {cols[0]:>26} {cols[1]:>26} {cols[2]:>26} {med[0] / med[2]:12.3f}")
    hip.hipFree(dev)
    eng.close()


def int8_arm():
    """The uint8 stand-in and its int8 twin on two handles, alternated round by round: ms per invoke (set_input + invoke + read
    output 4) at 1, 2 and 16 images, or per 640x480 frame of the classify batch (host in, host out). The uint8 rows are the yardstick."""
    import tfl_builder_q as BQ, tfl_models_q as MQ
    twin = MQ.mobilenetv2_yolact_q(np.random.default_rng(0))
    rounds = 15
    engs = {"uint8": ya.TfliteEngine(buf, max_images=64), "int8": ya.TfliteEngine(BQ.serialize(twin), max_images=64)}
    plain = ya.TfliteEngine(BQ.serialize(twin), tune=dict(tfl_fuse=0, tfl_group=0))
    x = rng.integers(0, 256, (16, 224, 224, 3), dtype=np.uint8)
    for e in (engs["int8"], plain):
        e.set_batch(2); e.set_input(x[:2]); e.invoke()
    assert all(np.array_equal(engs["int8"].output(k), plain.output(k)) for k in range(plain.output_count()))   # (fused and grouped = one launch per operator)
    plain.close()
    print("plans:", {k: e.plan_summary() for k, e in engs.items()})
    def row(label, fns):
        for _ in range(3):
            for f in fns.values(): f()
        t = np.array([[clock(f) for f in fns.values()] for _ in range(rounds)])
        med, lo, hi = np.median(t, 0), t.min(0), t.max(0)
        print(f"{label:>12} " + " ".join(f"{k:>6} {med[i]:8.3f} ({lo[i]:6.3f} .. {hi[i]:6.3f})" for i, k in enumerate(fns)) + f"   int8/uint8 {med[1] / med[0]:.3f}")
    if a.batch:
        W, H = 640, 480
        frames = rng.integers(0, 2 ** 32, (32, H, W), dtype=np.uint64).astype(np.uint32)
        out = np.empty_like(frames)
        print(f"classify batch, frames {W}x{H}, COMPAT_SANE, host in / host out; ms per BATCH, median of {rounds} alternated rounds (min .. max)")
        for n in (4, 8, 32):
            row(f"n = {n}", {k: (lambda e=e, n=n: e.classify_batch(frames_u32=frames[:n], n=n, width=W, height=H, mode=ya.COMPAT_SANE, out=out[:n])) for k, e in engs.items()})
    else:
        print(f"invoke 224x224 (set_input + invoke + read output 4); ms per invoke, median of {rounds} alternated rounds (min .. max)")
        for nb in (1, 2, 16):
            def one(e, nb=nb):
                e.set_batch(nb); e.set_input(x[:nb]); e.invoke(); return e.output(4)
            row(f"{nb} images", {k: (lambda e=e: one(e)) for k, e in engs.items()})
    for e in engs.values(): e.close()


def detect_arm():
    """Two handles on the stand-in - its uint8 heads, and the same heads behind DEQUANTIZE (float32: the mask kernel's float form) -
    alternated round by round: invoke alone (set_input + invoke + read output 4) and evaluate (set_input + evaluate + read image 0's
    detections, the one wait) per image count; then the tail's four launches on those outputs, timed by events."""
    import tfl_detect_cases as K
    rounds, S = 15, 224
    fmodel = K.dequantized_heads(M.mobilenetv2_yolact(np.random.default_rng(0)))
    engs = {"uint8": ya.TfliteEngine(buf, max_images=64), "float32": ya.TfliteEngine(bytes(B.serialize(fmodel)), max_images=64)}
    levels = [28, 14, 7, 3, 1]   # (S / 8, / 16, / 32, then two PAD + VALID stride-2 levels)
    pri = ya.tfl_priors(levels, S)
    for e in engs.values(): e.detect_setup(pri)
    x = rng.integers(0, 256, (64, S, S, 3), dtype=np.uint8)
    print(f"tflite detections, {len(model.ops)}-op stand-in (S = {S}, P = {len(pri)}, C = 81, proto {engs['uint8'].proto_dims()}), top_k 200, max_dets 100, conf_thresh 0.05; "
          f"the reference's own model file is absent: random weights, so the detections are those of noise")
    print(f"ms per IMAGE, median of {rounds} alternated rounds (min .. max); invoke = set_input + invoke + read output 4; evaluate = set_input + evaluate + read image 0's detections")
    for nb in (2, 16, 64):
        def inv(e):
            e.set_batch(nb); e.set_input(x[:nb]); e.invoke(); return e.output(4)
        def ev(e):
            e.set_batch(nb); e.set_input(x[:nb]); e.evaluate(); return e.detections(0, want_masks=False)
        fns = {f"{k} {w}": (lambda e=e, f=f: f(e)) for k, e in engs.items() for w, f in (("invoke", inv), ("evaluate", ev))}
        for _ in range(3):
            for f in fns.values(): f()
        t = np.array([[clock(f) for f in fns.values()] for _ in range(rounds)]) / nb
        med, lo, hi = np.median(t, 0), t.min(0), t.max(0)
        for i, k in enumerate(fns):
            print(f"{nb:3d} images  {k:>17}  {med[i]:8.4f} ({lo[i]:7.4f} .. {hi[i]:7.4f})")
        nd = {k: [len(e.detections(b, want_masks=False)[0]) for b in range(nb)] for k, e in engs.items()}
        # the tail alone, by events on the handle's stream (mean of 20 runs per launch): three rounds, the two handles alternated
        st = {k: [] for k in engs}
        for _ in range(3):
            for k, e in engs.items(): st[k].append(e.detect_stage_times(20))
        st = {k: np.array(v) for k, v in st.items()}
        for k in engs:
            m = np.median(st[k], 0)
            share = m.sum() / nb / med[list(fns).index(f"{k} evaluate")]
            print(f"{nb:3d} images  {k:>8} tail by events, ms per launch (whole batch): softmax+cand {m[0]:.4f}  class nms {m[1]:.4f}  top dets {m[2]:.4f}  masks {m[3]:.4f}"
                  f"  sum {m.sum():.4f} = {m.sum() / nb:.4f} per image = {100 * share:.1f} % of evaluate; detections per image {min(nd[k])} .. {max(nd[k])}")
        mq, mf = np.median(st["uint8"], 0)[3], np.median(st["float32"], 0)[3]
        print(f"{nb:3d} images  mask kernel: integer form (uint8 heads) {mq:.4f} ms, float form (float32 heads) {mf:.4f} ms, integer / float {mq / mf:.3f}")
    for e in engs.values(): e.close()


def instance_arm():
    """One handle on the stand-in (max_images = 64) with a detect setup: per n a classify batch of n frames and the tail on its 2n
    tiles, then instance_frames(0, n) on those detections - the frames left on the device, and copied to a host array that exists
    already - alternated round by round. For context the engine's instance_batch(0, n, read=False) on YOLACT-550's detections of n
    noise frames, in the same rounds: another network's detections, the same painter per image."""
    import ctypes as C
    W, H, rounds, S = 640, 480, 15, 224
    eng = ya.TfliteEngine(buf, max_images=64)
    eng.detect_setup(ya.tfl_priors([28, 14, 7, 3, 1], S))
    yeng = ya.Engine(input_size=550, backbone=50, max_batch=32, use_graph=False)
    yeng.load_weights(yeng.generate_weights(seed=1))
    yeng.set_input(np.random.default_rng(5).integers(0, 256, (32, 550, 550, 3), dtype=np.uint8))
    yeng.evaluate()
    ynd = [len(yeng.detections(b, want_masks=False)[0]) for b in range(32)]
    frames = rng.integers(0, 2 ** 32, (32, H, W), dtype=np.uint64).astype(np.uint32)
    out = np.empty_like(frames)
    cm = (1 + np.arange(80) % 3).astype(np.uint8)   # every foreground class painted
    cmp, outp = cm.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    print(f"tflite instance frames, {len(model.ops)}-op stand-in (S = {S}, proto {eng.proto_dims()}, max_dets 100), frames {W}x{H}, every class painted, min_score 0; "
          f"random weights, so the detections are those of noise")
    print(f"ms per camera FRAME, median of {rounds} alternated rounds (min .. max), 3 warm-ups; engine = yh_instance_batch on YOLACT-550's detections ({min(ynd)} .. {max(ynd)} per frame), frames left on the device")
    print(f"{'n':>3} {'dets per tile':>14} {'instance_frames, device':>28} {'instance_frames, host copy':>28} {'engine instance_batch':>28}")
    for n in (1, 4, 8, 32):
        eng.classify_batch(frames_u32=frames[:n], n=n, width=W, height=H, mode=ya.COMPAT_SANE, read=False)
        eng.detect()
        nd = [len(eng.detections(i, want_masks=False)[0]) for i in range(2 * n)]
        def device(): eng._chk(eng.L.yh_tfl_instance_frames(eng.h, 0, n, W, H, cmp, C.c_float(0.0), None))
        def host(): eng._chk(eng.L.yh_tfl_instance_frames(eng.h, 0, n, W, H, cmp, C.c_float(0.0), outp))
        def engine(): yeng.instance_batch(0, n, W, H, class_map=cm, read=False)
        for _ in range(3):
            device(); host(); engine()
        assert out[:n].any() and sum(len(eng.instances_of(b)) for b in range(n)) > 0
        t = np.array([[clock(device), clock(host), clock(engine)] for _ in range(rounds)]) / n
        med, lo, hi = np.median(t, 0), t.min(0), t.max(0)
        cols = [f"{med[k]:8.4f} ({lo[k]:7.4f} .. {hi[k]:7.4f})" for k in range(3)]
        print(f"{n:3d} {f'{min(nd)} .. {max(nd)}':>14} {cols[0]:>28} {cols[1]:>28} {cols[2]:>28}")
    yeng.close(); eng.close()


if a.instance:
    instance_arm()
    sys.exit(0)
if a.detect:
    detect_arm()
    sys.exit(0)
if a.int8:
    int8_arm()
    sys.exit(0)
if a.batch:
    batch_arm()
    sys.exit(0)
eng = ya.TfliteEngine(buf, tune=dict(tfl_graph=a.graph))
x = rng.integers(0, 256, (1, 224, 224, 3), dtype=np.uint8)
def invoke():
    eng.set_input(x); eng.invoke(); return eng.output(4)
got = invoke()
print(f"{len(model.ops)} ops, {len(buf) / 1e6:.1f} MB model; output 4: {got.shape}, {len(np.unique(got))} distinct codes")
t = []
for _ in range(a.invokes):
    t0 = time.perf_counter(); invoke(); t.append(time.perf_counter() - t0)
t = np.array(t[20:]) * 1e3
print(f"tfl_graph={a.graph}; invoke 224x224 (set_input + invoke + read output 4): median {np.median(t):.3f} ms, p99 {np.percentile(t, 99):.3f} ms")
frame = (rng.integers(0, 256, (480, 640, 3), dtype=np.uint32) * np.array([1 << 24, 1 << 16, 1 << 8], np.uint32)).sum(-1).astype(np.uint32).reshape(-1)
t = []
for _ in range(120):
    f = frame.copy(); t0 = time.perf_counter(); eng.classify_frame(f, 640, 480, ya.COMPAT_SANE); t.append(time.perf_counter() - t0)
t = np.array(t[20:]) * 1e3
print(f"classify 640x480 through the .tflite (two tiles): median {np.median(t):.3f} ms, p99 {np.percentile(t, 99):.3f} ms")
