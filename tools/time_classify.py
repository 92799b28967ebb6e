"""Wall-clock latency of the reference's own entry point: Yolact::classify on one 640x480 packed-u32
frame (src/yolact.rs:39; two 224x224 tiles), host buffer in, host buffer out, per call.
Usage: python tools/time_classify.py [--lib <other libyolact_hip.so>] [--batch]
--lib times another build of the library (e.g. one of the parent commit, `make -C tiny-object-detection_amd BUILD=build_old
LIBDIR=lib_old` in a checkout of it), to alternate with this one process by process on one box.
--batch times the classify batch instead (yh_classify_batch_u32, DESIGN.md §11 "Classify batch"): at 640x480, S = 224, SANE, for
n = 1, 2, 4, 8, 16, 32 frames per call, milliseconds PER FRAME of classify_batch host in / host out, of classify_batch from a device
pointer with nothing read back, and of n classify_frame calls (the baseline). A set is the mean of 20 back-to-back calls; the three
alternate set by set; median (min - max) of 5 sets after warm-up."""
import ctypes, os, socket, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-object-detection_amd"))
from yolact_amd import capi
argv = sys.argv[1:]
batch = "--batch" in argv
if "--lib" in argv:
    lib = os.path.abspath(argv[argv.index("--lib") + 1])
    capi.lib_path = lambda: lib
    have = ctypes.CDLL(lib)
    capi.SYMBOLS = [s for s in capi.SYMBOLS if hasattr(have, s[0])]   # (an older build lacks the newer entry points)
import yolact_amd as ya

rng = np.random.default_rng(0)
frame0 = (rng.integers(0, 256, (480, 640, 3), dtype=np.uint32) * np.array([1 << 24, 1 << 16, 1 << 8], np.uint32)).sum(-1).astype(np.uint32).reshape(-1)


def single_frame():
    for mode, name in ((ya.COMPAT_SANE, "sane"), (ya.COMPAT_STRICT, "strict")):
        y = ya.Yolact.init(seed=1, compat_mode=mode)
        t = []
        for i in range(220):
            f = frame0.copy()
            t0 = time.perf_counter()
            try:
                y.classify(f)
            except ya.YhError as e:     # strict mode reports YH_EDIVERGE where the reference would hang
                print(name, "classify raised", e); break
            t.append(time.perf_counter() - t0)
        if t:
            t = np.array(t[20:]) * 1e3
            print(f"classify 640x480 ({name}): median {np.median(t):.3f} ms, p99 {np.percentile(t, 99):.3f} ms, {1e3 / np.median(t):.0f} frames/s")


def batched(sets=5, reps=20):
    W, H = 640, 480
    print(f"box {socket.gethostname()}, {ya.version()}, {os.path.relpath(capi.lib_path(), ROOT)}, {sets} sets x {reps} calls, ms per frame: median (min-max)", flush=True)
    hip = None
    for n in (1, 2, 4, 8, 16, 32):
        eng = ya.Engine(input_size=224, max_batch=2 * n, use_graph=True)
        eng.load_weights(eng.generate_weights(seed=1))
        frames = np.stack([np.roll(frame0, 977 * b) for b in range(n)]).reshape(n, H, W)
        out = np.empty_like(frames)
        one = frame0.copy()

        def timed(fn):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            return (time.perf_counter() - t0) / reps / n * 1e3

        def host():
            eng.classify_batch(frames_u32=frames, width=W, height=H, mode=ya.COMPAT_SANE, out=out)

        def singles():
            for b in range(n):
                one[:] = frames[b].reshape(-1)
                eng.classify_frame(one, W, H, ya.COMPAT_SANE)

        host(); singles()                                             # warm-up: buffers, code objects, the two graphs
        # the device source: a copy of the frames in device memory of the library's own runtime
        if hip is None:
            hip = ctypes.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln))
        src = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(frames.nbytes)) == 0
        assert hip.hipMemcpy(src, frames.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(frames.nbytes), 1) == 0   # hipMemcpyHostToDevice

        def device():
            eng.classify_batch(frames_dev_ptr=src.value, n=n, width=W, height=H, mode=ya.COMPAT_SANE, out=False)

        device()
        T = dict(h=[], d=[], s=[])
        for _ in range(sets):
            T["h"].append(timed(host)); T["d"].append(timed(device)); T["s"].append(timed(singles))
        row = lambda v: f"{sorted(v)[len(v) // 2]:.4f} ({min(v):.4f}-{max(v):.4f})"
        med = lambda v: sorted(v)[len(v) // 2]
        print(f"n = {n:<2}  batch host in/out {row(T['h'])}   batch device in, no read-back {row(T['d'])}   "
              f"n x classify_frame {row(T['s'])}   ratio batch / singles {med(T['h']) / med(T['s']):.3f}", flush=True)
        hip.hipFree(src)
        eng.close()


if batch:
    batched()
else:
    single_frame()
