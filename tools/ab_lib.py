"""A/B of two BUILDS of the kernel library on one box: graph-replayed step time, the two libraries alternated process by process.
    python tools/ab_lib.py <libA.so> <libB.so> [batch = 64] [rounds = 4]
    python tools/ab_lib.py --tfl <libA.so> <libB.so> [rounds = 6]    the TFLite executor instead: the full-size uint8 stand-in's invoke at 1, 2 and 16 images
(build the other one with `make -C tiny-object-detection_amd BUILD=build_old LIBDIR=lib_old` in a checkout of the older tree)"""
import os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def child(lib, batch):
    sys.path.insert(0, os.path.join(ROOT, "tiny-object-detection_amd"))
    import yolact_amd as ya
    from yolact_amd import capi
    capi.lib_path = lambda: lib
    eng = ya.Engine(input_size=550, max_batch=batch, use_graph=True)
    eng.load_weights(eng.generate_weights(1))
    eng.set_input(np.random.default_rng(0).integers(0, 256, (batch, 550, 550, 3), dtype=np.uint8))
    for _ in range(3):
        eng.evaluate()
    eng.sync()
    steps = 100 if batch <= 8 else 20
    best = min(eng.time_steps(steps, True) / steps for _ in range(3))
    print(f"{best:.5f}")

def tfl_child(lib):
    """ms per invoke (set_input + invoke + read output 4) of tests/tfl_models.mobilenetv2_yolact at 1, 2 and 16 images: median of 200."""
    import ctypes, time
    for d in ("tiny-object-detection_amd", "tests"):
        sys.path.insert(0, os.path.join(ROOT, d))
    import yolact_amd as ya
    from yolact_amd import capi
    import tfl_builder as B, tfl_models as M
    capi.lib_path = lambda: lib
    L = ctypes.CDLL(lib)
    capi.SYMBOLS[:] = [s for s in capi.SYMBOLS if hasattr(L, s[0])]   # (an older build lacks the newer entry points: none is used here)
    rng = np.random.default_rng(0)
    eng = ya.TfliteEngine(bytes(B.serialize(M.mobilenetv2_yolact(rng))), max_images=16)
    x = rng.integers(0, 256, (16, 224, 224, 3), dtype=np.uint8)
    out = []
    for nb in (1, 2, 16):
        eng.set_batch(nb)
        t = []
        for _ in range(230):
            t0 = time.perf_counter(); eng.set_input(x[:nb]); eng.invoke(); eng.output(4); t.append(time.perf_counter() - t0)
        out.append(np.median(t[30:]) * 1e3)
    print(" ".join(f"{v:.5f}" for v in out))

def tfl_main(libs, rounds):
    ms = [[], []]
    for r in range(rounds):
        for i in (0, 1):
            o = subprocess.run([sys.executable, __file__, "--tfl-child", libs[i]], capture_output=True, text=True, check=True).stdout
            ms[i].append([float(v) for v in o.strip().splitlines()[-1].split()])
            print(f"round {r} {'AB'[i]} {os.path.relpath(libs[i], ROOT)}: " + "  ".join(f"{v:.4f}" for v in ms[i][-1]) + "  ms/invoke at 1, 2, 16 images", flush=True)
    a, b = np.array(ms[0]), np.array(ms[1])
    for k, nb in enumerate((1, 2, 16)):
        inside = a[:, k].min() <= np.median(b[:, k]) <= a[:, k].max()
        print(f"{nb:2d} images: A median {np.median(a[:, k]):.4f} ({a[:, k].min():.4f} .. {a[:, k].max():.4f})   B median {np.median(b[:, k]):.4f} ({b[:, k].min():.4f} .. {b[:, k].max():.4f})"
              f"   B's median {'inside' if inside else 'OUTSIDE'} A's run-to-run spread")

if __name__ == "__main__":
    if sys.argv[1] == "--tfl-child":
        tfl_child(sys.argv[2])
    elif sys.argv[1] == "--tfl":
        tfl_main([os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])], int(sys.argv[4]) if len(sys.argv) > 4 else 6)
    elif sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        libs = [os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])]
        batch = int(sys.argv[3]) if len(sys.argv) > 3 else 64
        rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 4
        ms = [[], []]
        for r in range(rounds):
            for i in (0, 1):
                out = subprocess.run([sys.executable, __file__, "--child", libs[i], str(batch)], capture_output=True, text=True, check=True).stdout
                ms[i].append(float(out.strip().splitlines()[-1]))
                print(f"round {r} {'AB'[i]} {os.path.relpath(libs[i], ROOT)}: {ms[i][-1]:.4f} ms/step", flush=True)
        for i in (0, 1):
            print(f"{'AB'[i]}: median {np.median(ms[i]):.4f} ms, min {min(ms[i]):.4f}  (batch {batch}, best of 3 x timed replays per process)")
