"""Static instruction counts of conv_igemm_f16's streaming forms: instructions before the first LDS-DMA and in all.
Compiles csrc/conv_igemm.hip to assembly for gfx950 (hipcc -O3 -S --cuda-device-only) and reads the kernels' bodies.
Usage: python tools/conv_prologue_count.py [--root CHECKOUT] [--hipcc PATH]"""
import argparse, os, re, subprocess, sys, tempfile

# template arguments <TCH, TM, WCH, WM, SMALLC, STAGES, EPI, SPLITK, MT, ML, FP8, RESUP / GEO, DUAL, TAIL, K3> as mangled digits
FORMS = [("plain 128x128", "128 128 2 2 0 1 2 0 32 0 0 0 0 0 0"), ("[3x3] 128x128", "128 128 2 2 0 1 2 0 32 0 0 0 0 0 1"),
         ("DUAL 128x128", "128 128 2 2 0 1 2 0 32 0 0 0 1 0 0"), ("RESUP 128x128", "128 128 2 2 0 1 2 0 32 0 0 1 0 0 0"),
         ("dense 1x1 128x128", "128 128 2 2 0 1 2 0 32 0 0 2 0 0 0"), ("plain 64x256", "64 256 1 4 0 1 2 0 32 0 0 0 0 0 0"),
         ("dense 1x1 64x256", "64 256 1 4 0 1 2 0 32 0 0 2 0 0 0")]


def is_instruction(line):
    return line.startswith("\t") and line.strip() and not line.lstrip().startswith((".", ";"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to read (default: this one)")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "hipcc"))
    a = ap.parse_args()
    src = os.path.join(os.path.abspath(a.root), "tiny-object-detection_amd", "csrc", "conv_igemm.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "conv_igemm.s")
        r = subprocess.run([a.hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", asm],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(r.stderr)
        text = open(asm).read()
    bodies = {}
    for m in re.finditer(r"^(_ZN2yh14conv_igemm_f16I[^\s:]+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        bodies[" ".join(re.findall(r"L[ib](\d+)E", m.group(1)))] = m.group(2)
    for name, key in FORMS:
        if key not in bodies:
            print(f"{name:20s} (not instantiated)")
            continue
        ins = [l.strip() for l in bodies[key].splitlines() if is_instruction(l)]
        first = next(i for i, l in enumerate(ins) if l.startswith("buffer_load") and " lds" in l)
        pre = ins[:first]
        vec = sum(l.startswith(("v_", "ds_", "buffer_", "global_")) for l in pre)
        print(f"{name:20s} before the first LDS-DMA {len(pre):4d} (vector {vec:4d}, scalar {sum(l.startswith('s_') for l in pre):4d})   static total {len(ins):5d}")


if __name__ == "__main__":
    main()
