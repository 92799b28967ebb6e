"""Registers / spills / LDS / scratch bytes of every kernel in lib/libyolact_hip.so (code-object metadata), optionally filtered by substrings.
Usage: python tools/kernel_meta.py [--lib DIR] [substr ...]   (DIR: another build's library directory, e.g. lib_old, under the package)"""
import os, re, subprocess, sys, tempfile, shutil, glob
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
args = sys.argv[1:]
libdir = "lib"
if args[:1] == ["--lib"]: libdir, args = args[1], args[2:]
so = os.path.join(ROOT, "tiny-object-detection_amd", libdir, "libyolact_hip.so")
tmp = tempfile.mkdtemp()
try:
    dst = os.path.join(tmp, "lib.so"); shutil.copy(so, dst)
    subprocess.run([LLVM + "/llvm-objdump", "--offloading", dst], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
    for co in sorted(glob.glob(dst + ".*gfx950")):
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count|\n\s+- \.args", notes):
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name or not re.search(r"\.vgpr_count", blk): continue
            f = lambda k: (re.search(r"\.%s:\s+(\d+)" % k, blk) or [None, "?"])[1]
            dem = subprocess.run(["c++filt", name.group(1)], capture_output=True, text=True).stdout.strip()
            dem = dem.replace("void yh::", "").replace("(yh::ConvParams)", "").replace("(yh::BneckParams)", "")
            if all(s in dem for s in args):
                print(f"vgpr {f('vgpr_count'):>3} sgpr {f('sgpr_count'):>3} spill {f('vgpr_spill_count'):>3} lds {f('group_segment_fixed_size'):>6} scratch {f('private_segment_fixed_size'):>4}  {dem[:150]}")
finally:
    shutil.rmtree(tmp)
