"""CPU: csrc/divmagic.h - the conv kernels' division by a launch constant as multiply-high and shift - against / and %, exhaustively
over every dividend the kernels form (0 <= m < M + 256, the largest tile's rows) for every divisor the networks produce.

The check is a stand-alone C++ program (tests/conv_divmagic_check.cpp) built with the host compiler: the header has no HIP
dependency."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiny-object-detection_amd", "csrc")


def _out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def net_maps(size):
    """Edges of the square feature maps a YOLACT of this input size convolves onto: stem, pool / layer 1, layers 2-4 (= P3-P5),
    P6, P7, and the protonet's upsampled map."""
    stem = _out(size, 7, 2, 3)
    l1 = _out(stem, 3, 2, 1)
    maps = [stem, l1]
    for _ in range(5):   # layers 2, 3, 4, then P6, P7: 3x3, stride 2, pad 1
        maps.append(_out(maps[-1], 3, 2, 1))
    return maps + [2 * maps[2]]


def cases():
    """(divisor, rows): rows = M + 256 for the largest M the divisor is used with (batch 64 covers batch 1's dividends)."""
    want = {}

    def add(d, rows):
        want[d] = max(want.get(d, 0), rows)

    for size in (550, 700):   # YOLACT-550 R50, YOLACT-700 R101: same map sizes per input size, whatever the depth
        maps = net_maps(size)
        levels = maps[2:7]                        # the shared head's five pyramid levels
        cells = sum(e * e for e in levels)        # ... laid end to end: the multi-level form's P * Q
        for batch in (1, 64):
            for e in maps:
                add(e * e, batch * e * e + 256)   # P * Q
                add(e, e * e)                     # Q: the dividend is the row within its image
            add(cells, batch * cells + 256)
            for e in levels:
                add(e, e * e)                     # a level's width: the dividend is the cell within its level
    big = 64 * 138 * 138                          # the largest M of the flagship step
    for d in (1, 2, 3, 5, 9, 25, 81, 324, 1225, 4761, 19044, big):
        add(d, big + 256)
    return sorted(want.items())


def test_net_maps_are_the_networks():
    assert net_maps(550) == [275, 138, 69, 35, 18, 9, 5, 138] and net_maps(700) == [350, 175, 88, 44, 22, 11, 6, 176]


def test_divmagic_exhaustive(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "conv_divmagic_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "conv_divmagic_check.cpp"), "-o", exe])
    cs = cases()
    assert {1, 2, 3, 5, 9, 25, 81, 324, 1225, 4761, 19044, 64 * 138 * 138, 6416, 10321, 175 * 175, 350 * 350} <= {d for d, _ in cs}
    args = [str(v) for c in cs for v in c]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok: %d divisors" % len(cs)), r.stdout + r.stderr
