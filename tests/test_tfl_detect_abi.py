"""CPU: the ABI of the TFLite detections (yh_tfl_detect_setup .. yh_tfl_masks_device, yh_tfl_op_detect): the symbols resolve in the
built library, the defaults are the documented ones, the ctypes mirror has the C struct's size and offsets, null handles are
refused, and tfl_priors has the documented shape. No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("yh_tfl_default_detect_config", "yh_tfl_detect_setup", "yh_tfl_evaluate", "yh_tfl_detect", "yh_tfl_read_detections",
        "yh_tfl_proto_dims", "yh_tfl_detections_device", "yh_tfl_detection_counts_device", "yh_tfl_masks_device", "yh_tfl_op_detect")


def test_symbols_resolve_and_are_declared(built):
    from yolact_amd import capi
    L = capi.load_library()
    declared = {s[0] for s in capi.SYMBOLS}
    pub = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read()
    for name in SYMS:
        assert getattr(L, name) is not None and name in declared
        assert (name + "(") in (dbg if name == "yh_tfl_op_detect" else pub), name
    assert "max_images * (C - 1) * P * 8" in pub          # the memory formula is part of the header


def test_default_config(built):
    from yolact_amd import capi
    L = capi.load_library()
    c = capi.TflDetectConfig()
    C.memset(C.byref(c), 0xAB, C.sizeof(c))
    L.yh_tfl_default_detect_config(C.byref(c))
    assert list(c.outputs) == [0, 1, 2, 3] and (c.top_k, c.max_dets, c.max_images) == (200, 100, 0)
    assert c.conf_thresh == np.float32(0.05) and c.nms_thresh == np.float32(0.5) and list(c.reserved) == [0, 0, 0, 0]
    L.yh_tfl_default_detect_config(None)                   # (a null pointer is ignored)


def test_config_layout_matches_the_header(built, tmp_path):
    from yolact_amd import capi
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yolact_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(yh_tfl_detect_config), offsetof(yh_tfl_detect_config, outputs),'
                   ' offsetof(yh_tfl_detect_config, top_k), offsetof(yh_tfl_detect_config, max_dets), offsetof(yh_tfl_detect_config, conf_thresh),'
                   ' offsetof(yh_tfl_detect_config, max_images), offsetof(yh_tfl_detect_config, reserved)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = capi.TflDetectConfig
    assert got == [C.sizeof(T), T.outputs.offset, T.top_k.offset, T.max_dets.offset, T.conf_thresh.offset, T.max_images.offset, T.reserved.offset]
    assert C.sizeof(T) == 52


def test_null_handles(built):
    from yolact_amd import capi
    L = capi.load_library()
    c = capi.TflDetectConfig()
    pr = np.zeros((3, 4), np.float32)
    n = C.c_int32()
    assert L.yh_tfl_detect_setup(None, C.byref(c), pr.ctypes.data_as(C.c_void_p), 3) == capi.EINVAL
    assert L.yh_tfl_evaluate(None) == capi.EINVAL and L.yh_tfl_detect(None) == capi.EINVAL
    assert L.yh_tfl_read_detections(None, 0, C.byref(n), None, 0, None, 0) == capi.EINVAL
    assert L.yh_tfl_proto_dims(None, None) == capi.EINVAL
    assert L.yh_tfl_detections_device(None) is None and L.yh_tfl_detection_counts_device(None) is None and L.yh_tfl_masks_device(None) is None


def test_tfl_priors_shape_order_and_python_surface(built):
    import inspect
    import yolact_amd as ya
    p = ya.tfl_priors([4, 2, 1], 64)
    assert p.dtype == np.float32 and p.shape == (3 * (16 + 4 + 1), 4)
    assert np.array_equal(p[:3, 0], np.float32([0.125] * 3)) and np.array_equal(p[3, :2], np.float32([0.375, 0.125]))   # level, row, column, anchor
    assert p[0, 2] == p[0, 3] == np.float32(np.float32(np.float32(24.0 * 64) / np.float32(550.0)) / np.float32(64))   # anchor 0: aspect 1
    assert p[48, 2] > p[0, 2] and p[1, 2] < p[0, 2] < p[2, 2]
    for m in ("detect_setup", "evaluate", "detect", "detections", "op_detect"):
        assert callable(getattr(ya.TfliteEngine, m))
    assert inspect.signature(ya.TfliteEngine.detections).parameters["want_masks"].default is True
