"""CPU: the ABI of the TFLite instance frames (yh_tfl_instance_batch .. yh_tfl_instance_row_width, yh_tfl_op_instance_frames;
DESIGN.md §11 "TFLite instance frames"): the library exports the six symbols, the headers declare them with the documented argument
counts - the single-op entry in the debug header only -, capi binds them, TfliteEngine has the five methods with the documented
signatures, null handles are refused, and the scene batch's comment names the new source. No GPU."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = {"yh_tfl_instance_batch": 8, "yh_tfl_instance_frames": 8, "yh_tfl_instance_device_frames": 1, "yh_tfl_instance_read": 5,
          "yh_tfl_instance_row_width": 1}
DEBUG = {"yh_tfl_op_instance_frames": 14}


def _code(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_symbols_are_exported_declared_and_bound(built):
    from yolact_amd import capi
    L = capi.load_library()
    pub, dbg = _code("yolact_hip.h"), _code("yolact_hip_debug.h")
    bound = {s[0]: s for s in capi.SYMBOLS}
    for name, nargs in list(PUBLIC.items()) + list(DEBUG.items()):
        src = dbg if name in DEBUG else pub
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name + " is not declared where it belongs"
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L, name), name + " is not exported"
        assert name in bound and len(bound[name][2]) == nargs, name
    assert not re.search(r"\byh_tfl_op_[a-z_]+\s*\(", pub)                # the drop-in header names no single-op entry
    assert "#define YH_ABI_VERSION 4" in open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    assert bound["yh_tfl_instance_device_frames"][1] is C.c_void_p


def test_python_surface(built):
    import yolact_amd as ya
    T = ya.TfliteEngine
    for name in ("instance_batch", "instance_frames"):
        p = inspect.signature(getattr(T, name)).parameters
        assert list(p) == ["self", "first", "n", "width", "height", "class_map", "min_score", "read"], (name, list(p))
        assert p["class_map"].default is None and p["min_score"].default == 0.0 and p["read"].default is True
    assert list(inspect.signature(T.instance_device_frames).parameters) == ["self"]
    assert list(inspect.signature(T.instances_of).parameters) == ["self", "i"]
    p = inspect.signature(T.op_instance_frames).parameters
    assert list(p) == ["self", "masks", "class_ids", "scores", "counts", "width", "height", "class_map", "min_score"]


def test_null_handles(built):
    from yolact_amd import capi
    L = capi.load_library()
    n = C.c_int32()
    assert L.yh_tfl_instance_batch(None, 0, 1, 8, 8, None, C.c_float(0.0), None) == capi.EINVAL
    assert L.yh_tfl_instance_frames(None, 0, 1, 8, 8, None, C.c_float(0.0), None) == capi.EINVAL
    assert L.yh_tfl_instance_device_frames(None) is None
    assert L.yh_tfl_instance_read(None, 0, C.byref(n), None, 0) == capi.EINVAL
    assert L.yh_tfl_instance_row_width(None) == capi.EINVAL
    assert L.yh_tfl_op_instance_frames(None, None, None, None, None, 1, 0, 1, 1, 8, 8, None, C.c_float(0.0), None) == capi.EINVAL


def test_the_scene_batch_names_the_new_source():
    pub = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    comment = pub[:pub.index("int yh_scene_batch_stage_frames(")].rsplit("/*", 1)[1]
    assert "yh_tfl_instance_device_frames" in comment
    # ... and the detections' device pointers no longer promise a reader to come
    assert "will read" not in pub[pub.index("yh_tfl_proto_dims("):pub.index("yh_tfl_masks_device(")]
