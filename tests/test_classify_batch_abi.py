"""The surface of the classify batch (yh_classify_batch_u32, yh_classify_batch_device_frames and the two single-kernel hooks;
DESIGN.md §11 "Classify batch") on the CPU: the built library exports the four symbols, the two headers declare them (the public one
never names a yh_op_* entry), and the ctypes table binds them with the declared number of arguments."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = (("yh_classify_batch_u32", 9), ("yh_classify_batch_device_frames", 1))
HOOKS = (("yh_op_classify_pre_batch", 7), ("yh_op_classify_post_batch", 8))


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _declared_args(src, name):
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_library_exports_the_classify_batch_symbols(built):
    from yolact_amd import capi
    L = capi.load_library()
    for name, _ in PUBLIC + HOOKS:
        assert hasattr(L, name), name


def test_headers_declare_them_and_the_table_binds_them():
    from yolact_amd import capi
    bound = {s[0]: s for s in capi.SYMBOLS}
    pub, dbg = _header("yolact_hip.h"), _header("yolact_hip_debug.h")
    for names, src in ((PUBLIC, pub), (HOOKS, dbg)):
        for name, nargs in names:
            assert _declared_args(src, name) == nargs, name
            assert name in bound and len(bound[name][2]) == nargs, name
    text = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    assert "yh_op_classify" not in text
    # the comment of yh_scene_batch_stage_frames names the new device pointer as a source
    comment = text[text.index("yh_scene_batch_stage for slots"):text.index("int yh_scene_batch_stage_frames")]
    assert "yh_classify_batch_device_frames" in comment


def test_python_surface():
    from yolact_amd import capi
    from yolact_amd.yolact import Yolact
    sig = inspect.signature(capi.Engine.classify_batch).parameters
    assert list(sig)[1:] == ["frames_u32", "frames_dev_ptr", "n", "width", "height", "mode", "out"]
    assert sig["frames_u32"].default is None and sig["frames_dev_ptr"].default is None and sig["out"].default is True
    for m in ("classify_batch_device_frames", "op_classify_pre_batch", "op_classify_post_batch"):
        assert callable(getattr(capi.Engine, m)), m
    assert inspect.signature(Yolact.init).parameters["max_batch"].default == 2
    sig = inspect.signature(Yolact.classify_batch).parameters
    assert list(sig)[1:] == ["frames", "width", "height"] and sig["width"].default == 640 and sig["height"].default == 480
