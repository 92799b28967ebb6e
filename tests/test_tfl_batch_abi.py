"""CPU: the ABI of the TFLite executor's batch entry points (yh_tfl_create_batch, yh_tfl_classify_batch_u32): what they refuse before
any device is touched, and the ctypes mirror of what the headers declare. No GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_create_batch_refuses_max_images_outside_1_to_512_without_a_device(built):
    from yolact_amd import capi
    import tfl_builder as B
    import tfl_models as M
    L = capi.load_library()
    blob = bytes(B.serialize(M.single_op("RELU", np.random.default_rng(0))))
    assert capi.tfl_validate(blob)[0]
    assert capi.TFL_MAX_IMAGES == int(re.search(r"#define YH_TFL_MAX_IMAGES (\d+)", _header("yolact_hip.h")).group(1)) == 512
    for bad in (0, -1, 513, 1 << 30):
        h = C.c_void_p(0xDEAD)
        assert L.yh_tfl_create_batch(blob, len(blob), 0, bad, C.byref(h)) == capi.EINVAL and not h.value
        assert b"max_images" in L.yh_tfl_last_error(None)
        h = C.c_void_p(0xDEAD)
        assert L.yh_tfl_create_batch_tuned(blob, len(blob), 0, bad, None, C.byref(h)) == capi.EINVAL and not h.value
    # device -1 does not exist anywhere: a max_images inside the range gets past the range check and fails on the device instead
    h = C.c_void_p()
    assert L.yh_tfl_create_batch(blob, len(blob), -1, 512, C.byref(h)) == capi.EHIP and not h.value
    assert L.yh_tfl_create_batch(None, 0, 0, 4, C.byref(h)) == capi.EINVAL
    assert L.yh_tfl_create_batch(blob, len(blob), 0, 4, None) == capi.EINVAL


def test_null_handles(built):
    from yolact_amd import capi
    L = capi.load_library()
    f = np.zeros(16, np.uint32)
    p = f.ctypes.data_as(C.c_void_p)
    assert L.yh_tfl_classify_batch_u32(None, p, 0, 1, 4, 4, capi.COMPAT_SANE, p, None) == capi.EINVAL
    assert L.yh_tfl_classify_batch_device_frames(None) is None
    assert L.yh_tfl_set_batch(None, 3) == capi.EINVAL


def test_python_surface(built):
    import inspect
    from yolact_amd import capi
    from yolact_amd.yolact import Yolact
    assert inspect.signature(capi.TfliteEngine.__init__).parameters["max_images"].default == 2
    sig = inspect.signature(capi.TfliteEngine.classify_batch).parameters
    assert [sig[k].default for k in ("out", "read")] == [None, True]
    assert "max_batch" in inspect.signature(Yolact.init).parameters

