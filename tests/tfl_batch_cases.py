"""Cases and helpers of the TFLite executor's tests at more than two images per invoke (tests/test_gpu_tflite_batch.py,
tests/test_gpu_tflite_classify_batch.py): seeded single-CONV_2D cases whose 16- and 32-pixel tiles straddle image boundaries, the
per-image comparison against oracle/tfl_oracle.py, and the device copies the classify batch's tests need."""
import ctypes as C

import numpy as np

import tfl_builder as B
import tfl_models as M
from tfl_cases import oracle_images   # noqa: F401  (the oracle's value of every tensor per image of x, each image alone)

# ------------------------------------------------------------------ single CONV_2D at 3 and 5 images
# pixels per image 35, 9, 36 (SAME, stride 1) - no multiple of 16, so at 3 and 5 images a 16-pixel tile and a 32-pixel tile hold pixels
# of two images (9: of up to four) and M = pixels x images is no multiple of 16 (36 x 3 = 108, 35 x 5 = 175, 9 x 5 = 45 ...)
CONV_HW = ((5, 7), (3, 3), (9, 4))
CONV_CI = (4, 16, 24, 64, 96, 160)
CONV_CO = (5, 16, 24, 33, 40)
CONV_ACTS = (0, 1, 2, 3)          # none, RELU, RELU_N1_TO_1, RELU6
N_CONV_CASES = 40


def conv_cases():
    """[(h, w, ci, co, k, stride, padding, act)] x 40, seeded; every listed value of every parameter occurs."""
    rng = np.random.default_rng(2024)
    cases = []
    for i in range(N_CONV_CASES):
        h, w = CONV_HW[i % 3]
        ci, co = CONV_CI[int(rng.integers(0, 6))] if i >= 6 else CONV_CI[i], CONV_CO[int(rng.integers(0, 5))] if i >= 5 else CONV_CO[i]
        k = 1 if (i // 3) % 2 == 0 else 3
        stride, padding, act = 1 + (i // 6) % 2, (i // 12) % 2, CONV_ACTS[i % 4]
        cases.append((h, w, ci, co, k, stride, padding, act))
    for col, vals in ((2, CONV_CI), (3, CONV_CO), (4, (1, 3)), (5, (1, 2)), (6, (0, 1)), (7, CONV_ACTS)):
        assert {c[col] for c in cases} == set(vals), (col, vals)
    assert {(c[0], c[1]) for c in cases} == set(CONV_HW)
    return cases


def conv_case_model(i, case):
    """The model of case i and its input for 5 images."""
    h, w, ci, co, k, stride, padding, act = case
    rng = np.random.default_rng(7000 + i)
    m = M.single_op("CONV_2D", rng, h=h, w=w, ci=ci, co=co, k=k, stride=stride, padding=padding, act=act)
    x = rng.integers(0, 256, (5, h, w, ci), dtype=np.uint8)
    return m, x


def check_tensor(eng, model, index, wants, nb, label=""):
    """Tensor `index` of an engine at nb images == the oracle's per image; False if the plan never writes it (folded)."""
    import yolact_amd as ya
    t = model.tensors[index]
    try:
        got = eng.tensor(index, t.shape, B.NP_TYPE[t.dtype])
    except ya.YhError as e:
        assert e.code == ya.capi.ESTATE and "folded" in str(e), (label, index, t.name, str(e))
        return False
    got = got.reshape(nb, -1)
    for i in range(nb):
        assert np.array_equal(got[i], np.asarray(wants[i][index]).reshape(-1)), (label, t.name, "image", i)
    return True


def check_outputs(eng, model, wants, nb, label=""):
    outs = []
    for k, o in enumerate(model.outputs):
        got = eng.output(k)
        outs.append(got)
        for i in range(nb):
            want = np.asarray(wants[i][o])
            assert got.dtype == want.dtype and np.array_equal(got.reshape(nb, -1)[i], want.reshape(-1)), (label, model.tensors[o].name, i)
    return outs


# ------------------------------------------------------------------ device memory through the HIP library the package loaded
def _hip():
    path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), "libamdhip64.so")
    return C.CDLL(path)


def device_u32(ptr, n):
    """n uint32 from device memory."""
    out = np.zeros(n, np.uint32)
    assert _hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0   # hipMemcpyDeviceToHost
    return out


class DeviceCopy:
    """A device copy of a host uint32 array (hipMalloc + hipMemcpy through the HIP library), freed by close()."""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr, np.uint32)
        self.hip = _hip()
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(arr.nbytes)) == 0
        self.ptr = p.value
        assert self.hip.hipMemcpy(C.c_void_p(self.ptr), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), 1) == 0   # hipMemcpyHostToDevice

    def close(self):
        if self.ptr:
            self.hip.hipFree(C.c_void_p(self.ptr))
            self.ptr = None


def code(fn):
    """The YhError code fn() raises, 0 if none."""
    from yolact_amd import capi
    try:
        fn()
    except capi.YhError as e:
        return e.code
    return 0
