"""-m gpu: every compiled (tile, form) instance of conv_igemm_f16, alone, against the CPU oracle - bit for bit - and the proof that it
was that instance which ran. The cases are tests/conv_form_cases.py's (tests/test_conv_form_cases.py holds them against the table the
library was compiled with, on the CPU: a (tile, form) without a case does not ship); each runs through a single-op entry point with
the tile forced (tune.op_tile), a split-K forced where the case is one (tune.op_kslices), and then

  * np.array_equal against the oracle's output - integer data, every float32 sum exact, one f16 rounding: no tolerance anywhere;
  * yh_debug_last_conv_forms == the case's (tile, form), plus splitk_reduce_f16 behind a split-K: a case "for" the dense 1x1 form
    that silently ran the plain one, or on another tile, fails here.

Every entry point stages its output between guards of 0xFF, 4096 bytes in front and 256 rows behind row M - 1, and checks them itself
(YH_EOVERFLOW; tests/test_gpu_op_guards.py runs every (tile, form) at the shapes where that decides something)."""
import numpy as np
import pytest

import conv_form_cases as F
from test_gpu_ops import _forced, eng  # noqa: F401  (the module's engine fixture)

pytestmark = pytest.mark.gpu


def _codes(oracle, a):
    return oracle.quantize_e4m3(a)


def _run(eng, oracle, cid):
    c, t = F.CASES[cid], F.build(cid)
    kind = c["kind"]
    if kind == "conv":
        return eng.op_conv2d(t["x"], t["w"], t["bias"], c["stride"], c["pad"], t["res"], c["act"])
    if kind == "levels":
        return eng.op_conv2d_levels(t["x"], F.LEVELS, t["w"], t["bias"], act=c["act"])
    if kind == "dual":
        return eng.op_conv2d_dual(t["x1"], t["x2"], c["stride2"], t["w"], t["bias"], act=c["act"])
    if kind == "resup":
        return eng.op_conv2d_resup(t["x"], t["w"], t["bias"], t["res_lo"], act=c["act"])
    if kind == "tail":
        return eng.op_conv2d_tail(t["x"], t["w"], t["bias"], t["w2"], t["bias2"], act=c["act"])
    if kind == "tail_fp8":
        return eng.op_conv2d_tail(_codes(oracle, t["x"]), _codes(oracle, t["w"]), t["bias"], t["w2"], t["bias2"], act=c["act"], scale=t["scale"])
    if kind == "levels_fp8":
        return eng.op_conv2d_levels_fp8(_codes(oracle, t["x"]), F.LEVELS, _codes(oracle, t["w"]), t["scale"], t["bias"], act=c["act"])
    assert kind == "fp8"
    return eng.op_conv2d_fp8(_codes(oracle, t["x"]), _codes(oracle, t["w"]), t["scale"], t["bias"], 1, c["k"] // 2, t["res"], c["act"])[0]


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_instance_alone_is_the_oracle(eng, oracle, cid):
    want = F.reference(cid, oracle)
    got = _forced(eng, F.tuning(cid), lambda: _run(eng, oracle, cid))
    ran = eng.last_conv_forms()
    assert ran == F.expected_kernels(cid), (cid, ran)
    assert eng.last_conv_launches() == 1
    diff = got.reshape(want.shape) != want
    at = np.argwhere(diff)[:4]
    print(f"{cid}: {int(np.count_nonzero(diff))} of {want.size} elements differ")
    assert got.size == want.size and not diff.any(), (cid, [(i.tolist(), float(got.reshape(want.shape)[tuple(i)]), float(want[tuple(i)])) for i in at])


def _refused(eng, ya, tune, fn):
    """fn under `tune` must be refused with YH_EINVAL before any launch: the handle's launch count and list stay as they were."""
    before = (eng.last_conv_launches(), eng.last_conv_forms())
    with pytest.raises(ya.YhError) as ei:
        _forced(eng, tune, fn)
    assert ei.value.code == ya.capi.EINVAL, str(ei.value)
    assert (eng.last_conv_launches(), eng.last_conv_forms()) == before
    return str(ei.value)


def test_one_refusal_per_entry_point(eng, oracle, built):
    """A tile without the form, a convolution to other than 256 channels for the fused tail, an fp8 tile handed to an f16 entry point
    (and the reverse): YH_EINVAL with a message, and nothing launched - the same calls on a tile that has the form are the cases above."""
    ya = built
    T = F.TILES
    # a known state first: one split-K case = two kernels on the list
    first = "conv-64x64_S3-SPLITK-m105-k1c128-s2"
    _forced(eng, F.tuning(first), lambda: _run(eng, oracle, first))
    assert eng.last_conv_forms() == F.expected_kernels(first) and len(eng.last_conv_forms()) == 2
    one = lambda kind, tile: next(i for i in F.CASE_IDS if F.CASES[i]["kind"] == kind and F.CASES[i]["tile"] == tile)
    conv, lev, dual, resup = one("conv", "128x128"), one("levels", "128x128"), one("dual", "128x128"), one("resup", "128x128")
    tail, tail8, fp8, lev8 = one("tail", "256x256_M16"), one("tail_fp8", "256x256_FP8"), one("fp8", "256x256_FP8"), one("levels_fp8", "256x256_FP8")
    run = lambda cid: (lambda: _run(eng, oracle, cid))
    # an fp8 tile id handed to the f16 entry points
    for cid in (conv, lev):
        _refused(eng, ya, dict(op_tile=T["256x256_FP8"]), run(cid))
    assert "fused-tail" in _refused(eng, ya, dict(op_tile=T["256x256_FP8"]), run(tail))
    # a tile lacking the form
    _refused(eng, ya, dict(op_tile=T["64x256"]), run(lev))                       # no multi-level form
    _refused(eng, ya, dict(op_tile=T["96x128_K1"]), run(conv))                   # multi-level form only
    _refused(eng, ya, dict(op_tile=T["128x128"], op_kslices=2), run("conv-128x128_S3-SPLITK-m105-k1c128-s2"))   # no split-K form
    assert "two-source" in _refused(eng, ya, dict(op_tile=T["128x256"]), run(dual))
    assert "upsampled-residual" in _refused(eng, ya, dict(op_tile=T["128x256"]), run(resup))
    assert "fused-tail" in _refused(eng, ya, dict(op_tile=T["128x128"]), run(tail))
    assert "fused-tail" in _refused(eng, ya, dict(op_tile=T["128x128_FP8"]), run(tail8))
    assert "fp8 tile" in _refused(eng, ya, dict(op_tile=T["256x256_M16"]), run(fp8))
    assert "fp8 tile" in _refused(eng, ya, dict(op_tile=T["64x64_FP8"]), run(lev8))          # an fp8 tile without the multi-level form
    assert "not a tile id" in _refused(eng, ya, dict(op_tile=4), run(conv))                  # (a retired id)
    # the fused tail runs on exactly 256 channels
    t = F.build(tail)
    for cout in (248, 264):
        w = np.resize(t["w"], (cout,) + t["w"].shape[1:])
        msg = _refused(eng, ya, {}, lambda: eng.op_conv2d_tail(t["x"], w, np.resize(t["bias"], cout), t["w2"], t["bias2"]))
        assert "256 channels" in msg
    t8 = F.build(tail8)
    w8 = _codes(oracle, np.resize(t8["w"], (264,) + t8["w"].shape[1:]))
    msg = _refused(eng, ya, {}, lambda: eng.op_conv2d_tail(_codes(oracle, t8["x"]), w8, np.resize(t8["bias"], 264), t8["w2"], t8["bias2"],
                                                          scale=np.resize(t8["scale"], 264)))
    assert "256 channels" in msg
    # ... and the handle still runs: the first case again, same bits
    got = _forced(eng, F.tuning(first), lambda: _run(eng, oracle, first))
    assert np.array_equal(got, F.reference(first, oracle))


def test_unforced_fp8_entry_keeps_the_256_tile(eng, oracle):
    """tune.op_tile = -1 stays the 256 x 256 fp8 tile: every existing caller of yh_op_conv2d_fp8 keeps its kernel."""
    cid = "fp8-256x256_FP8-PLAIN-m105-k1c128"
    got = _run(eng, oracle, cid)
    assert eng.last_conv_forms() == [(F.TILES["256x256_FP8"], "PLAIN")]
    assert np.array_equal(got, F.reference(cid, oracle))
