"""-m gpu: how the convolution kernels round. Every f16 tensor they write is specified as the round-to-nearest-even of the float32
value after bias, residual and activation, and nowhere earlier (Precision). The integer tests of tests/test_gpu_ops.py
cannot see that: their sums are integers f16 holds. The cases of tests/dyadic_cases.py make every operand an integer times a power
of two, so that every float32 partial sum of any order is exact and 12 to 22 bits wide (tests/test_dyadic_cases.py proves it on the
CPU, and that a kernel which rounds toward zero, holds partial sums in f16 or rounds before bias and residual are added differs on
at least 5 % of the outputs). Every comparison here is np.array_equal against the float64 reference rounded once: conv_igemm_f16
on every tile and form the op entries reach, splitk_reduce_f16, the two-launch plans, the two-source form, stem_pool_f16 and the
fp8 conv's epilogue. The twelve bottleneck launches take their dyadic case in tests/test_gpu_bneck_op.py."""
import numpy as np
import pytest

import dyadic_cases as D
from test_gpu_ops import _DUAL_TILES, _TILES, _forced

pytestmark = pytest.mark.gpu

_SPLIT_K = [("128x128_S3", 2), ("128x128_S3", 3), ("64x64_S3", 4), ("64x64_S3", 5)]      # the ring tiles have the split-K forms
_HEAD = [(t, 0) for t in _TILES] + _SPLIT_K
_DUAL = [(t, 0) for t in _DUAL_TILES] + [("128x128_S3", 2), ("128x128_S3", 3), ("64x64_S3", 2), ("64x64_S3", 5)]


@pytest.fixture(scope="module")
def eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=2, use_graph=False)
    yield e
    e.close()


def _same(got, cid, what=""):
    want = D.reference(D.build(cid))
    diff = got != want
    print(f"{cid} {what}: {int(np.count_nonzero(diff))} of {want.size} elements differ")
    at = np.argwhere(diff)[:4]
    assert got.shape == want.shape and np.array_equal(got, want), (cid, what, [(i.tolist(), float(got[tuple(i)]), float(want[tuple(i)])) for i in at])


def _tune(tiles, tile, kslices):
    env = {"op_tile": tiles[tile]}
    if kslices:
        env.update(op_kslices=kslices)
    return env


def _conv(eng, c):
    return eng.op_conv2d(c["x"], c["w"], c["bias"], c["stride"], c["pad"], c["res"], c["act"])


def _levels(eng, c):
    return eng.op_conv2d_levels(c["x"], c["sizes"], c["w"], c["bias"], act=c["act"])


@pytest.mark.parametrize("tile,kslices", _HEAD)
def test_every_head_tile_plain_form(eng, tile, kslices):
    """Ragged M, residual, ReLU on every tile a head conv can be launched on, and the split-K forms of the ring tiles (the slabs and
    splitk_reduce_f16's sum must stay float32: K = 1152 is 18 steps, so 2 .. 5 slices all split)."""
    c = D.build("head_3x3")
    got = _forced(eng, _tune(_TILES, tile, kslices), lambda: _conv(eng, c))
    assert eng.last_conv_launches() == 1
    _same(got, "head_3x3", f"{tile}/{kslices}")


@pytest.mark.parametrize("tile,kslices", _HEAD)
@pytest.mark.parametrize("k", [3, 1])
def test_every_head_tile_multilevel_form(eng, tile, kslices, k):
    """... and their multi-level forms (levels 9, 5, 3, 1 laid end to end; at k = 1, K = 128 is two steps: more slices than that
    leave the launch unsplit, as in test_conv_multilevel_exact_on_integers)."""
    cid = f"levels_k{k}"
    got = _forced(eng, _tune(_TILES, tile, kslices), lambda: _levels(eng, D.build(cid)))
    assert eng.last_conv_launches() == 1
    _same(got, cid, f"{tile}/{kslices}")


@pytest.mark.parametrize("cid", ["big_64_256_k3", "big_256_512_k1", "big_64_351_k3", "deep_k2048"])
def test_default_plan(eng, cid):
    """The tiles the op entry picks itself: 256x256 (16x16x32 MFMA, split epilogue) with and without residual and activation, 128x256
    with a ragged channel tail, and K = 2048."""
    got = _conv(eng, D.build(cid))
    assert eng.last_conv_launches() == 1
    _same(got, cid)


@pytest.mark.parametrize("cid", ["split_64_256_k3", "split_512_351_k1"])
def test_two_launch_plans(eng, cid):
    """The wave-quantisation tail and the channel split, reached by planning for a 4-CU chip: the reference's bits, and so the single
    launch's."""
    c = D.build(cid)
    single = _conv(eng, c)
    assert eng.last_conv_launches() == 1
    eng.set_tuning(plan_cus=4)
    try:
        split = _conv(eng, c)
        assert eng.last_conv_launches() == 2          # the plan under test was really taken
    finally:
        eng.reset_tuning("plan_cus")
    _same(split, cid, "split")
    _same(single, cid, "single")
    assert np.array_equal(split, single)


@pytest.mark.parametrize("chsplit", [1, 2])
def test_head_remainder_on_96_channel_tiles(eng, chsplit):
    """The shared head's channels 256 .. 350 on the 96-channel streaming tile (chsplit 1) and on the 128-channel one (chsplit 2)."""
    c = D.build("rem96_k3")
    eng.set_tuning(plan_cus=4, chsplit=chsplit)
    try:
        got = _levels(eng, c)
        assert eng.last_conv_launches() == 2
    finally:
        eng.reset_tuning("plan_cus", "chsplit")
    _same(got, "rem96_k3", f"chsplit {chsplit}")


@pytest.mark.parametrize("tile,kslices", _DUAL)
def test_dual_source(eng, tile, kslices):
    """The two-source 1x1 form on every tile it is instantiated for, split-K slices starting before and after the switch of sources
    (K = 384 is 6 steps, the switch after 2): the reference of the channel-concatenated tensors."""
    c = D.build("dual_s2")
    got = _forced(eng, _tune(_DUAL_TILES, tile, kslices), lambda: eng.op_conv2d_dual(c["x1"], c["x2"], c["stride2"], c["w"], c["bias"], act=c["act"]))
    assert eng.last_conv_launches() == 1
    _same(got, "dual_s2", f"{tile}/{kslices}")


@pytest.mark.parametrize("cid", ["stem_n2_S30", "stem_n1_S34"])
def test_stem_pool(eng, oracle, cid):
    """stem_pool_f16: the stem bit for bit; the pool is the maximum of ROUNDED stem values (the oracle's pool of the reference stem),
    with and without the stem output."""
    c = D.build(cid)
    stem, pool = eng.op_stem_pool(c["x"], c["w"], c["bias"])
    _same(stem, cid, "stem")
    want_pool = oracle.maxpool3x3s2(D.reference(c))
    assert np.array_equal(pool, want_pool), int(np.count_nonzero(pool != want_pool))
    none, pool2 = eng.op_stem_pool(c["x"], c["w"], c["bias"], want_stem=False)
    assert none is None and np.array_equal(pool2, want_pool)


@pytest.mark.parametrize("cid", D.FP8_IDS)
def test_fp8_epilogue(eng, oracle, cid):
    """The fp8 conv's epilogue: integer codes (the block-scaled MFMA is exact there), per-channel scale 2^-9 .. 2^-4, bias k / 4096,
    residual k / 1024 - acc * scale + bias + res is exact in float32 and wider than f16, rounded once."""
    c = D.build(cid)
    xc, wc = oracle.quantize_e4m3(c["xi"]), oracle.quantize_e4m3(c["wi"])
    got, _ = eng.op_conv2d_fp8(xc, wc, c["scale"], c["bias"], c["stride"], c["pad"], c["res"], c["act"])
    _same(got, cid)
    # ... and of the small-batch fp8 tiles (128 x 128: id 23, 64 x 64: id 24), which the entry point runs when tune.op_tile names them
    for name, tile in (("128x128_FP8", 23), ("64x64_FP8", 24)):
        got, _ = _forced(eng, {"op_tile": tile}, lambda: eng.op_conv2d_fp8(xc, wc, c["scale"], c["bias"], c["stride"], c["pad"], c["res"], c["act"]))
        assert eng.last_conv_forms() == [(tile, "PLAIN")]
        _same(got, cid, name)
