"""-m gpu: the convolution path at the ends of f16's range, and what a non-finite value may and may not reach. The rest of the suite
stays inside the comfortable middle of f16 on purpose and compares float32 values, which cannot see the sign of a zero and never
accepts a NaN. Every comparison here is bits.same_bits: bit patterns, -0 != +0, NaN positions exact (sign and payload free).

  * the grid of tests/test_gpu_rounding.py - head_3x3 on every (tile, kslices), the multi-level forms, the two-source form, the
    default and two-launch plans, the 96-channel remainder, the stem with and without its output, the fp8 epilogue - on the cases
    of tests/range_cases.py: f16 subnormal x, subnormal w, subnormal outputs with normal operands, and overflow (outputs exactly
    on 65520, one grid step below, on 65504; a residual that alone carries the sum over; tanh of sums past +-65520, of +0 and of
    subnormals). tests/test_range_cases.py proves on the CPU that every float32 partial sum of these cases is exact, so the one
    rounding of the specification - ReLU first, then round to nearest even: +0 for a tiny negative sum, inf from 65520 on - is the
    only one, and that a kernel which flushes subnormal operands or results, saturates, rounds toward zero or applies ReLU to
    the rounded value differs;
  * the twelve bottleneck launches on their subnormal and overflow case: b and y reach inf in LDS, a' is inf, NaN -> 0 or finite
    exactly where three float64 convolutions say;
  * non-finite isolation: one whole image of every input replaced by NaN (E4M3: code 0x7F), first, middle and last - every case of
    tests/conv_form_cases.py, every form and multi-image shape of tests/bneck_cases.py, bilinear and max pool. The other images'
    outputs keep the bits of the unpoisoned reference: no tap, halo row, zero-weight column or row past M of a neighbouring image
    contributes, not even times zero. The poisoned image equals the oracle's output on the same input;
  * bilinear_f16, bilinear2x_f16 and maxpool3x3s2_f16 at 24 and 256 channels (the lane's t / c8 split with c8 = 3 and 32), and on
    inputs that mix +-0, +-subnormal, +-65504 and +-inf."""
import contextlib

import numpy as np
import pytest

import bneck_cases as B
import conv_form_cases as F
import dyadic_cases as D
import range_cases as R
from bits import same_bits
from test_gpu_bneck_op import _form, _launch
from test_gpu_conv_forms import _run
from test_gpu_conv_geometry import PLAIN_TILES
from test_gpu_ops import _DUAL_TILES, _TILES, _forced
from test_gpu_rounding import _DUAL, _HEAD, _conv, _levels, _tune

pytestmark = pytest.mark.gpu

FAMS = list(R.RANGE_FAMILIES)


@pytest.fixture(scope="module")
def eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=2, use_graph=False)
    yield e
    e.close()


def _same(got, vid, what="", oracle=None):
    same_bits(got, R.reference(vid, oracle), f"{vid} {what}")


# ---- the rounding grid on the range cases ----
@pytest.mark.parametrize("fam", FAMS + ["ovf_res"])
@pytest.mark.parametrize("tile,kslices", _HEAD)
def test_every_head_tile_plain_form(eng, tile, kslices, fam):
    vid = f"head_3x3/{fam}"
    c = R.build(vid)
    got = _forced(eng, _tune(_TILES, tile, kslices), lambda: _conv(eng, c))
    assert eng.last_conv_launches() == 1
    _same(got, vid, f"{tile}/{kslices}")


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("tile,kslices", _HEAD)
@pytest.mark.parametrize("k", [3, 1])
def test_every_head_tile_multilevel_form(eng, tile, kslices, k, fam):
    vid = f"levels_k{k}/{fam}"
    got = _forced(eng, _tune(_TILES, tile, kslices), lambda: _levels(eng, R.build(vid)))
    assert eng.last_conv_launches() == 1
    _same(got, vid, f"{tile}/{kslices}")


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("cid", ["big_64_256_k3", "big_256_512_k1", "big_64_351_k3", "deep_k2048"])
def test_default_plan(eng, cid, fam):
    vid = f"{cid}/{fam}"
    got = _conv(eng, R.build(vid))
    assert eng.last_conv_launches() == 1
    _same(got, vid)


@pytest.mark.parametrize("tile", [None] + PLAIN_TILES)
def test_tanh_of_overflowing_zero_and_subnormal_sums(eng, oracle, tile):
    """act = 2 with the first tanh channel inside a channel tile of every width: below it the plain rounding (inf, -0, subnormals),
    from it on oracle.spec_tanhf of the float32 sum - +-1 for sums past +-65520, +0 for a +0 sum, the subnormal itself."""
    vid = "big_256_512_k1/ovf_tanh"
    c = R.build(vid)
    tune = {"op_tanh_from": R.TANH_FROM}
    if tile is not None:
        tune["op_tile"] = tile
    got = _forced(eng, tune, lambda: _conv(eng, c))
    assert eng.last_conv_launches() == 1
    _same(got, vid, f"tile {tile}", oracle)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("cid", ["split_64_256_k3", "split_512_351_k1"])
def test_two_launch_plans(eng, cid, fam):
    vid = f"{cid}/{fam}"
    c = R.build(vid)
    single = _conv(eng, c)
    assert eng.last_conv_launches() == 1
    eng.set_tuning(plan_cus=4)
    try:
        split = _conv(eng, c)
        assert eng.last_conv_launches() == 2          # the plan under test was really taken
    finally:
        eng.reset_tuning("plan_cus")
    _same(split, vid, "split")
    _same(single, vid, "single")


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("chsplit", [1, 2])
def test_head_remainder_on_96_channel_tiles(eng, chsplit, fam):
    vid = f"rem96_k3/{fam}"
    eng.set_tuning(plan_cus=4, chsplit=chsplit)
    try:
        got = _levels(eng, R.build(vid))
        assert eng.last_conv_launches() == 2
    finally:
        eng.reset_tuning("plan_cus", "chsplit")
    _same(got, vid, f"chsplit {chsplit}")


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("tile,kslices", _DUAL)
def test_dual_source(eng, tile, kslices, fam):
    vid = f"dual_s2/{fam}"
    c = R.build(vid)
    got = _forced(eng, _tune(_DUAL_TILES, tile, kslices), lambda: eng.op_conv2d_dual(c["x1"], c["x2"], c["stride2"], c["w"], c["bias"], act=c["act"]))
    assert eng.last_conv_launches() == 1
    _same(got, vid, f"{tile}/{kslices}")


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("cid", ["stem_n2_S30", "stem_n1_S34"])
def test_stem_pool(eng, oracle, cid, fam):
    """stem_pool_f16: a tiny negative sum is +0 (ReLU, then the rounding), 65520 is inf; the pool is the oracle's pool of the
    reference stem, with and without the stem output."""
    vid = f"{cid}/{fam}"
    c = R.build(vid)
    stem, pool = eng.op_stem_pool(c["x"], c["w"], c["bias"])
    _same(stem, vid, "stem")
    want_pool = oracle.maxpool3x3s2(R.reference(vid))
    same_bits(pool, want_pool, f"{vid} pool")
    none, pool2 = eng.op_stem_pool(c["x"], c["w"], c["bias"], want_stem=False)
    assert none is None
    same_bits(pool2, want_pool, f"{vid} pool alone")


@pytest.mark.parametrize("fam", ["sub_out", "ovf"])
@pytest.mark.parametrize("cid", D.FP8_IDS)
def test_fp8_epilogue(eng, oracle, cid, fam):
    """The fp8 conv's epilogue with the whole power of two on the per-channel scale: fma(acc, scale, bias) + res lands on the
    subnormal grid / past 65504."""
    vid = f"{cid}/{fam}"
    c = R.build(vid)
    xc, wc = oracle.quantize_e4m3(c["xi"]), oracle.quantize_e4m3(c["wi"])
    got, _ = eng.op_conv2d_fp8(xc, wc, c["scale"], c["bias"], c["stride"], c["pad"], c["res"], c["act"])
    _same(got, vid)
    for name, tile in (("128x128_FP8", 23), ("64x64_FP8", 24)):
        got, _ = _forced(eng, {"op_tile": tile}, lambda: eng.op_conv2d_fp8(xc, wc, c["scale"], c["bias"], c["stride"], c["pad"], c["res"], c["act"]))
        assert eng.last_conv_forms() == [(tile, "PLAIN")]
        _same(got, vid, name)


# ---- the twelve bottleneck launches ----
@pytest.mark.parametrize("fam", R.CHAIN_FAMILIES)
@pytest.mark.parametrize("form", B.FORM_IDS)
def test_bneck_form_on_range_case(eng, oracle, form, fam):
    sym, planes, tm, nxt, dual = _form(form)
    c = R.chain_build(form, fam)
    want = R.chain_reference(form, fam, oracle)
    out = _launch(eng, form, c)
    same_bits(out["y"], want["y"], f"{form} {fam} y")
    if nxt:
        same_bits(out["a_next"], want["a_next"], f"{form} {fam} a_next")
    else:
        assert out["a_next"] is None
    if c["xn"]:
        d = out["a_next8"] != want["a_next8"]
        print(f"{form} {fam} a_next8: {int(d.sum())} of {d.size} codes differ")
        assert not d.any(), np.argwhere(d)[:4].tolist()


# ---- non-finite isolation ----
def _images(n):
    return [0, n - 1] if n == 2 else [0, 1, n - 1]


@contextlib.contextmanager
def _tensors(cid, t):
    """conv_form_cases with this case's tensors replaced: its reference() and the GPU test's _run() both read build(cid)."""
    build, cached = F.build, F._REF.pop(cid, None)
    F.build = lambda i: t if i == cid else build(i)
    try:
        yield
    finally:
        F.build = build
        F._REF.pop(cid, None)
        if cached is not None:
            F._REF[cid] = cached


def _poisoned(t, img, keys):
    out = dict(t)
    for k in keys:
        if t.get(k) is not None:
            v = np.array(t[k], np.float32)
            v[img] = np.nan
            out[k] = v
    return out


@pytest.mark.parametrize("cid", [i for i in F.CASE_IDS if F.build(i)[("x1" if F.CASES[i]["kind"] == "dual" else "x")].shape[0] >= 2])
def test_conv_case_with_one_image_of_nan(eng, oracle, cid):
    """Every (tile, form) instance with one whole image of x, x1 / x2, res, res_lo NaN (fp8 kinds: the NaN code 0x7F): the other
    images keep the unpoisoned reference's bits, the poisoned one is the oracle's on the same input (NaN, or 0 behind a ReLU)."""
    c, t = F.CASES[cid], F.build(cid)
    clean = F.reference(cid, oracle)
    n = clean.shape[0]
    assert oracle.quantize_e4m3(np.array([np.nan], np.float32))[0] == 0x7F
    for img in _images(n):
        with _tensors(cid, _poisoned(t, img, ("x", "x1", "x2", "res", "res_lo"))):
            want = F.reference(cid, oracle)
            got = _forced(eng, F.tuning(cid), lambda: _run(eng, oracle, cid))
        assert eng.last_conv_forms() == F.expected_kernels(cid) and eng.last_conv_launches() == 1
        got = got.reshape(clean.shape)
        others = [i for i in range(n) if i != img]
        same_bits(got[others], clean[others], f"{cid} image {img} NaN: the other images")
        same_bits(got[img], want[img], f"{cid} image {img} NaN: the image itself")


_BNECK_NAN = [(form, cid) for form in B.FORM_IDS for cid in B.case_ids(form)
              if not cid.startswith(B.REAL) and B.build(_form(form)[1], cid)["n"] >= 2 and not (_form(form)[1] == 256 and B.build(256, cid)["gap"])]


@pytest.mark.parametrize("form,cid", _BNECK_NAN, ids=[f"{f}-{c}" for f, c in _BNECK_NAN])
def test_bneck_case_with_one_image_of_nan(eng, oracle, form, cid):
    """... and every bottleneck launch on its multi-image shapes (the gap case: NaN behind every image as well): a, res, x2."""
    sym, planes, tm, nxt, dual = _form(form)
    c = B.build(planes, cid)
    clean = B.reference(c, oracle)
    for img in _images(c["n"]):
        p = _poisoned(c, img, ("a", "res", "x2"))
        _, (b, y, an) = R.chain_stages(p)
        if c["gap"]:
            eng.set_tuning(op_xgap=c["gap"])
        try:
            out = _launch(eng, form, p)
        finally:
            if c["gap"]:
                eng.reset_tuning("op_xgap")
        others = [i for i in range(c["n"]) if i != img]
        pairs = [("y", y)] + ([("a_next", an)] if nxt else [])
        for name, want in pairs:
            same_bits(out[name][others], clean[name][others], f"{form} {cid} image {img} NaN: {name} of the other images")
            same_bits(out[name][img], want[img], f"{form} {cid} image {img} NaN: {name} of the image itself")
        if c["xn"]:
            want8 = oracle.quantize_e4m3(an * c["inv_scale"])
            assert np.array_equal(out["a_next8"][others], clean["a_next8"][others]) and np.array_equal(out["a_next8"][img], want8[img])


# ---- element-wise kernels ----
_BIL = [(2, 2, 4, 4), (5, 7, 9, 13), (6, 10, 12, 20)]          # bilinear2x_f16 (all border), bilinear_f16, bilinear2x_f16 with an interior
_POOL = [(7, 9), (12, 12)]
_ENDS = np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, -(2.0 ** -15), 2.0 ** -14, 65504.0, -65504.0, np.inf, -np.inf, 1.0, -1.5, 1024.0],
                 np.float32)


def _normal(seed, shape):
    return np.random.default_rng(seed).normal(0, 2, shape).astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("c", [24, 256])
@pytest.mark.parametrize("h,w,ho,wo", _BIL)
def test_bilinear_bit_exact_at_other_channel_counts(eng, oracle, h, w, ho, wo, c):
    x = _normal(h + c, (3, h, w, c))
    same_bits(eng.op_bilinear(x, ho, wo), oracle.bilinear(x, ho, wo, f16=True), f"bilinear {h}x{w} c{c}")


@pytest.mark.parametrize("c", [24, 256])
@pytest.mark.parametrize("h,w", _POOL)
def test_maxpool_bit_exact_at_other_channel_counts(eng, oracle, h, w, c):
    x = _normal(w + c, (3, h, w, c))
    same_bits(eng.op_maxpool(x), oracle.maxpool3x3s2(x), f"maxpool {h}x{w} c{c}")


@pytest.mark.parametrize("c", [24, 64, 256])
@pytest.mark.parametrize("h,w,ho,wo", _BIL)
def test_bilinear_with_one_image_of_nan(eng, oracle, h, w, ho, wo, c):
    x = _normal(h + c, (3, h, w, c))
    clean = oracle.bilinear(x, ho, wo, f16=True)
    for img in _images(3):
        xp = x.copy()
        xp[img] = np.nan
        got = eng.op_bilinear(xp, ho, wo)
        others = [i for i in range(3) if i != img]
        same_bits(got[others], clean[others], f"bilinear {h}x{w} c{c} image {img} NaN: the other images")
        same_bits(got[img], oracle.bilinear(xp, ho, wo, f16=True)[img], f"bilinear {h}x{w} c{c} image {img} NaN: the image itself")
        assert np.isnan(got[img]).all()


@pytest.mark.parametrize("c", [24, 64, 256])
@pytest.mark.parametrize("h,w", _POOL)
def test_maxpool_with_one_image_of_nan(eng, oracle, h, w, c):
    x = _normal(w + c, (3, h, w, c))
    clean = oracle.maxpool3x3s2(x)
    for img in _images(3):
        xp = x.copy()
        xp[img] = np.nan
        got = eng.op_maxpool(xp)
        others = [i for i in range(3) if i != img]
        same_bits(got[others], clean[others], f"maxpool {h}x{w} c{c} image {img} NaN: the other images")
        same_bits(got[img], oracle.maxpool3x3s2(xp)[img], f"maxpool {h}x{w} c{c} image {img} NaN: the image itself")


@pytest.mark.parametrize("c", [24, 64])
@pytest.mark.parametrize("h,w,ho,wo", _BIL)
def test_bilinear_on_range_ends(eng, oracle, h, w, ho, wo, c):
    """+-0, +-subnormal, +-65504, +-inf mixed: sums that overflow, inf - inf and 0 * inf (a clamped border weight) are NaN where the
    oracle's are, subnormal results are kept, zeros keep their sign."""
    x = np.random.default_rng(h * c).choice(_ENDS, (3, h, w, c))
    want = oracle.bilinear(x, ho, wo, f16=True)
    assert np.isnan(want).any() and np.isinf(want).any() and ((want != 0) & (np.abs(want) < 2.0 ** -14)).any()
    same_bits(eng.op_bilinear(x, ho, wo), want, f"bilinear {h}x{w} c{c} range ends")


@pytest.mark.parametrize("c", [24, 64])
@pytest.mark.parametrize("h,w", _POOL)
def test_maxpool_on_range_ends(eng, oracle, h, w, c):
    x = np.random.default_rng(w * c).choice(_ENDS, (3, h, w, c))
    x[1, :3, :3] = np.random.default_rng(c).choice(_ENDS[[0, 1, 3, 5, 10]], (3, 3, c))       # windows whose maximum is a zero, or negative
    x[2, -3:, -3:] = -np.inf
    want = oracle.maxpool3x3s2(x)
    assert np.isinf(want).any() and (want == 0).any() and (want == -np.inf).any()
    same_bits(eng.op_maxpool(x), want, f"maxpool {h}x{w} c{c} range ends")
