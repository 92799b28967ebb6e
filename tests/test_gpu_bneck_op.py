"""-m gpu: every bottleneck launch of csrc/bneck.hip - the eleven rows of kBneckChains by symbol, and bneck_xn_f16 - alone through
yh_op_bneck_f16 on the edge shapes of tests/bneck_cases.py, bit for bit against that module's numpy reference (three convolutions in
float64 with the f16 roundings in between; tests/test_bneck_cases.py ties it to the oracle and proves that integer data makes
every summation order exact). No tolerance anywhere: y, a_next and bneck_xn_f16's E4M3 codes are compared with np.array_equal.
The dyadic case of every form (operands on power-of-two grids, sums exact in float32 and far wider than f16) is compared the same
way: there b, y and a' are really rounded, so a chain that rounds in the wrong place or the wrong way fails it.
The op stages every output as all single-op entry points do (OpStaging, csrc/engine_ops.hip): 4096 guard bytes in front of it and 256
guard rows behind it, all 0xFF, YH_EOVERFLOW if the launch changed one; the output itself is filled with the same NaN pattern first,
so a row the kernel skipped shows as well; every input lies between bands of NaN.

The one real-valued case per form is held against the same three convolutions as three single-op launches on the streaming tiles
the chain = 0 plan gives these layers, forced with tune.op_tile: TILE_64x256_K1 (id 22) for the convolutions with 64 output
channels, TILE_128x128_K1 (id 21) for all others (its [3x3] form for the 128-plane conv_b, its two-source form for the first
block's expand conv); bneck_xn_f16's codes against op_quantize_e4m3 of the separate launches' a'."""
import numpy as np
import pytest

import bneck_cases as B

pytestmark = pytest.mark.gpu

TILE_128x128_K1, TILE_64x256_K1 = 21, 22
PARAMS = [(form, cid) for form in B.FORM_IDS for cid in B.case_ids(form)]


@pytest.fixture(scope="module")
def eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=2, use_graph=False)
    yield e
    e.close()


def _form(form):
    return B.FORMS[B.FORM_IDS.index(form)]


def _launch(eng, form, c, **over):
    sym, planes, tm, nxt, dual = _form(form)
    kw = dict(planes=planes, tile_m=tm, a=c["a"], w3=c["w3"], bias3=c["bias3"], res=c["res"], x2=c["x2"], stride2=c["stride2"])
    if not c["xn"]:
        kw.update(w2=c["w2"], bias2=c["bias2"], stride=c["stride"])
    if nxt:
        kw.update(w1n=c["w1n"], bias1n=c["bias1n"])
    if c["xn"]:
        kw.update(inv_scale=c["inv_scale"])
    kw.update(over)
    return eng.op_bneck(**kw)


_SEPARATE = {}


def _separate(eng, c):
    """The case's b -> y -> a' (-> codes) as single-op launches on the streaming tiles, once per (planes, case)."""
    key = (c["planes"], c["id"])
    if key in _SEPARATE:
        return _SEPARATE[key]
    small = TILE_64x256_K1 if c["planes"] == 64 else TILE_128x128_K1
    one = lambda w: w[:, None, None, :]

    def on(tile, fn, *args):
        eng.set_tuning(op_tile=tile)
        try:
            return fn(*args)
        finally:
            eng.reset_tuning("op_tile")
    b = c["a"] if c["xn"] else on(small, eng.op_conv2d, c["a"], c["w2"], c["bias2"], c["stride"], 1, None, 1)
    if c["x2"] is not None:
        y = on(TILE_128x128_K1, eng.op_conv2d_dual, b, c["x2"], c["stride2"], c["w3"], c["bias3"], 1)
    else:
        y = on(TILE_128x128_K1, eng.op_conv2d, b, one(c["w3"]), c["bias3"], 1, 0, c["res"], 1)
    an = on(small, eng.op_conv2d, y, one(c["w1n"]), c["bias1n"], 1, 0, None, 1)
    out = dict(y=y, a_next=an)
    if c["xn"]:
        bits = an.astype(np.float16).view(np.uint16)
        codes = np.zeros(an.shape, np.uint8)
        for v in np.unique(c["inv_scale"]):
            sel = c["inv_scale"] == v
            codes[..., sel] = eng.op_quantize_e4m3(bits, float(v))[..., sel]
        out["a_next8"] = codes
    _SEPARATE[key] = out
    return out


def _same(name, got, want, form, cid):
    print(f"{form} {cid} {name}: {int(np.count_nonzero(got != want))} of {want.size} elements differ")
    assert got.shape == want.shape and np.array_equal(got, want), (form, cid, name, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("form,cid", PARAMS, ids=[f"{f}-{c}" for f, c in PARAMS])
def test_form_on_case(eng, oracle, form, cid):
    import yolact_amd as ya
    sym, planes, tm, nxt, dual = _form(form)
    c = B.build(planes, cid)
    if c["gap"]:
        eng.set_tuning(op_xgap=c["gap"])
    try:
        if c["xn"] and c["gap"]:     # bneck_xn_f16 reads b as dense rows: there is no image stride to get wrong, the op refuses
            with pytest.raises(ya.YhError) as ei:
                _launch(eng, form, c)
            assert ei.value.code == ya.capi.EINVAL and "op_xgap" in str(ei.value)
            return
        out = _launch(eng, form, c)
    finally:
        if c["gap"]:
            eng.reset_tuning("op_xgap")
    want = _separate(eng, c) if c["real"] else B.reference(c, oracle)
    _same("y", out["y"], want["y"], form, cid)
    if nxt:
        _same("a_next", out["a_next"], want["a_next"], form, cid)
    else:
        assert out["a_next"] is None
    if c["xn"]:
        _same("a_next8", out["a_next8"], want["a_next8"], form, cid)


@pytest.mark.parametrize("which", ["f16_only", "e4m3_only"])
def test_xn_writes_either_output_alone(eng, oracle, which):
    """fill_xn_params asks for a' as f16, as E4M3 codes, or both (test_form_on_case): each alone, with the other pointer null."""
    c = B.build(256, "n3_7x11")
    want = B.reference(c, oracle)
    if which == "f16_only":
        out = _launch(eng, B.XN, c, inv_scale=None)
        assert out["a_next8"] is None
        _same("a_next", out["a_next"], want["a_next"], B.XN, c["id"])
    else:
        out = _launch(eng, B.XN, c, want_a_next=False)
        assert out["a_next"] is None
        _same("a_next8", out["a_next8"], want["a_next8"], B.XN, c["id"])
    _same("y", out["y"], want["y"], B.XN, c["id"])


REFUSALS = [
    ("planes_96", "bneck_chain_f16<64,64,next>", "7x9", dict(planes=96), {}),
    ("tile_m_32", "bneck_chain_f16<64,64,next>", "7x9", dict(tile_m=32), {}),
    ("tile_m_32_128_planes", "bneck_chain_f16<128,64>", "7x9", dict(tile_m=32), {}),
    ("no_256_pixel_tile_at_128_planes", "bneck_chain_f16<128,128,next>", "7x9", dict(tile_m=256), {}),
    ("dual_without_w1n", "bneck_chain_f16<64,128,next,dual>", "7x9_x2s1", dict(w1n=None, bias1n=None), {}),
    ("dual_with_res", "bneck_chain_f16<64,128,next,dual>", "7x9_x2s1", dict(res=np.zeros((1, 7, 9, 256), np.float32)), {}),
    ("dual_on_a_tile_without_that_form", "bneck_chain_f16<64,128,next,dual>", "7x9_x2s1", dict(tile_m=64), {}),
    ("x2_short_of_the_output_grid", "bneck_chain_f16<64,128,next,dual>", "7x9_x2s1", dict(stride2=2), {}),
    ("xn_without_res", B.XN, "7x9", dict(res=None), {}),
    ("xn_with_neither_output", B.XN, "7x9", dict(want_a_next=False, inv_scale=None), {}),
    ("xn_on_128_pixel_tiles", B.XN, "7x9", dict(tile_m=128), {}),
    ("chain_without_res_or_x2", "bneck_chain_f16<64,64>", "7x9", dict(res=None), {}),
    ("stride_3", "bneck_chain_f16<64,64>", "7x9", dict(stride=3), {}),
    ("op_xgap_12", "bneck_chain_f16<64,64,next>", "7x9", {}, dict(op_xgap=12)),
]


@pytest.mark.parametrize("name,form,cid,over,tune", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(eng, name, form, cid, over, tune):
    """YH_EINVAL with a message and no launch for what launch_bneck has no kernel for (the same call without the change runs:
    test_form_on_case)."""
    import yolact_amd as ya
    c = B.build(_form(form)[1], cid)
    if tune:
        eng.set_tuning(**tune)
    try:
        with pytest.raises(ya.YhError) as ei:
            _launch(eng, form, c, **over)
    finally:
        if tune:
            eng.reset_tuning(*tune)
    assert ei.value.code == ya.capi.EINVAL and "bneck op:" in str(ei.value), str(ei.value)
