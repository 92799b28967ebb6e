"""-m gpu: the conv kernels' row geometry - divisions by P * Q, Q and a level's width as multiply-high and shift (csrc/divmagic.h),
the dense 1x1 form whose source offset is m * C, the weight pieces issued ahead of the row arithmetic, the per-tile scalar guard
of the tanh / E4M3 epilogue - on every streaming tile, the 64 x 64 tile and the 256 x 256 tile, integer-exact against the
oracle's convolution (small integers: every product and partial sum is exact in f32, any summation order gives the same bits).

Shapes are the smallest that cross each boundary: 3 frames of 5 x 7 and of 9 x 9, so M (105, 243) is a multiple of no tile and
rows of two frames share a tile; pyramid levels 5, 3, 2, 1, 1 (all five level boundaries inside one tile).

Two test switches of the single-op conv entry points reach what a plain call cannot: tune.op_xgap stages every image with extra
elements (NaN) behind it - a non-dense image stride, which must NOT take the m * C form - and tune.op_tanh_from sets the first
tanh channel (inside, at the edge of, beyond a channel tile). The forms no single op expresses run through small engines, each
compared bit for bit with the engine form that does not use the kernel path under test: the upsampled residual (3 x 3 -> 5 x 5
and 18 x 18 -> 35 x 35, against bilinear + add: tune.upfuse = 0), the head (tanh from channel 255, non-dense output strides)
under two launch plans, a bottleneck chain and the expand + next-reduce launch on 64-pixel tiles against chain = 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# ConvTile ids (csrc/yh_internal.h)
K1_128, K1_64x256, K1_96, T64, T256 = 21, 22, 27, 16, 8
PLAIN_TILES = [K1_128, K1_64x256, T64, T256]
FRAMES = [(3, 5, 7), (3, 9, 9)]


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


@pytest.fixture(scope="module")
def eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=2, use_graph=False)
    yield e
    e.close()


def _forced(eng, tune, fn):
    eng.set_tuning(**tune)
    try:
        return fn()
    finally:
        eng.reset_tuning(*tune)


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


@pytest.mark.parametrize("n,h,w", FRAMES)
@pytest.mark.parametrize("tile", PLAIN_TILES)
@pytest.mark.parametrize("k,stride,pad", [(1, 1, 0),    # dense 1x1: the streaming tiles' m * C form
                                          (1, 2, 0),    # 1x1 whose rows are not the input's pixels: the general form
                                          (3, 1, 1), (3, 2, 1)])
def test_conv_rows_exact_on_integers(eng, oracle, tile, n, h, w, k, stride, pad):
    rng = np.random.default_rng(tile * 100 + h * 10 + k + stride)
    cin, cout = 128, 136                          # two k-steps per tap; a ragged channel tile on every tile width
    x, wt, b = _ints(rng, -3, 3, (n, h, w, cin)), _ints(rng, -2, 2, (cout, k, k, cin)), _ints(rng, -4, 4, cout)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    r = _ints(rng, -5, 5, (n, ho, wo, cout))
    y = _forced(eng, {"op_tile": tile}, lambda: eng.op_conv2d(x, wt, b, stride, pad, r, 1))
    assert np.array_equal(y, oracle.conv2d(x, wt, b, stride, pad, r, 1, f16=True))


@pytest.mark.parametrize("n,h,w", FRAMES)
@pytest.mark.parametrize("tile", PLAIN_TILES)
@pytest.mark.parametrize("xgap", [8, 200])
def test_1x1_with_a_non_dense_image_stride_exact_on_integers(eng, oracle, tile, n, h, w, xgap):
    """A 1x1, stride-1, unpadded conv whose input images lie xgap elements apart more than H * W * C (the gap holds NaN): row m's
    source is n * x_img_stride + rem * C, not m * C. The streaming tiles must take their general form - with the dense form's
    offsets every row of the second and third frame would read shifted data or the gap - and every tile must match the oracle."""
    rng = np.random.default_rng(tile + xgap + h)
    cin, cout = 128, 136
    x, wt, b = _ints(rng, -3, 3, (n, h, w, cin)), _ints(rng, -2, 2, (cout, 1, 1, cin)), _ints(rng, -4, 4, cout)
    yo = oracle.conv2d(x, wt, b, 1, 0, None, 1, f16=True)
    dense = _forced(eng, {"op_tile": tile}, lambda: eng.op_conv2d(x, wt, b, 1, 0, None, 1))
    gapped = _forced(eng, {"op_tile": tile, "op_xgap": xgap}, lambda: eng.op_conv2d(x, wt, b, 1, 0, None, 1))
    assert np.array_equal(dense, yo)
    assert np.array_equal(gapped, yo)


@pytest.mark.parametrize("tile", [K1_128, T256])
def test_3x3_with_a_non_dense_image_stride_exact_on_integers(eng, oracle, tile):
    rng = np.random.default_rng(tile)
    x, wt, b = _ints(rng, -3, 3, (3, 5, 7, 64)), _ints(rng, -2, 2, (136, 3, 3, 64)), _ints(rng, -4, 4, 136)
    y = _forced(eng, {"op_tile": tile, "op_xgap": 72}, lambda: eng.op_conv2d(x, wt, b, 1, 1, None, 0))
    assert np.array_equal(y, oracle.conv2d(x, wt, b, 1, 1, None, 0, f16=True))


_TANH_REF = {}


def _tanh_case(oracle):
    """x, w, bias in eighths / sixteenths (every sum exact) and the oracle's outputs without and with tanh on every channel."""
    if not _TANH_REF:
        rng = np.random.default_rng(17)
        x, wt = _ints(rng, -1, 1, (3, 5, 7, 64)) / 8, _ints(rng, -1, 1, (136, 1, 1, 64)) / 8
        b = _ints(rng, -4, 4, 136) / 16
        _TANH_REF.update(x=x, wt=wt, b=b, y0=oracle.conv2d(x, wt, b, 1, 0, None, 0, f16=True), y2=oracle.conv2d(x, wt, b, 1, 0, None, 2, f16=True))
    return _TANH_REF


# 136 output channels: one ragged 128-channel tile + 8, three 64-channel tiles, one 256-channel tile
@pytest.mark.parametrize("tanh_from", [5,      # inside the first tile and inside an 8-channel store group
                                       63, 64,  # last channel of / first channel after a 64-channel tile
                                       100,     # inside a tile
                                       127, 128,  # last channel of / first channel after the 128-channel tile
                                       130,     # inside the ragged last tile
                                       136])    # beyond every channel: no tanh at all
@pytest.mark.parametrize("tile", PLAIN_TILES)
def test_tanh_from_inside_at_the_edge_of_and_beyond_a_tile(eng, oracle, tile, tanh_from):
    """Channels below tanh_from equal the oracle's plain conv, channels from it on the oracle's tanh of it, bit for bit: the per-tile
    scalar guard may neither drop a tile's first / last tanh channel nor apply tanh to a tile below the boundary."""
    c = _tanh_case(oracle)
    y = _forced(eng, {"op_tile": tile, "op_tanh_from": tanh_from}, lambda: eng.op_conv2d(c["x"], c["wt"], c["b"], 1, 0, None, 2))
    want = np.where(np.arange(136) >= tanh_from, c["y2"], c["y0"])
    assert not np.array_equal(c["y0"], c["y2"])
    assert np.array_equal(y, want), np.nonzero((y != want).any(axis=(0, 1, 2)))[0]


@pytest.mark.parametrize("tile", PLAIN_TILES)
def test_tanh_on_every_channel_takes_the_guarded_epilogue(eng, oracle, tile):
    """act = 2 (tanh_from = 0: every tile holds tanh channels) takes the guarded branch, act = 0 the plain one: both equal the
    oracle's convolution with that activation bit for bit (eighths and sixteenths: every sum is exact)."""
    rng = np.random.default_rng(tile)
    x, wt = _ints(rng, -1, 1, (3, 5, 7, 64)) / 8, _ints(rng, -1, 1, (136, 1, 1, 64)) / 8
    b = _ints(rng, -4, 4, 136) / 16
    y0 = _forced(eng, {"op_tile": tile}, lambda: eng.op_conv2d(x, wt, b, 1, 0, None, 0))
    y2 = _forced(eng, {"op_tile": tile}, lambda: eng.op_conv2d(x, wt, b, 1, 0, None, 2))
    assert np.array_equal(y0, oracle.conv2d(x, wt, b, 1, 0, None, 0, f16=True))
    assert np.array_equal(y2, oracle.conv2d(x, wt, b, 1, 0, None, 2, f16=True))
    assert not np.array_equal(y0, y2)


@pytest.mark.parametrize("n,ho,wo", FRAMES)
@pytest.mark.parametrize("tile,kslices", [(K1_128, 0), (T64, 0), (T256, 0), (T64, 2)])
@pytest.mark.parametrize("stride2", [1, 2])
def test_two_source_rows_exact_on_integers(eng, oracle, tile, kslices, stride2, n, ho, wo):
    """The two-source form: the second tensor's rows are recomputed at the switch (stride2 = 1 and 2). kslices = 2 over
    1 + 3 k-steps: the second slice starts at k-step 2, inside the second source."""
    rng = np.random.default_rng(tile + stride2 + ho)
    c1, c2, cout = 64, 192, 136
    h2, w2 = (ho - 1) * stride2 + 1, (wo - 1) * stride2 + 1
    x1, x2 = _ints(rng, -3, 3, (n, ho, wo, c1)), _ints(rng, -3, 3, (n, h2, w2, c2))
    wt, b = _ints(rng, -2, 2, (cout, c1 + c2)), _ints(rng, -4, 4, cout)
    env = {"op_tile": tile}
    if kslices: env.update(op_kslices=kslices)
    y = _forced(eng, env, lambda: eng.op_conv2d_dual(x1, x2, stride2, wt, b, act=1))
    cat = np.concatenate([x1, x2[:, ::stride2, ::stride2]], axis=-1)
    assert np.array_equal(y, oracle.conv2d(cat, wt.reshape(cout, 1, 1, c1 + c2), b, 1, 0, None, 1, f16=True))


@pytest.mark.parametrize("tile,cout", [(K1_128, 136), (K1_96, 95), (T64, 136), (T256, 136)])
@pytest.mark.parametrize("k", [1, 3])
def test_five_levels_exact_on_integers(eng, oracle, tile, cout, k):
    """Five pyramid levels of 5^2, 3^2, 2^2, 1^2, 1^2 cells in 3 frames: each level equals the oracle's conv of that level alone."""
    rng = np.random.default_rng(tile + k)
    sizes, n, cin = [5, 3, 2, 1, 1], 3, 64
    cells = sum(s * s for s in sizes)
    x, wt, b = _ints(rng, -3, 3, (n, cells, cin)), _ints(rng, -2, 2, (cout, k, k, cin)), _ints(rng, -4, 4, cout)
    y = _forced(eng, {"op_tile": tile}, lambda: eng.op_conv2d_levels(x, sizes, wt, b, act=1))
    off = 0
    for s_ in sizes:
        xl = x[:, off:off + s_ * s_].reshape(n, s_, s_, cin)
        yo = oracle.conv2d(xl, wt, b, 1, k // 2, None, 1, f16=True).reshape(n, s_ * s_, cout)
        assert np.array_equal(y[:, off:off + s_ * s_], yo), s_
        off += s_ * s_


def _engine_outputs(ya, S, n, img, tensors, **tune):
    e = ya.Engine(input_size=S, max_batch=n, use_graph=False, conf_thresh=0.005, tune=tune)
    e.load_weights(e.generate_weights(1))
    e.set_input(img)
    e.evaluate()
    names = [p["name"] for p in e.profile(with_tail=False, reps=1)]
    out = [e.tensor(t) for t in tensors] + [e.output(i) for i in range(4)]
    e.close()
    return names, out


@pytest.mark.parametrize("S,n,plan_cus", [(70, 3, -1), (70, 3, 1), (550, 1, 4)])
def test_upsampled_residual_is_bitwise_bilinear_plus_add(built, S, n, plan_cus):
    """Input 70: the FPN levels are 9, 5, 3 (lat4 adds 3 x 3 -> 5 x 5); input 550: 69, 35, 18 (lat4 adds 18 x 18 -> 35 x 35).
    plan_cus 1 / 4 plan as for a tiny chip, which sends the laterals down the streaming tile's upsampled-residual form."""
    import yolact_amd as ya
    img = np.random.default_rng(S).integers(0, 256, (n, S, S, 3), dtype=np.uint8)
    tune = {} if plan_cus < 0 else {"plan_cus": plan_cus}
    names, fused = _engine_outputs(ya, S, n, img, ("lat5", "lat4", "lat3", "p3"), upfuse=1, **tune)
    names0, plain = _engine_outputs(ya, S, n, img, ("lat5", "lat4", "lat3", "p3"), upfuse=0, **tune)
    if plan_cus > 0:   # the form this case is about: both laterals on the streaming tile (its upsampled-residual form)
        for lat in ("lat3", "lat4"):
            assert "conv_igemm_f16<128,128,2,2,0,1>:" + lat in names, [nm for nm in names if nm.endswith((":lat4", ":lat3"))]
    assert any(nm.startswith(("bilinear_f16:up", "bilinear2x_f16:up")) for nm in names0) and not any(":up" in nm for nm in names)
    for a, b in zip(fused, plain):
        assert np.array_equal(a, b)


def test_head_tanh_boundary_and_strided_outputs_under_two_plans(built):
    """The shared head writes 351 channels, tanh from channel 255 on, with a non-dense image stride (the levels of a frame laid end
    to end). Planned for a 2-CU chip with tune.chsplit it runs as a 256-channel launch (255: inside the tile) plus a 96-channel
    streaming launch from channel 256 (wholly tanh); without, as one launch of 128-channel tiles (tiles 0: beyond, 1: inside, 2:
    wholly tanh). All three tiles accumulate with the 16x16x32 MFMA in the same K order, so the plans are bit-compatible: the mask
    coefficients and every other head output must agree bit for bit."""
    import yolact_amd as ya
    S, n = 134, 2
    img = np.random.default_rng(5).integers(0, 256, (n, S, S, 3), dtype=np.uint8)
    na, a = _engine_outputs(ya, S, n, img, ("p3",), chsplit=1, plan_cus=2)
    nb, b = _engine_outputs(ya, S, n, img, ("p3",), chsplit=0, plan_cus=2)
    print([nm for nm in na + nb if "head_out" in nm])
    assert any(nm.endswith("/ch256-351") for nm in na) and not any("/ch" in nm for nm in nb)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert np.abs(a[3]).max() <= 1.0 and np.abs(a[3]).max() > 0.0      # output 2, the mask coefficients: tanh was applied


def test_chain_and_xn_on_64_pixel_tiles_equal_separate_launches(built):
    """One bottleneck chain and one expand + next-reduce launch on 64-pixel tiles (tune.chain bits 0, 1, 4), 2 frames of 134 x 134
    (34 x 34, 17 x 17 and 9 x 9 maps: M is a multiple of no tile): bit for bit the separate launches of chain = 0."""
    import yolact_amd as ya
    S, n = 134, 2
    img = np.random.default_rng(6).integers(0, 256, (n, S, S, 3), dtype=np.uint8)
    t = ("c2", "c3", "c4", "c5")
    names, fused = _engine_outputs(ya, S, n, img, t, chain=17 + 2)
    names0, plain = _engine_outputs(ya, S, n, img, t, chain=0)
    assert any(nm.startswith("bneck_chain_f16<64,64") for nm in names) and any(nm.startswith("bneck_xn_f16") for nm in names), names
    assert not any(nm.startswith("bneck_") for nm in names0)
    for a, b in zip(fused, plain):
        assert np.array_equal(a, b)
