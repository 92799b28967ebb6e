"""-m gpu: the fp8 configuration pinned EXACTLY (yh_config.precision = YH_PRECISION_FP8; BASELINE.json configs[4]).
tests/test_gpu_fp8.py and tests/test_gpu_fp8_sweep.py take the engine's own scales as an input of their checker and carry a summation
bound; a wrong scale, one weight code off by a step or an epilogue that rounds an activation code the wrong way stay inside it. Every
piece below has an exact answer - a single f32 operation or an order-free maximum on f16-representable data - and is compared with
array_equal on bit patterns: the calibrated scales (the formula on the f16 tensors), absmax_channels_f16 on crafted data, the refusal of
an overflowed calibration, the E4M3 weight codes and row scales of all 19 layers, the E4M3 activation codes of every producing epilogue,
the decoding debug reader, and plan_fp8's write flags under yh_config.fp8_f16_layers. The reference is numpy plus oracle.quantize_e4m3 /
oracle.e4m3_decode_table; no oracle forward runs. The only tolerance in the file is the one-ulp bound of
tests/test_gpu_ops.py::test_conv_vs_oracle on the teacher-forced f16 convolutions of the fp8_f16_layers test.

Geometry: R50 at 160 pixels, two frames, seeded weights (as tests/test_gpu_fp8.py): pyramid levels 20, 10, 5, 3, 2 = 538 cells, 1076
rows at two frames (no multiple of the calibration kernel's rows per workgroup), all 19 E4M3 layers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TH = 0.005
S = 160
F32 = np.float32

L3 = [f"l3b{b}" for b in range(6)]
L4 = [f"l4b{b}" for b in range(3)]
GROUPS = {1: ["head_t"], 2: ["proto0", "proto1", "proto2", "proto3"], 4: ["p3", "p4", "p5", "p6", "p7"], 8: [n + "_b" for n in L3 + L4]}
ALL_LAYERS = GROUPS[8] + ["p5", "p6", "p7", "p4", "p3"] + GROUPS[1] + GROUPS[2]   # in execution order, as yh_fp8_layer_info lists them
PYR = ("p3", "p4", "p5", "p6", "p7")
# an E4M3 layer -> the named tensor(s) it reads (p6, p7, head_t, proto0 read slices of ONE allocation, the pyramid: its scales belong to it)
INPUT_OF = {**{n + "_b": (n + "_a",) for n in L3 + L4}, "p5": ("lat5",), "p4": ("lat4",), "p3": ("lat3",), "p6": PYR, "p7": PYR, "head_t": PYR,
            "proto0": PYR, "proto1": ("proto0",), "proto2": ("proto1",), "proto3": ("proto_up",)}
# a tensor -> the E4M3 layers that read it, i.e. whose channel scales are its allocation's
READERS = {}
for _l, _ts in INPUT_OF.items():
    for _t in _ts:
        READERS.setdefault(_t, []).append(_l)
# every named tensor that can have an E4M3 twin, in plan order (a twin exists where some E4M3 layer reads the tensor)
TWINS = [n + "_a" for n in L3 + L4] + ["lat5", "p5", "p6", "p7", "lat4", "p4", "lat3", "p3", "proto0", "proto1", "proto_up"]
# ... of which the production plan keeps these ONLY as E4M3 (every reader is an E4M3 layer); lat5 and lat4 are also read in f16, by the
# lateral below them (the top-down add), and exist in both forms (csrc/fp8.hip, plan_fp8)
Q_ONLY = [n for n in TWINS if n not in ("lat5", "lat4")]


def conv_index(layer):
    """Canonical conv index (the weight blob's order, csrc/weights.hip:build_conv_table) of an E4M3 layer of R50."""
    if layer[0] == "l":
        L, b = int(layer[1]), int(layer[3])
        first = 1
        for nb in (3, 4, 6, 3)[:L - 1]:
            first += 3 * nb + 1
        return first + (1 if b == 0 else 4 + 3 * (b - 1) + 1)
    return {"p5": 56, "p4": 57, "p3": 58, "p6": 59, "p7": 60, "proto0": 61, "proto1": 62, "proto2": 63, "proto3": 64, "head_t": 66}[layer]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def expected_scales(x, per_tensor=False):
    """csrc/fp8.hip, yh_fp8_calibrate, on the f16 tensor x [rows][C] (held as f32): every step one f32 operation."""
    m = np.abs(x).reshape(-1, x.shape[-1]).max(0).astype(F32)
    amax = m.max()
    a = np.full_like(m, amax) if per_tensor else np.maximum(F32(2) * m, amax * F32(0.0625)).astype(F32)
    return np.where(a > 0, a / F32(448), F32(1)).astype(F32), m, amax


def layer_input(tensors, layer, frames=slice(None)):
    """[rows][C]: the rows of every frame of the allocation the layer reads."""
    parts = [tensors[t][frames] for t in INPUT_OF[layer]]
    c = parts[0].shape[-1]
    return np.concatenate([p.reshape(p.shape[0], -1, c) for p in parts], axis=1).reshape(-1, c)


def expected_weights(oracle, w, s_c):
    """csrc/fp8.hip, refresh_fp8_scales: w [cout][k][k][cin] f32 (f16 values), s_c [cin] -> (codes [cout][k*k*cin], s_w [cout])."""
    cout = w.shape[0]
    t = (w.reshape(cout, -1, w.shape[-1]) * s_c.astype(F32)[None, None, :]).astype(F32).reshape(cout, -1)   # K index = tap * C + c
    aw = np.abs(t).max(1).astype(F32)
    sw = np.where(aw > 0, aw / F32(448), F32(1)).astype(F32)
    inv = (F32(1) / sw).astype(F32)
    codes = np.stack([oracle.quantize_e4m3(t[o], float(inv[o])) for o in range(cout)])
    return codes, sw


def expected_codes(oracle, x, s_c):
    """The producers' E4M3 write: e4m3((float)f16 value * (1 / s[channel])), one f32 division per channel, one f32 multiply per element."""
    inv = (F32(1) / s_c.astype(F32)).astype(F32)
    return oracle.quantize_e4m3((x.astype(F32) * inv).astype(F32), 1.0), (x.astype(F32) * inv).astype(F32)


def scales_of(eng, tensor):
    """The channel scales of the allocation `tensor` lies in: those of any E4M3 layer of this handle that reads it."""
    sc = dict(eng.fp8_channel_scales())
    for l in READERS[tensor]:
        if l in sc:
            return sc[l]
    raise AssertionError(f"{tensor} has an E4M3 twin but no E4M3 reader")


def twins_of(eng, frame=0):
    """{name: codes} of every named tensor whose E4M3 form the handle's plan writes (the others answer YH_ESTATE)."""
    import yolact_amd as ya
    out = {}
    for name in TWINS + ["c3", "c4", "c5", "proto2", "proto3", "l3b0_b", "l4b0_b", "head_t0", "proto"]:
        try:
            out[name] = eng.tensor_e4m3(name, frame)
        except ya.YhError as e:
            assert e.code == ya.capi.ESTATE and "E4M3" in str(e), (name, str(e))
    return out


def check_activation_codes(oracle, eng, frames=(0, 1)):
    """Item 5 on a debug_tensors = 1 handle: codes == e4m3(f16 value / s_c) for every tensor with a twin. Returns the names checked."""
    table = oracle.e4m3_decode_table()
    pos = np.sort(table[:0x7F].astype(np.float64))                  # 0 .. 448
    mids = (pos[1:] + pos[:-1]) / 2                                  # the rounding boundaries of |q|
    names = []
    for f in frames:
        tw = twins_of(eng, f)
        for name, codes in tw.items():
            assert name in TWINS, f"{name}: an E4M3 twin nobody reads"
            x = eng.tensor_frame(name, f)
            want, q = expected_codes(oracle, x, scales_of(eng, name))
            assert codes.shape == x.shape and x.any(), name
            assert np.array_equal(codes, want), (name, f, int((codes != want).sum()), codes.size)
            # the comparison proves something only if some element sits where a wrong rounding would show
            aq = np.abs(q.astype(np.float64)).ravel()
            j = np.clip(np.searchsorted(mids, aq), 1, len(mids) - 1)
            near = np.minimum(np.abs(aq - mids[j]) / mids[j], np.abs(aq - mids[j - 1]) / mids[j - 1])
            assert (aq >= 448.0).any() or (near <= 2.0 ** -8).any(), f"{name}: no element saturates or lies near a rounding boundary"
        names = list(tw)
    return names


@pytest.fixture(scope="module")
def ctx(built, oracle):
    """F: f16, production plan. Fd: f16, debug tensors. P: fp8, production plan, graph replay, calibrated on the two frames. D: fp8, debug
    tensors, P's scales. P0: P's plan without tune.dsfuse, P's scales.
    Why two f16 handles and P0: debug_tensors = 1 switches tune.dsfuse off (the projection shortcut of a stage's first block becomes a
    tensor again), and the fused form skips ONE f16 rounding by design - it is the one fusion that is not
    bit-identical to its separate launches. A debug handle's c2 .. c5 therefore differ from a production handle's by f16 rounding noise,
    in either precision; everything exact below compares handles with the same arithmetic."""
    import bench
    import yolact_amd as ya

    class Ctx:
        pass
    c = Ctx()
    c.ya = ya
    c.img = np.random.default_rng(8).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    c.F = ya.Engine(input_size=S, max_batch=2, use_graph=False, conf_thresh=TH)
    c.blob = c.F.generate_weights(seed=1)
    c.convs = bench.parse_blob(c.blob)
    c.F.load_weights(c.blob)
    names = sorted({t for ts in INPUT_OF.values() for t in ts} | {"c3", "c4", "c5"} | {n + s for n in L3 + L4 for s in ("_a", "_b")}
                   | {n for n in L3[:-1] + L4[:-1]})
    c.F.set_input(c.img[:1]); c.F.evaluate()
    c.f_one = {n: c.F.tensor(n) for n in names}                    # frame 0 evaluated alone
    c.F.set_input(c.img); c.F.evaluate()
    c.f = {n: c.F.tensor(n) for n in names}
    c.f_heads = [c.F.output(i) for i in range(4)]
    c.Fd = ya.Engine(input_size=S, max_batch=2, use_graph=False, debug_tensors=True, conf_thresh=TH)
    c.Fd.load_weights(c.blob); c.Fd.set_input(c.img); c.Fd.evaluate()
    c.fd = {n: c.Fd.tensor(n) for n in names}
    c.P = ya.Engine(input_size=S, max_batch=2, use_graph=True, precision=ya.PRECISION_FP8, conf_thresh=TH)
    c.P.load_weights(c.blob)
    c.P.set_input(c.img); c.P.fp8_calibrate(); c.P.evaluate()
    c.scales = c.P.fp8_channel_scales()
    c.p_heads = [c.P.output(i) for i in range(4)]
    c.D = ya.Engine(input_size=S, max_batch=2, use_graph=False, precision=ya.PRECISION_FP8, debug_tensors=True, conf_thresh=TH)
    c.D.load_weights(c.blob)
    for i, (_, v) in enumerate(c.scales):
        c.D.fp8_set_layer_scale(i, v)
    c.D.set_input(c.img); c.D.evaluate()
    c.P0 = ya.Engine(input_size=S, max_batch=2, use_graph=True, precision=ya.PRECISION_FP8, conf_thresh=TH, tune=dict(dsfuse=0))
    c.P0.load_weights(c.blob)
    for i, (_, v) in enumerate(c.scales):
        c.P0.fp8_set_layer_scale(i, v)
    c.P0.set_input(c.img); c.P0.evaluate()
    yield c
    for e in (c.F, c.Fd, c.P, c.D, c.P0):
        e.close()


def fp8_engine(ctx, **kw):
    kw.setdefault("use_graph", False)
    return ctx.ya.Engine(input_size=S, max_batch=2, precision=ctx.ya.PRECISION_FP8, conf_thresh=TH, **kw)


# ---- 1. calibration ------------------------------------------------------------------------------------------------------------------
def test_calibrated_scales_are_the_formula_on_the_f16_tensors(ctx):
    """s[c] = max(2 m_c, amax / 16) / 448 (1 where that is 0) of the tensors an f16 handle computes, bit for bit - which also pins
    csrc/fp8.hip's statement that the calibration forward IS the f16 forward (of a handle with the same plan: the fixture's note) - per
    channel and with fp8_per_tensor = 1 (a = amax)."""
    assert [n for n, _ in ctx.scales] == ALL_LAYERS and len(ALL_LAYERS) == 19
    floor_taken = False
    for name, got in ctx.scales:
        want, m, amax = expected_scales(layer_input(ctx.f, name))
        assert got.dtype == F32 and np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))
        floor_taken |= bool((m < amax / F32(32)).any())
    assert floor_taken, "no channel takes the amax / 16 floor: the max() of the formula is not exercised"
    T = fp8_engine(ctx, fp8_per_tensor=True)
    T.load_weights(ctx.blob); T.set_input(ctx.img); T.fp8_calibrate()
    for name, got in T.fp8_channel_scales():
        want, _, _ = expected_scales(layer_input(ctx.f, name), per_tensor=True)
        assert np.array_equal(bits(got), bits(want)), name
    T.close()


def test_calibration_reads_only_the_frames_last_set(ctx):
    """max_batch = 2: two frames evaluated, then ONE frame set and calibrated - the stale second image of every tensor does not count."""
    E = fp8_engine(ctx)
    E.load_weights(ctx.blob); E.set_input(ctx.img); E.fp8_calibrate(); E.evaluate()
    E.set_input(ctx.img[:1]); E.fp8_calibrate()
    differs = False
    for name, got in E.fp8_channel_scales():
        want, _, _ = expected_scales(layer_input(ctx.f_one, name))
        assert np.array_equal(bits(got), bits(want)), name
        differs |= not np.array_equal(bits(want), bits(expected_scales(layer_input(ctx.f, name))[0]))
    assert differs, "the second frame never holds a channel maximum: the test would pass with it counted"
    E.close()


# ---- 2. absmax_channels_f16 ------------------------------------------------------------------------------------------------------------
def crafted(rows, C, salt):
    """[rows][C] f16 bit patterns: the 65 536 patterns in a scrambled order (an odd multiplier permutes each run of 65 536 elements, and
    every run is shifted against the one before so that a pattern does not stay in one channel), NaN and Inf made finite; channel 1's
    maximum is negative (-65504), channel 2 holds only signed zeros and subnormals, channel 3 only -0."""
    i = np.arange(rows * C, dtype=np.uint64)
    p = ((i * 40503 + (i >> 16) * 12347 + 977 * salt) & 0xFFFF).astype(np.uint16).reshape(rows, C)
    p = np.where((p & 0x7C00) == 0x7C00, p & 0xBFFF, p).astype(np.uint16)
    p[rows // 2, 1] = 0xFBFF
    p[:, 2] &= 0x83FF
    p[:, 3] = 0x8000
    return p


def absmax_ref(p):
    return np.abs(p.view(np.float16).astype(F32)).max(0).astype(F32).view(np.uint32)


@pytest.mark.parametrize("C", [8, 64, 256, 512, 2048])
def test_absmax_channels_on_crafted_data(ctx, C):
    """Bit patterns against numpy: rows below, at and above one workgroup's row count, the calibration's own 1076, and more rows than
    one pass of the grid (1024 workgroups of 256 / (C / 8) rows)."""
    seen = set()
    for i, rows in enumerate((1, 7, 8, 9, 1076, 1024 * (256 // (C // 8)) + 3)):
        p = crafted(rows, C, i)
        seen |= set(np.unique(p).tolist())
        got = ctx.F.op_absmax_channels_f16(p)
        want = absmax_ref(p)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (C, rows, np.flatnonzero(got != want)[:8].tolist())
        assert want[1] == F32(65504).view(np.uint32) and want[3] == 0 and want[2] < F32(2.0 ** -14).view(np.uint32) and (rows < 1076 or want[2] > 0)
    assert len(seen) == 65536 - 2 * 1024, "not every finite f16 pattern was fed"


@pytest.mark.parametrize("C", [8, 64, 256, 512, 2048])
def test_absmax_channels_lets_nan_and_inf_win(ctx, C):
    """yh_fp8_calibrate refuses a forward that overflowed by testing !(max < 3e38): ONE NaN (quiet, negative or signalling), +Inf or
    -Inf in a channel, in the first, a middle or the last row, must come back as a pattern that fails that test; the neighbours stay
    exact. (The kernel used to keep `a > m ? a : m`, which drops a NaN: a channel with a NaN and no Inf calibrated from its finite values.)"""
    rows = 1076 if C < 2048 else 1027                              # (2048 channels: one row per workgroup, 1027 rows are two passes of the grid)
    base = crafted(rows, C, 5)
    want = absmax_ref(base)
    c0 = C // 2 + 1
    for r in (0, rows // 2 + 1, rows - 1):
        for pat in (0x7E00, 0xFE00, 0x7C01, 0x7C00, 0xFC00):
            p = base.copy()
            p[r, c0] = pat
            got = ctx.F.op_absmax_channels_f16(p)
            v = got.view(F32)[c0]
            assert not (v < F32(3.0e38)), (C, r, hex(pat), hex(int(got[c0])))
            assert (np.isinf(v) and v > 0) if pat in (0x7C00, 0xFC00) else np.isnan(v), (C, r, hex(pat), hex(int(got[c0])))
            others = np.arange(C) != c0
            assert np.array_equal(got[others], want[others]), (C, r, hex(pat))


def test_absmax_channels_rejects_what_its_launcher_rejects(ctx):
    for C in (12, 24, 4096):                                        # no multiple of 8; 256 % (C / 8) != 0; C / 8 > 256
        with pytest.raises(ctx.ya.YhError) as e:
            ctx.F.op_absmax_channels_f16(np.zeros((4, C), np.uint16))
        assert e.value.code == ctx.ya.capi.EINVAL


# ---- 3. calibration refusal ------------------------------------------------------------------------------------------------------------
def test_overflowed_calibration_is_refused_and_changes_nothing(ctx):
    """The blob with l3b0_a's weights (canonical conv 24, a 1x1 convolution) times 2^18 still loads - every weight stays a finite f16 -
    and the f16 forward then holds Inf in l3b0_a, the input of the E4M3 layer l3b0_b (asserted on an f16 handle first). On an fp8 handle
    loaded with that blob and given the scales calibrated for the good weights (a stored calibration), yh_fp8_calibrate must return
    YH_ESTATE naming the layer, and what the source promises for a failed calibration holds: the scales are unchanged and the next
    evaluate gives the same output bits as before the refused call. (u8 frames cannot overflow a network whose calibration succeeded,
    and re-loading weights discards the scales, so "calibrated, then overflowing" is reached through stored scales.)"""
    ya = ctx.ya
    bad = ctx.blob.copy()
    off = 16
    for i, (w, _) in enumerate(ctx.convs):                          # record layout: csrc/weights.hip:check_blob
        cout, kh, kw, cin = w.shape
        off += 16
        ne = cout * kh * kw * cin
        if i == conv_index("l3b0_b") - 1:
            assert (cout, kh, cin) == (256, 1, 512)
            wv = bad[off:off + 2 * ne].view(np.float16)
            wv[:] = (wv.astype(F32) * F32(2.0 ** 18)).astype(np.float16)
            assert np.isfinite(wv.astype(F32)).all()
        off += ((2 * ne + 15) & ~15) + ((4 * cout + 15) & ~15)
    assert off == bad.size and not np.array_equal(bad, ctx.blob)
    Fb = ya.Engine(input_size=S, max_batch=2, use_graph=False, debug_tensors=True, conf_thresh=TH)
    Fb.load_weights(bad); Fb.set_input(ctx.img); Fb.evaluate()
    assert np.isinf(Fb.tensor("l3b0_a")).any()
    Fb.close()
    E = fp8_engine(ctx, use_graph=True)
    E.load_weights(bad)
    for i, (_, v) in enumerate(ctx.scales):
        E.fp8_set_layer_scale(i, v)
    E.set_input(ctx.img); E.evaluate()
    before = [E.output(i).view(np.uint32).copy() for i in range(4)]
    with pytest.raises(ya.YhError) as e:
        E.fp8_calibrate()
    assert e.value.code == ya.capi.ESTATE and "l3b0_b" in str(e.value) and "overflowed" in str(e.value), str(e.value)
    for (n0, v0), (n1, v1) in zip(ctx.scales, E.fp8_channel_scales()):
        assert n0 == n1 and np.array_equal(bits(v0), bits(v1)), n0
    E.evaluate()
    for i in range(4):
        assert np.array_equal(E.output(i).view(np.uint32), before[i]), i
    E.close()


# ---- 4. weight codes and row scales ------------------------------------------------------------------------------------------------------
def test_weight_codes_and_row_scales_of_all_layers(ctx, oracle):
    """t = w * s_c (one f32 multiply, K index = tap * C + c), s_w = max_k |t| / 448, codes = e4m3(t * (1 / s_w)): all 19 layers, codes and
    scales as the kernels read them. Then the refresh by allocation: new scales for p6's input - the pyramid - change p6, p7, head_t and
    proto0 to their new expected codes and leave every other layer's bytes alone; re-loading the blob discards the scales (YH_ESTATE)
    and setting the stored ones again reproduces the codes and the heads."""
    ya = ctx.ya
    W = fp8_engine(ctx)
    W.load_weights(ctx.blob)
    with pytest.raises(ya.YhError) as e:
        W.fp8_weights(0)                                            # no scales yet
    assert e.value.code == ya.capi.ESTATE
    for i, (_, v) in enumerate(ctx.scales):
        W.fp8_set_layer_scale(i, v)
    first = {}
    for i, (name, s_c) in enumerate(ctx.scales):
        codes, sw = W.fp8_weights(i)
        w = ctx.convs[conv_index(name)][0]
        assert codes.shape == (w.shape[0], 9 * w.shape[3]) and w.shape[1] == 3, name
        want_codes, want_sw = expected_weights(oracle, w, s_c)
        assert np.array_equal(bits(sw), bits(want_sw)), (name, int((bits(sw) != bits(want_sw)).sum()))
        assert np.array_equal(codes, want_codes), (name, int((codes != want_codes).sum()), codes.size)
        assert (codes & 0x7F).max() == 0x7E                          # every row's maximum lands on +-448
        first[name] = (codes, sw)
        pc, ps = ctx.P.fp8_weights(i)                               # (the calibrating handle made the same bytes)
        assert np.array_equal(pc, codes) and np.array_equal(bits(ps), bits(sw)), name
    # partial refresh
    idx = {n: i for i, (n, _) in enumerate(ctx.scales)}
    s_new = (dict(ctx.scales)["p6"] * np.where(np.arange(256) % 2 == 0, F32(1.5), F32(0.8125))).astype(F32)
    W.fp8_set_layer_scale(idx["p6"], s_new)
    for name, i in idx.items():
        codes, sw = W.fp8_weights(i)
        if name in ("p6", "p7", "head_t", "proto0"):
            want_codes, want_sw = expected_weights(oracle, ctx.convs[conv_index(name)][0], s_new)
            assert np.array_equal(codes, want_codes) and np.array_equal(bits(sw), bits(want_sw)), name
            assert not np.array_equal(codes, first[name][0]), name
        else:
            assert np.array_equal(codes, first[name][0]) and np.array_equal(bits(sw), bits(first[name][1])), name
    # a re-load discards the scales; the stored ones bring everything back
    W.load_weights(ctx.blob)
    for i in range(len(ctx.scales)):
        with pytest.raises(ya.YhError) as e:
            W.fp8_weights(i)
        assert e.value.code == ya.capi.ESTATE
    for i, (_, v) in enumerate(ctx.scales):
        W.fp8_set_layer_scale(i, v)
    for name, i in idx.items():
        codes, sw = W.fp8_weights(i)
        assert np.array_equal(codes, first[name][0]) and np.array_equal(bits(sw), bits(first[name][1])), name
    W.set_input(ctx.img); W.evaluate()
    for i in range(4):
        assert np.array_equal(W.output(i), ctx.p_heads[i]), i
    W.close()


# ---- 5. activation codes -----------------------------------------------------------------------------------------------------------------
def test_activation_codes_are_the_quantiser_on_the_f16_value(ctx, oracle):
    """Every producing epilogue's E4M3 write (e4m3_pack4, not the e4m3_code the quantise op tests) against the f16 value the same
    launch wrote, on the debug_tensors = 1 handle: 1x1 f16 conv epilogues (l3b1_a: the expand + next-reduce launch or the plain conv,
    l4b0_a), the laterals, E4M3 convs writing E4M3 (proto0, p5), the stride-2 one (p6), the bilinear (proto_up), all pyramid levels."""
    names = check_activation_codes(oracle, ctx.D)
    assert sorted(names) == sorted(TWINS), sorted(set(TWINS) ^ set(names))
    for must in ("l3b1_a", "l4b0_a", "lat5", "proto0", "p5", "p6", "proto_up", "p3", "p4", "p7"):
        assert must in names, must
    with pytest.raises(ctx.ya.YhError) as e:
        ctx.Fd.tensor_e4m3("p3", 0)                                 # an f16 handle has no E4M3 form of anything
    assert e.value.code == ctx.ya.capi.ESTATE


# ---- 6. the production plan ---------------------------------------------------------------------------------------------------------------
def test_production_plan_writes_the_same_codes_and_the_reader_decodes_them(ctx, oracle):
    """P0 (fused launches, graph replay) against D (one launch per op, every tensor in both forms): the same codes in every tensor with a
    twin, in plan order, and the same heads - the fused forms (expand + next-reduce launch, upsample in the lateral's epilogue,
    prototype conv in proto3's) are bit-identical to the separate launches. For the tensors the production plan P holds only as E4M3,
    yh_debug_read_tensor (dequant_e4m3_f32, which every other fp8 test reads through) returns table[code] * s[channel] exactly; the two
    it holds in both forms are consistent (codes = the quantiser on the f16 form).
    P itself cannot be compared with D: tune.dsfuse legitimately skips one f16 rounding in c2 .. c5 (the fixture's note), so P's first
    E4M3 tensor in plan order, l3b0_a, already differs from D's (near zero by dozens of codes: a code step there is tiny). What P's
    l3b0_a must be is known exactly all the same: no E4M3 layer lies upstream of it, so it is the quantiser applied to the l3b0_a of the
    f16 handle with P's plan (F) - asserted here, with no tolerance."""
    table = oracle.e4m3_decode_table()
    for f in range(2):
        t0, td, tp = twins_of(ctx.P0, f), twins_of(ctx.D, f), twins_of(ctx.P, f)
        assert sorted(t0) == sorted(TWINS) == sorted(td) == sorted(tp)
        for name in TWINS:
            assert np.array_equal(t0[name], td[name]), (name, f, int((t0[name] != td[name]).sum()), "first tensor in plan order whose two forms disagree")
            got = ctx.P.tensor_frame(name, f)
            if name in Q_ONLY:
                want = (table[tp[name]] * scales_of(ctx.P, name).astype(F32)).astype(F32)
                assert not np.isnan(want).any() and np.array_equal(bits(got), bits(want)), (name, f)
            else:                                                   # both forms: the reader returns the f16 one
                assert np.array_equal(tp[name], expected_codes(oracle, got, scales_of(ctx.P, name))[0]), (name, f)
                assert np.array_equal(ctx.P0.tensor_frame(name, f), ctx.D.tensor_frame(name, f)), (name, f)
        assert np.array_equal(tp["l3b0_a"], expected_codes(oracle, ctx.f["l3b0_a"][f], scales_of(ctx.P, "l3b0_a"))[0]), f
        assert not np.array_equal(tp["l3b0_a"], td["l3b0_a"])       # (the docstring's statement; if this ever fails, compare P with D throughout)
    for i in range(4):
        assert np.array_equal(ctx.D.output(i), ctx.P0.output(i)), i


# ---- 7. yh_config.fp8_f16_layers ------------------------------------------------------------------------------------------------------------
def test_f16_layer_masks_remove_exactly_their_group(ctx):
    for mask, group in GROUPS.items():
        E = fp8_engine(ctx, fp8_f16_layers=mask)
        assert [n for n, _ in E.fp8_layers()] == [n for n in ALL_LAYERS if n not in group], mask
        E.close()


def test_no_e4m3_layer_left_is_the_f16_network(ctx):
    """fp8_f16_layers = 15: no E4M3 layer, nothing to calibrate - the handle is ready once its weights are loaded (it used to be refused
    with an empty list of missing layers), calibrating it is a harmless no-op, and its heads are the f16 handle's bit for bit."""
    E = fp8_engine(ctx, fp8_f16_layers=15, use_graph=True)
    assert E.fp8_layers() == []
    E.load_weights(ctx.blob); E.set_input(ctx.img)
    E.evaluate()
    for i in range(4):
        assert np.array_equal(E.output(i), ctx.f_heads[i]), ("before calibrating", i)
    E.fp8_calibrate()
    assert E.fp8_layers() == []
    E.evaluate()
    for i in range(4):
        assert np.array_equal(E.output(i), ctx.f_heads[i]), ("after calibrating", i)
    E.load_weights(ctx.blob); E.evaluate()                          # (a re-load leaves it ready too)
    assert np.array_equal(E.output(0), ctx.f_heads[0])
    E.close()


# one kept convolution per group: (output tensor, input tensor, stride)
KEPT = {1: [(f"head_t{l}", f"p{l + 3}", 1) for l in range(5)], 2: [("proto1", "proto0", 1)], 4: [("p6", "p5", 2)], 8: [("l4b1_b", "l4b1_a", 1)]}
KEPT_LAYER = {1: "head_t", 2: "proto1", 4: "p6", 8: "l4b1_b"}


@pytest.mark.parametrize("mask", [1, 2, 4, 8])
def test_kept_f16_layers_read_f16_and_the_rest_still_quantises_exactly(ctx, oracle, mask):
    """A debug_tensors = 1 handle with one group kept in f16, calibrated on the same frames: the remaining E4M3 twins are still the
    quantiser applied to the f16 value (item 5), and a kept convolution reads an f16 tensor its producer really wrote this step - its
    input is non-zero and its output is the f16 convolution of that input (teacher-forced; f32 accumulation on both sides, only the
    summation order differs: the one-ulp bound of tests/test_gpu_ops.py::test_conv_vs_oracle). Reading decoded E4M3 values instead, or a
    stale buffer, is a 6 % error. The production plan of the same mask (without tune.dsfuse: the fixture's note) gives the same heads.
    Mask 8: the backbone is the f16 debug handle's, bit for bit."""
    M = fp8_engine(ctx, fp8_f16_layers=mask, debug_tensors=True)
    M.load_weights(ctx.blob); M.set_input(ctx.img); M.fp8_calibrate(); M.evaluate()
    names = check_activation_codes(oracle, M)
    # (mask 1: the f16 head trunk was the only reader of p4 and p7 - p6 reads p5, p7 reads p6, proto0 reads p3 - so they lose their twins)
    gone = {1: ["p4", "p7"], 2: ["proto0", "proto1", "proto_up"], 4: ["lat5", "lat4", "lat3"], 8: [n + "_a" for n in L3 + L4]}[mask]
    assert sorted(names) == sorted(n for n in TWINS if n not in gone), mask
    w, b = ctx.convs[conv_index(KEPT_LAYER[mask])]
    for y_name, x_name, stride in KEPT[mask]:
        x, got = M.tensor(x_name), M.tensor(y_name)
        assert x.any() and got.any(), (x_name, y_name)
        want = oracle.conv2d(x, w, b, stride, 1, None, 1 if y_name != "p6" else 0, f16=True)
        tol = 2.0 ** -10 * np.maximum(np.abs(want), 1.0) + 1e-3
        assert got.shape == want.shape and (np.abs(got - want) <= tol).all(), (y_name, float(np.abs(got - want).max()))
    if mask == 8:
        for n in ["c3", "c4", "c5"] + [n + s for n in L3 + L4 for s in ("_a", "_b")] + L3[:-1] + L4[:-1]:
            assert np.array_equal(M.tensor(n), ctx.fd[n]), n
    Pm = fp8_engine(ctx, fp8_f16_layers=mask, use_graph=True, tune=dict(dsfuse=0))
    Pm.load_weights(ctx.blob)
    for i, (_, v) in enumerate(M.fp8_channel_scales()):
        Pm.fp8_set_layer_scale(i, v)
    Pm.set_input(ctx.img); Pm.evaluate()
    for i in range(4):
        assert np.array_equal(Pm.output(i), M.output(i)), (mask, i)
    if mask == 8:                                                   # ... and the production plan's backbone is the production f16 handle's
        Pf = fp8_engine(ctx, fp8_f16_layers=mask, use_graph=True)
        Pf.load_weights(ctx.blob)
        for i, (_, v) in enumerate(M.fp8_channel_scales()):
            Pf.fp8_set_layer_scale(i, v)
        Pf.set_input(ctx.img); Pf.evaluate()
        for n in ["c3", "c4", "c5"] + [n + s for n in L3 + L4 for s in ("_a", "_b")] + L3[:-1] + L4[:-1]:
            assert np.array_equal(Pf.tensor(n), ctx.f[n]), n
        Pf.close()
    Pm.close(); M.close()
