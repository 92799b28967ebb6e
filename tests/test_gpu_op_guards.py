"""-m gpu: the single-op entry points leave memory outside their outputs alone, and read nothing outside their inputs that reaches a
result. Every entry point stages each output between guards of 0xFF (4096 bytes in front, 256 rows behind row M - 1) and each input
between 4096-byte bands of NaN, and answers YH_EOVERFLOW - a YhError here - when a launch changed a guard byte (DESIGN.md section 5,
Bounds). So a case passes when the call returns (guards intact) AND the output equals the CPU oracle bit for bit (nothing outside an
input was read into it): integer data, every float32 sum exact, no tolerance anywhere.

  * the check checks: yh_debug_guard_selfcheck changes one guard byte by a copy, at each end of each guard, and must be caught;
  * every (tile, form) of the compiled conv table at the row and channel counts where its store guards decide something - the cases
    of tests/op_guard_cases.py, generated from the table's own R and T - and the proof that it was that instance which ran;
  * the resize, pool, stem, quantise and absmax kernels at their smallest and their ragged shapes."""
import time

import numpy as np
import pytest

import conv_form_cases as F
import op_guard_cases as G
from test_gpu_ops import _forced, eng, f16  # noqa: F401  (the module's engine fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(built):
    from yolact_amd import capi
    return {r["tile"]: r for r in capi.conv_forms()}


# ---- the check of the checker

@pytest.mark.parametrize("where,side,byte", [(1, "front", 4095), (2, "back", 0), (3, "back", 256 * 64 * 2 - 1), (4, "front", 0)])
def test_selfcheck_catches_one_changed_byte_at_each_end_of_each_guard(eng, built, where, side, byte):
    """3 rows x 64 f16 staged as an output: 4096 bytes in front, 256 rows of 128 bytes behind. One byte changed by hipMemcpy."""
    ya = built
    eng.guard_selfcheck(0)                               # nothing changed: YH_OK
    with pytest.raises(ya.YhError) as ei:
        eng.guard_selfcheck(where)
    msg = str(ei.value)
    assert ei.value.code == ya.capi.EOVERFLOW, msg
    assert "guard selfcheck: stored" in msg and f"y {side} guard, byte {byte} " in msg and "is 0x00" in msg, msg
    if side == "back":
        assert "y rows past M" in msg and f"(row M + {byte // 128})" in msg, msg
    else:
        assert "in front of y" in msg and f"({4096 - byte} in front of the payload)" in msg, msg
    eng.guard_selfcheck(0)                               # ... and the handle is as it was


def test_selfcheck_refuses_other_positions(eng, built):
    for where in (-1, 5):
        with pytest.raises(built.YhError) as ei:
            eng.guard_selfcheck(where)
        assert ei.value.code == built.capi.EINVAL


# ---- every (tile, form) at its tile boundaries

def _codes(oracle, a):
    return oracle.quantize_e4m3(a)


def _run(eng, oracle, c, t):
    kind, act = c["kind"], c["act"]
    if kind == "conv":
        return eng.op_conv2d(t["x"], t["w"], t["bias"], 1, c["k"] // 2, t.get("res"), act)
    if kind == "fp8":
        return eng.op_conv2d_fp8(_codes(oracle, t["x"]), _codes(oracle, t["w"]), t["scale"], t["bias"], 1, c["k"] // 2, t.get("res"), act)[0]
    if kind == "levels":
        return eng.op_conv2d_levels(t["x"], c["levels"], t["w"], t["bias"], act=act)
    if kind == "levels_fp8":
        return eng.op_conv2d_levels_fp8(_codes(oracle, t["x"]), c["levels"], _codes(oracle, t["w"]), t["scale"], t["bias"], act=act)
    if kind == "dual":
        return eng.op_conv2d_dual(t["x"], t["x2"], c["stride2"], t["w"], t["bias"], act=act)
    if kind == "resup":
        return eng.op_conv2d_resup(t["x"], t["w"], t["bias"], t["res_lo"], act=act)
    if kind == "tail":
        return eng.op_conv2d_tail(t["x"], t["w"], t["bias"], t["w2"], t["bias2"], act=act)
    assert kind == "tail_fp8"
    return eng.op_conv2d_tail(_codes(oracle, t["x"]), _codes(oracle, t["w"]), t["bias"], t["w2"], t["bias2"], act=act, scale=t["scale"])


@pytest.mark.parametrize("tile", sorted(F.TILES, key=F.TILES.get))
def test_tile_boundaries_guards_intact_and_bits_are_the_oracles(eng, oracle, table, tile):
    """All cases of one tile (op_guard_cases.cases_of): each returns - no guard byte of its output changed, no byte of the split-K
    workspace behind the last slice - equals the oracle bit for bit, and ran as the (tile, form) it is a case for; together they
    reach every form the table lists for the tile, and the R + 1 rows case of every form is among them."""
    row = table[F.TILES[tile]]
    assert (row["tch"], row["fp8"]) == (F.TILE_CH[tile], tile.endswith("FP8"))
    cases = G.cases_of(row)
    reached, t0 = set(), time.time()
    for c in cases:
        t = G.build(c)
        want = G.reference(c, t, oracle)
        got = _forced(eng, G.tuning(c), lambda: _run(eng, oracle, c, t))       # (a changed guard byte raises YhError: YH_EOVERFLOW)
        ran = eng.last_conv_forms()
        expect = [(c["tile"], c["form"])] * eng.last_conv_launches() + ([(-1, "REDUCE")] if c["kslices"] else [])
        assert ran == expect, (c["id"], ran)
        diff = got.reshape(want.shape) != want
        assert got.size == want.size and not diff.any(), (c["id"], int(np.count_nonzero(diff)), np.argwhere(diff)[:4].tolist())
        reached.add(c["form"])
    print(f"{tile}: {len(cases)} cases, {time.time() - t0:.2f} s")
    assert reached == set(row["forms"]), (tile, reached)
    for form in row["forms"]:
        if form not in ("ML", "ML_SPLITK", "K3"):      # (their rows are level cells and a 5 x 7 grid)
            assert any(c["form"] == form and c["n"] == 1 and c["h"] == row["tm"] + 1 for c in cases), (tile, form, "no R + 1 case")


def test_the_tiles_are_the_tables(table):
    """The parametrisation above names every row of the compiled table (tests/test_conv_form_cases.py holds conv_form_cases' mirror
    against it on the CPU), so the (tile, form) pairs the tile tests reach are exactly the table's."""
    assert sorted(F.TILES.values()) == sorted(table)
    assert sum(len(r["forms"]) for r in table.values()) == len({(c["tile"], c["form"]) for r in table.values() for c in G.cases_of(r)})


# ---- resize, pool, stem, quantise, absmax

def _same_bits(got, want, what):
    diff = ~((got == want) | (np.isnan(got) & np.isnan(want))) if got.dtype.kind == "f" else got != want
    print(f"{what}: {int(np.count_nonzero(diff))} of {want.size} elements differ")
    assert got.shape == want.shape and not diff.any(), (what, np.argwhere(diff)[:4].tolist(), got[diff][:4].tolist(), want[diff][:4].tolist())


@pytest.mark.parametrize("c", [8, 64, 72])
@pytest.mark.parametrize("h,w,ho,wo", [(1, 1, 2, 2), (3, 1, 6, 2), (5, 7, 9, 13), (2, 2, 5, 3)])
def test_bilinear_guards_and_bits(eng, oracle, h, w, ho, wo, c):
    x = f16(np.random.default_rng(h * 100 + c).normal(0, 2, (2, h, w, c)))
    _same_bits(eng.op_bilinear(x, ho, wo), oracle.bilinear(x, ho, wo, f16=True), f"bilinear {h}x{w} -> {ho}x{wo} c{c}")


@pytest.mark.parametrize("c", [8, 64, 72])
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (7, 9), (8, 8)])
def test_maxpool_guards_and_bits(eng, oracle, h, w, c):
    x = f16(np.random.default_rng(h * 100 + c).normal(0, 2, (2, h, w, c)))
    _same_bits(eng.op_maxpool(x), oracle.maxpool3x3s2(x), f"maxpool {h}x{w} c{c}")


@pytest.mark.parametrize("S", [8, 16, 18, 30, 34])
def test_stem_pool_guards_and_bits(eng, oracle, S):
    """Two images; with and without the stem output (without: the launch may not write the staged stem buffer's guards either).
    f16 form: small integers, every sum exact. rgb8 form: the loader normalises, (v - mean) / std rounded to f16, so the data are no
    integers - the weights then have ONE non-zero tap per output channel, +-2^e, at a position that moves over all 7 x 7 x 3 with the
    channel: the accumulator is one exact product, acc + bias (an integer) is exact in float32, and the f16 rounding is the only one."""
    rng = np.random.default_rng(S)
    b = rng.integers(-30, 31, 64).astype(np.float32)
    x = rng.integers(-4, 5, (2, S, S, 3)).astype(np.float32)
    wt = rng.integers(-3, 4, (64, 7, 7, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    mean, sd = np.array([123.68, 116.78, 103.94], np.float32), np.array([58.40, 57.12, 57.38], np.float32)
    xn = ((rgb.astype(np.float32) - mean) / sd).astype(np.float16).astype(np.float32)
    w1 = np.zeros((64, 147), np.float32)
    w1[np.arange(64), (np.arange(64) * 37 + S) % 147] = np.where(np.arange(64) % 2, -1.0, 1.0) * 2.0 ** (np.arange(64) % 4 - 1)
    w1 = w1.reshape(64, 7, 7, 3)
    for run, src, ref_x, w in ((eng.op_stem_pool, x, x, wt), (eng.op_stem_pool_rgb8, rgb, xn, w1)):
        so = oracle.conv2d(ref_x, w, b, 2, 3, None, 1, f16=True)
        po = oracle.maxpool3x3s2(so)
        stem, pool = run(src, w, b)
        assert np.count_nonzero(so) > so.size // 8
        _same_bits(stem, so, f"{run.__name__} S {S}: stem")
        _same_bits(pool, po, f"{run.__name__} S {S}: pool")
        none, pool2 = run(src, w, b, want_stem=False)
        assert none is None
        _same_bits(pool2, po, f"{run.__name__} S {S}: pool alone")


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_quantize_guards_and_bits(eng, oracle, n):
    x = f16(np.random.default_rng(n).normal(0, 40, n))
    got = eng.op_quantize_e4m3(x.astype(np.float16).view(np.uint16), 0.37)
    _same_bits(got, oracle.quantize_e4m3(x, 0.37), f"quantize {n}")


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_absmax_guards_and_bits(eng, rows, C):
    """out_bits[c] = the bit pattern of max over rows of |x[r][c]| as float32: an exact operation, numpy is the reference."""
    x = np.random.default_rng(rows + C).normal(0, 3, (rows, C)).astype(np.float16)
    got = eng.op_absmax_channels_f16(x.view(np.uint16))
    _same_bits(got, np.abs(x.astype(np.float32)).max(0).view(np.uint32), f"absmax {rows} x {C}")
