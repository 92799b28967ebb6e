"""One case table for conv_igemm_f16's compiled instances: every (tile, form) of kConvTiles (csrc/conv_igemm.hip) run alone, through
a single-op entry point with the tile forced, against the CPU oracle - bit for bit. Not a test: tests/test_conv_form_cases.py proves on
the CPU that the cases cover exactly the table the library was compiled with (yh_conv_forms) and that every comparison may be exact;
tests/test_gpu_conv_forms.py runs the kernels and checks which (tile, form) really ran (yh_debug_last_conv_forms).

The rule: a (tile, form) without a case here does not ship, and a case whose (tile, form) has left the table is stale. Both fail the CPU
suite.

Data are the integer grids of the exact tests of tests/test_gpu_ops.py: x in [-3, 3], w in [-2, 2], bias in [-4, 4], residuals in
[-5, 5]; for fp8, E4M3 codes that decode to integers in [-4, 4] / [-3, 3] and per-channel scales 2^-3 .. 2^0. While the sum of
|products| of a convolution stays below 2^24, every float32 partial sum of any summation order is an exact integer (times the scale's
power of two), so the one f16 rounding of the specification is the only rounding and the kernels must equal the oracle exactly.

Shapes are the smallest that reach the edges: M = n P Q = 105 rows (n = 3, 5 x 7: below every tile, two image boundaries inside one
tile) and 270 rows (n = 2, 9 x 15: 14 rows past a multiple of 64, 128 and 256); one cout per tile width that leaves a partial last
channel tile (40 / 72 / 104 / 136 / 264 for 32 / 64 / 96 / 128 / 256 channels per tile), 95 and 351 where the entry point pads a
cout % 8 != 0; K depths of 1, 2 and 9 steps (1x1 on 64 and 128 channels, 3x3 on 64; fp8: 1x1 and 3x3 on 128), so that the
three-stage rings run shorter than, as long as and longer than the ring.

A case: kind (the entry point), tile, form (the form its launch must take: the GPU test asserts it), the shape, and the tuning that
forces the launch (kslices: a split-K, xgap / stride: what keeps a 1x1 launch off the dense form)."""
import functools
import zlib

import numpy as np

# ConvTile ids (csrc/yh_internal.h)
TILES = {"128x128": 0, "64x256": 1, "32x256": 2, "64x256_SMALLC": 3, "128x256": 5, "128x128_S3": 7, "256x256_M16": 8, "128x128_M16": 12,
         "128x128_S3_M16": 13, "128x256_M16": 15, "64x64_S3": 16, "256x256_FP8": 20, "128x128_K1": 21, "64x256_K1": 22, "128x128_FP8": 23,
         "64x64_FP8": 24, "96x128_K1": 27}
# channels per tile (checked against yh_conv_forms by the CPU test), and the cout that leaves a partial last channel tile
TILE_CH = {"128x128": 128, "64x256": 64, "32x256": 32, "64x256_SMALLC": 64, "128x256": 128, "128x128_S3": 128, "256x256_M16": 256,
           "128x128_M16": 128, "128x128_S3_M16": 128, "128x256_M16": 128, "64x64_S3": 64, "256x256_FP8": 256, "128x128_K1": 128,
           "64x256_K1": 64, "128x128_FP8": 128, "64x64_FP8": 64, "96x128_K1": 96}
PARTIAL = {32: 40, 64: 72, 96: 104, 128: 136, 256: 264}
LEVELS = (9, 5, 3, 2, 1)          # the FPN levels of a 70-pixel input: 120 cells
ROWS_A, ROWS_B = (3, 5, 7), (2, 9, 15)      # (n, P, Q): M = 105, 270
RING = ("128x128_S3", "64x64_S3")

CASES = {}


def _add(kind, tile, form, tag, **kw):
    cid = f"{kind}-{tile}-{form}-{tag}"
    assert cid not in CASES, cid
    kw.setdefault("cout", PARTIAL[TILE_CH[tile]])
    CASES[cid] = dict(kw, kind=kind, tile=tile, form=form)


def _conv(tile, form, tag, rows, k, cin, res=False, act=0, stride=1, **kw):
    n, P, Q = rows   # the OUTPUT grid; the input is the smallest that gives it
    pad = k // 2
    h, w = (P - 1) * stride + k - 2 * pad, (Q - 1) * stride + k - 2 * pad
    _add("conv", tile, form, tag, n=n, h=h, w=w, cin=cin, k=k, stride=stride, pad=pad, res=res, act=act, **kw)


# ---- yh_op_conv2d_f16: PLAIN on every f16 tile that has it, K3 / LIN on the streaming tiles, SPLITK on the rings
for _t in ("128x128", "64x256", "32x256", "128x256", "128x128_S3", "256x256_M16", "128x128_M16", "128x128_S3_M16", "128x256_M16", "64x64_S3"):
    _conv(_t, "PLAIN", "m105-k1c64", ROWS_A, 1, 64)
    _conv(_t, "PLAIN", "m270-k3c64", ROWS_B, 3, 64, res=True, act=1)
    _conv(_t, "PLAIN", "m270-k1c128", ROWS_B, 1, 128, act=1)
# (cin = 3 takes the small-C tile whatever tune.op_tile says: 3x3 is two K steps, 7x7 stride 2 seven)
_conv("64x256_SMALLC", "PLAIN", "m105-k3", ROWS_A, 3, 3, act=1, tile_forced=False)
_add("conv", "64x256_SMALLC", "PLAIN", "m270-k7s2", n=2, h=18, w=30, cin=3, k=7, stride=2, pad=3, res=True, act=1, tile_forced=False)
for _t in ("128x128_K1", "64x256_K1"):
    # a 1x1 launch stays off the dense form when its images are not laid end to end (op_xgap) or its stride is 2
    _conv(_t, "PLAIN", "m105-k1c64-xgap8", ROWS_A, 1, 64, act=1, xgap=8)
    _conv(_t, "PLAIN", "m270-k1c128-s2", ROWS_B, 1, 128, res=True, stride=2)
    _conv(_t, "LIN", "m105-k1c64", ROWS_A, 1, 64)
    _conv(_t, "LIN", "m270-k1c128", ROWS_B, 1, 128, res=True, act=1)
    _conv(_t, "LIN", "m105-k1c256", ROWS_A, 1, 256, act=1)
_conv("64x256_K1", "PLAIN", "m270-k3c64", ROWS_B, 3, 64, res=True, act=1)
_conv("128x128_K1", "K3", "m270-k3c64", ROWS_B, 3, 64, res=True, act=1)
_conv("128x128_K1", "K3", "m105-k3c128", ROWS_A, 3, 128)
for _t in RING:
    _conv(_t, "SPLITK", "m270-k3c64-s2", ROWS_B, 3, 64, res=True, act=1, kslices=2)        # 9 steps: slices of 5 and 4
    _conv(_t, "SPLITK", "m105-k3c64-s9", ROWS_A, 3, 64, kslices=9)                         # one step per slice
    _conv(_t, "SPLITK", "m105-k1c128-s2", ROWS_A, 1, 128, act=1, kslices=2)

# ---- yh_op_conv2d_levels_f16: ML on every tile that has it (351: the shared head's channels; 95: its remainder on 96-channel tiles)
for _t in ("128x128", "128x256", "128x128_S3", "256x256_M16", "128x128_M16", "128x128_S3_M16", "128x256_M16", "64x64_S3", "128x128_K1", "96x128_K1"):
    _add("levels", _t, "ML", "n2-k3c64", n=2, cin=64, k=3, act=1)
    _add("levels", _t, "ML", "n3-k1c128", n=3, cin=128, k=1, act=0)
for _t in ("128x256", "128x256_M16"):
    _add("levels", _t, "ML", "n2-k3c64-cout351", n=2, cin=64, k=3, act=1, cout=351)
_add("levels", "96x128_K1", "ML", "n3-k3c64-cout95", n=3, cin=64, k=3, act=1, cout=95)
_add("levels", "96x128_K1", "ML", "n2-k1c128-cout95", n=2, cin=128, k=1, act=1, cout=95)
for _t in RING:
    _add("levels", _t, "ML_SPLITK", "n2-k3c64-s2", n=2, cin=64, k=3, act=1, kslices=2)
    _add("levels", _t, "ML_SPLITK", "n3-k1c128-s2", n=3, cin=128, k=1, act=0, kslices=2)

# ---- yh_op_conv2d_dual_f16: DUAL, and DUAL_SPLITK with slices that start before, at and after the switch of sources
for _t in ("128x128", "128x128_S3", "256x256_M16", "128x128_M16", "128x128_S3_M16", "64x64_S3", "128x128_K1"):
    _add("dual", _t, "DUAL", "m105-c64+64", rows=ROWS_A, c1=64, c2=64, stride2=1, act=1)
    _add("dual", _t, "DUAL", "m270-c64+128-s2", rows=ROWS_B, c1=64, c2=128, stride2=2, act=0)
for _t in RING:
    _add("dual", _t, "DUAL_SPLITK", "m270-c64+128-s2-k2", rows=ROWS_B, c1=64, c2=128, stride2=2, act=1, kslices=2)
    _add("dual", _t, "DUAL_SPLITK", "m105-c64+128-k3", rows=ROWS_A, c1=64, c2=128, stride2=1, act=1, kslices=3)

# ---- yh_op_conv2d_resup_f16: RESUP on its seven tiles (lo -> hi), and the reduce kernel's resize under a forced split-K
for _t in ("128x128", "128x128_S3", "256x256_M16", "128x128_M16", "128x128_S3_M16", "64x64_S3", "128x128_K1"):
    _add("resup", _t, "RESUP", "n3-3to5-c64", n=3, lo=(3, 3), hi=(5, 5), cin=64, act=0)
    _add("resup", _t, "RESUP", "n2-5x7to9x13-c128", n=2, lo=(5, 7), hi=(9, 13), cin=128, act=1)
    _add("resup", _t, "RESUP", "n2-1to2-c64", n=2, lo=(1, 1), hi=(2, 2), cin=64, act=0)
for _t in ("128x128_S3", "128x128_K1"):
    _add("resup", _t, "RESUP", "n1-18to35-c64", n=1, lo=(18, 18), hi=(35, 35), cin=64, act=0)
for _t in RING:
    _add("resup", _t, "SPLITK", "n2-5x7to9x13-c192-s2", n=2, lo=(5, 7), hi=(9, 13), cin=192, act=1, kslices=2)     # 3 steps: 2 + 1
    _add("resup", _t, "SPLITK", "n3-3to5-c256-s4", n=3, lo=(3, 3), hi=(5, 5), cin=256, act=0, kslices=4)           # kslices = ksteps

# ---- yh_op_conv2d_tail_f16 / _fp8: TAIL (cout is 256 by definition; the second conv writes 32 channels)
for _tag, _rows, _k, _cin in (("m105-k3c64", ROWS_A, 3, 64), ("m270-k3c64", ROWS_B, 3, 64), ("m105-k1c64", ROWS_A, 1, 64), ("m270-k1c128", ROWS_B, 1, 128)):
    _add("tail", "256x256_M16", "TAIL", _tag, rows=_rows, k=_k, cin=_cin, act=1, cout=256)
_add("tail_fp8", "256x256_FP8", "TAIL", "m105-k1c128", rows=ROWS_A, k=1, cin=128, act=1, cout=256)
_add("tail_fp8", "256x256_FP8", "TAIL", "m270-k3c128", rows=ROWS_B, k=3, cin=128, act=1, cout=256)
_add("tail_fp8", "256x256_FP8", "TAIL", "m105-k3c128-noact", rows=ROWS_A, k=3, cin=128, act=0, cout=256)

# ---- yh_op_conv2d_fp8 / yh_op_conv2d_levels_fp8: the three fp8 tiles, partial channel tiles included
for _t in ("256x256_FP8", "128x128_FP8", "64x64_FP8"):
    _add("fp8", _t, "PLAIN", "m105-k1c128", rows=ROWS_A, k=1, cin=128, res=True, act=0)
    _add("fp8", _t, "PLAIN", "m270-k3c128", rows=ROWS_B, k=3, cin=128, res=False, act=1)
    _add("fp8", _t, "PLAIN", "m270-k1c256", rows=ROWS_B, k=1, cin=256, res=True, act=1)
for _t in ("256x256_FP8", "128x128_FP8"):
    _add("levels_fp8", _t, "ML", "n2-k3c128", n=2, cin=128, k=3, act=1)
    _add("levels_fp8", _t, "ML", "n3-k1c128", n=3, cin=128, k=1, act=0)

CASE_IDS = list(CASES)
# A case's data come from a generator seeded with crc32(id) + SEEDS.get(id, 0). The RESUP cases listed here take the first seed for
# which acc + (bias + res) and (acc + bias) + res give the same f16 bits at every element (tests/test_conv_form_cases.py asserts it for
# all of them): where a resize weight is rounding noise (a target pixel centre that falls on a source pixel centre) and the source
# beside it is not 0, the resized residual is a tiny non-integer, and an element whose acc + bias is exactly 0 then keeps it in one
# order and loses it in the other.
SEEDS = {"resup-128x128-RESUP-n3-3to5-c64": 1, "resup-128x128_S3-RESUP-n2-5x7to9x13-c128": 3, "resup-256x256_M16-RESUP-n3-3to5-c64": 1,
         "resup-256x256_M16-RESUP-n2-5x7to9x13-c128": 1, "resup-128x128_S3_M16-RESUP-n3-3to5-c64": 2,
         "resup-128x128_K1-RESUP-n2-5x7to9x13-c128": 1, "resup-128x128_K1-RESUP-n1-18to35-c64": 5}
assert set(SEEDS) <= set(CASES)
GUARDED = ("tail", "tail_fp8")       # kinds whose cout is the tile's 256 by definition: no partial last channel tile to ask for


def covered():
    """The (tile id, form name) pairs the cases are for."""
    return {(TILES[c["tile"]], c["form"]) for c in CASES.values()}


def tuning(cid):
    """The yh_tuning fields that force the case's launch."""
    c = CASES[cid]
    t = {}
    if c.get("tile_forced", True):
        t["op_tile"] = TILES[c["tile"]]
    if c.get("kslices"):
        t["op_kslices"] = c["kslices"]
    if c.get("xgap"):
        t["op_xgap"] = c["xgap"]
    return t


def expected_kernels(cid):
    """What yh_debug_last_conv_forms must list after the case: its (tile id, form), and the reduce kernel behind a split-K."""
    c = CASES[cid]
    k = [(TILES[c["tile"]], c["form"])]
    return k + [(-1, "REDUCE")] if c["form"].endswith("SPLITK") else k


def rows_of(cid):
    """M = n P Q of the case's (first) convolution."""
    c = CASES[cid]
    if c["kind"] in ("levels", "levels_fp8"):
        return c["n"] * sum(s * s for s in LEVELS)
    if c["kind"] == "resup":
        return c["n"] * c["hi"][0] * c["hi"][1]
    if c["kind"] == "conv":
        return c["n"] * ((c["h"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1) * ((c["w"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1)
    n, P, Q = c["rows"]
    return n * P * Q


@functools.lru_cache(maxsize=None)
def build(cid):
    """The case's tensors: float32 arrays of small integers (fp8 kinds: the integers the codes decode to), read-only."""
    c = CASES[cid]
    kind, cout = c["kind"], c["cout"]
    rng = np.random.default_rng(zlib.crc32(cid.encode()) + SEEDS.get(cid, 0))
    ints = lambda lim, *shape: rng.integers(-lim, lim + 1, shape).astype(np.float32)
    fp8 = kind in ("fp8", "levels_fp8", "tail_fp8")
    xl, wl = (4, 3) if fp8 else (3, 2)
    t = dict(bias=ints(4, cout))
    if fp8:
        t["scale"] = (2.0 ** rng.integers(-3, 1, cout)).astype(np.float32)
    if kind == "conv":
        P, Q = (c["h"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1, (c["w"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1
        t.update(x=ints(xl, c["n"], c["h"], c["w"], c["cin"]), w=ints(wl, cout, c["k"], c["k"], c["cin"]))
        t["res"] = ints(5, c["n"], P, Q, cout) if c["res"] else None
    elif kind in ("levels", "levels_fp8"):
        t.update(x=ints(xl, c["n"], sum(s * s for s in LEVELS), c["cin"]), w=ints(wl, cout, c["k"], c["k"], c["cin"]))
    elif kind == "dual":
        n, P, Q = c["rows"]
        s2 = c["stride2"]
        h2, w2 = (P - 1) * s2 + 1 + (s2 - 1), (Q - 1) * s2 + 1       # (odd source size under stride 2: the last row is never read)
        t.update(x1=ints(xl, n, P, Q, c["c1"]), x2=ints(xl, n, h2, w2, c["c2"]), w=ints(wl, cout, c["c1"] + c["c2"]))
    elif kind == "resup":
        t.update(x=ints(xl, c["n"], *c["hi"], c["cin"]), w=ints(wl, cout, 1, 1, c["cin"]), res_lo=ints(5, c["n"], *c["lo"], cout))
    elif kind in ("tail", "tail_fp8"):
        n, P, Q = c["rows"]
        t.update(x=ints(xl, n, P, Q, c["cin"]), w=ints(wl, cout, c["k"], c["k"], c["cin"]), w2=ints(2, 32, 256), bias2=ints(4, 32))
    else:
        n, P, Q = c["rows"]
        k = c["k"]
        t.update(x=ints(xl, n, P, Q, c["cin"]), w=ints(wl, cout, k, k, c["cin"]))
        t["res"] = ints(5, n, P, Q, cout) if c["res"] else None
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float32)


def _act(v, act):
    return np.where(v > 0, v, 0.0) if act else v       # (the spec's v > 0 ? v : 0: a NaN becomes 0; np.maximum would keep it)


def dual_cat(c, t):
    n, P, Q = c["rows"]
    s2 = c["stride2"]
    return np.ascontiguousarray(np.concatenate([t["x1"], t["x2"][:, ::s2, ::s2][:, :P, :Q]], -1))


def _levels(fn, x, n, cin):
    """fn(level image [n][s][s][cin]) -> [n][s][s][c'] on every level, laid end to end again."""
    out, off = [], 0
    for s in LEVELS:
        out.append(fn(np.ascontiguousarray(x[:, off:off + s * s]).reshape(n, s, s, cin)).reshape(n, s * s, -1))
        off += s * s
    return np.concatenate(out, 1)


def convolutions(cid):
    """Every convolution of the case as (x, w, stride, pad) with the FIRST one's operands (the tail's second follows from its output):
    what accumulator() and magnitudes() run the oracle on. Level cases: one entry per level."""
    c, t = CASES[cid], build(cid)
    kind = c["kind"]
    if kind in ("levels", "levels_fp8"):
        convs, off = [], 0
        for s in LEVELS:
            convs.append((np.ascontiguousarray(t["x"][:, off:off + s * s]).reshape(c["n"], s, s, c["cin"]), t["w"], 1, c["k"] // 2))
            off += s * s
        return convs
    if kind == "dual":
        cat = dual_cat(c, t)
        return [(cat, t["w"].reshape(c["cout"], 1, 1, -1), 1, 0)]
    if kind == "conv":
        return [(t["x"], t["w"], c["stride"], c["pad"])]
    if kind == "resup":
        return [(t["x"], t["w"], 1, 0)]
    return [(t["x"], t["w"], 1, c["k"] // 2)]


def _acc(oracle, cid, absolute=False):
    """The exact accumulators (float32 integers) of the case's first convolution(s): [M'][cout] blocks in row order."""
    cout = CASES[cid]["cout"]
    z = np.zeros(cout, np.float32)
    f = np.abs if absolute else (lambda a: a)
    return [oracle.conv2d(f(x), f(w), z, s, p, None, 0, f16=False) for x, w, s, p in convolutions(cid)]


def _side(cid, oracle):
    """bias, residual (None, or what the kernel adds: for resup the oracle's f16 resize of res_lo) and scale of the first convolution."""
    c, t = CASES[cid], build(cid)
    res = t.get("res")
    if c["kind"] == "resup":
        res = oracle.bilinear(t["res_lo"], c["hi"][0], c["hi"][1], f16=True)
    return t["bias"], res, t.get("scale")


_REF = {}


def reference(cid, oracle):
    """The expected output, from the CPU oracle alone (computed once per case, read-only)."""
    if cid in _REF:
        return _REF[cid]
    c, t = CASES[cid], build(cid)
    kind, cout, act = c["kind"], c["cout"], c["act"]
    bias, res, scale = _side(cid, oracle)
    if kind == "conv":
        r = oracle.conv2d(t["x"], t["w"], bias, c["stride"], c["pad"], res, act, f16=True)
    elif kind == "levels":
        r = _levels(lambda xl: oracle.conv2d(xl, t["w"], bias, 1, c["k"] // 2, None, act, f16=True), t["x"], c["n"], c["cin"])
    elif kind == "dual":
        r = oracle.conv2d(dual_cat(c, t), t["w"].reshape(cout, 1, 1, -1), bias, 1, 0, None, act, f16=True)
    elif kind == "resup":
        # (acc + bias) + res, activation, one rounding: the oracle's order is the kernel's
        r = oracle.conv2d(t["x"], t["w"], bias, 1, 0, res, act, f16=True)
    elif kind == "tail":
        mid = oracle.conv2d(t["x"], t["w"], bias, 1, c["k"] // 2, None, act, f16=True)          # the f16-rounded intermediate
        r = oracle.conv2d(mid, t["w2"].reshape(32, 1, 1, 256), t["bias2"], 1, 0, None, 1, f16=True)
    else:
        # fp8: the oracle's convolution of the DECODED operands; acc * scale + bias (+ res) is exact in float64, rounded once
        acc = _acc(oracle, cid)
        acc = np.concatenate([a.reshape(c["n"], -1, cout) for a in acc], 1) if kind == "levels_fp8" else acc[0]
        v = acc.astype(np.float64) * scale.astype(np.float64) + bias.astype(np.float64)
        if res is not None:
            v = v + res
        r = f16(_act(v, act))
        if kind == "tail_fp8":
            r = oracle.conv2d(r, t["w2"].reshape(32, 1, 1, 256), t["bias2"], 1, 0, None, 1, f16=True)
    r = np.ascontiguousarray(r, np.float32)
    r.setflags(write=False)
    _REF[cid] = r
    return r


def magnitudes(cid, oracle):
    """max over outputs of sum |x| |w| (+ |bias| + |res|) for every convolution of the case, the tail's second included: below 2^24
    every float32 partial sum of any order is exact."""
    c, t = CASES[cid], build(cid)
    bias, res, _ = _side(cid, oracle)
    m = max(float(a.max()) for a in _acc(oracle, cid, absolute=True)) + float(np.abs(bias).max()) + (float(np.abs(res).max()) if res is not None else 0.0)
    out = [m]
    if c["kind"] in ("tail", "tail_fp8"):
        # the intermediate t = f16(act(conv + bias)) is bounded by the first magnitude; the second conv sums 256 of |t| |w2|
        if c["kind"] == "tail":
            mid = oracle.conv2d(t["x"], t["w"], bias, 1, c["k"] // 2, None, c["act"], f16=True)
        else:
            mid = f16(_act(_acc(oracle, cid)[0].astype(np.float64) * t["scale"] + bias, c["act"]))
        m2 = oracle.conv2d(np.abs(mid), np.abs(t["w2"]).reshape(32, 1, 1, 256), np.zeros(32, np.float32), 1, 0, None, 0, f16=False)
        out.append(float(m2.max()) + float(np.abs(t["bias2"]).max()))
    return out


def resup_orders(cid, oracle):
    """A RESUP case's output in the kernel's order, f16(act((acc + bias) + res)), and in the other, f16(act(acc + (bias + res))), in
    float32 arithmetic on the exact accumulator: the CPU test asserts that both equal the reference at EVERY element, so that the
    comparison does not hang on which of the two a kernel takes."""
    c = CASES[cid]
    bias, res, _ = _side(cid, oracle)
    acc = _acc(oracle, cid)[0].astype(np.float32)
    b = bias.astype(np.float32)
    kernel = f16(_act((acc + b).astype(np.float32) + res, c["act"]))
    other = f16(_act(acc + (b + res).astype(np.float32), c["act"]))
    return kernel, other
