"""Edge-shape cases for the bottleneck launches of csrc/bneck.hip (the eleven rows of kBneckChains and bneck_xn_f16) and an
independent reference for them. Not a test: tests/test_bneck_cases.py proves on the CPU that every case keeps the conditions the
exact comparison rests on, tests/test_gpu_bneck_op.py runs each form on each case through yh_op_bneck_f16. numpy only (the E4M3
codes of bneck_xn_f16 take the oracle's quantiser, handed in by the caller).

One launch computes, for M = n P Q output pixels,
    b  = f16(relu(conv3x3(a; stride, pad 1) + bias2))          planes -> planes (bneck_xn_f16: a IS b)
    y  = f16(relu(w3 [b ; x2] + bias3 (+ res)))                planes (+ 64) -> 4 planes
    a' = f16(relu(w1n y + bias1n))                             4 planes -> planes
Integer cases: a in [-3, 3] (bneck_xn_f16's b in [0, 3]), weights in {-1, 0, 1}, biases in [-4, 4], res / x2 in [-5, 5]. Every
product and every partial sum is then an integer below 2^24 (bounds() computes the worst case), so every summation order gives the
same float32 and the kernels must equal reference() bit for bit. Wider weights overflow a' to inf at 128 planes: keep the ranges.

Dyadic cases (DYADIC, one per form): the integer cases cannot see how a chain rounds - their sums are integers f16 mostly holds -
so these make every operand an integer times a power of two (DYADIC_GRIDS). Stage i's products and partial sums are then
multiples of 2^-g_i (c["g"]), float32 holds each exactly while sum |x| |w| + |bias| + |res| stays below 2^(22 - g_i), and the
sums carry far more than f16's 11 bits: b, y and a' are each really rounded, once, and a chain that rounds twice, rounds toward
zero or carries b or y to the next stage unrounded differs from reference() in many elements."""
import functools
import zlib

import numpy as np

# (symbol of bneck_symbol, planes, pixel tile, next block's reduce conv, two-source first block): the rows of kBneckChains in
# csrc/bneck.hip, written out, then the eight-wave launch of the 256-plane blocks
FORMS = [
    ("bneck_chain_f16<64,128,next,dual>", 64, 128, True, True),
    ("bneck_chain_f16<64,256,next>", 64, 256, True, False),
    ("bneck_chain_f16<64,256>", 64, 256, False, False),
    ("bneck_chain_f16<64,128,next>", 64, 128, True, False),
    ("bneck_chain_f16<64,128>", 64, 128, False, False),
    ("bneck_chain_f16<64,64,next>", 64, 64, True, False),
    ("bneck_chain_f16<64,64>", 64, 64, False, False),
    ("bneck_chain_f16<128,128,next>", 128, 128, True, False),
    ("bneck_chain_f16<128,128>", 128, 128, False, False),
    ("bneck_chain_f16<128,64,next>", 128, 64, True, False),
    ("bneck_chain_f16<128,64>", 128, 64, False, False),
    ("bneck_xn_f16", 256, 64, True, False),
]
FORM_IDS = [f[0] for f in FORMS]
XN = "bneck_xn_f16"

# (id, n, H, W of a, stride, tune.op_xgap). M = n P Q against the pixel tiles 64 / 128 / 256: below, on and one past each, a single
# row, a single column, a 1 x 1 map (every tap but the centre padded), H != W throughout, images that straddle tiles.
SHAPES = [
    ("1x1", 1, 1, 1, 1, 0),
    ("1x70", 1, 1, 70, 1, 0),
    ("70x1", 1, 70, 1, 1, 0),
    ("5x13", 1, 5, 13, 1, 0),
    ("13x5", 1, 13, 5, 1, 0),
    ("7x9", 1, 7, 9, 1, 0),            # M = 63
    ("8x8", 1, 8, 8, 1, 0),            # 64
    ("8x16", 1, 8, 16, 1, 0),          # 128
    ("3x43", 1, 3, 43, 1, 0),          # 129
    ("15x17", 1, 15, 17, 1, 0),        # 255
    ("16x16", 1, 16, 16, 1, 0),        # 256
    ("257x1", 1, 257, 1, 1, 0),
    ("n3_7x11", 3, 7, 11, 1, 0),       # M = 231: 77 rows per image, tiles straddle images, ragged last tile on every tile size
    ("n2_17x19", 2, 17, 19, 1, 0),     # M = 646
    ("n3_7x11_gap8", 3, 7, 11, 1, 8),  # a_img_stride = 7 * 11 * planes + 8
    ("s2_9x14", 1, 9, 14, 2, 0),       # conv_b at stride 2: P x Q = 5 x 7 (no launch of the engine takes it)
    ("s2_n2_8x5", 2, 8, 5, 2, 0),      # ... 4 x 3, two images
]
SHAPE_IDS = [s[0] for s in SHAPES]
REAL = "real_n3_7x11"                  # the one real-valued case: normal data, weights scaled by 1 / sqrt(K)
DYADIC = "dy_n3_7x11"                  # the one dyadic case: compared with reference(), like the integer cases
# planes -> (a = k / qa with |k| <= ka (bneck_xn_f16's b: 0 <= k <= ka), w2 = k / q2 with |k| <= q2 / 2, w3 = k / q3 with |k| <= q3,
# w1n = k / q1 with |k| <= q1, the share of w3 and w1n kept nonzero, res = k / qr with |k| <= kr). bias2, bias3 and bias1n lie on
# their stage's product grid 2^-g with |bias| <= 1; x2 = k / (qa q2) with |x2| <= 2. Wider ranges pass 2^22 at the third stage.
DYADIC_GRIDS = {
    64:  dict(qa=32, ka=16, q2=32, q3=2, q1=1, dens=1.0, qr=1024, kr=2048),
    128: dict(qa=32, ka=16, q2=32, q3=2, q1=1, dens=0.5, qr=1024, kr=2048),
    256: dict(qa=64, ka=128, q2=1, q3=8, q1=2, dens=0.5, qr=512, kr=2048),
}


def case_ids(form):
    """The cases of one form. Chains: every shape; the two-source form takes each at stride2 = 1 (x2 of P x Q) and at stride2 = 2 (x2 of
    (2P - 1) x 2Q: no launch of the engine takes that). bneck_xn_f16 has no conv_b, so no stride-2 shapes; it reads dense rows, so
    the op refuses the gap case (the GPU test asserts the refusal)."""
    sym, planes, tm, nxt, dual = FORMS[FORM_IDS.index(form)]
    if dual:
        return [f"{s}_x2s{k}" for s in SHAPE_IDS for k in (1, 2)] + [REAL + "_x2s1", DYADIC + "_x2s1"]
    if planes == 256:
        return [s for s in SHAPE_IDS if not s.startswith("s2_")] + [REAL, DYADIC]
    return SHAPE_IDS + [REAL, DYADIC]


def h16(a):
    return np.asarray(a).astype(np.float16).astype(np.float32)


def out_dim(h, stride):
    return (h - 1) // stride + 1       # 3 x 3, pad 1


@functools.lru_cache(maxsize=None)
def build(planes, case_id):
    """The tensors of one case for `planes` (float32 holding f16-representable values; shared by the forms of that plane count):
    a, w2 [planes][3][3][planes], bias2, w3 [4 planes][planes (+ 64)], bias3, res or x2 + stride2, w1n [planes][4 planes], bias1n,
    and for 256 planes inv_scale [256]. Treat them as read-only: the reference is computed once."""
    x2s = 0
    shape_id = case_id
    if "_x2s" in case_id:
        shape_id, k = case_id.rsplit("_x2s", 1)
        x2s = int(k)
    real, dyadic = shape_id == REAL, shape_id == DYADIC
    sid, n, H, W, stride, gap = SHAPES[SHAPE_IDS.index("n3_7x11" if real or dyadic else shape_id)]
    xn = planes == 256
    assert not (xn and (stride != 1 or x2s)) and not (x2s and planes != 64)
    P, Q = out_dim(H, stride), out_dim(W, stride)
    rng = np.random.default_rng(zlib.crc32(f"{planes}/{case_id}".encode()))
    C4, K3 = 4 * planes, planes + (64 if x2s else 0)
    H2, W2 = (P, Q) if x2s == 1 else (2 * P - 1, 2 * Q)
    if real:
        nrm = lambda shape, k=1.0: h16(rng.normal(0, 1, shape) / np.sqrt(k))
        a = nrm((n, H, W, planes))
        c = dict(a=np.maximum(a, 0) if xn else a, w2=nrm((planes, 3, 3, planes), 9 * planes), bias2=rng.normal(0, 0.1, planes).astype(np.float32),
                 w3=nrm((C4, K3), K3), bias3=rng.normal(0, 0.1, C4).astype(np.float32),
                 w1n=nrm((planes, C4), C4), bias1n=rng.normal(0, 0.1, planes).astype(np.float32))
        side = lambda shape: nrm(shape)
    elif dyadic:
        d = DYADIC_GRIDS[planes]
        dy = lambda q, lim, shape, lo=None: (rng.integers(-lim if lo is None else lo, lim + 1, shape) / q).astype(np.float32)
        thin = lambda w: w * (rng.random(w.shape) < d["dens"]).astype(np.float32)
        q_b = d["qa"] * d["q2"]                    # the grids of the three stages' sums: 1 / q_b, 1 / q_y, 1 / q_a
        q_y, q_a = q_b * d["q3"], q_b * d["q3"] * d["q1"]
        g = tuple(int(np.log2(q)) for q in (q_b, q_y, q_a))
        c = dict(a=dy(d["qa"], d["ka"], (n, H, W, planes), lo=0 if xn else None), w2=dy(d["q2"], d["q2"] // 2, (planes, 3, 3, planes)),
                 bias2=dy(q_b, q_b, planes), w3=thin(dy(d["q3"], d["q3"], (C4, K3))), bias3=dy(q_y, q_y, C4),
                 w1n=thin(dy(d["q1"], d["q1"], (planes, C4))), bias1n=dy(q_a, q_a, planes))
        side = lambda shape: dy(q_b, 2 * q_b, shape) if x2s else dy(d["qr"], d["kr"], shape)
    else:
        ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
        c = dict(a=ints(0 if xn else -3, 3, (n, H, W, planes)), w2=ints(-1, 1, (planes, 3, 3, planes)), bias2=ints(-4, 4, planes),
                 w3=ints(-1, 1, (C4, K3)), bias3=ints(-4, 4, C4), w1n=ints(-1, 1, (planes, C4)), bias1n=ints(-4, 4, planes))
        side = lambda shape: ints(-5, 5, shape)
    if x2s:
        c.update(x2=side((n, H2, W2, 64)), res=None)
    else:
        c.update(res=side((n, P, Q, C4)), x2=None)
    if xn:
        # five reciprocal scales dealt at random over the channels (a channel mix-up shows; the real-valued case's expected codes take
        # one quantiser launch per value): a' / 19 .. a' / 96 spreads the codes over E4M3's range and saturates the largest
        c["inv_scale"] = rng.choice(np.array([1 / 19, 1 / 32, 1 / 45, 1 / 64, 1 / 96] if not real else [24.0, 32.0, 45.0, 64.0, 90.0], np.float32), 256)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dict(c, id=case_id, planes=planes, n=n, H=H, W=W, P=P, Q=Q, M=n * P * Q, stride=stride, stride2=x2s or 1, gap=gap, real=real, xn=xn,
                dyadic=dyadic, g=g if dyadic else None)


def _conv3x3(a, w, stride, P, Q):
    """[n][H][W][C] x [O][3][3][C] -> [n][P][Q][O], pad 1, in float64 (exact on the integer cases: every sum is far below 2^53)."""
    n, H, W, C = a.shape
    ap = np.zeros((n, H + 2, W + 2, C), np.float64)
    ap[:, 1:H + 1, 1:W + 1] = a
    acc = np.zeros((n, P, Q, w.shape[0]), np.float64)
    for r in range(3):
        for s in range(3):
            acc += ap[:, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride] @ w[:, r, s, :].astype(np.float64).T
    return acc


def _x2_rows(c):
    s2 = c["stride2"]
    return c["x2"][:, :s2 * (c["P"] - 1) + 1:s2, :s2 * (c["Q"] - 1) + 1:s2]


def stages(c, absolute=False):
    """The three pre-activation sums (float64) and the rounded tensors b, y, a' (float32). absolute: sum |x| |w| + |bias| + |res|
    instead, with the same rounded tensors in between - the bound on every partial sum of any summation order."""
    f = np.abs if absolute else (lambda v: v)
    d = lambda v: f(np.asarray(v, np.float64))
    if c["xn"]:
        s1, b = None, c["a"]
    else:
        s1 = _conv3x3(d(c["a"]), d(c["w2"]), c["stride"], c["P"], c["Q"]) + d(c["bias2"])
        b = h16(np.maximum(_conv3x3(c["a"], c["w2"], c["stride"], c["P"], c["Q"]) + c["bias2"].astype(np.float64), 0))
    k = np.concatenate([b, _x2_rows(c)], -1) if c["x2"] is not None else b
    side = c["res"] if c["res"] is not None else 0.0
    s2 = d(k) @ d(c["w3"]).T + d(c["bias3"]) + d(side)
    y = h16(np.maximum(k.astype(np.float64) @ c["w3"].astype(np.float64).T + c["bias3"] + side, 0))
    s3 = d(y) @ d(c["w1n"]).T + d(c["bias1n"])
    an = h16(np.maximum(y.astype(np.float64) @ c["w1n"].astype(np.float64).T + c["bias1n"], 0))
    return (s1, s2, s3), (b, y, an)


_REF = {}


def reference(c, oracle=None):
    """dict(b, y, a_next[, a_next8]) of an integer or dyadic case, computed once per case. a_next8 (256 planes; needs the oracle module):
    the E4M3 codes of the float32 product a' * inv_scale[channel]."""
    assert not c["real"]
    key = (c["planes"], c["id"])
    if key not in _REF:
        b, y, an = stages(c)[1]
        _REF[key] = dict(b=b, y=y, a_next=an)
    r = _REF[key]
    if c["xn"] and oracle is not None and "a_next8" not in r:
        r["a_next8"] = oracle.quantize_e4m3(r["a_next"] * c["inv_scale"])
    return r
