"""Rounding cases for the single-op convolutions (conv_igemm_f16 on every tile and form the op entries reach, splitk_reduce_f16,
stem_pool_f16, the fp8 conv's epilogue) and an independent reference for them. Not a test: tests/test_dyadic_cases.py proves on the
CPU that every case keeps the conditions the exact comparison rests on, tests/test_gpu_rounding.py runs the kernels on them.
numpy only.

The integer cases of the rest of the suite cannot see how a kernel rounds: their sums are integers below 2048, which f16 holds.
Here every operand is an integer times a power of two, an f16 value: x, w = k / 64 with |k| <= 32 (the stem's x: |k| <= 128), the
residual k / 64 with |r| <= 2, the bias k / 4096 with |bias| <= 2 - a multiple of the products' grid 2^-12 = 2^-G. Every product and
every partial sum of every summation order is then a multiple of 2^-G, and while sum |x| |w| + |bias| + |res| stays below
2^(22 - G) float32 holds each of them exactly, with two bits to spare. So the float32 accumulator of any kernel is the exact sum, a
number of 12 to 22 significant bits, and the one rounding the specification has -
    y = f16(act(conv(x, w) + bias + res)),   round to nearest, ties to even
- really happens: most outputs need it, a good share are exact ties. reference() computes that in float64 (exact) with one
astype(np.float16), and the kernels must equal it bit for bit.

The fp8 cases keep the decoded operands small integers (the block-scaled MFMA is exact only there, tests/test_gpu_fp8.py) and
make the epilogue fractional: scale 2^-9 .. 2^-4 per channel, bias k / 4096, residual k / 1024."""
import functools
import zlib

import numpy as np

G = 12                                  # every case's sums are multiples of 2^-G

# id -> (kind, parameters). conv: (n, h, w, cin, cout, k, res, act); levels: (sizes, n, cin, cout, k), ReLU, no residual;
# dual: (n, ho, wo, c1, c2, stride2, cout), ReLU; stem: (n, S), ReLU; fp8: (n, h, w, cin, cout, k, stride, pad, res), ReLU
CASES = {
    "head_3x3":         ("conv", (2, 13, 11, 128, 192, 3, True, 1)),       # ragged M, 192 channels: a ragged channel tile on every tile
    "levels_k3":        ("levels", ([9, 5, 3, 1], 3, 128, 256, 3)),
    "levels_k1":        ("levels", ([9, 5, 3, 1], 3, 128, 256, 1)),
    "big_64_256_k3":    ("conv", (3, 13, 11, 64, 256, 3, True, 1)),        # default plan: 256x256 tile, 16x16x32 MFMA, split epilogue
    "big_256_512_k1":   ("conv", (3, 13, 11, 256, 512, 1, False, 0)),      # ... no residual, no activation: negative outputs round too
    "big_64_351_k3":    ("conv", (3, 13, 11, 64, 351, 3, False, 1)),       # 128x256 tile, ragged channel tail
    "deep_k2048":       ("conv", (1, 18, 18, 2048, 256, 1, True, 0)),
    "split_64_256_k3":  ("conv", (5, 17, 16, 64, 256, 3, True, 1)),        # two-launch plans when planned for 4 CUs
    "split_512_351_k1": ("conv", (3, 21, 16, 512, 351, 1, True, 1)),
    "rem96_k3":         ("levels", ([13, 9, 5, 3], 6, 64, 351, 3)),
    "dual_s2":          ("dual", (2, 13, 11, 128, 256, 2, 256)),
    "stem_n2_S30":      ("stem", (2, 30)),
    "stem_n1_S34":      ("stem", (1, 34)),
    "fp8_128_256_k3":   ("fp8", (2, 13, 11, 128, 256, 3, 1, 1, True)),     # the three shapes of test_conv_fp8_exact_on_integers
    "fp8_256_512_k1":   ("fp8", (1, 16, 16, 256, 512, 1, 1, 0, False)),
    "fp8_128_200_k3s2": ("fp8", (3, 9, 9, 128, 200, 3, 2, 1, False)),
}
CASE_IDS = list(CASES)
F16_IDS = [i for i in CASE_IDS if CASES[i][0] != "fp8"]
FP8_IDS = [i for i in CASE_IDS if CASES[i][0] == "fp8"]


def out_dim(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


@functools.lru_cache(maxsize=None)
def build(case_id):
    """The tensors of one case: float32 arrays of f16-representable values on the grids of the module docstring (fp8: xi, wi hold the
    decoded integers of the codes). Read-only: the reference is computed once."""
    kind, prm = CASES[case_id]
    rng = np.random.default_rng(zlib.crc32(case_id.encode()))
    dy = lambda q, lim, shape: (rng.integers(-lim, lim + 1, shape) / q).astype(np.float32)
    c = dict(res=None, act=1, stride=1)
    if kind == "conv":
        n, h, w, cin, cout, k, res, act = prm
        c.update(x=dy(64, 32, (n, h, w, cin)), w=dy(64, 32, (cout, k, k, cin)), bias=dy(4096, 8192, cout), pad=k // 2, act=act)
        if res:
            c["res"] = dy(64, 128, (n, h, w, cout))
    elif kind == "levels":
        sizes, n, cin, cout, k = prm
        c.update(x=dy(64, 32, (n, sum(s * s for s in sizes), cin)), w=dy(64, 32, (cout, k, k, cin)), bias=dy(4096, 8192, cout), pad=k // 2,
                 sizes=list(sizes))
    elif kind == "dual":
        n, ho, wo, c1, c2, s2, cout = prm
        h2, w2 = (ho - 1) * s2 + 1 + (s2 - 1), (wo - 1) * s2 + 1     # (odd source size under stride 2: the last row is never read)
        c.update(x1=dy(64, 32, (n, ho, wo, c1)), x2=dy(64, 32, (n, h2, w2, c2)), w=dy(64, 32, (cout, c1 + c2)), bias=dy(4096, 8192, cout),
                 stride2=s2, pad=0)
    elif kind == "stem":
        n, S = prm
        c.update(x=dy(64, 128, (n, S, S, 3)), w=dy(64, 32, (64, 7, 7, 3)), bias=dy(4096, 8192, 64), stride=2, pad=3)
    else:
        n, h, w, cin, cout, k, stride, pad, res = prm
        ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
        c.update(xi=ints(-4, 4, (n, h, w, cin)), wi=ints(-3, 3, (cout, k, k, cin)), scale=(2.0 ** rng.integers(-9, -3, cout)).astype(np.float32),
                 bias=dy(4096, 8192, cout), stride=stride, pad=pad)
        if res:
            c["res"] = dy(1024, 2048, (n, out_dim(h, k, stride, pad), out_dim(w, k, stride, pad), cout))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dict(c, id=case_id, kind=kind, g=G)


def _im2col(x, k, stride, pad):
    """[n][H][W][C] -> [n P Q][(r, s, c)] in float64: the rows w.reshape(cout, -1) multiplies."""
    n, H, W, C = x.shape
    P, Q = out_dim(H, k, stride, pad), out_dim(W, k, stride, pad)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, C), np.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = [xp[:, r:r + stride * (P - 1) + 1:stride, s:s + stride * (Q - 1) + 1:stride] for r in range(k) for s in range(k)]
    return np.concatenate(cols, -1).reshape(n * P * Q, k * k * C), (n, P, Q)


def dual_cat(c):
    """The two-source form's input as one tensor: [x1 | x2 at stride2]."""
    n, ho, wo, _ = c["x1"].shape
    s2 = c["stride2"]
    return np.concatenate([c["x1"], c["x2"][:, ::s2, ::s2][:, :ho, :wo]], -1)


_GEMM = {}


def _gemm(c):
    """The case as one matrix product (float64): A [M][K], W [cout][K], side [M][cout] = bias + res, per-channel scale, output shape."""
    if c["id"] in _GEMM:
        return _GEMM[c["id"]]
    kind = c["kind"]
    w = c["wi"] if kind == "fp8" else c["w"]
    cout = w.shape[0]
    if kind == "levels":
        n, cells, cin = c["x"].shape
        blocks, off = [], 0
        for s in c["sizes"]:
            a, _ = _im2col(c["x"][:, off:off + s * s].reshape(n, s, s, cin), w.shape[1], 1, c["pad"])
            blocks.append(a.reshape(n, s * s, -1))
            off += s * s
        A, shape = np.concatenate(blocks, 1).reshape(n * cells, -1), (n, cells, cout)
    elif kind == "dual":
        cat = dual_cat(c)
        A, shape = cat.reshape(-1, cat.shape[-1]).astype(np.float64), cat.shape[:3] + (cout,)
    else:
        A, npq = _im2col(c["xi"] if kind == "fp8" else c["x"], w.shape[1], c["stride"], c["pad"])
        shape = npq + (cout,)
    side = np.broadcast_to(c["bias"].astype(np.float64), (A.shape[0], cout))
    if c["res"] is not None:
        side = side + c["res"].reshape(-1, cout).astype(np.float64)
    scale = c["scale"].astype(np.float64) if kind == "fp8" else np.ones(cout)
    _GEMM[c["id"]] = (A, w.reshape(cout, -1).astype(np.float64), side, scale, shape)
    return _GEMM[c["id"]]


def _act(c, v):
    return np.maximum(v, 0) if c["act"] else v


def exact(c):
    """act(conv + bias + res) in float64: the exact value (every term a multiple of 2^-G far below 2^53 of them)."""
    A, W, side, scale, shape = _gemm(c)
    return _act(c, (A @ W.T) * scale + side).reshape(shape)


_REF = {}


def reference(c):
    """The specification: the exact value rounded to f16 once (float32 array, computed once per case)."""
    if c["id"] not in _REF:
        r = exact(c).astype(np.float16).astype(np.float32)
        r.setflags(write=False)
        _REF[c["id"]] = r
    return _REF[c["id"]]


def magnitude(c):
    """sum |x| |w| (|scale|) + |bias| + |res| per output, float64: the bound on every partial sum of any summation order."""
    A, W, side, scale, shape = _gemm(c)
    s = np.abs(c["bias"].astype(np.float64)) + (np.abs(c["res"].reshape(-1, W.shape[0]).astype(np.float64)) if c["res"] is not None else 0.0)
    return ((np.abs(A) @ np.abs(W).T) * scale + s).reshape(shape)


def rtz16(v):
    """float64 -> f16, rounded toward zero (as float32)."""
    h = np.asarray(v, np.float64).astype(np.float16)
    bits = h.view(np.uint16).copy()
    bits[np.abs(h.astype(np.float64)) > np.abs(v)] -= 1        # sign-magnitude: one step toward zero
    return bits.view(np.float16).astype(np.float32)


def is_tie(v):
    """Which float64 values lie exactly half way between two neighbouring f16 values."""
    v = np.asarray(v, np.float64)
    lo = rtz16(v).astype(np.float16)
    hi = np.nextafter(lo, np.where(v < 0, -np.inf, np.inf).astype(np.float16)).astype(np.float64)
    lo = lo.astype(np.float64)
    return (lo != v) & (np.abs(v - lo) == np.abs(hi - v))


# ---- mutants of the reference: what a subtly wrong kernel would compute (only to show that the cases are sensitive) ----
_h = lambda v: v.astype(np.float16).astype(np.float64)


def mutant_rtz(c):
    """The last conversion rounds toward zero."""
    return rtz16(exact(c))


def mutant_f16_partials(c):
    """The sum over each half of K is rounded to f16 before the halves are added (split-K slabs or a staging image held in f16)."""
    A, W, side, scale, shape = _gemm(c)
    half = A.shape[1] // 2
    acc = _h(A[:, :half] @ W[:, :half].T) + _h(A[:, half:] @ W[:, half:].T)
    return _act(c, acc * scale + side).astype(np.float16).astype(np.float32).reshape(shape)


def mutant_round_before_side(c):
    """The accumulator is rounded to f16, then bias and residual are added, then it is rounded again."""
    A, W, side, scale, shape = _gemm(c)
    return _act(c, _h(A @ W.T) * scale + side).astype(np.float16).astype(np.float32).reshape(shape)


MUTANTS = {"rtz": mutant_rtz, "f16_partials": mutant_f16_partials, "round_before_side": mutant_round_before_side}


def shares(c):
    """The measures tests/test_dyadic_cases.py bounds, as fractions of the nonzero outputs (nonzero: of all outputs)."""
    v, ref = exact(c), reference(c)
    nz = ref != 0
    cnt = max(int(nz.sum()), 1)
    out = dict(nonzero=float(nz.mean()), rounded=float(((ref.astype(np.float64) != v) & nz).sum() / cnt), tie=float((is_tie(v) & nz).sum() / cnt),
               bits=float(np.log2(magnitude(c).max()) + c["g"]))
    for name, fn in MUTANTS.items():
        out[name] = float(((fn(c) != ref) & nz).sum() / cnt)
    return out
