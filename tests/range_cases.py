"""Range-end cases for the single-op convolutions and an independent reference for them: f16 subnormal operands, outputs on the
subnormal grid and signed zeros, overflow to inf, tanh and E4M3 saturation at the ends. Not a test: tests/test_range_cases.py proves
on the CPU that every case keeps the conditions the bit comparison rests on, tests/test_gpu_range.py runs the kernels. numpy only.

Every case is a case of tests/dyadic_cases.py scaled by powers of two: x by 2^a, the weights of output channel o by 2^b[o], and
bias, residual and the fp8 per-channel scale of channel o by 2^(a + b[o]) (fp8: the codes stay, the whole scale goes on `scale`).
Every product and partial sum of channel o is then the original's times 2^(a + b[o]): a multiple of 2^(a + b[o] - G), below
2^(22 + a + b[o] - G), which float32 holds exactly (its exponent range is far from both ends here). The exactness argument of
dyadic_cases.py carries over unchanged, the float32 value that reaches a kernel's final conversion is the exact one, and the one
rounding of the specification,
    y = f16(act(conv(x, w) + bias + res)),   ReLU as v > 0 ? v : 0, BEFORE the rounding,
is computed here in float64 with one astype(np.float16): 65520 -> inf, 2^-25 -> 0, 3 * 2^-25 -> 2^-23, a negative sum under ReLU ->
+0, a negative sum above -2^-25 without activation -> -0.

Families (variant ids are "<dyadic case>/<family>"):
  sub_x, sub_w, sub_out   the same total scale 2^t per channel, placed on x (every x = k 2^-24: subnormal), on w (every w subnormal)
                          or split so that the operands stay normal and only the outputs are subnormal. The three have the same exact
                          values, so one reference: an operand flush fails one placement, an output flush all three.
                          t = -16 (split: 2^-8 each, x and w >= 2^-14): a third to all of the outputs are subnormal, one in
                          sixteen of those an exact tie of the 2^-24 grid, and the sums are multiples of 2^-28, so those within
                          2^-25 of zero round to +-0. The small cases (SUB_MOVED) have too few of these: there the bias of 20
                          channels is moved by a few grid steps so that one output each becomes +2^-28 (16 channels: nonzero,
                          rounds to zero) or -2^-28 (4 channels: +0 under ReLU, never -0).
  ovf                     scaled by the smallest power of two at which at least 5 % of the outputs are inf - the share a saturating
                          kernel must differ on (max |exact| is then 2 .. 11 times 65504; at about 2 times, 1 % are) -, and the bias
                          of 24 channels (48 without activation) moved by multiples of the grid so that outputs sit exactly on
                          65520 (the tie that must round to inf), on the grid point below it (-> 65504) and on 65504.
  ovf_res                 head_3x3 with conv and bias at 2^12, where no sum reaches 65504 alone, and the residual at 2^14 (still a
                          multiple of the grid): only the residual carries sums over.
  ovf_tanh                big_256_512_k1 with act = 2: channel exponents cycle over overflow, normal and subnormal, two channels have
                          zero weights (pre-activation +0, and a tiny negative bias); expected oracle.spec_tanhf of the float32 sum
                          from channel TANH_FROM on (inside a tile of every width), the plain rounding below it.

Chains (chain_build, chain_reference): the dyadic case of every form of bneck_cases.FORMS with a, the weights and the biases and
residual of each stage scaled by powers of two (CHAIN_EXP), recomputed stage by stage with each stage rounded to f16 - scaling does
not commute with rounding on the subnormal grid, so nothing is derived from the unscaled reference. "sub": a and w2 subnormal or
nearly, b, y and a' around 2^-18 .. 2^-14; "ovf": b and y reach inf in LDS, and the next stage must give inf, NaN (inf times a zero
weight, inf - inf) and, after ReLU, 0 exactly where the three float64 convolutions here do."""
import functools

import numpy as np

import bneck_cases as B
import dyadic_cases as D
from bits import diff_bits

G = D.G
F16_MAX, F16_OVF = 65504.0, 65520.0            # the largest f16, and the tie between it and 2^16: rounds to inf
SUB_T = -16                                    # total exponent of the subnormal family ...
SUB_T_CASE = {"fp8_128_256_k3": -14}           # ... but this case's residual k / 1024 must stay an f16 value: k 2^-24
SUB_MOVED = ("stem_n2_S30", "stem_n1_S34", "fp8_128_256_k3", "fp8_128_200_k3s2")
SUB_FAMILIES = ("sub_x", "sub_w", "sub_out")
TANH_FROM = 100
TANH_T = (15, 0, -18, -14)                     # ovf_tanh: total exponent of channel o is TANH_T[o % 4]
TANH_ZERO = (6, 102)                           # ... but these have zero weights and bias 0: pre-activation +0
TANH_NEG = (7, 103)                            # ... and these zero weights and bias -2^-26: rounds to -0 / tanh of a tiny negative
# the overflow family's total exponent per case (tests/test_range_cases.py asserts the inf share and the maximum it gives)
OVF_T = {"head_3x3": 14, "levels_k3": 14, "levels_k1": 15, "big_64_256_k3": 14, "big_256_512_k1": 15, "big_64_351_k3": 15,
         "deep_k2048": 13, "split_64_256_k3": 14, "split_512_351_k1": 14, "rem96_k3": 15, "dual_s2": 15, "stem_n2_S30": 14,
         "stem_n1_S34": 14, "fp8_128_256_k3": 14, "fp8_256_512_k1": 14, "fp8_128_200_k3s2": 14}
OVF_RES_T, OVF_RES_EXTRA = 12, 2               # ovf_res: conv and bias at 2^12 (never past 65504), the residual at 2^14 (|res| <= 2^15)


def families(cid):
    kind = D.CASES[cid][0]
    f = ["sub_out", "ovf"] if kind == "fp8" else list(SUB_FAMILIES) + ["ovf"]
    if cid == "head_3x3":
        f.append("ovf_res")
    if cid == "big_256_512_k1":
        f.append("ovf_tanh")
    return f


VARIANTS = [f"{cid}/{fam}" for cid in D.CASE_IDS for fam in families(cid)]
RANGE_FAMILIES = SUB_FAMILIES + ("ovf",)      # the families every GPU test of the grid runs (fp8: sub_out and ovf)


def variants(cid):
    return [f"{cid}/{fam}" for fam in families(cid)]


def _cout(base):
    return (base["wi"] if base["kind"] == "fp8" else base["w"]).shape[0]


def exponents(vid):
    """(a, b[cout]): x is scaled by 2^a, channel o's weights by 2^b[o]; a + b is the channel's total exponent t."""
    cid, fam = vid.split("/")
    base = D.build(cid)
    o = np.arange(_cout(base))
    if fam in SUB_FAMILIES:
        t = np.full(len(o), SUB_T_CASE.get(cid, SUB_T))
    elif fam == "ovf_tanh":
        t = np.array(TANH_T)[o % len(TANH_T)]
    else:
        t = np.full(len(o), OVF_RES_T if fam == "ovf_res" else OVF_T[cid])
    if base["kind"] == "fp8":
        return 0, t
    if fam == "sub_x":
        return -18, t + 18
    if fam == "sub_w":
        return int(t[0]) + 18, np.full(len(o), -18)
    if fam == "ovf_tanh":
        return 0, t
    a = int(t.max()) // 2                      # sub_out: (-8, -8), x and w = k 2^-14: normal; ovf: half each
    return a, t - a


@functools.lru_cache(maxsize=None)
def build(vid):
    """The variant's tensors (float32, read-only), with the keys of dyadic_cases.build; t [cout] is the channels' total exponent."""
    cid, fam = vid.split("/")
    base = D.build(cid)
    a, b = exponents(vid)
    t = a + b
    fa, fb, ft = np.float32(2.0) ** a, (2.0 ** b).astype(np.float32), (2.0 ** t).astype(np.float32)
    c = dict(base, id=vid, base=cid, family=fam, a=a, b=b, t=t)
    wshape = (-1,) + (1,) * (base["wi" if base["kind"] == "fp8" else "w"].ndim - 1)
    if base["kind"] == "fp8":
        c["scale"] = base["scale"] * ft
    else:
        for k in ("x", "x1", "x2"):
            if base.get(k) is not None:
                c[k] = base[k] * fa
        c["w"] = base["w"] * fb.reshape(wshape)
    c["bias"] = base["bias"] * ft
    if base["res"] is not None:
        c["res"] = base["res"] * (ft * np.float32(2.0 ** OVF_RES_EXTRA) if fam == "ovf_res" else ft)
    if fam == "ovf_tanh":
        c["act"] = 2
        w, bias = c["w"].copy(), c["bias"].copy()
        w[list(TANH_ZERO + TANH_NEG)] = 0
        bias[list(TANH_ZERO)] = 0
        bias[list(TANH_NEG)] = -2.0 ** -26
        c.update(w=w, bias=bias)
    if fam == "ovf" or (fam in SUB_FAMILIES and cid in SUB_MOVED):
        c["bias"] = (c["bias"].astype(np.float64) + _moves(cid, fam == "ovf")).astype(np.float32)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _pre_of(c):
    """conv + bias + res of a case's own tensors in float64 (exact: every term a multiple of one grid per channel)."""
    A, W, side, scale, shape = D._gemm(c)
    D._GEMM.pop(c["id"], None)                 # (the variants' matrices are not kept: the references below are)
    return ((A @ W.T) * scale + side).reshape(shape)


@functools.lru_cache(maxsize=None)
def _base_pre(cid):
    return _pre_of(D.build(cid))


def _targets(grid, act, ovf):
    """The values the moved biases put one output each on: (value, channels)."""
    if not ovf:
        return [grid] * 16 + [-grid] * 4
    pos = [F16_OVF] * 8 + [F16_OVF - grid] * 8 + [F16_MAX] * 8
    return pos if act else pos + [-v for v in pos]


@functools.lru_cache(maxsize=None)
def _moves(cid, ovf):
    """The bias move per channel (float64, multiples of the grid 2^(t - G)): for each target value the unused channel that has an
    output nearest to it is moved so that this output sits exactly on it."""
    base = D.build(cid)
    t = OVF_T[cid] if ovf else SUB_T_CASE.get(cid, SUB_T)
    pre = _base_pre(cid).reshape(-1, _cout(base)) * 2.0 ** t
    grid = 2.0 ** (t - G)
    delta = np.zeros(pre.shape[1])
    used = np.zeros(pre.shape[1], bool)
    for target in _targets(grid, base["act"], ovf):
        d = np.abs(pre - target).min(0)
        d[used] = np.inf
        o = int(np.argmin(d))
        m = int(np.argmin(np.abs(pre[:, o] - target)))
        delta[o] = target - pre[m, o]
        used[o] = True
    return delta


_PRE, _REF = {}, {}


def _key(vid):
    cid, fam = vid.split("/")
    return f"{cid}/sub" if fam in SUB_FAMILIES else vid


def pre(vid):
    """The exact pre-activation sums (float64), computed once per family from the variant's own scaled tensors (the three subnormal
    placements share theirs: tests/test_range_cases.py proves they are equal)."""
    k = _key(vid)
    if k not in _PRE:
        p = _pre_of(build(vid))
        p.setflags(write=False)
        _PRE[k] = p
    return _PRE[k]


def relu(v):
    return np.where(v > 0, v, 0.0)             # (np.maximum propagates NaN and may keep -0; the spec and the C oracle do neither)


def exact(vid):
    """act(pre) in float64 for act 0 / 1 (ovf_tanh has reference() only)."""
    c = build(vid)
    assert c["act"] in (0, 1)
    return relu(pre(vid)) if c["act"] else pre(vid)


def h16(v):
    with np.errstate(over="ignore"):
        return np.asarray(v).astype(np.float16).astype(np.float32)


def reference(vid, oracle=None):
    """The specification's output (float32 array, computed once). ovf_tanh needs the oracle module for spec_tanhf."""
    k = _key(vid)
    if k not in _REF:
        if vid.endswith("/ovf_tanh"):
            p = pre(vid)
            p32 = p.astype(np.float32)
            assert np.array_equal(p32.astype(np.float64), p)           # the float32 sum is the exact one
            r = h16(p)
            ch = p32[..., TANH_FROM:]
            th = np.array([oracle.spec_tanhf(v) for v in ch.reshape(-1)], np.float32).reshape(ch.shape)
            r[..., TANH_FROM:] = h16(th)
        else:
            r = h16(exact(vid))
        r.setflags(write=False)
        _REF[k] = r
    return _REF[k]


def magnitude_bits(vid):
    """log2 of the largest (sum |x| |w| |scale| + |bias| + |res|) / grid over the outputs: below 22, float32 holds every partial sum."""
    c = build(vid)
    m = D.magnitude(c)
    D._GEMM.pop(vid, None)
    return float(np.log2((m / 2.0 ** (c["t"] - float(G))).max()))


# ---- mutants of the reference: what a subtly wrong kernel would compute ----
_SUBN = 2.0 ** -14


def _flush(v):
    return np.where(np.abs(v) < _SUBN, np.copysign(0.0, v), v).astype(v.dtype)


def _with(vid, **kw):
    c = dict(build(vid), **kw)
    c["id"] = vid + "#mutant"
    p = _pre_of(c)
    return h16(relu(p) if c["act"] else p)


def mutant_flush_x(vid):
    """Subnormal x (x1, x2) reads as zero."""
    c = build(vid)
    return _with(vid, **{k: _flush(c[k]) for k in ("x", "x1", "x2") if c.get(k) is not None})


def mutant_flush_w(vid):
    return _with(vid, w=_flush(build(vid)["w"]))


def mutant_flush_out(vid):
    """Subnormal results are written as (signed) zero."""
    return _flush(reference(vid))


def mutant_saturate(vid):
    r = reference(vid)
    return np.where(np.isinf(r), np.copysign(np.float32(F16_MAX), r), r)


def mutant_relu_after_round_keeps_sign(vid):
    """Rounds first, then max(o, 0) on the f16 value with a maximum that returns its first operand on a tie: a tiny negative sum
    becomes -0 and stays -0."""
    r = h16(pre(vid))
    return np.where(r > 0, r, np.where(np.signbit(r) & (r == 0), np.float32(-0.0), np.float32(0.0))).astype(np.float32)


def mutant_rtz(vid):
    return D.rtz16(exact(vid))


MUTANTS = {"flush_x": mutant_flush_x, "flush_w": mutant_flush_w, "flush_out": mutant_flush_out, "saturate": mutant_saturate,
           "relu_after_round_keeps_sign": mutant_relu_after_round_keeps_sign, "rtz": mutant_rtz}


def aimed(vid):
    """The mutants a variant must tell from the reference."""
    c = build(vid)
    fam = c["family"]
    if fam == "ovf_tanh":
        return []
    m = ["rtz"]
    if fam in SUB_FAMILIES:
        m.append("flush_out")
        if c["act"]:
            m.append("relu_after_round_keeps_sign")
        if fam == "sub_x":
            m.append("flush_x")
        if fam == "sub_w":
            m.append("flush_w")
    elif fam == "ovf":
        m.append("saturate")
    return m


def census(vid):
    """The measures tests/test_range_cases.py bounds."""
    c = build(vid)
    ref = reference(vid) if c["family"] != "ovf_tanh" else None
    out = dict(bits=magnitude_bits(vid))
    if ref is None:
        return out
    p, v = pre(vid), exact(vid)
    fin = np.isfinite(ref) & (ref != 0)
    out.update(size=ref.size, subnormal=float(((ref != 0) & (np.abs(ref) < _SUBN)).mean()),
               tie=float((D.is_tie(np.where(fin, v, 1.0)) & fin).sum() / max(int(fin.sum()), 1)),
               to_zero=int(((v != 0) & (ref == 0)).sum()), relu_neg_tiny=int(((p < 0) & (p > -2.0 ** -25)).sum()) if c["act"] else 0,
               minus_zero=int(((ref == 0) & np.signbit(ref)).sum()), inf=float(np.isinf(ref).mean()), max=float(np.abs(p).max()),
               on_ovf=int((v == F16_OVF).sum()), below_ovf=int((v == F16_OVF - 2.0 ** (c["t"].max() - float(G))).sum()), on_max=int((v == F16_MAX).sum()),
               on_novf=int((v == -F16_OVF).sum()), below_novf=int((v == -F16_OVF + 2.0 ** (c["t"].max() - float(G))).sum()), on_nmax=int((v == -F16_MAX).sum()))
    if c["family"] == "ovf_res":
        alone = p - c["res"].astype(np.float64)
        out.update(alone_max=float(np.abs(alone).max()), res_over=int(np.isinf(ref).sum()))
    for name in aimed(vid):
        d = diff_bits(MUTANTS[name](vid), ref)
        out[name] = int(d.sum()) if name == "relu_after_round_keeps_sign" else float(d.mean())
    return out


# ---- bottleneck chains ----
# family -> planes -> exponents (a, w2, w3, w1n): a 2^ea, w2 2^e2 (so bias2 and the two-source form's x2 2^(ea + e2) = 2^s1), w3 2^e3
# (bias3, res 2^(s1 + e3) = 2^s2), w1n 2^e1 (bias1n 2^(s2 + e1) = 2^s3); bneck_xn_f16's a IS b, scaled 2^s1 = 2^ea.
#   sub: b, y at 2^-18, a' at 2^-20: every a (k 2^-19, |k| <= 16; bneck_xn_f16: k 2^-24) and every nonzero b is subnormal, about half
#        of y and a'. res and x2 are ROUNDED to f16 after the scaling (k 2^-28 is no f16 value): multiples of 2^-24, so of the grid.
#   ovf: s1, s2, s3 put the largest b, y and a' at 1.2 .. 2 times 65504: a few b and y are inf in LDS, and a' has inf, NaN -> 0, finite.
CHAIN_EXP = {"sub": {64: (-14, -4, 0, -2), 128: (-14, -4, 0, -2), 256: (-18, 0, 0, -2)},
             "ovf": {64: (7, 6, -2, -3), 128: (7, 6, -2, -3), 256: (11, 0, 0, -3)}}
CHAIN_FAMILIES = ("sub", "ovf")


@functools.lru_cache(maxsize=None)
def chain_build(form, fam):
    """The scaled dyadic case of one form (a dict with the keys of bneck_cases.build), s = (s1, s2, s3) the stages' exponents."""
    sym, planes, tm, nxt, dual = B.FORMS[B.FORM_IDS.index(form)]
    base = B.build(planes, B.DYADIC + ("_x2s1" if dual else ""))
    ea, e2, e3, e1 = CHAIN_EXP[fam][planes]
    s1 = ea + (0 if base["xn"] else e2)
    s2 = s1 + e3
    s3 = s2 + e1
    f = lambda v, e: None if v is None else (v * np.float32(2.0 ** e)).astype(np.float32)
    r16 = lambda v: None if v is None else h16(v)
    c = dict(base, id=f"{base['id']}/{fam}", family=fam, s=(s1, s2, s3), a=f(base["a"], s1 if base["xn"] else ea), w2=f(base["w2"], e2),
             bias2=f(base["bias2"], s1), w3=f(base["w3"], e3), bias3=f(base["bias3"], s2), res=r16(f(base["res"], s2)), x2=r16(f(base["x2"], s1)),
             w1n=f(base["w1n"], e1), bias1n=f(base["bias1n"], s3))
    if base["xn"]:
        # a' * inv_scale = 128 times (even channels: past 448) and twice (odd channels: down into E4M3's subnormals) the unscaled case's
        c["inv_scale"] = (base["inv_scale"] * 2.0 ** (np.where(np.arange(256) % 2, 1, 7) - float(s3))).astype(np.float32)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def chain_stages(c, absolute=False):
    """bneck_cases.stages with ReLU as v > 0 ? v : 0 (a NaN becomes 0) and inf, NaN allowed: the three pre-activation sums (float64)
    and the rounded b, y, a' (float32). absolute: sum |x| |w| + |bias| + |res| with the same rounded tensors in between."""
    f = np.abs if absolute else (lambda v: v)
    d = lambda v: f(np.asarray(v, np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        if c["xn"]:
            s1, b = None, c["a"]
        else:
            s1 = B._conv3x3(d(c["a"]), d(c["w2"]), c["stride"], c["P"], c["Q"]) + d(c["bias2"])
            b = h16(relu(B._conv3x3(c["a"], c["w2"], c["stride"], c["P"], c["Q"]) + c["bias2"].astype(np.float64)))
        k = np.concatenate([b, B._x2_rows(c)], -1) if c["x2"] is not None else b
        side = c["res"] if c["res"] is not None else 0.0
        s2 = d(k) @ d(c["w3"]).T + d(c["bias3"]) + d(side)
        y = h16(relu(k.astype(np.float64) @ c["w3"].astype(np.float64).T + c["bias3"] + side))
        s3 = d(y) @ d(c["w1n"]).T + d(c["bias1n"])
        an = h16(relu(y.astype(np.float64) @ c["w1n"].astype(np.float64).T + c["bias1n"]))
    return (s1, s2, s3), (b, y, an)


_CHAIN_REF = {}


def chain_reference(form, fam, oracle=None):
    """dict(b, y, a_next[, a_next8]) of chain_build(form, fam), computed once per (planes, case)."""
    c = chain_build(form, fam)
    key = (c["planes"], c["id"])
    if key not in _CHAIN_REF:
        b, y, an = chain_stages(c)[1]
        _CHAIN_REF[key] = dict(b=b, y=y, a_next=an)
    r = _CHAIN_REF[key]
    if c["xn"] and oracle is not None and "a_next8" not in r:
        with np.errstate(invalid="ignore", over="ignore"):
            r["a_next8"] = oracle.quantize_e4m3(r["a_next"] * c["inv_scale"])
    return r
