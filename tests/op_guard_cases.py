"""The shapes at which a conv kernel's store guards decide something, for every (tile, form) of kConvTiles: generated from the
compiled table (capi.conv_forms(): R rows and T channels per tile, the forms it is instantiated in), never from retyped constants.
Not a test: tests/test_gpu_op_guards.py runs the cases through the single-op entry points, whose staging puts 0xFF guards around
every output and NaN bands around every input (Bounds), and compares each with the CPU oracle bit for bit.

Rows.   M = 1, R - 1, R, R + 1, 2 R + 1 as ONE image of M x 1 pixels under a 1x1 convolution: the last row tile holds 1, R - 1, R,
        1 and 1 rows. R + 1 is odd, so two equal images cannot make it: the two-image case has R / 2 + 1 rows per image, M = R + 2 -
        the image boundary falls inside the first tile, two rows into the second. One 3x3, pad 1 case at 2 images of 5 x 7.
Channels.  cout = 8, T - 8, T, T + 8 where positive: a lone 8-channel chunk, a tile short of one chunk, a full tile, a second tile
        of one chunk. The rule for shapes an entry point refuses: the fused tail runs on exactly 256 channels (its entry answers
        YH_EINVAL otherwise), so its cases keep cout = 256 = T only.
Forms.  plain (and with a residual); dense 1x1 (LIN) where the tile has it - the same launches with tune.op_xgap = 8 stay PLAIN;
        the streaming 3x3 form; multi-level with level sizes [isqrt(R - 10), 3, 1], so two level boundaries and the image's end fall
        inside the first tile (and, with two images, an image boundary too); two-source at stride2 1 and 2; upsampled residual;
        fused tail; forced split-K with 2 and 3 slices on the tiles that have it (two-source: 64 + 128 channels, so the slices start
        before, at and after the switch of sources).
Data.   conv_form_cases' integer grids: x in [-3, 3], w in [-2, 2], bias in [-4, 4], residuals in [-5, 5]; fp8: integers in
        [-4, 4] / [-3, 3] as E4M3 codes, scales 2^-3 .. 2^0. 64 input channels (128 on fp8 tiles and under a split-K of 2, 192
        under one of 3; 3 on the small-C tile): sum |x| |w| <= 9 * 192 * 6 < 2^24, so every float32 partial sum of any order is
        exact and the one f16 rounding of the specification is the only rounding. The upsampled residual is the oracle's f16
        bilinear of integers; the oracle adds it in the kernel's order, (acc + bias) + res."""
import math
import zlib

import numpy as np

from conv_form_cases import TILES

SPLIT_CIN = {0: 64, 2: 128, 3: 192}      # kslices -> input channels: one K step of 64 per slice


def _rows(R):
    """(tag, n, P) of the 1x1 cases: n images of P x 1 pixels."""
    return [(f"m{m}", 1, m) for m in (1, R - 1, R, R + 1, 2 * R + 1)] + [(f"m{R + 2}-2img", 2, R // 2 + 1)]


def _couts(T, form):
    return [256] if form == "TAIL" else [c for c in (8, T - 8, T, T + 8) if c > 0]


def cases_of(row):
    """Every case of one row of the table: dicts with kind (the entry point), form (what the launch must run as), shape, tuning."""
    R, T, fp8, out = row["tm"], row["tch"], row["fp8"], []
    smallc = row["tile"] == TILES["64x256_SMALLC"]

    def add(kind, form, tag, **kw):
        c = dict(dict(kslices=0, xgap=0, res=False, act=1, stride2=1), kind=kind, form=form, tile=row["tile"], R=R, T=T, **kw)
        c["id"] = f"t{row['tile']}-{form}-{kind}-{tag}-c{c['cout']}" + ("-res" if c["res"] else "")
        out.append(c)

    for form in row["forms"]:
        ks = (2, 3) if form.endswith("SPLITK") else (0,)
        for cout in _couts(T, form):
            for k_sl in ks:
                cin = 3 if smallc else 128 if fp8 and not k_sl else SPLIT_CIN[k_sl]
                sl = f"-s{k_sl}" if k_sl else ""
                if form in ("PLAIN", "LIN", "K3", "SPLITK"):
                    kind = "fp8" if fp8 else "conv"
                    xgap = 8 if form == "PLAIN" and "LIN" in row["forms"] else 0
                    if form != "K3":
                        for tag, n, P in _rows(R):
                            add(kind, form, tag + sl, n=n, h=P, w=1, cin=cin, cout=cout, k=1, kslices=k_sl, xgap=xgap)
                            if P in (R + 1, R // 2 + 1):
                                add(kind, form, tag + sl, n=n, h=P, w=1, cin=cin, cout=cout, k=1, kslices=k_sl, xgap=xgap, res=True)
                    # 3x3 on this tile: the streaming tile's own form where it has one, PLAIN elsewhere (a split-K stays a split-K)
                    if form in ("K3", "SPLITK") or (form == "PLAIN" and "K3" not in row["forms"]):
                        add(kind, form, "k3-2x5x7" + sl, n=2, h=5, w=7, cin=cin, cout=cout, k=3, kslices=k_sl, res=form == "K3")
                    if form == "SPLITK" and "RESUP" in row["forms"]:
                        for tag, n, P in _rows(R):
                            add("resup", form, tag + sl, n=n, h=P, w=1, cin=cin, cout=cout, k=1, kslices=k_sl)
                elif form in ("ML", "ML_SPLITK"):
                    levels = (math.isqrt(R - 10), 3, 1)
                    for n in (1, 2):
                        for k in (1, 3):
                            add("levels_fp8" if fp8 else "levels", form, f"n{n}k{k}" + sl, n=n, levels=levels, cin=cin, cout=cout, k=k, kslices=k_sl)
                elif form in ("DUAL", "DUAL_SPLITK"):
                    for s2 in (1, 2):
                        for tag, n, P in _rows(R):
                            add("dual", form, f"{tag}-x{s2}" + sl, n=n, h=P, w=1, cin=64, c2=128 if k_sl else 64, cout=cout, k=1, kslices=k_sl, stride2=s2)
                elif form == "RESUP":
                    for tag, n, P in _rows(R):
                        add("resup", form, tag, n=n, h=P, w=1, cin=cin, cout=cout, k=1)
                else:
                    assert form == "TAIL", form
                    kind = "tail_fp8" if fp8 else "tail"
                    for tag, n, P in _rows(R):
                        add(kind, form, tag, n=n, h=P, w=1, cin=cin, cout=cout, k=1)
                    add(kind, form, "k3-2x5x7", n=2, h=5, w=7, cin=cin, cout=cout, k=3)
    return out


def tuning(c):
    t = {} if c["cin"] == 3 else {"op_tile": c["tile"]}       # (cin = 3 takes the small-C tile whatever tune.op_tile says)
    if c["kslices"]:
        t["op_kslices"] = c["kslices"]
    if c["xgap"]:
        t["op_xgap"] = c["xgap"]
    return t


def build(c):
    """The case's tensors: float32 arrays of small integers (fp8 kinds: the integers the codes decode to)."""
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    ints = lambda lim, *shape: rng.integers(-lim, lim + 1, shape).astype(np.float32)
    fp8 = c["kind"] in ("fp8", "levels_fp8", "tail_fp8")
    xl, wl = (4, 3) if fp8 else (3, 2)
    cout, cin, k, n = c["cout"], c["cin"], c["k"], c["n"]
    t = dict(bias=ints(4, cout), w=ints(wl, cout, k, k, cin))
    if fp8:
        t["scale"] = (2.0 ** rng.integers(-3, 1, cout)).astype(np.float32)
    if c["kind"] in ("levels", "levels_fp8"):
        t["x"] = ints(xl, n, sum(s * s for s in c["levels"]), cin)
        return t
    t["x"] = ints(xl, n, c["h"], c["w"], cin)
    if c["kind"] == "dual":
        s2 = c["stride2"]
        t["x2"] = ints(xl, n, (c["h"] - 1) * s2 + 1, (c["w"] - 1) * s2 + 1, c["c2"])
        t["w"] = ints(wl, cout, cin + c["c2"])
    elif c["kind"] == "resup":
        t["res_lo"] = ints(5, n, (c["h"] + 1) // 2, 1, cout)
    elif c["kind"] in ("tail", "tail_fp8"):
        t.update(w2=ints(2, 32, 256), bias2=ints(4, 32))
    if c["res"]:
        t["res"] = ints(5, n, c["h"], c["w"], cout)
    return t


def _act(v, act):
    return np.where(v > 0, v, 0.0) if act else v


def _f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float32)


def reference(c, t, oracle):
    """The expected output, from the CPU oracle alone."""
    kind, cout, k, act = c["kind"], c["cout"], c["k"], c["act"]
    pad = k // 2
    z = np.zeros(cout, np.float32)

    def conv(x):      # one 'same' stride-1 convolution of the case's first layer on an NHWC image
        if kind in ("fp8", "levels_fp8", "tail_fp8"):   # exact in float64 from the exact accumulator, rounded once
            v = oracle.conv2d(x, t["w"], z, 1, pad, None, 0, f16=False).astype(np.float64) * t["scale"].astype(np.float64) + t["bias"].astype(np.float64)
            return _f16(_act(v + t["res"] if c["res"] else v, act))
        return oracle.conv2d(x, t["w"], t["bias"], 1, pad, t.get("res"), act, f16=True)

    if kind in ("levels", "levels_fp8"):
        out, off = [], 0
        for s in c["levels"]:
            out.append(conv(np.ascontiguousarray(t["x"][:, off:off + s * s]).reshape(c["n"], s, s, c["cin"])).reshape(c["n"], s * s, cout))
            off += s * s
        return np.concatenate(out, 1)
    if kind == "dual":
        s2 = c["stride2"]
        cat = np.ascontiguousarray(np.concatenate([t["x"], t["x2"][:, ::s2, ::s2]], -1))
        return oracle.conv2d(cat, t["w"].reshape(cout, 1, 1, -1), t["bias"], 1, 0, None, act, f16=True)
    if kind == "resup":
        up = oracle.bilinear(t["res_lo"], c["h"], c["w"], f16=True)
        return oracle.conv2d(t["x"], t["w"], t["bias"], 1, 0, up, act, f16=True)
    r = conv(t["x"])
    if kind in ("tail", "tail_fp8"):
        r = oracle.conv2d(r, t["w2"].reshape(32, 1, 1, 256), t["bias2"], 1, 0, None, 1, f16=True)
    return r
