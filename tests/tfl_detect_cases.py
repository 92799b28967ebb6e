"""Deterministic cases for the TFLite detection tail (csrc/tfl_detect.hip K1q .. K4q; DESIGN.md §11 "TFLite detections"), built
ON THE QUANTISED GRID: every tensor is bytes (or float32) with a scale and a zero point, as a .tflite model leaves it - the f16
cases of tests/tail_cases.py do not lie on one. Not a test: tests/test_tfl_detect_cases.py proves on the CPU that every case does
what it claims, tests/test_gpu_tfl_detect.py runs them through yh_tfl_op_detect. numpy only.

A case is a dict: loc [n][P][4], conf [n][P][C], mask [n][P][32], proto [n][hp][wp][32]; quant role -> (scale, zero_point);
priors [P][4]; cfg (top_k, max_dets, conf_thresh, nms_thresh); plus what it claims about itself.

The host supplies the priors, so a case chooses them: grid_priors puts P disjoint squares on a 16 x 16 grid (pitch 1/16, side
0.05), and with loc at its zero point a prior's box is the prior itself. Equal conf rows give equal scores (the same operations on
the same bytes): exact ties across priors, and - two columns holding one byte - across classes."""
import numpy as np

import tail_cases as T

decode, suppressors = T.decode, T.suppressors     # the geometry helpers are shared with the f16 cases

F = np.float32
P0 = 250                   # not a multiple of 3 or of 64: K1q's second workgroup holds 122 priors, its last wave 58
DT = {"u8": np.uint8, "i8": np.int8, "f32": np.float32}
LIM = {"u8": (0, 255), "i8": (-128, 127)}
# kind combinations (loc, conf, mask, proto) of the op_detect sweep
COMBOS = {
    "all_u8": ("u8", "u8", "u8", "u8"), "all_i8": ("i8", "i8", "i8", "i8"), "all_f32": ("f32", "f32", "f32", "f32"),
    "u8proto_i8mask": ("u8", "i8", "i8", "u8"), "i8proto_u8mask": ("i8", "u8", "u8", "i8"), "f32proto_u8mask": ("u8", "u8", "u8", "f32"),
}
ZPS = {"u8": (0, 128, 255), "i8": (-128, 0, 127)}
CFG = dict(top_k=200, max_dets=100, conf_thresh=0.05, nms_thresh=0.5)
POW2 = dict(loc=0.125, conf=0.0625, mask=0.0078125, proto=0.0625)     # every scale a power of two: rule 3 = rule 4
ODD = dict(loc=0.125, conf=0.0625, mask=0.0173, proto=0.05)           # the issue's 0.05 / 0.0173: the chain rounds


def grid_priors(P=P0, side=0.05):
    k = np.arange(P)
    return np.stack([(k % 16 + 0.5) / 16, (k // 16 + 0.5) / 16, np.full(P, side), np.full(P, side)], 1).astype(F)


def code(kind, zp, v):
    """The element of `kind` that stands for the integer value v above the zero point (v = q - z)."""
    q = np.asarray(v, np.int64) + zp
    lo, hi = LIM[kind]
    assert q.min() >= lo and q.max() <= hi, (kind, zp, int(q.min()), int(q.max()))
    return q.astype(DT[kind])


def random_case(kinds, zps, n, C, hp, wp, seed, P=P0, scales=POW2, cfg=None, priors=None):
    """n images of random bytes: conf logits spread over the whole byte (with scale 1/16 most priors give one candidate), loc a
    few codes around its zero point (boxes near their priors: neighbours overlap now and then), coefficients and prototypes of
    both signs. A float32 tensor holds the values a quantised one with (scale, zero point 0) would."""
    rng = np.random.default_rng(seed)
    shapes = dict(loc=(n, P, 4), conf=(n, P, C), mask=(n, P, 32), proto=(n, hp, wp, 32))
    spread = dict(loc=40, conf=128, mask=128, proto=128)
    case, quant = {}, {}
    for role, kind, zp in zip(("loc", "conf", "mask", "proto"), kinds, zps):
        if kind == "f32":
            v = rng.integers(-spread[role], spread[role], shapes[role])
            case[role] = (v.astype(F) * F(scales[role])).astype(F)
        else:
            lo, hi = LIM[kind]
            q = np.clip(rng.integers(-spread[role], spread[role], shapes[role]) + zp, lo, hi)
            case[role] = q.astype(DT[kind])
            quant[role] = (scales[role], zp)
    return dict(case, quant=quant, priors=grid_priors(P) if priors is None else priors, cfg=dict(cfg or CFG), n=n, P=P, C=C, hp=hp, wp=wp)


def quiet(kinds, zps, n, C, hp, wp, seed, P=P0, scales=POW2, cfg=None, priors=None):
    """A case without any candidate - background far above every class - whose loc sits on its zero point (box = prior) and whose
    other tensors are random_case's; the builders below raise single conf rows out of it."""
    case = random_case(kinds, zps, n, C, hp, wp, seed, P, scales, cfg, priors)
    for role, kind, zp in zip(("loc", "conf"), kinds[:2], zps[:2]):
        assert kind != "f32"
        case[role][...] = code(kind, zp, 0)
    k, z = kinds[1], zps[1]
    lo, hi = LIM[k]
    case["conf"][..., 0] = hi                    # background: the largest byte
    case["conf"][..., 1:] = lo                   # classes: the smallest (255 codes x 1/16 = 16 below: e^-16 / 1 < 0.05)
    case["bg"], case["off"] = hi, lo
    return case


def raise_class(case, b, prior, cls, below_bg):
    """Prior `prior` of image b becomes a candidate of foreground class cls (column cls + 1): its logit `below_bg` codes under the
    background's (0: p = 1/2 at two live columns)."""
    case["conf"][b, prior, cls + 1] = int(case["bg"]) - below_bg


def ties(kinds=COMBOS["all_u8"], zps=(128, 128, 128, 128), C=6, hp=16, wp=16):
    """Exact ties: priors 3, 77, 130 (two workgroups of K1q) carry one conf row - classes 1 and 3 on the same byte - so six
    candidates share one score: inside a class they rank by prior, across classes by class."""
    case = quiet(kinds, zps, 1, C, hp, wp, 31)
    for pr in (130, 3, 77):
        raise_class(case, 0, pr, 1, 2)
        raise_class(case, 0, pr, 3, 2)
    raise_class(case, 0, 200, 2, 0)              # and one better detection of its own
    case["tied"] = [(1, 3), (1, 77), (1, 130), (3, 3), (3, 77), (3, 130)]
    return case


def topk_cut(n_cand, top_k=8, kinds=COMBOS["all_u8"], zps=(128, 128, 128, 128), C=6, hp=16, wp=16):
    """n_cand = top_k - 1 / top_k / top_k + 1 candidates in class 2, the last three of them tied: the cut at top_k falls inside
    the tie and keeps the smaller priors."""
    case = quiet(kinds, zps, 1, C, hp, wp, 32, cfg=dict(CFG, top_k=top_k))
    priors = [240 - 7 * i for i in range(n_cand)]          # descending priors: a better score at a larger prior
    for i, pr in enumerate(priors):
        raise_class(case, 0, pr, 2, min(i, n_cand - 3))    # the last three share a byte
    case["cand_priors"], case["tie_priors"] = priors, sorted(priors[-3:])
    return case


def dets_cut(n_surv, max_dets=6, kinds=COMBOS["all_u8"], zps=(128, 128, 128, 128), C=6, hp=16, wp=16):
    """n_surv = max_dets - 1 / max_dets / max_dets + 1 survivors (disjoint boxes, no suppression), the last three tied across the
    classes 0, 2, 4: the cut at max_dets keeps the smaller classes."""
    case = quiet(kinds, zps, 1, C, hp, wp, 33, cfg=dict(CFG, max_dets=max_dets))
    for i in range(n_surv):
        tied = i >= n_surv - 3
        cls = (4, 2, 0)[n_surv - 1 - i] if tied else 1
        raise_class(case, 0, 10 + 9 * i, cls, n_surv - 3 if tied else i)
    case["tie_classes"] = [0, 2, 4]
    return case


def suppress_pair(on, kinds=COMBOS["all_u8"], zps=(128, 128, 128, 128), C=6, hp=16, wp=16):
    """Two candidates of one class on neighbouring priors 20 and 21; `on`: the worse one's box is moved onto the better one's
    (-100 codes of 1/8 = -12.5 loc units = one pitch to the left: IoU 1), and is suppressed. Otherwise both survive."""
    case = quiet(kinds, zps, 1, C, hp, wp, 34)
    raise_class(case, 0, 20, 1, 0)
    raise_class(case, 0, 21, 1, 3)
    if on:
        case["loc"][0, 21, 0] = code(kinds[0], zps[0], -100)     # cx moves by -100 / 8 * 0.1 * 0.05 = -0.0625: one pitch
    case["pair"] = (20, 21)
    return case


def threshold_group(kinds=COMBOS["all_u8"], zps=(128, 128, 128, 128), C=6, hp=16, wp=16):
    """Five priors share one score (and one better prior stands above it); conf_thresh is then set on that score and one ulp
    either side (thresholds())."""
    case = quiet(kinds, zps, 1, C, hp, wp, 35)
    for pr in (5, 64, 127, 128, 249):
        raise_class(case, 0, pr, 0, 20)
    raise_class(case, 0, 100, 0, 1)
    case["shared_priors"] = [5, 64, 127, 128, 249]
    return case


def thresholds(shared_score):
    s = F(shared_score)
    return [float(np.nextafter(s, F(0))), float(s), float(np.nextafter(s, F(1)))]


def empty_then_full(kinds=COMBOS["all_u8"], zps=(128, 128, 128, 128), C=6, hp=16, wp=16):
    """(a case without any candidate, a full random case of the same geometry): run one after the other on one handle."""
    return quiet(kinds, zps, 2, C, hp, wp, 36), random_case(kinds, zps, 2, C, hp, wp, 37)


WINDOWS = {   # box (cx, cy, w, h) -> the crop window it must give on a 16 x 16 map (x0, x1, y0, y1: pixels [x0, x1) x [y0, y1))
    "hang_left": ((0.02, 0.5, 0.3, 0.2), (0, 4, 6, 11)), "hang_right": ((0.97, 0.5, 0.3, 0.2), (13, 16, 6, 11)),
    "hang_top": ((0.5, 0.03, 0.2, 0.3), (6, 11, 0, 4)), "hang_bottom": ((0.5, 0.98, 0.2, 0.3), (6, 11, 13, 16)),
    "whole": ((0.5, 0.5, 1.5, 1.5), (0, 16, 0, 16)), "pixel_corner": ((-0.01, -0.01, 0.01, 0.01), (0, 1, 0, 1)),
    "out_right": ((1.3, 0.5, 0.1, 0.1), (0, 0, 0, 0)),
}


def windows(kinds=COMBOS["all_u8"], zps=(128, 128, 128, 128), C=6, hp=16, wp=16, scales=POW2):
    """One detection per entry of WINDOWS, its prior being the box (loc on its zero point): windows that hang over every edge,
    the whole map, a single pixel in the corner and a box beside the map (an empty window). Every prototype dot product is
    positive (prototypes and coefficients all above their zero points), so a mask IS its window."""
    names = list(WINDOWS)
    pri = grid_priors()
    at = [17 + 31 * i for i in range(len(names))]
    for pr, nm in zip(at, names):
        pri[pr] = WINDOWS[nm][0]
    case = quiet(kinds, zps, 1, C, hp, wp, 38, scales=scales, priors=pri)
    for i, pr in enumerate(at):
        raise_class(case, 0, pr, i % (C - 1), i)
    for role, kind, zp in (("mask", kinds[2], zps[2]), ("proto", kinds[3], zps[3])):
        if kind == "f32":
            case[role][...] = F(scales[role]) * F(3)
        else:
            case[role][...] = code(kind, zp, 1)      # (a zero point at the top of its type has no code above it: not for this case)
    case["at"], case["names"] = at, names
    return case


def band(kinds=COMBOS["all_u8"], zps=(128, 128, 128, 128), C=6, hp=16, wp=16, scales=ODD):
    """Pixels on and around S = 0 under the scales 0.05 / 0.0173. One detection whose window is the whole map; its coefficient 0
    is 3 codes above the zero point, the others random. Row 0 of the prototype map sits on the zero point (S = 0: off by rule 3),
    row 1 has channel 0 one code above and the rest on the zero point (S = 3: on, and inside the band), row 2 one code below
    (S = -3); the other rows are random_case's."""
    pri = grid_priors()
    pri[40] = (0.5, 0.5, 1.5, 1.5)
    case = quiet(kinds, zps, 1, C, hp, wp, 39, scales=scales, priors=pri)
    raise_class(case, 0, 40, 1, 0)
    case["mask"][0, 40, 0] = code(kinds[2], zps[2], 3)
    for row, v in ((0, 0), (1, 1), (2, -1)):
        case["proto"][0, row] = code(kinds[3], zps[3], 0)
        case["proto"][0, row, :, 0] = code(kinds[3], zps[3], v)
    case["rows"] = {0: 0, 1: 3, 2: -3}
    return case


def saturated(sign, kinds=COMBOS["all_u8"], C=6, hp=16, wp=16):
    """Every byte at an extreme. Prototypes at the top of their type over a zero point at the bottom (+255 each), coefficients
    likewise (sign > 0) or at the bottom over a zero point at the top (-255 each): |S| = 32 * 255^2 at every pixel. conf and loc
    hold only their extreme bytes too (loc's scale is small enough for the decode to stay finite)."""
    zp = {k: LIM[k] for k in ("u8", "i8")}
    zps = (zp[kinds[0]][0], zp[kinds[1]][0], zp[kinds[2]][0] if sign > 0 else zp[kinds[2]][1], zp[kinds[3]][0])
    case = quiet(kinds, zps, 1, C, hp, wp, 40, scales=dict(POW2, loc=0.0078125))
    rng = np.random.default_rng(41)
    lo, hi = LIM[kinds[0]]
    case["loc"][...] = np.where(rng.random(case["loc"].shape) < 0.5, lo, hi).astype(DT[kinds[0]])
    lo, hi = LIM[kinds[1]]
    case["conf"][..., 1:] = np.where(rng.random(case["conf"][..., 1:].shape) < 0.02, hi, lo).astype(DT[kinds[1]])
    case["mask"][...] = LIM[kinds[2]][1] if sign > 0 else LIM[kinds[2]][0]
    case["proto"][...] = LIM[kinds[3]][1]
    case["S"] = sign * 32 * 255 * 255
    return case


# ---------------------------------------------------------------------------------------------- small models for the setup rules
def heads_model(dtype="u8", P=20, C=6, hp=4, wp=5, break_rule=None):
    """A five-operator model (tfl_builder_q objects) with the four head outputs: input x [1,P,4]; loc = QUANTIZE(x); conf and mask
    = x joined with constants along the last axis; proto = the same join reshaped to [1,hp,wp,32] (hp * wp = P). break_rule bends
    one output so that exactly one rule of yh_tfl_detect_setup fails:
      "loc5" loc is [1,P,5]; "C1" conf is [1,4P,1]; "mask16" mask is [1,2P,16]; "proto16" proto is [1,hp,2wp,16]; "P" conf is
      [1,P/2,2C]; "scale0" / "scale_inf" / "scale_neg" mask's scale is 0 / inf / -1; "per_channel" mask carries 32 scales;
      "axis0" a fifth output joins along the image axis (the model runs one image per invoke); "kind" loc is an int32 tensor;
      "const_head" mask is a constant of the model (stored once, not per image); "zp_range" mask's zero point lies outside its type."""
    from tfl_builder_q import Model, Op, T as QT
    assert hp * wp == P and P % 2 == 0
    rng = np.random.default_rng(50)
    lo, hi = LIM[dtype]
    m = Model()
    const = lambda name, shape: m.add(QT(name, shape, dtype, data=rng.integers(lo, hi + 1, shape).astype(DT[dtype]), scale=0.0625, zp=lo + 128))
    x = m.add(QT("x", (1, P, 4), dtype, scale=0.0625, zp=lo + 128))
    loc = m.add(QT("loc", (1, P, 4), dtype, scale=0.125, zp=lo + 120))
    m.ops.append(Op("QUANTIZE", [x], [loc]))
    if break_rule == "loc5":
        loc5 = m.add(QT("loc5", (1, P, 5), dtype, scale=0.0625, zp=lo + 128))
        m.ops.append(Op("CONCATENATION", [x, const("l1", (1, P, 1))], [loc5], axis=2))
        loc = loc5
    conf = m.add(QT("conf", (1, P, C), dtype, scale=0.0625, zp=lo + 128))
    m.ops.append(Op("CONCATENATION", [x, const("c1", (1, P, C - 4))], [conf], axis=2))
    j = m.add(QT("joined", (1, P, 32), dtype, scale=0.0625, zp=lo + 128))
    m.ops.append(Op("CONCATENATION", [x, const("j1", (1, P, 28))], [j], axis=2))

    def reshaped(name, src, shape, **kw):
        y = m.add(QT(name, shape, dtype, **dict(dict(scale=0.0625, zp=lo + 128), **kw)))
        m.ops.append(Op("RESHAPE", [src], [y], new_shape=list(shape)))
        return y
    if break_rule == "C1":
        conf = reshaped("conf1", x, (1, 4 * P, 1))
    if break_rule == "P":
        conf = reshaped("confP", conf, (1, P // 2, 2 * C))
    bad_scale = {"scale0": 0.0, "scale_inf": float("inf"), "scale_neg": -1.0}
    if break_rule in bad_scale:
        mask = reshaped("mask", j, (1, P, 32), scale=bad_scale[break_rule])
    elif break_rule == "per_channel":
        mask = reshaped("mask", j, (1, P, 32), scale=np.linspace(0.01, 0.02, 32).astype(F), zp=lo + 128, qdim=2)
    elif break_rule == "mask16":
        mask = reshaped("mask", j, (1, 2 * P, 16))
    elif break_rule == "zp_range":
        mask = reshaped("mask", j, (1, P, 32), zp=hi + 45)
    elif break_rule == "const_head":
        mask = const("mask_const", (1, P, 32))
    else:
        mask = j
    proto = reshaped("proto", j, (1, hp, 2 * wp, 16) if break_rule == "proto16" else (1, hp, wp, 32))
    if break_rule == "kind":
        loc = m.add(QT("loc_i32", (1, P, 4), "i32", data=rng.integers(-9, 9, (1, P, 4)).astype(np.int32)))
    m.inputs, m.outputs = [x], [loc, conf, mask, proto]
    if break_rule == "axis0":
        two = m.add(QT("two", (2, P, 4), dtype, scale=0.0625, zp=lo + 128))
        m.ops.append(Op("CONCATENATION", [x, const("other", (1, P, 4))], [two], axis=0))
        m.outputs.append(two)
    return m


RULES = {"loc5": "loc must be [1,P,4]", "C1": "C >= 2", "mask16": "mask must be [1,P,32]", "proto16": "proto must be [1,hp,wp,32]",
         "P": "disagree on the number of priors", "scale0": "finite and positive", "scale_inf": "finite and positive",
         "scale_neg": "finite and positive", "axis0": "image axis", "kind": "must be uint8, int8 or float32",
         "const_head": "is a constant of the model", "zp_range": "zero point of mask lies outside"}
# ("per_channel": the reader refuses such a file already. A head "never written by the fused plan" cannot be built: the fusion pass
# counts a graph output as a reader of its tensor and never folds it away.)


def dequantized_heads(m):
    """A uint8 model of tests/tfl_models.py (tfl_builder objects) with DEQUANTIZE behind its four heads: float32 outputs 0 .. 3, as
    today's converter ends a graph. The model is changed in place and returned."""
    import tfl_builder as B
    for i in range(4):
        t = m.tensors[m.outputs[i]]
        y = m.add(B.T(t.name + "_f32", t.shape, "f32"))
        m.ops.append(B.Op("DEQUANTIZE", [m.outputs[i]], [y]))
        m.outputs[i] = y
    return m
