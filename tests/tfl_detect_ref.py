"""The pinned meaning of the TFLite detections (DESIGN.md §11 "TFLite detections"), restated on the CPU. Not a test: the reference
of tests/test_tfl_detect_cases.py (CPU) and tests/test_gpu_tfl_detect.py (GPU, compared bit for bit).

The tail reads four head tensors of one image - loc [P][4], conf [P][C], mask [P][32], proto [hp][wp][32] - each uint8, int8 or
float32, a quantised one with one scale and one zero point:

  1. Dequantisation. A quantised element's value is v = (float)(q - z) * scale: the integer difference converted to float32
     (exact), then ONE float32 multiply (oracle.dequant_u8 / yolact.rs:177). A float32 element is itself.
  2. Scores, candidates, decode, NMS, ranking and crop windows are oracle/orc_detect.c on those values, operation for operation
     (the spec exp, the sequential softmax sum, the tie rules: candidates by (score desc, prior asc), detections by (score desc,
     class asc, rank asc)). Priors are indexed by the prior: there is no "three anchors per cell", P is arbitrary.
  3. Mask, mask and proto both quantised: pixel (x, y) of detection d is on iff it lies inside d's crop window and
         S = sum_k (proto_q[y, x, k] - z_p) * (mask_q[prior_d, k] - z_m) > 0        in exact integers (|S| <= 32 * 255^2):
     the sign of the dot product of the represented values (both scales are positive), not of a rounded float32 chain.
  4. Mask, either of the two float32: the oracle's chain acc = fmaf(proto[k], coef[k], acc), k = 0 .. 31, on the values of rule 1,
     then acc > 0, inside the crop window.

Rules 3 and 4 give the same bit wherever every step of the float32 chain is exact - with power-of-two scales always (the
integers are below 2^24, the partial sums below 2^21). For other scales they can differ only where |S| < BAND (derivation in
DESIGN.md; in units of S the chain's error is below 32 * 2^-24 * 32 * 255^2 + 2^-23 * 32 * 255^2 < 4.3)."""
import numpy as np

F = np.float32
# |S| >= BAND: the float32 chain of rule 4 has the sign of S - for scales in the normal range: the derivation assumes that no value,
# product or partial sum underflows (scale_p * scale_m far above 2^-126; with tiny scales the products turn subnormal or zero and the
# chain loses the sign). Rule 3 itself needs no such assumption.
BAND = 5
KINDS = {np.dtype(np.uint8): "u8", np.dtype(np.int8): "i8", np.dtype(np.float32): "f32"}
ROLES = ("loc", "conf", "mask", "proto")


def dequant(q, scale=1.0, zero_point=0):
    """Rule 1."""
    q = np.asarray(q)
    if q.dtype == np.float32:
        return q
    assert q.dtype in (np.uint8, np.int8), q.dtype
    return ((q.astype(np.int32) - np.int32(zero_point)).astype(F) * F(scale)).astype(F)


def values(img, quant):
    """The four tensors of one image as float32 values (rule 1). quant: role -> (scale, zero_point) for the quantised ones."""
    return {r: dequant(img[r], *quant.get(r, (1.0, 0))) for r in ROLES}


def crop_window(box, hp, wp):
    """orc_detect.c's crop window (xa, xb, ya, yb) of a detection's box, in its float32 arithmetic."""
    b = [F(v) for v in box]
    fw, fh = F(wp), F(hp)
    x1, x2, y1, y2 = b[0] * fw, b[2] * fw, b[1] * fh, b[3] * fh
    xa, xb = min(x1, x2) - F(1.0), max(x1, x2) + F(1.0)
    ya, yb = min(y1, y2) - F(1.0), max(y1, y2) + F(1.0)
    xa = F(0.0) if xa < F(0.0) else xa
    ya = F(0.0) if ya < F(0.0) else ya
    xb = fw if xb > fw else xb
    yb = fh if yb > fh else yb
    return xa, xb, ya, yb


def inside(box, hp, wp):
    """bool [hp][wp]: the pixels of the crop window."""
    xa, xb, ya, yb = crop_window(box, hp, wp)
    xs, ys = np.arange(wp, dtype=F), np.arange(hp, dtype=F)
    return ((ys >= ya) & (ys < yb))[:, None] & ((xs >= xa) & (xs < xb))[None, :]


def int_sums(proto_q, z_p, coef_q, z_m):
    """Rule 3's S for every pixel: int64 [hp][wp]."""
    p = proto_q.astype(np.int64) - int(z_p)
    c = coef_q.astype(np.int64) - int(z_m)
    return p @ c


def both_quantised(img):
    return img["mask"].dtype != np.float32 and img["proto"].dtype != np.float32


def detect(oracle, img, quant, priors, cfg, want_sums=False):
    """One image: (detections as oracle.detect returns them, masks uint8 [nd][hp][wp]) by rules 1 - 4. cfg: top_k, max_dets,
    conf_thresh, nms_thresh. want_sums: also S int64 [nd][hp][wp] (rule 3; None under rule 4) and the windows bool [nd][hp][wp]."""
    v = values(img, quant)
    C = img["conf"].shape[-1]
    hp, wp = img["proto"].shape[:2]
    dets, omasks = oracle.detect(v["loc"], v["conf"], v["mask"], v["proto"], priors, num_classes=C, **cfg)
    sums, wins = None, np.zeros((len(dets), hp, wp), bool)
    for d, det in enumerate(dets):
        wins[d] = inside(det["box"], hp, wp)
    if both_quantised(img):
        z_p, z_m = quant["proto"][1], quant["mask"][1]
        sums = np.zeros((len(dets), hp, wp), np.int64)
        for d, det in enumerate(dets):
            sums[d] = int_sums(img["proto"], z_p, img["mask"][det["prior"]], z_m)
        masks = (wins & (sums > 0)).astype(np.uint8)
    else:
        masks = omasks
    return (dets, masks, sums, wins) if want_sums else (dets, masks)


def oracle_on_values(oracle, img, quant, priors, cfg):
    """oracle.detect itself on the dequantised tensors: rule 4 everywhere."""
    v = values(img, quant)
    return oracle.detect(v["loc"], v["conf"], v["mask"], v["proto"], priors, num_classes=img["conf"].shape[-1], **cfg)


def image(case, b):
    return {r: case[r][b] for r in ROLES}


def bits(x):
    return int(np.array(x, F).view(np.uint32))


def tuples(dets):
    """(class, prior, score bits, box bits) per detection: what the GPU must reproduce."""
    return [(d["class_id"], d["prior"], bits(d["score"]), tuple(bits(v) for v in d["box"])) for d in dets]
