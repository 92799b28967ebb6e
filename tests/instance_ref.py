"""The instance frame restated (DESIGN.md §11 "Instance frame"): numpy int64, no float anywhere in the masks' arithmetic (the one
float operation of the definition is the comparison score >= min_score, done in float32 as the device does it).

Inputs: the detections of one frame in rank order (score descending, as yh_read_detections returns them) - binary masks
M_d [Hp][Wp], class ids, scores -, the target size W x H, a class map (foreground class -> output class 0..3) and min_score.
Outputs: the frame uint32 [H][W] of class << 24 | id << 16 and the instance table int32 [m][4] = (rank, class, id, pixels won)."""
import numpy as np


def default_class_map(num_classes=81):
    """The reference's model (yolact.rs:99-101, :113-115): foreground class 0 a red robot (1), 1 a blue robot (2), 2 a ball (3)."""
    cm = np.zeros(num_classes - 1, np.uint8)
    cm[:3] = (1, 2, 3)
    return cm


def axis_taps(out, inp):
    """Per output coordinate o of an axis resized from `inp` to `out` samples with half-pixel centres: the two taps and the weight
    of the second in units of 1 / (2 out): n = max((2 o + 1) inp - out, 0), t0 = n div 2 out, f = n mod 2 out, t1 = min(t0 + 1, inp - 1)."""
    o = np.arange(out, dtype=np.int64)
    n = np.maximum((2 * o + 1) * inp - out, 0)
    t0, f = n // (2 * out), n % (2 * out)
    return t0, np.minimum(t0 + 1, inp - 1), f


def upsample(mask, W, H):
    """The bilinear resize of a binary mask [Hp][Wp] to [H][W] thresholded at > 0.5, exactly: S > 2 W H, a tie is off."""
    m = (np.asarray(mask) != 0).astype(np.int64)
    Hp, Wp = m.shape
    u0, u1, fx = axis_taps(W, Wp)
    v0, v1, fy = axis_taps(H, Hp)
    fx, fy = fx[None, :], fy[:, None]
    S = ((2 * W - fx) * (2 * H - fy) * m[v0][:, u0] + fx * (2 * H - fy) * m[v0][:, u1]
         + (2 * W - fx) * fy * m[v1][:, u0] + fx * fy * m[v1][:, u1])
    return S > 2 * W * H


def ranks(class_ids, scores, class_map=None, min_score=0.0, num_classes=81):
    """Per detection (rank order): (eligible, output class, id). Eligible iff class_map[class_id] != 0 and score >= min_score; the id
    is the number of eligible detections of the same output class with smaller rank."""
    cm = default_class_map(num_classes) if class_map is None else np.asarray(class_map, np.uint8)
    out, seen = [], {}
    for k, s in zip(np.asarray(class_ids, np.int64).tolist(), np.asarray(scores, np.float32)):
        c = int(cm[k])
        ok = c != 0 and bool(s >= np.float32(min_score))
        out.append((ok, c if ok else 0, seen.get(c, 0) if ok else 0))
        if ok:
            seen[c] = seen.get(c, 0) + 1
    return out


def instance_frame(masks, class_ids, scores, W, H, class_map=None, min_score=0.0, num_classes=81):
    """frame uint32 [H][W], table int32 [m][4]: a pixel belongs to the eligible detection of smallest rank whose upsampled mask is on."""
    frame = np.zeros((H, W), np.uint32)
    free = np.ones((H, W), bool)
    table = []
    for d, (ok, c, i) in enumerate(ranks(class_ids, scores, class_map, min_score, num_classes)):
        if not ok:
            continue                                  # paints nothing, occludes nothing
        won = upsample(masks[d], W, H) & free
        frame[won] = (c << 24) | (i << 16)
        free &= ~won
        table.append((d, c, i, int(won.sum())))
    return frame, np.array(table, np.int32).reshape(-1, 4)


def class_image(frame):
    """The (class, id) image uint8 [H][W][2] that Scene.append takes, from a packed frame."""
    return np.stack([(frame >> 24).astype(np.uint8), ((frame >> 16) & 0xFF).astype(np.uint8)], -1)


def disc_masks(rng, n, hp, wp, rmax=None):
    """n seeded binary disc masks [n][hp][wp]."""
    yy, xx = np.mgrid[0:hp, 0:wp]
    rmax = rmax or max(2, min(hp, wp) // 3)
    out = np.zeros((n, hp, wp), np.uint8)
    for d in range(n):
        cx, cy, r = rng.integers(0, wp), rng.integers(0, hp), rng.integers(1, rmax + 1)
        out[d] = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
    return out
