"""Deterministic edge cases for the detection tail (csrc/detect.hip K1 .. K4). Not a test: builders of head
tensors for tests/test_tail_cases.py (which proves on the CPU oracle that every case does what it claims) and for
tests/test_gpu_tail_edges.py (which runs them through yh_op_detect and compares with the oracle bit for bit). numpy only.

Every builder takes the engine's priors [P][4] (cx, cy, w, h) and the prototype map's hp, wp and returns a dict with
    loc [n][P][4], conf [n][P][C], mask [n][P][32], proto [n][hp][wp][32]   float32 holding f16-representable values
    cfg                                                                    top_k, max_dets, conf_thresh, nms_thresh
plus what the case claims about itself. CASES at the end lists them with the input size and class count they are meant for.

A decoded box follows loc completely: cx = q.x + 0.1 l0 q.z, w = q.z exp(0.2 l2) (aim() inverts that, up to the f16 rounding of
loc). A logit row (background b, one class z, every other class -100) has s = fl(1 + e(z - b)) whatever the class's column: the
other terms vanish in the sequential sum, so equal (b, z) give equal scores in different classes - exact ties across classes."""
import numpy as np

F32 = np.float32
BG = 12.0          # background logit of the recipe: class logits fall from 16, score = e / (1 + e), e = exp(z - 12)
OFF = -100.0       # a class that is no candidate under any positive threshold (its e is exp(-87), absorbed by s >= 1)


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------------------------------------- geometry helpers
def aim(q, cx, cy, w, h):
    """loc row that decodes prior q to the box (cx, cy, w, h), rounded to f16."""
    return h16([(cx - q[0]) / (0.1 * q[2]), (cy - q[1]) / (0.1 * q[3]), 5.0 * np.log(w / q[2]), 5.0 * np.log(h / q[3])])


def decode(pri, loc):
    """Boxes (x1, y1, x2, y2) in float64: close to the spec's float32 decode, for geometry that is far from any threshold."""
    q, l = np.asarray(pri, np.float64), np.asarray(loc, np.float64)
    cx, cy = q[:, 0] + l[:, 0] * 0.1 * q[:, 2], q[:, 1] + l[:, 1] * 0.1 * q[:, 3]
    w, h = q[:, 2] * np.exp(0.2 * l[:, 2]), q[:, 3] * np.exp(0.2 * l[:, 3])
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)


def suppressors(boxes, thr):
    """Fast-NMS on boxes in rank order: for every rank j the ranks i < j with IoU(i, j) > thr (empty = j survives)."""
    b = np.asarray(boxes, np.float64)
    iw = np.clip(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), 0, None)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = iw * ih
    uni = area[:, None] + area[None, :] - inter
    iou = np.where(uni > 0, inter / np.where(uni > 0, uni, 1), 0)
    return [np.nonzero(iou[:j, j] > thr)[0].tolist() for j in range(len(b))]


def grid_targets(K):
    """K pairwise disjoint boxes: centres on a ceil(sqrt(K)) grid inside [0.05, 0.95]^2, side 0.4 pitch."""
    g = int(np.ceil(np.sqrt(K)))
    pitch = 0.9 / g
    return [(0.05 + (k % g + 0.5) * pitch, 0.05 + (k // g + 0.5) * pitch) for k in range(K)], 0.4 * pitch


def rank_logit(r, K):
    """Class logit of rank r of K: strictly decreasing, >= 3 f16 steps apart up to K = 256, score 0.98 .. 0.12."""
    return float(h16(16.0 - 6.0 * r / max(K, 1)))


def blank(priors, hp, wp, C, n, seed, bg=BG):
    """n frames without any candidate: background bg, classes OFF; random boxes, coefficients of both signs, prototypes >= 0."""
    rng = np.random.default_rng(seed)
    P = len(priors)
    loc = h16(rng.normal(0, 0.3, (n, P, 4)))
    conf = np.full((n, P, C), OFF, np.float32)
    conf[:, :, 0] = bg
    mask = h16(np.tanh(rng.normal(0, 1, (n, P, 32))))
    proto = h16(np.maximum(rng.normal(0, 1, (n, hp, wp, 32)), 0))
    return loc, conf, mask, proto


def k1_place(C, prior):
    """(workgroup, wave, lane) that decides `prior` in K1: 64 cells per workgroup; the 81-class kernel gives wave k anchor k and
    lane l the cell l, the generic kernel a lane per prior in prior order."""
    cell, a = divmod(int(prior), 3)
    if C == 81:
        return cell // 64, a, cell % 64
    tid = (cell % 64) * 3 + a
    return cell // 64, tid // 64, tid % 64


def k1_last_rows(P):
    """Rows (cells) in the last K1 workgroup."""
    cells = P // 3
    return cells - (cells - 1) // 64 * 64


# ---------------------------------------------------------------------------------------------- (a) every NMS pair
def nms_subcases():
    """(K, i, j, dense): K candidates of one class, rank j sits on rank i's box (i, j None: nobody is suppressed). dense: all but
    about a hundred ranks are suppressed by design, so that ranks past max_dets = 128 stay visible in the frame's detections."""
    subs = [(1, None, None, False)]
    for K in range(2, 11):
        subs.append((K, None, None, False))
        subs += [(K, i, j, False) for j in range(1, K) for i in range(j)]
    for dense in (False, True):
        for K in (255, 256):
            m = K // 2
            subs += [(K, i, j, dense) for i, j in ((0, K - 1), (m - 1, m), (0, m), (3, m), (m, m + 1), (K - 2, K - 1))]
    return subs


DENSE_BASE = 100   # dense sub-cases: ranks below this keep a position of their own, the others sit on one of them


def nms_pairs(priors, hp, wp, C=65):
    """(yh_create admits (C - 1) top_k <= 16384: top_k = 256 goes with at most 65 classes)"""
    P = len(priors)
    subs = nms_subcases()
    rng = np.random.default_rng(101)
    # pack: a big K takes a frame alone; small ones share frames on disjoint priors, one class each, at most 120 candidates a
    # frame so that every survivor (and a wrong extra one) is inside max_dets
    frames, cur = [], None
    for s in subs:
        K = s[0]
        if K > 10:
            frames.append([s])
            continue
        if cur is None or sum(t[0] for t in cur) + K > 120 or len(cur) == C - 1:
            cur = []
            frames.append(cur)
        cur.append(s)
    n = len(frames)
    loc, conf, mask, proto = blank(priors, hp, wp, C, n, 1)
    out = []
    for f, fs in enumerate(frames):
        perm = rng.permutation(P)
        used = 0
        cols = rng.permutation(np.arange(1, C))
        for c, (K, i, j, dense) in enumerate(fs):
            pr = perm[used:used + K]
            used += K
            cen, side = grid_targets(K + 1)          # (position K is spare)
            pos = list(range(K))
            if dense:
                assert j >= DENSE_BASE
                for r in range(DENSE_BASE, K):
                    t = (r - DENSE_BASE) % DENSE_BASE
                    pos[r] = t if t != i else (t + 1) % DENSE_BASE
                if i >= DENSE_BASE:
                    pos[i] = K
            if j is not None:
                pos[j] = pos[i]
            for r in range(K):
                loc[f, pr[r]] = aim(priors[pr[r]], cen[pos[r]][0], cen[pos[r]][1], side, side)
                conf[f, pr[r], cols[c]] = rank_logit(r, K)
            sup = suppressors(decode(priors[pr], loc[f, pr]), 0.5)
            out.append(dict(frame=f, class_id=int(cols[c]) - 1, K=K, i=i, j=j, dense=dense, priors=[int(p) for p in pr], sup=sup,
                            kept=[int(pr[r]) for r in range(K) if not sup[r]]))
    return dict(loc=loc, conf=conf, mask=mask, proto=proto, subs=out,
                cfg=dict(top_k=256, max_dets=128, conf_thresh=0.05, nms_thresh=0.5))


# ---------------------------------------------------------------------------------------------- (b) scores on the threshold
def threshold(priors, hp, wp, C):
    """Frame 0: a group of 60 priors with one logit row, so one score t in class `col`; candidates clearly above and below it in
    that class and in another. Frames 1 .. 4: in class `col` exactly one prior has that row - in lane 0 / lane 63 of a K1 wave,
    in the first / last row of the ragged last K1 workgroup - and every other prior is far below. conf_thresh is not in cfg: the
    tests take t from the oracle (probe) and run threshold_cfgs(t)."""
    P = len(priors)
    assert P // 3 > 64 and k1_last_rows(P) < 64
    loc, conf, mask, proto = blank(priors, hp, wp, C, 5, 2, bg=4.0)
    col, col2 = C // 2, C - 2
    group = list(range(40, 100))
    conf[0, group, col] = 2.0
    # (the others of class `col` are decided by the OTHER K1 workgroup: in the group's own waves no lane is above the threshold,
    # so a wave-wide shortcut that skips too much loses the group here too, not only the single priors of frames 1 .. 4)
    conf[0, 213:223, col] = 7.0                  # clearly above
    conf[0, 233:243, col] = 0.0                  # clearly below: score 0.018
    conf[:, 200:210, col2] = 6.0                 # another class, every frame
    first_ragged = (P // 3 - 1) // 64 * 64 * 3
    if C == 81:
        singles = [("lane0", 1), ("lane63", 63 * 3 + 2), ("ragged_first", first_ragged), ("ragged_last", P - 1)]
    else:
        singles = [("lane0", 64), ("lane63", 127), ("ragged_first", first_ragged), ("ragged_last", P - 1)]
    for f, (_, p) in enumerate(singles, 1):
        conf[f, p, col] = 2.0
    return dict(loc=loc, conf=conf, mask=mask, proto=proto, group=group, class_id=col - 1, probe=(0, col - 1, group[0]),
                singles=[(f, name, p) for f, (name, p) in enumerate(singles, 1)],
                cfg=dict(top_k=200, max_dets=128, nms_thresh=1.0))


def threshold_cfgs(case, t):
    """The three configurations around the score t (float32): one ulp below, t itself, one ulp above."""
    t = F32(t)
    return [dict(case["cfg"], conf_thresh=float(v)) for v in (np.nextafter(t, F32(0)), t, np.nextafter(t, F32(1)))]


def probe_score(case, detect, priors, C):
    """The probed (frame, class, prior)'s score under `detect` (the oracle's) at a threshold far below it."""
    f, cid, p = case["probe"]
    dets, _ = detect(case["loc"][f], case["conf"][f], case["mask"][f], case["proto"][f], priors, num_classes=C,
                     **dict(case["cfg"], conf_thresh=0.05), want_masks=False)
    (s,) = [d["score"] for d in dets if d["class_id"] == cid and d["prior"] == p]
    return F32(s)


# ---------------------------------------------------------------------------------------------- (c) subnormal probabilities
def subnormal(priors, hp, wp, C):
    """conf_thresh = 0: every (class, prior) is a candidate. Each row ties the background with class `col` (sometimes a third
    class) at the maximum 40, so s >= 2; every other class sits 86.75 .. 100 below: e = exp(-86.75 .. -87) is a small normal
    number and e / s a subnormal one, of a few different values. All priors decode to one box, so each class keeps its best
    candidate only and the frame has C - 1 detections, all but one or two with subnormal scores."""
    P = len(priors)
    rng = np.random.default_rng(3)
    loc, conf, mask, proto = blank(priors, hp, wp, C, 1, 3, bg=40.0)
    col, col3 = 3, 5
    lows = h16([-60.0, -47.0, -46.875, -46.75])
    for c in range(1, C):                        # (a class's best e differs from class to class)
        conf[0, :, c] = rng.choice(lows[:2 + c % 3], P)
    conf[0, :, col] = 40.0
    conf[0, rng.random(P) < 0.3, col3] = 40.0
    for p in range(P):
        loc[0, p] = aim(priors[p], 0.5, 0.45, 0.3, 0.4)
    return dict(loc=loc, conf=conf, mask=mask, proto=proto,
                cfg=dict(top_k=200 if C == 81 else 256, max_dets=128, conf_thresh=0.0, nms_thresh=0.5))


# ---------------------------------------------------------------------------------------------- (d) ragged last K1 workgroup
RAGGED_SIZES = {185: 1, 89: 2, 73: 11, 129: 24, 225: 62, 273: 64}    # input size -> rows in the last workgroup of 64 cells


def ragged(priors, hp, wp, C):
    """Random heads as in test_tail_random_logits_both_class_counts; the first and the last cell's priors are sure candidates."""
    P = len(priors)
    rng = np.random.default_rng(1000 + P + C)
    loc = h16(rng.normal(0, 0.4, (2, P, 4)))
    conf = rng.normal(0, 2.0, (2, P, C))
    conf[:, :, 0] += 3.0
    for k, p in enumerate((0, 1, 2, P - 3, P - 2, P - 1)):
        conf[:, p, :] = 0.0
        conf[:, p, 1 + (5 * k + 2) % (C - 1)] = 12.0
    mask = h16(np.tanh(rng.normal(0, 1, (2, P, 32))))
    proto = h16(np.maximum(rng.normal(0, 1, (2, hp, wp, 32)), 0))
    return dict(loc=loc, conf=h16(conf), mask=mask, proto=proto, last_cell=[P - 3, P - 2, P - 1],
                cfg=dict(top_k=200, max_dets=100, conf_thresh=0.05, nms_thresh=0.5))


# ---------------------------------------------------------------------------------------------- (e) cuts at the limits
def full_keys(priors, hp, wp, C=65):
    """Every prior a candidate of every class: (C - 1) top_k = 16384 survivors, K3's key array is full. Frame 0 near-equal
    random logits, frame 1 all logits equal: 16384 equal scores, class then rank decide the 128 kept."""
    P = len(priors)
    assert P >= 256 and (C - 1) * 256 == 16384
    rng = np.random.default_rng(5)
    loc, conf, mask, proto = blank(priors, hp, wp, C, 2, 5)
    conf[0] = h16(rng.normal(0, 0.02, (P, C)))
    conf[1] = 0.0
    return dict(loc=loc, conf=conf, mask=mask, proto=proto, cfg=dict(top_k=256, max_dets=128, conf_thresh=0.001, nms_thresh=1.0))


def topk_cut(priors, hp, wp, top_k, C=81):
    """One class with top_k - 1, top_k and top_k + 1 candidates (frames 0, 1, 2). Logits fall with rank down to rank top_k - 1 and
    stay there: candidate top_k + 1 ties with candidate top_k, and prior order decides which of them is cut. Ranks 1 .. m - 9 sit
    on rank 0's box and are suppressed, so the last ranks are among the detections also at top_k = 256 > max_dets."""
    P = len(priors)
    rng = np.random.default_rng(600 + top_k)
    loc, conf, mask, proto = blank(priors, hp, wp, C, 3, 6)
    col, frames = 7, []
    for f, m in enumerate((top_k - 1, top_k, top_k + 1)):
        pr = rng.permutation(P)[:m]
        lg = np.array([rank_logit(min(r, top_k - 1), top_k) for r in range(m)])
        order = sorted(range(m), key=lambda r: (-lg[r], pr[r]))           # the spec's rank: score desc, prior asc
        pr, lg = pr[order], lg[order]
        cen, side = grid_targets(10)
        for r in range(m):
            k = 0 if 1 <= r < m - 8 else (0 if r == 0 else 1 + r - max(1, m - 8))
            loc[f, pr[r]] = aim(priors[pr[r]], cen[k][0], cen[k][1], side, side)
            conf[f, pr[r], col] = lg[r]
        K = min(m, top_k)
        sup = suppressors(decode(priors[pr[:K]], loc[f, pr[:K]]), 0.5)
        frames.append(dict(m=m, ranked=[int(p) for p in pr], logits=lg.tolist(), kept=[int(pr[r]) for r in range(K) if not sup[r]]))
    return dict(loc=loc, conf=conf, mask=mask, proto=proto, class_id=col - 1, frames=frames,
                cfg=dict(top_k=top_k, max_dets=128, conf_thresh=0.05, nms_thresh=0.5))


TIE_COLS = (4, 8, 10)      # the tie group's classes (columns), dealt round robin


def dets_cut(priors, hp, wp, max_dets, C=81):
    """max_dets - 1, max_dets, max_dets + 1 and max_dets + 3 survivors (frames 0 .. 3), nothing suppressed. The last min(6, m) of
    them tie in score over the classes of TIE_COLS: where m > max_dets the cut runs through the tie group and class, then rank,
    decide. Tie members of a higher class have the lower priors, and all of them lower priors than the rest."""
    P = len(priors)
    rng = np.random.default_rng(700 + max_dets)
    loc, conf, mask, proto = blank(priors, hp, wp, C, 4, 7)
    frames = []
    for f, m in enumerate((max_dets - 1, max_dets, max_dets + 1, max_dets + 3)):
        g = min(6, m)
        tie = [(c, g - 1 - k) for k, c in enumerate(sorted(TIE_COLS[t % 3] - 1 for t in range(g)))]   # (class_id, prior)
        for cid, p in tie:
            conf[f, p, cid + 1] = rank_logit(1, 1)                         # 10: score 0.119
        rest = g + rng.permutation(P - g)[:m - g]
        for r, p in enumerate(rest):
            conf[f, p, 6] = rank_logit(r, m)
        frames.append(dict(m=m, tie=tie))
    return dict(loc=loc, conf=conf, mask=mask, proto=proto, frames=frames,
                cfg=dict(top_k=200, max_dets=max_dets, conf_thresh=0.05, nms_thresh=1.0))


# ---------------------------------------------------------------------------------------------- (f) mask groups, crop windows
# A crop window that begins / ends exactly on a pixel needs x1 wp and y2 hp to be integers IN FLOAT32. Aiming a box at centres and
# sizes that are multiples of 1 / wp does not give that: loc is f16, so the decoded centre moves in steps of ulp16(l0) 0.1 q.z and
# the size in relative steps of 0.2 ulp16(l2) - 1e-5 .. 1e-3 of the map for an ordinary l0, l2 - while the float32 grid near an edge
# is 3e-8 wide; an aimed box misses the pixel coordinate by thousands of float32 steps. Only a shift |l0| < 2^-7 is fine enough
# (f16 keeps its relative precision), so _edge_on_pixel searches the f16 sizes for one that leaves such a small shift to the
# pixel coordinate and then the f16 neighbours of that shift for an exact hit, evaluating the spec's float32 decode itself
# (spec_expf below restates DESIGN.md §Spec-exp). tests/test_tail_cases.py holds the hit against the oracle's own box.
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def spec_expf(x):
    """DESIGN.md §Spec-exp in numpy float32 (fma through float64: one extra rounding in 2^-29 of the cases)."""
    x = np.clip(np.asarray(x, np.float32), F32(-87), F32(88))
    n = np.rint(x * F32(1.44269504088896341))
    r = _fma(n, F32(-0.693359375), x)
    r = _fma(n, F32(2.12194440e-4), r)
    p = np.full_like(r, F32(1.9875691500e-4))
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = _fma(p, r, F32(c))
    y = _fma(p, r * r, r) + F32(1)
    return (y.view(np.int32) + (n.astype(np.int32) << 23)).view(np.float32)


def _edge_on_pixel(c, s, m, upper):
    """(l_shift, l_size, k): f16 loc values with which the spec's float32 decode of a prior (centre c, size s) along one axis of an
    m-pixel map puts the box's lower edge (upper: its upper edge) EXACTLY on k / m, 2 <= k <= m - 2; None if there is none."""
    c, s = F32(c), F32(s)
    bits = np.arange(0x0400, 0x4A00, dtype=np.uint16)                      # positive normal f16 up to 12
    l2 = np.concatenate([bits, bits | 0x8000]).view(np.float16).astype(np.float32)
    w = s * spec_expf(l2 * F32(0.2))
    l2, w = l2[(w > 2.5 / m) & (w < 0.45)], w[(w > 2.5 / m) & (w < 0.45)]
    half = w.astype(np.float64) / 2
    k = np.rint((c + half if upper else c - half) * m)
    shift = (k / m - half if upper else k / m + half) - c                  # where the centre has to go
    l0 = shift / (0.1 * float(s))
    ok = (np.abs(l0) < 2.0 ** -7) & (np.abs(l0) > 2.0 ** -13) & (k >= 2) & (k <= m - 2)
    for a, b, kk in zip(l0[ok], l2[ok], k[ok]):
        cand = (np.float16(a).view(np.uint16).astype(np.int32) + np.arange(-6, 7)).astype(np.uint16).view(np.float16).astype(np.float32)
        wv = s * spec_expf(np.full(cand.shape, b, np.float32) * F32(0.2))
        cx = c + (cand * F32(0.1)) * s
        lo = cx - wv * F32(0.5)
        edge = (wv + lo) if upper else lo
        hit = np.nonzero(edge * F32(m) == F32(kk))[0]
        if len(hit):
            return float(cand[hit[0]]), float(b), int(kk)
    return None


def exact_window(priors, hp, wp):
    """(prior, loc row, kx, ky): a box whose x1 wp and y2 hp are the integers kx, ky in float32 - its crop window begins exactly
    on pixel column kx - 1 and ends exactly before pixel row ky + 1."""
    for p in range(len(priors) - 1, -1, -1):
        q = priors[p]
        if not 0.1 < q[2] < 0.3:
            continue
        ex, ey = _edge_on_pixel(q[0], q[2], wp, False), _edge_on_pixel(q[1], q[3], hp, True)
        if ex and ey:
            return p, np.array([ex[0], ey[0], ex[1], ey[1]], np.float32), ex[2], ey[2]
    raise AssertionError("no prior decodes onto the pixel grid")


KINDS = ("hang_left", "hang_right", "hang_top", "hang_bottom", "out_left", "out_right", "out_top", "out_bottom", "whole", "pixel",
         "exact")
_WINDOWS = dict(hang_left=(0.02, 0.30, 0.30, 0.25), hang_right=(0.97, 0.60, 0.30, 0.35), hang_top=(0.40, 0.03, 0.35, 0.30),
                hang_bottom=(0.60, 0.98, 0.25, 0.30), out_left=(-0.50, 0.40, 0.20, 0.30), out_right=(1.50, 0.50, 0.20, 0.30),
                out_top=(0.50, -0.50, 0.30, 0.20), out_bottom=(0.45, 1.50, 0.30, 0.20), whole=(0.50, 0.50, 1.20, 1.20))
MASK_BATCHES = (1, 2, 3, 8, 9)         # gridDim.z of K4: 8, 8, 2, 2, 1


def mask_group_size(max_dets, z):
    """K4's detections per gridDim.z group."""
    return ((max_dets + z - 1) // z + 3) & ~3


def mask_counts(max_dets):
    cs = {0, 1, 3, 4, 5, max_dets}
    for z in (8, 2, 1):
        per = mask_group_size(max_dets, z)
        cs |= {per - 1, per, per + 1}
    return sorted(c for c in cs if 0 <= c <= max_dets)


def mask_groups(priors, hp, wp, max_dets, C=81):
    """Frames with detection counts around K4's group sizes (counts[f] detections in frame f, nothing suppressed), then eight more
    full frames. Detection r of frame f has the window kind KINDS[(r + f) % 11] for r < 11 and a random interior box after that.
    Prototypes are strictly positive, coefficients of both signs. `calls` lists the frames of every yh_op_detect call: all
    count frames in chunks of n consecutive ones (wrapping) for n in MASK_BATCHES - the frames of a call have different counts
    wherever there are n different counts, and every count otherwise (max_dets = 5 has five) -, then nine empty frames, then nine
    full ones (stale counters and masks)."""
    P = len(priors)
    counts = mask_counts(max_dets)
    nc = len(counts)
    counts = counts + [max_dets] * 8
    F = len(counts)
    rng = np.random.default_rng(800 + max_dets)
    loc, conf, mask, proto = blank(priors, hp, wp, C, F, 8)
    proto = h16(rng.uniform(0.05, 1.0, proto.shape))
    pe, loc_e, kx, ky = exact_window(priors, hp, wp)
    others = np.array([p for p in range(P) if p != pe])
    kinds = []
    for f, k in enumerate(counts):
        pr = rng.permutation(others)[:k]
        kf = []
        for r in range(k):
            kind = KINDS[(r + f) % len(KINDS)] if r < len(KINDS) else "interior"
            p = int(pr[r])
            if kind == "exact":
                p = pe
                loc[f, p] = loc_e
            elif kind == "pixel":
                loc[f, p] = aim(priors[p], (int(rng.integers(2, wp - 2)) + 0.5) / wp, (int(rng.integers(2, hp - 2)) + 0.5) / hp, 0.2 / wp, 0.2 / hp)
            elif kind == "interior":
                loc[f, p] = aim(priors[p], rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.1, 0.5), rng.uniform(0.1, 0.5))
            else:
                loc[f, p] = aim(priors[p], *_WINDOWS[kind])
            co = np.tanh(rng.normal(0, 1, 32))
            co += (0.0 if kind == "whole" else 0.03) - co.mean()      # (acc: about 0.5 x 32 x this mean, +- 1 from pixel to pixel)
            mask[f, p] = h16(np.abs(co) if kind in ("pixel", "exact") else co)
            conf[f, p, 1 + (7 * r + f) % (C - 1)] = rank_logit(r, k)
            kf.append((p, kind))
        kinds.append(kf)
    calls = []
    for n in MASK_BATCHES:
        calls += [[(i * n + k) % nc for k in range(n)] for i in range((nc + n - 1) // n)]
    calls += [[0] * 9, [nc - 1] + list(range(nc, F))]
    return dict(loc=loc, conf=conf, mask=mask, proto=proto, counts=counts, kinds=kinds, calls=calls, exact=(pe, kx, ky),
                cfg=dict(top_k=200, max_dets=max_dets, conf_thresh=0.05, nms_thresh=1.0))


# ---------------------------------------------------------------------------------------------- the list
# (id, input size, classes, builder, keyword arguments); `threshold` cases carry no conf_thresh (threshold_cfgs)
CASES = [("a_nms_pairs", 64, 65, nms_pairs, {})]
CASES += [(f"b_threshold_C{C}", 64, C, threshold, dict(C=C)) for C in (81, 21, 80)]
CASES += [(f"c_subnormal_C{C}", 64, C, subnormal, dict(C=C)) for C in (81, 21)]
CASES += [(f"d_ragged_S{S}_C{C}", S, C, ragged, dict(C=C)) for S in RAGGED_SIZES for C in (81, 21)]
CASES += [("e1_full_keys", 64, 65, full_keys, {})]
CASES += [(f"e2_topk_cut_{k}", 64, C, topk_cut, dict(top_k=k, C=C)) for k, C in ((1, 81), (2, 81), (255, 65), (256, 65))]
CASES += [(f"e3_dets_cut_{k}", 64, 81, dets_cut, dict(max_dets=k)) for k in (1, 127, 128)]
CASES += [(f"f_mask_groups_S{S}_{k}", S, 81, mask_groups, dict(max_dets=k)) for S, k in ((64, 5), (64, 11), (64, 128), (128, 11), (128, 128))]
CASE_IDS = [c[0] for c in CASES]


def build(case_id, priors, hp, wp):
    cid, S, C, fn, kw = CASES[CASE_IDS.index(case_id)]
    case = fn(np.asarray(priors, np.float32), hp, wp, **kw)
    for k in ("loc", "conf", "mask", "proto"):
        assert case[k].dtype == np.float32 and np.array_equal(case[k], h16(case[k])), (case_id, k)
    assert (C - 1) * case.get("cfg", {}).get("top_k", 1) <= 16384 and case["conf"].shape[2] == C
    return dict(case, id=cid, S=S, C=C)


# ---------------------------------------------------------------------------------------------- shared by the two test files
_GEOMETRY = {}


def geometry(oracle, S):
    """(priors, hp, wp) at input size S from oracle.Net(50, S, 81, 1); `oracle` is the oracle module (the tests' fixture). Neither
    depends on the class count, and the GPU test holds every engine's priors against these."""
    if S not in _GEOMETRY:
        net = oracle.Net(50, S, 81, 1)
        _GEOMETRY[S] = (net.priors(), net.hp, net.wp)
    return _GEOMETRY[S]


def reference(oracle, case, f, priors, cfg=None):
    """The oracle's (detections, masks) of frame f under cfg (default: the case's own)."""
    return oracle.detect(case["loc"][f], case["conf"][f], case["mask"][f], case["proto"][f], priors, num_classes=case["C"],
                         **(cfg or case["cfg"]))


def tuples(dets):
    return [(d["class_id"], d["prior"], d["score"], d["box"]) for d in dets]
