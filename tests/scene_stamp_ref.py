"""Frames in which every pixel's bump is VISIBLE in the height map (DESIGN.md §11 "A max is tested with visible contributors").
CPU only. The map is a max over bumps, so on a dense frame nearly every pixel's stamp lies under a taller neighbour's and a kernel
that mishandles that pixel still gives the right map. Here a frame is a quiet background (nothing stamps, nothing is a ball) plus a
few stamping pixels whose depths are chosen so that their windows [x - L, x + L) x [ny - L, ny + L) are pairwise disjoint: each map
cell then has at most one contributor, and a wrong or missing tap of ANY pixel changes the map.

A frame is a Frame(depth u16 [H][W], ci u8 [H][W][2], stamps), stamps a tuple of (x, y, ny, L): pixel (x, y) stamps a bump of
half-width L (10 terrain, 20 robot) around map cell (x, ny)."""
import collections
import functools
import math

import numpy as np

F = np.float32
TERRAIN_L, ROBOT_L = 10, 20
Frame = collections.namedtuple("Frame", "depth ci stamps")


def target_row(H, W, x, y, depth):
    """The map row ny = H - dic at which pixel (x, y) of depth `depth` stamps: the oracle's float32 expression (orc_scene.c, pt_cloud.comp
    main), one rounding per operator. Scalars or arrays."""
    x, y, depth = np.asarray(x), np.asarray(y), np.asarray(depth)
    ty = F(0.55430907) * y.astype(F) * F(2) / F(H)
    tx = F(0.9489646) * x.astype(F) * F(2) / F(W)
    cy = F(1) / np.sqrt(F(1) + ty * ty)
    cx = F(1) / np.sqrt(F(1) + tx * tx)
    d = depth.astype(F) * cy * cx
    dic = np.trunc(F(H) * d / F(4000)).astype(np.int64)
    return H - dic


def depth_for(H, W, x, y, ny):
    """The uint16 depth for which pixel (x, y) stamps at map row ny (<= H: depth is at least 0). One depth step moves H * d / 4000 by
    less than 1 (H < 4000), so every row down from H is hit until the depth runs out of 16 bits (ValueError)."""
    dic = H - ny
    if dic < 0:
        raise ValueError(f"row {ny} is beyond H = {H}: no depth reaches it")
    ty, tx = 0.55430907 * y * 2 / H, 0.9489646 * x * 2 / W
    per_step = H / 4000 / math.sqrt(1 + ty * ty) / math.sqrt(1 + tx * tx)      # float64 estimate of d(H * d / 4000) / d(depth)
    est = math.ceil(dic / per_step)                                            # about the smallest depth that reaches dic
    for c in (est, est + 1, est - 1, est + 2, est - 2):
        if 0 <= c <= 65535 and int(target_row(H, W, x, y, c)) == ny:
            return np.uint16(c)
    raise ValueError(f"no uint16 depth puts pixel ({x}, {y}) of a {H} x {W} frame at row {ny}")


def quiet(H, W):
    """Nothing stamps and nothing is a ball: every pixel class 3 (ball) with id 150 (beyond the 100-entry table), depth 0."""
    ci = np.empty((H, W, 2), np.uint8)
    ci[..., 0], ci[..., 1] = 3, 150
    return np.zeros((H, W), np.uint16), ci


def with_stamps(H, W, stamps, cls):
    """The quiet frame plus the given (x, y, ny, L) stamps; `cls` is the class byte of every stamping pixel (or a callable (x, y, L) -> class)."""
    depth, ci = quiet(H, W)
    for (x, y, ny, L) in stamps:
        depth[y, x] = depth_for(H, W, x, y, ny)
        ci[y, x] = (cls(x, y, L) if callable(cls) else cls, 0)
    depth.flags.writeable = ci.flags.writeable = False
    return Frame(depth, ci, tuple(stamps))


def _stride(H):
    s = max(H // 3, 1) | 1
    while math.gcd(s, H) != 1:
        s += 2
    return s


@functools.lru_cache(maxsize=None)
def isolated_frames(H, W, cls, L):
    """A tuple of frames in which every pixel of the H x W shape is class `cls` exactly once, every stamp isolated. Frame (x0, f) holds
    columns x0, x0 + 2L, ... and target rows t0, t0 + 2L, ... <= H with t0 = (f + x0) mod 2L: windows 2L apart in both directions. A column
    hands its pixel rows to the targets in a stride order (coprime with H), so that the pixels that meet a given map row - a band seam, a
    frame edge - come from every lane position of the stamping kernel, not from one residue of y."""
    P, s = 2 * L, _stride(H)
    frames = []
    for x0 in range(min(P, W)):
        cols = list(range(x0, W, P))
        done = 0                                                # pixel rows handed out so far (the same count in every column of the class)
        f = 0
        while done < H:
            targets = list(range((f + x0) % P, H + 1, P))[:H - done]
            stamps = [(x, ((done + j) * s + 5 * x + x // 16) % H, ny, L) for x in cols for j, ny in enumerate(targets)]
            frames.append(with_stamps(H, W, stamps, cls))
            done += len(targets)
            f += 1
    return tuple(frames)


def windows_disjoint(stamps):
    w = [(x - L, x + L, ny - L, ny + L) for (x, _, ny, L) in stamps]
    return all(a[1] <= b[0] or b[1] <= a[0] or a[3] <= b[2] or b[3] <= a[2] for i, a in enumerate(w) for b in w[i + 1:])


def _oracle():
    import oracle
    return oracle


def audit(frames, maps=None):
    """Asserts every frame's windows pairwise disjoint and its oracle map zero outside them; returns (seen, hidden): the (frame index,
    x, y) of the stamps with / without a nonzero map cell inside their window. `maps`: the frames' oracle maps, when the caller has them."""
    seen, hidden = [], []
    for i, fr in enumerate(frames):
        assert windows_disjoint(fr.stamps), (i, fr.stamps)
        m = _oracle().scene(fr.depth, fr.ci, 1)["map"] if maps is None else maps[i]
        H, W = m.shape
        inside = np.zeros((H, W), bool)
        for (x, y, ny, L) in fr.stamps:
            win = (slice(max(ny - L, 0), max(min(ny + L, H), 0)), slice(max(x - L, 0), max(min(x + L, W), 0)))
            inside[win] = True
            (seen if m[win].any() else hidden).append((i, x, y))
        assert not m[~inside].any(), i
    return seen, hidden


@functools.lru_cache(maxsize=None)
def isolated_maps(H, W, cls, L):
    """The oracle's map of every frame of isolated_frames(H, W, cls, L): computed once, shared by the tests, read-only."""
    maps = []
    for fr in isolated_frames(H, W, cls, L):
        m = _oracle().scene(fr.depth, fr.ci, 1)["map"]
        m.flags.writeable = False
        maps.append(m)
    return tuple(maps)


def bump_f64(val, L):
    """The bump of height parameter val and half-width L in float64 (pt_cloud.comp:44-76): [2L][2L] taps trunc(val / (1 + C1^(2 r / L - 1))),
    C1 = val / 0.1 - 1, r the distance to the centre tap (L, L); values below 1 give 0. Returns (taps u32, real values f64)."""
    C1 = val / 0.1 - 1
    d = np.arange(2 * L, dtype=np.float64) - L
    r = np.sqrt(d[:, None] ** 2 + d[None, :] ** 2)
    real = val / (1 + C1 ** (2 * r / L - 1)) if C1 > 0 else np.zeros_like(r)
    return np.where(real >= 1, np.trunc(real), 0).astype(np.uint32), real


# ---------------------------------------------------------------------------------------------- the other frame sets of test_scene_stamp.py
def _frozen(depth, ci, stamps=()):
    depth, ci = np.ascontiguousarray(depth, np.uint16), np.ascontiguousarray(ci, np.uint8)
    depth.flags.writeable = ci.flags.writeable = False
    return Frame(depth, ci, tuple(stamps))


EDGE_COLUMNS = lambda W: (0, 1, 15, 16, 31, 32, W - 2, W - 1)
EDGE_ROWS = lambda H, L: (-L - 5, -L, -L + 1, -1, 0, 1, H - 2, H - 1, H)
ROBOT_CLASSES = (1, 2, 7, 255)   # red, blue, and two unknown classes: every class but 0 and 3 is a robot (pt_cloud.comp's else branch)


@functools.lru_cache(maxsize=None)
def edge_frames(H, W):
    """One isolated stamp per frame at target rows around and beyond the frame's top and bottom (a window wholly above the map, one cell
    into it, across row 0, at the last rows) in the strip-edge columns, as terrain and as robot (classes in turn); then whole frames at
    depth 65535 (every target far above the map) and depth 0 (every target is row H), every pixel terrain, then robot."""
    frames, i = [], 0
    for L, classes in ((TERRAIN_L, (0,)), (ROBOT_L, ROBOT_CLASSES)):
        for ny in EDGE_ROWS(H, L):
            for x in EDGE_COLUMNS(W):
                y = 2 + (13 * i) % (H - 2)                    # any pixel row can be sent anywhere; rows >= 2 so that a terrain bump is nonzero
                frames.append(with_stamps(H, W, [(x, y, ny, L)], classes[i % len(classes)]))
                i += 1
    for d in (65535, 0):
        for c in (0, 1):
            ci = np.zeros((H, W, 2), np.uint8)
            ci[..., 0] = c
            frames.append(_frozen(np.full((H, W), d, np.uint16), ci))
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def ball_frames(H, W):
    """Every pixel a ball. (0) all 100 ids, each in every 16-column strip and on both sides of row 64, ids 99 / 100 / 255 side by side,
    depths 0 .. 6000; (1) one id on every pixel: count W * H; (2) frame 0's ids at depth 65535: every target row far below zero."""
    rng = np.random.default_rng(70 * W + H)
    yy, xx = np.mgrid[0:H, 0:W]
    ci = np.empty((H, W, 2), np.uint8)
    ci[..., 0] = 3
    ci[..., 1] = (xx + W * yy) % 103                          # 100, 101, 102: beyond the table
    ci[5, 10:13, 1] = (99, 100, 255)
    ci[66, 33:36, 1] = (255, 99, 100)
    depth = rng.integers(0, 6001, (H, W)).astype(np.uint16)
    one = ci.copy()
    one[..., 1] = 7
    return (_frozen(depth, ci), _frozen(rng.integers(0, 6001, (H, W)), one), _frozen(np.full((H, W), 65535), ci))


@functools.lru_cache(maxsize=None)
def decode_frame(H, W):
    """Pixels running through every class value 0 .. 255 with ids 0, 99, 100 and 255 (every pair: H * W >= 1024), depths 0 .. 6000."""
    assert H * W >= 1024
    rng = np.random.default_rng(H * 1000 + W)
    k = np.arange(H * W).reshape(H, W)
    ci = np.stack([k % 256, np.array([0, 99, 100, 255])[(k // 256) % 4]], -1)
    return _frozen(rng.integers(0, 6001, (H, W)), ci)


def dense_frame(rng, H, W):
    """The dense frame of tests/test_scene.py (_frame): every pixel a random depth, almost every pixel stamps."""
    depth = rng.integers(200, 4000, (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.03] = 0
    ci = np.zeros((H, W, 2), np.uint8)
    ci[H // 5:H // 3, W // 4:W // 2, 0] = 1
    ci[H // 2:H // 2 + H // 8, W // 2:W // 2 + W // 6, 0] = 2
    ci[H // 8:H // 8 + 6, W // 8:W // 8 + 7] = (3, 5)
    ci[H - 12:H - 5, W - 20:W - 9] = (3, 0)
    ci[3:5, 3:5] = (3, 200)
    ci[0:2, :, 0] = 7
    return _frozen(depth, ci)


def sparse_frame(rng, H, W):
    """About one pixel in forty stamps or is a ball, on the quiet background: random class, depth 0 .. 6000 (targets above the map included)."""
    depth, ci = quiet(H, W)
    on = rng.random((H, W)) < 1 / 40
    on[rng.integers(0, H), rng.integers(0, W)] = True          # (never empty, however small the frame)
    n = int(on.sum())
    depth[on] = rng.integers(0, 6001, n)
    ci[on] = np.stack([rng.choice([0, 0, 1, 2, 3, 7], n), rng.integers(0, 100, n)], -1)
    return _frozen(depth, ci)
