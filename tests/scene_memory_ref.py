"""The scene memory (DESIGN.md §11 "Scene memory") restated in numpy: carry, fade and fuse of the map, the connection fields of a
height map in float32 single operations, and the ball table's rules. Imports nothing from the library: the tests compare the
library against this, and this against the oracle and against known answers worked out by hand."""
import numpy as np

IDENTITY = (65536, 0, 0, 0, 65536, 0)
BALL_LIMIT = 1 << 20


def affine(q16, x, y):
    """floor((a x + b y + c + 2^15) / 2^16) for both rows of q16 = (a, b, c, d, e, f), in Python integers (or int64 arrays: the
    products stay below 2^52 for every argument the definition passes)."""
    a, b, c, d, e, f = (int(v) for v in q16)
    return (a * x + b * y + c + 32768) >> 16, (d * x + e * y + f + 32768) >> 16


def carry_map(M, gather_q16, keep):
    """P'[y][x] = (M[sy][sx] * keep) >> 8 with (sx, sy) = affine(gather_q16, x, y), 0 where the source lies outside the frame."""
    H, W = M.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    sx, sy = affine(gather_q16, x, y)
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    P = np.zeros((H, W), np.uint64)
    P[inside] = M[sy[inside], sx[inside]]
    return ((P * np.uint64(keep)) >> np.uint64(8)).astype(np.uint32)


def fuse(N, M, gather_q16, keep):
    return np.maximum(N.astype(np.uint32), carry_map(M, gather_q16, keep))


def fields(F):
    """world, conn0, conn1 of a SANE frame whose height map is F (pt_cloud_weights.comp as DESIGN.md §Scene freezes it):
    world = (x, F, y, 0); conn1 = lengths to (x, y+1), (x-1, y+1), (x-1, y), (x-1, y-1); conn0 = the conn1 entries that
    (x, y-1), (x+1, y-1), (x+1, y), (x+1, y+1) hold for the same edges; -1 off the frame. float32, one operation at a time."""
    H, W = F.shape
    X = np.tile(np.arange(W, dtype=np.float32), (H, 1))
    Y = np.tile(np.arange(H, dtype=np.float32)[:, None], (1, W))
    Z = F.astype(np.float32)
    world = np.stack([X, Z, Y, np.zeros((H, W), np.float32)], -1)
    conn1 = np.full((H, W, 4), -1.0, np.float32)
    for k, (ox, oy) in enumerate(((0, 1), (-1, 1), (-1, 0), (-1, -1))):
        me = (slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox)))
        ot = (slice(max(0, oy), H + min(0, oy)), slice(max(0, ox), W + min(0, ox)))
        dx, dy, dz = X[me] - X[ot], Z[me] - Z[ot], Y[me] - Y[ot]
        conn1[me + (k,)] = np.sqrt((dx * dx + dy * dy) + dz * dz)
    conn0 = np.full((H, W, 4), -1.0, np.float32)
    for k, (ox, oy) in enumerate(((0, -1), (1, -1), (1, 0), (1, 1))):
        me = (slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox)))
        ot = (slice(max(0, oy), H + min(0, oy)), slice(max(0, ox), W + min(0, ox)))
        conn0[me + (k,)] = conn1[ot + (k,)]
    assert world.dtype == conn0.dtype == conn1.dtype == np.float32
    return world, conn0, conn1


def balls_step(B, frame_balls, carry_q16, max_age, W, H):
    """One frame of the ball table. B i32 [100][4] = (x, y, count, age), frame_balls f32 [100][4] = the frame's own rows.
    Returns (new B, the frame's `balls` output)."""
    nB = np.zeros((100, 4), np.int32)
    out = np.zeros((100, 4), np.float32)
    for k in range(100):
        if frame_balls[k, 2] > 0:                                   # seen
            nB[k] = (int(frame_balls[k, 0]), int(frame_balls[k, 1]), int(frame_balls[k, 2]), 0)
            out[k] = frame_balls[k]
            continue
        x, y, count, age = (int(v) for v in B[k])
        if count > 0 and age + 1 <= max_age:                        # remembered
            cx, cy = affine(carry_q16, x, y)
            if abs(cx) >= BALL_LIMIT or abs(cy) >= BALL_LIMIT:
                continue
            nB[k] = (cx, cy, count, age + 1)
            if 0 <= cx < W and 0 <= cy < H:
                out[k] = (np.float32(cx), np.float32(cy), np.float32(count), np.float32(age))
    return nB, out


class Memory:
    """The memory of one handle: append(N, frame_balls, ..) is yh_scene_append_memory given the frame's stamps and balls."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.reset()

    def reset(self):
        self.M = np.zeros((self.H, self.W), np.uint32)
        self.B = np.zeros((100, 4), np.int32)

    def append(self, N, frame_balls, gather_q16=IDENTITY, carry_q16=IDENTITY, keep=224, max_age=30):
        F = fuse(N, self.M, gather_q16, keep)
        self.M = F.copy()
        self.B, balls = balls_step(self.B, frame_balls, carry_q16, max_age, self.W, self.H)
        world, conn0, conn1 = fields(F)
        return dict(map=F, world=world, conn0=conn0, conn1=conn1, balls=balls)
