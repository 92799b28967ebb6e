"""The planner on the 8-connected grid (DESIGN.md §11 "Diagonals"), restated on the CPU for tests/test_scene_path8.py on top of
path_ref: the same pixels, equation and association, fl(fl(d[u] + c(v,u)) + |h[v] - h[u]|), the minimum over up to eight neighbours.

Edge lengths of v = (x, y), layouts of Scene.read(): the four straight ones as path_ref has them, up-left conn1[y,x,3], up-right
conn0[y,x,1], down-left conn1[y,x,1], down-right conn0[y,x,3]; off-frame entries are never edges. Neighbour order: left, right,
up, down, up-left, up-right, down-left, down-right (path_ref's order is a prefix: ties prefer straight moves). A SANE diagonal is
sqrt((1 + dy^2) + 1) >= sqrt(2) >= 1, so path_ref's uniqueness argument carries over and two solvers give the same bits.
Rotations: with k in 0 .. 4 the number of 45-degree steps between the heading into a node and the heading out of it,
float32((4 - k) * pi / 4)."""
import heapq

import numpy as np

import path_ref as R

INF = R.INF
# (dx, dy) of the neighbour u of v, in the successor's order
STEPS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))
ROT = tuple(np.float32((4 - k) * np.pi / 4) for k in range(5))      # pi, 3 pi / 4, pi / 2, pi / 4, 0
_COMPASS = {(1, 0): 0, (1, 1): 1, (0, 1): 2, (-1, 1): 3, (-1, 0): 4, (-1, -1): 5, (0, -1): 6, (1, -1): 7}


def _lengths(conn0, conn1):
    """The length of v's edge towards each of its eight neighbours, in the order of STEPS."""
    return (conn1[..., 2], conn0[..., 2], conn0[..., 0], conn1[..., 0], conn1[..., 3], conn0[..., 1], conn1[..., 1], conn0[..., 3])


def _windows(H, W, dx, dy):
    """(slices of v, slices of u = v + (dx, dy)) over the pixels v whose neighbour u lies in the frame."""
    ys = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
    xs = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
    return (ys[0], xs[0]), (ys[1], xs[1])


def candidates8(d, hmap, conn0, conn1):
    """The eight candidates of every pixel, in the order of STEPS; +inf where the frame ends."""
    H, W = d.shape
    h = hmap.astype(np.float32)
    out = []
    for (dx, dy), c in zip(STEPS, _lengths(conn0, conn1)):
        o = np.full(d.shape, INF, np.float32)
        v, u = _windows(H, W, dx, dy)
        o[v] = (d[u] + c[v]) + np.abs(h[v] - h[u])
        assert o.dtype == np.float32
        out.append(o)
    return out


def jacobi8(hmap, conn0, conn1, targets):
    """Whole-grid sweeps to the fixed point; returns (d, sweeps)."""
    t = R._target_mask(hmap.shape, targets)
    d = np.where(t, np.float32(0), INF).astype(np.float32)
    sweeps = 0
    while True:
        new = np.minimum.reduce([d] + candidates8(d, hmap, conn0, conn1))
        new[t] = 0
        sweeps += 1
        if np.array_equal(new, d):
            return d, sweeps
        d = new


def dijkstra8(hmap, conn0, conn1, targets):
    """Heap Dijkstra from all targets; python floats that always hold f32 values."""
    H, W = hmap.shape
    h = hmap.astype(np.float32).ravel().tolist()
    lens = [c.astype(np.float32).ravel().tolist() for c in _lengths(conn0, conn1)]
    d = [float("inf")] * (H * W)
    heap = []
    for x, y in targets:
        d[y * W + x] = 0.0
        heap.append((0.0, y * W + x))
    heapq.heapify(heap)
    done = [False] * (H * W)
    while heap:
        du, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        x, y = u % W, u // W
        # relaxing v from u uses v's own edge towards u: v = u - step, for every step that leads from a pixel of the frame to u
        for (dx, dy), c in zip(STEPS, lens):
            vx, vy = x - dx, y - dy
            if 0 <= vx < W and 0 <= vy < H:
                v = vy * W + vx
                cv = R._f32(R._f32(du + c[v]) + abs(h[v] - h[u]))
                if cv < d[v]:
                    d[v] = cv
                    heapq.heappush(heap, (cv, v))
    return np.array(d, np.float32).reshape(H, W)


def equation_residual8(d, hmap, conn0, conn1, targets):
    """Pixels at which d does NOT satisfy its defining equations (0 at targets, the minimum candidate elsewhere), bitwise."""
    t = R._target_mask(d.shape, targets)
    want = np.minimum.reduce(candidates8(d, hmap, conn0, conn1))
    want[t] = 0
    return int((want.view(np.uint32) != d.view(np.uint32)).sum())


def successors8(d, hmap, conn0, conn1, targets):
    """next[v]: linear index of the first neighbour (order of STEPS) whose candidate equals d[v] bitwise; -1 at targets."""
    H, W = d.shape
    idx = np.arange(H * W, dtype=np.int32).reshape(H, W)
    nxt = np.full((H, W), -1, np.int32)
    for c, (dx, dy) in reversed(list(zip(candidates8(d, hmap, conn0, conn1), STEPS))):
        hit = (c.view(np.uint32) == d.view(np.uint32)) & np.isfinite(c)
        nxt[hit] = idx[hit] + (dy * W + dx)
    nxt[R._target_mask(d.shape, targets)] = -1
    return nxt


def rotation(before, at, after):
    """rot at the node `at` between the steps before -> at and at -> after (each to one of the eight neighbours)."""
    a = _COMPASS[(int(at[0] - before[0]), int(at[1] - before[1]))]
    b = _COMPASS[(int(after[0] - at[0]), int(after[1] - at[1]))]
    k = (a - b) % 8
    return ROT[min(k, 8 - k)]


def walk8(d, nxt, start):
    """(path int32 [L][2] of (x, y) from start to a target, directions f32 [L-1][2] of (magnitude, rotation))."""
    H, W = d.shape
    node = start[1] * W + start[0]
    nodes = [node]
    while nxt.flat[node] >= 0:
        node = int(nxt.flat[node])
        nodes.append(node)
        assert len(nodes) <= H * W
    path = np.array([(n % W, n // W) for n in nodes], np.int32).reshape(-1, 2)
    dirs = np.zeros((len(nodes) - 1, 2), np.float32)
    for i in range(len(nodes) - 1):
        dirs[i, 0] = d.flat[nodes[i]] - d.flat[nodes[i + 1]]
        if i > 0:
            dirs[i, 1] = rotation(path[i - 1], path[i], path[i + 1])
    return path, dirs


def fields_from_edges(Rt, D, DR, DL, hmap=None):
    """(map, conn0, conn1) from one length per edge, f32 [H][W] each: Rt[y, x] the edge (x, y) - (x + 1, y), D to (x, y + 1), DR to
    (x + 1, y + 1), DL to (x - 1, y + 1); entries whose other end is off the frame are ignored (-1 in the fields). Both ends of an
    edge get the same length, as in a SANE frame. The map is flat (zero) unless given."""
    H, W = Rt.shape
    conn0 = np.full((H, W, 4), -1, np.float32)
    conn1 = np.full((H, W, 4), -1, np.float32)
    conn0[:, :-1, 2] = Rt[:, :-1]; conn1[:, 1:, 2] = Rt[:, :-1]
    conn1[:-1, :, 0] = D[:-1, :]; conn0[1:, :, 0] = D[:-1, :]
    conn0[:-1, :-1, 3] = DR[:-1, :-1]; conn1[1:, 1:, 3] = DR[:-1, :-1]
    conn1[:-1, 1:, 1] = DL[:-1, 1:]; conn0[1:, :-1, 1] = DL[:-1, 1:]
    return (np.zeros((H, W), np.uint32) if hmap is None else hmap.astype(np.uint32)), conn0, conn1


def tile_rounds(hmap, conn0, conn1, targets, T=32, corner_flags=True):
    """A synchronous emulation of the device solver: T x T tiles with a one-cell halo. In a round every flagged tile reads a snapshot
    of the field taken at the start of the round, relaxes its own cells to the fixed point for that halo, writes back what got
    smaller and flags, for the next round, the tile across every border on which a cell moved and - with corner_flags - the tile
    diagonally across every corner cell that moved. Round 0's flags: the same rule applied to the targets' drop from +inf to 0,
    plus their own tiles. Returns (d, rounds in which some tile ran)."""
    H, W = hmap.shape
    ty, tx = (H + T - 1) // T, (W + T - 1) // T
    d = np.full((H, W), INF, np.float32)
    flags = np.zeros((ty, tx), bool)

    def flag(nxt, bx, by):
        if 0 <= bx < tx and 0 <= by < ty:
            nxt[by, bx] = True

    def flag_moved(nxt, bx, by, moved):
        """moved: bool [h][w] over the tile's cells (ragged tiles are smaller than T: they have no tile beyond the short side)"""
        h, w = moved.shape
        sides = ((-1, 0, moved[:, 0].any()), (1, 0, w == T and moved[:, -1].any()), (0, -1, moved[0, :].any()), (0, 1, h == T and moved[-1, :].any()))
        for sx, sy, m in sides:
            if m:
                flag(nxt, bx + sx, by + sy)
        if corner_flags:
            for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
                cy, cx = (0 if sy < 0 else T - 1), (0 if sx < 0 else T - 1)
                if cy < h and cx < w and moved[cy, cx]:
                    flag(nxt, bx + sx, by + sy)

    for x, y in targets:
        d[y, x] = 0
        bx, by = x // T, y // T
        flags[by, bx] = True
        moved = np.zeros((min(T, H - by * T), min(T, W - bx * T)), bool)
        moved[y % T, x % T] = True
        flag_moved(flags, bx, by, moved)
    rounds = 0
    while flags.any():
        rounds += 1
        assert rounds <= H * W
        snap, nxt = d.copy(), np.zeros_like(flags)
        for by, bx in zip(*np.nonzero(flags)):
            y0, y1, x0, x1 = by * T, min(by * T + T, H), bx * T, min(bx * T + T, W)
            wy, wx = slice(max(y0 - 1, 0), min(y1 + 1, H)), slice(max(x0 - 1, 0), min(x1 + 1, W))      # the tile and its halo
            iy, ix = slice(y0 - wy.start, y1 - wy.start), slice(x0 - wx.start, x1 - wx.start)          # the tile inside that window
            loc = snap[wy, wx].copy()
            while True:
                new = np.minimum.reduce([loc] + candidates8(loc, hmap[wy, wx], conn0[wy, wx], conn1[wy, wx]))
                if np.array_equal(new[iy, ix], loc[iy, ix]):
                    break
                loc[iy, ix] = new[iy, ix]                         # (the halo stays what the snapshot had)
            moved = loc[iy, ix] < snap[y0:y1, x0:x1]
            d[y0:y1, x0:x1] = np.minimum(d[y0:y1, x0:x1], loc[iy, ix])
            flag_moved(nxt, bx, by, moved)
        flags = nxt
    return d, rounds


def late_corner(n=64, T=32):
    """The fields on which a solver without the corner rule stops early (DESIGN.md §11 "Diagonals"): n x n, flat, straight edges 1
    and diagonals 1.5; every edge at A = (T - 1, T - 1) costs 10 000 except A - (T, T - 1) = 1 and A - (T, T) = 1.5; every other
    edge with exactly one end in the tile x >= T, y >= T costs 5 000. With the target at (0, 0) the cheap way into that tile is
    through A alone, A gets its final cost only when the tile right of it has run, and the one tile that reads A across a corner
    is the diagonal one. Returns (map, conn0, conn1)."""
    Rt, D = np.ones((n, n), np.float32), np.ones((n, n), np.float32)
    DR, DL = np.full((n, n), 1.5, np.float32), np.full((n, n), 1.5, np.float32)
    A = (T - 1, T - 1)
    inside = lambda p: p[0] >= T and p[1] >= T
    for arr, (dx, dy) in ((Rt, (1, 0)), (D, (0, 1)), (DR, (1, 1)), (DL, (-1, 1))):
        for y in range(n):
            for x in range(n):
                p, q = (x, y), (x + dx, y + dy)
                if not (0 <= q[0] < n and 0 <= q[1] < n):
                    continue
                if A in (p, q):
                    other = q if p == A else p
                    arr[y, x] = 1 if other == (T, T - 1) else 1.5 if other == (T, T) else 10000
                elif inside(p) != inside(q):
                    arr[y, x] = 5000
    return fields_from_edges(Rt, D, DR, DL)
