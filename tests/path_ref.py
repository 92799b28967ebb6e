"""The path planner's frozen definition (DESIGN.md §11 "Path planner"), restated on the CPU for tests/test_scene_path.py: what
modify_path (src/path.rs:25-120) was meant to compute on the scene's fields. All arithmetic is np.float32 in the association
fl(fl(d[u] + c(v,u)) + |h[v] - h[u]|) (path.rs:59's left-to-right sum).

Fields are those of Scene.read(): map u32 [H][W], conn0 / conn1 f32 [H][W][4]. Edge lengths of v = (x, y): left conn1[y,x,2],
right conn0[y,x,2], up conn0[y,x,0], down conn1[y,x,0]; off-frame entries are never edges. Neighbour order: left, right, up, down.
Two independent solvers (a heap Dijkstra and whole-grid Jacobi sweeps) give the same bits: every c >= 1 makes fl(d + w) > d
while d < 2^24, so the equations have one solution.

Every function takes conn = 4 or 8, the grid's connectivity (DESIGN.md §11 "Diagonals"): with 8 the minimum is over up to eight
neighbours, the order continues up-left conn1[y,x,3], up-right conn0[y,x,1], down-left conn1[y,x,1], down-right conn0[y,x,3] (the
4-connected order is a prefix: ties prefer straight moves). A SANE diagonal is sqrt((1 + dy^2) + 1) >= sqrt(2) >= 1, so the
uniqueness argument carries over. Rotations: with k in 0 .. 4 the number of 45-degree steps between the heading into a node and the
heading out of it, float32((4 - k) * pi / 4): pi straight on, pi / 2 for a right angle (all a 4-connected route has)."""
import ctypes
import heapq

import numpy as np

INF = np.float32(np.inf)
PI, HALF_PI = np.float32(np.pi), np.float32(np.pi / 2)
# (dx, dy) of the neighbour u of v, in the successor's order; the first conn of them are the grid's
STEPS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))
ROT = tuple(np.float32((4 - k) * np.pi / 4) for k in range(5))      # pi, 3 pi / 4, pi / 2, pi / 4, 0
_COMPASS = {(1, 0): 0, (1, 1): 1, (0, 1): 2, (-1, 1): 3, (-1, 0): 4, (-1, -1): 5, (0, -1): 6, (1, -1): 7}


def size_ok(W, H):
    """The planner's size guard: costs stay below 2^24."""
    return (W + H) * (2 * max(H, 101) + 1) < 2 ** 24


def sane_connections(hmap):
    """conn0 / conn1 as a YH_COMPAT_SANE frame gives them for this height map (world = (x, map, y), lengths
    sqrt((dx*dx + dy*dy) + dz*dz) in f32, -1 off the frame): conn1 = (down, down-left, left, up-left), conn0 = the same edges
    from the other end (up, up-right, right, down-right)."""
    H, W = hmap.shape
    h = hmap.astype(np.float32)
    conn1 = np.full((H, W, 4), -1, np.float32)
    for k, (oy, ox) in enumerate(((1, 0), (1, -1), (0, -1), (-1, -1))):
        ys, xs = np.mgrid[0:H, 0:W]
        qy, qx = ys + oy, xs + ox
        ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
        dy = h[ys[ok], xs[ok]] - h[qy[ok], qx[ok]]
        dx, dz = np.float32(-ox), np.float32(-oy)
        conn1[ys[ok], xs[ok], k] = np.sqrt((dx * dx + dy * dy) + dz * dz)
    conn0 = np.full((H, W, 4), -1, np.float32)
    conn0[1:, :, 0] = conn1[:-1, :, 0]
    conn0[1:, :-1, 1] = conn1[:-1, 1:, 1]
    conn0[:, :-1, 2] = conn1[:, 1:, 2]
    conn0[:-1, :-1, 3] = conn1[1:, 1:, 3]
    return conn0, conn1


def _lengths(conn0, conn1):
    """The length of v's edge towards each of its eight neighbours, in the order of STEPS."""
    return (conn1[..., 2], conn0[..., 2], conn0[..., 0], conn1[..., 0], conn1[..., 3], conn0[..., 1], conn1[..., 1], conn0[..., 3])


def _windows(H, W, dx, dy):
    """(slices of v, slices of u = v + (dx, dy)) over the pixels v whose neighbour u lies in the frame."""
    ys = slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy))
    xs = slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx))
    return (ys[0], xs[0]), (ys[1], xs[1])


def candidates(d, hmap, conn0, conn1, conn=4):
    """The conn candidates of every pixel, in the order of STEPS; +inf where the frame ends."""
    H, W = d.shape
    h = hmap.astype(np.float32)
    out = []
    for (dx, dy), c in zip(STEPS[:conn], _lengths(conn0, conn1)):
        o = np.full(d.shape, INF, np.float32)
        v, u = _windows(H, W, dx, dy)
        o[v] = (d[u] + c[v]) + np.abs(h[v] - h[u])
        assert o.dtype == np.float32
        out.append(o)
    return out


def _target_mask(shape, targets):
    m = np.zeros(shape, bool)
    for x, y in targets:
        m[y, x] = True
    return m


def jacobi(hmap, conn0, conn1, targets, conn=4):
    """Whole-grid sweeps to the fixed point; returns (d, sweeps)."""
    t = _target_mask(hmap.shape, targets)
    d = np.where(t, np.float32(0), INF).astype(np.float32)
    sweeps = 0
    while True:
        new = np.minimum.reduce([d] + candidates(d, hmap, conn0, conn1, conn))
        new[t] = 0
        sweeps += 1
        if np.array_equal(new, d):
            return d, sweeps
        d = new


_c_float = ctypes.c_float


def _f32(x):   # a double sum of two f32 values, rounded to f32, is their f32 sum
    return _c_float(x).value


def dijkstra(hmap, conn0, conn1, targets, conn=4):
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
        for (dx, dy), c in zip(STEPS[:conn], lens):
            vx, vy = x - dx, y - dy
            if 0 <= vx < W and 0 <= vy < H:
                v = vy * W + vx
                cv = _f32(_f32(du + c[v]) + abs(h[v] - h[u]))
                if cv < d[v]:
                    d[v] = cv
                    heapq.heappush(heap, (cv, v))
    return np.array(d, np.float32).reshape(H, W)


def equation_residual(d, hmap, conn0, conn1, targets, conn=4):
    """Pixels at which d does NOT satisfy its defining equations (0 at targets, the minimum candidate elsewhere), bitwise."""
    t = _target_mask(d.shape, targets)
    want = np.minimum.reduce(candidates(d, hmap, conn0, conn1, conn))
    want[t] = 0
    return int((want.view(np.uint32) != d.view(np.uint32)).sum())


def successors(d, hmap, conn0, conn1, targets, conn=4):
    """next[v]: linear index of the first neighbour (order of STEPS) whose candidate equals d[v] bitwise; -1 at targets."""
    H, W = d.shape
    idx = np.arange(H * W, dtype=np.int32).reshape(H, W)
    nxt = np.full((H, W), -1, np.int32)
    for c, (dx, dy) in reversed(list(zip(candidates(d, hmap, conn0, conn1, conn), STEPS))):
        hit = (c.view(np.uint32) == d.view(np.uint32)) & np.isfinite(c)
        nxt[hit] = idx[hit] + (dy * W + dx)
    nxt[_target_mask(d.shape, targets)] = -1
    return nxt


def rotation(before, at, after):
    """rot at the node `at` between the steps before -> at and at -> after (each to one of the eight neighbours)."""
    a = _COMPASS[(int(at[0] - before[0]), int(at[1] - before[1]))]
    b = _COMPASS[(int(after[0] - at[0]), int(after[1] - at[1]))]
    k = (a - b) % 8
    return ROT[min(k, 8 - k)]


def walk(d, nxt, start, conn=4):
    """(path int32 [L][2] of (x, y) from start to a target, directions f32 [L-1][2] of (magnitude, rotation)); every step is one of
    the grid's first conn."""
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
        assert tuple(int(v) for v in path[i + 1] - path[i]) in STEPS[:conn]
        if i > 0:
            dirs[i, 1] = rotation(path[i - 1], path[i], path[i + 1])
    return path, dirs


def ball_targets(balls, n, W, H):
    """The first n balls in id order that have pixels, at their truncated means (scene.rs:321); those outside the frame dropped."""
    out = []
    for k in [k for k in range(len(balls)) if balls[k, 2] > 0][:n]:
        x, y = int(balls[k, 0]), int(balls[k, 1])
        if 0 <= x < W and 0 <= y < H:
            out.append((x, y))
    return out


def serpentine(H, W, pitch=8, wall=400):
    """A corridor of height 0 between walls: full-width rows every `pitch` rows, joined at alternating ends. Returns (map, start,
    target): the corridor's two ends. Crossing a wall band costs 2 * (wall + sqrt(1 + wall^2)) + pitch - 2 > 1600, more than the
    longest way round (2 W), so the geodesic follows the corridor: H / pitch crossings of the frame."""
    m = np.full((H, W), wall, np.uint32)
    rows = list(range(pitch // 2, H, pitch))
    for k, y in enumerate(rows):
        m[y, :] = 0
        if k + 1 < len(rows):
            m[y:rows[k + 1], W - 1 if k % 2 == 0 else 0] = 0
    last = len(rows) - 1
    return m, (0, rows[0]), ((W - 1 if last % 2 == 0 else 0), rows[last])
