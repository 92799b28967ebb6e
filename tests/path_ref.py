"""The path planner's frozen definition (DESIGN.md §11 "Path planner"), restated on the CPU for tests/test_scene_path.py: what
modify_path (src/path.rs:25-120) was meant to compute on the scene's fields. All arithmetic is np.float32 in the association
fl(fl(d[u] + c(v,u)) + |h[v] - h[u]|) (path.rs:59's left-to-right sum).

Fields are those of Scene.read(): map u32 [H][W], conn0 / conn1 f32 [H][W][4]. Edge lengths of v = (x, y): left conn1[y,x,2],
right conn0[y,x,2], up conn0[y,x,0], down conn1[y,x,0]; off-frame entries are never edges. Neighbour order: left, right, up, down.
Two independent solvers (a heap Dijkstra and whole-grid Jacobi sweeps) give the same bits: every c >= 1 makes fl(d + w) > d
while d < 2^24, so the equations have one solution."""
import ctypes
import heapq

import numpy as np

INF = np.float32(np.inf)
PI, HALF_PI = np.float32(np.pi), np.float32(np.pi / 2)


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


def _edges(hmap, conn0, conn1):
    return hmap.astype(np.float32), conn1[..., 2], conn0[..., 2], conn0[..., 0], conn1[..., 0]


def candidates(d, hmap, conn0, conn1):
    """The four candidates of every pixel, in the order left, right, up, down; +inf where the frame ends."""
    h, cl, cr, cu, cd = _edges(hmap, conn0, conn1)
    out = [np.full(d.shape, INF, np.float32) for _ in range(4)]
    out[0][:, 1:] = (d[:, :-1] + cl[:, 1:]) + np.abs(h[:, 1:] - h[:, :-1])
    out[1][:, :-1] = (d[:, 1:] + cr[:, :-1]) + np.abs(h[:, :-1] - h[:, 1:])
    out[2][1:, :] = (d[:-1, :] + cu[1:, :]) + np.abs(h[1:, :] - h[:-1, :])
    out[3][:-1, :] = (d[1:, :] + cd[:-1, :]) + np.abs(h[:-1, :] - h[1:, :])
    assert all(o.dtype == np.float32 for o in out)
    return out


def _target_mask(shape, targets):
    m = np.zeros(shape, bool)
    for x, y in targets:
        m[y, x] = True
    return m


def jacobi(hmap, conn0, conn1, targets):
    """Whole-grid sweeps to the fixed point; returns (d, sweeps)."""
    t = _target_mask(hmap.shape, targets)
    d = np.where(t, np.float32(0), INF).astype(np.float32)
    sweeps = 0
    while True:
        new = np.minimum.reduce([d] + candidates(d, hmap, conn0, conn1))
        new[t] = 0
        sweeps += 1
        if np.array_equal(new, d):
            return d, sweeps
        d = new


_c_float = ctypes.c_float


def _f32(x):   # a double sum of two f32 values, rounded to f32, is their f32 sum
    return _c_float(x).value


def dijkstra(hmap, conn0, conn1, targets):
    """Heap Dijkstra from all targets; python floats that always hold f32 values."""
    H, W = hmap.shape
    h, cl, cr, cu, cd = (a.astype(np.float32).ravel().tolist() for a in _edges(hmap, conn0, conn1))
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
        # relaxing v from u uses v's own edge towards u: v right of u goes LEFT to reach u, and so on
        if x + 1 < W:
            v = u + 1
            c = _f32(_f32(du + cl[v]) + abs(h[v] - h[u]))
            if c < d[v]:
                d[v] = c; heapq.heappush(heap, (c, v))
        if x > 0:
            v = u - 1
            c = _f32(_f32(du + cr[v]) + abs(h[v] - h[u]))
            if c < d[v]:
                d[v] = c; heapq.heappush(heap, (c, v))
        if y + 1 < H:
            v = u + W
            c = _f32(_f32(du + cu[v]) + abs(h[v] - h[u]))
            if c < d[v]:
                d[v] = c; heapq.heappush(heap, (c, v))
        if y > 0:
            v = u - W
            c = _f32(_f32(du + cd[v]) + abs(h[v] - h[u]))
            if c < d[v]:
                d[v] = c; heapq.heappush(heap, (c, v))
    return np.array(d, np.float32).reshape(H, W)


def equation_residual(d, hmap, conn0, conn1, targets):
    """Pixels at which d does NOT satisfy its defining equations (0 at targets, the minimum candidate elsewhere), bitwise."""
    t = _target_mask(d.shape, targets)
    want = np.minimum.reduce(candidates(d, hmap, conn0, conn1))
    want[t] = 0
    return int((want.view(np.uint32) != d.view(np.uint32)).sum())


def successors(d, hmap, conn0, conn1, targets):
    """next[v]: linear index of the first neighbour (left, right, up, down) whose candidate equals d[v] bitwise; -1 at targets."""
    H, W = d.shape
    idx = np.arange(H * W, dtype=np.int32).reshape(H, W)
    nxt = np.full((H, W), -1, np.int32)
    for c, off in reversed(list(zip(candidates(d, hmap, conn0, conn1), (-1, 1, -W, W)))):
        hit = (c.view(np.uint32) == d.view(np.uint32)) & np.isfinite(c)
        nxt[hit] = idx[hit] + off
    nxt[_target_mask(d.shape, targets)] = -1
    return nxt


def walk(d, nxt, start):
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
            straight = (path[i - 1] + path[i + 1] == 2 * path[i]).all()
            dirs[i, 1] = PI if straight else HALF_PI
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
