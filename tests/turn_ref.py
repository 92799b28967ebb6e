"""The turn-aware planner's frozen definition (DESIGN.md §11 "Turns"), restated on the CPU for tests/test_scene_turn.py. States are
(pixel, heading); everything not said here - fields, edge lengths, h = float32(map), the association of the drive candidate - is
path_ref's 8-connected planner.

Heading h in 0 .. 7 is path_ref._COMPASS's index: 0 right (1, 0), 1 down-right, 2 down, 3 down-left, 4 left, 5 up-left, 6 up
(0, -1), 7 up-right; h + 1 is clockwise on the image (y down), indices wrap. State (v, h) may
  drive to (v + s_h, h):          fl(fl(d[h][v + s_h] + c(v, v + s_h)) + |h[v] - h[v + s_h]|), if that pixel is in the frame,
  turn  to (v, h - 1), (v, h + 1): fl(d[h -+ 1][v] + tau), tau the price of 45 degrees in place, 1 <= tau <= 1024.
d f32 [8][H][W]: 0 at every target in every layer, elsewhere the minimum of the up to three candidates. Every weight is >= 1, so
fl(d + w) > d below 2^24: one solution, reached bit for bit by a heap Dijkstra and by whole-grid Jacobi sweeps alike.
act u8 [8][H][W]: 255 at targets, else the first of (drive 0, turn to h - 1 = 1, turn to h + 1 = 2) whose candidate equals d
bitwise. The route follows act from (start, h0); turns in place add no node; turns[i] is the signed number of 45-degree steps made
at node i before driving (+ towards h + 1), directions[i] = (d[h_i][n_i] - d[h_i][n_i+1], ROT[|turns[i]|])."""
import heapq

import numpy as np

import path_ref as R

INF = R.INF
HEADINGS = tuple(sorted(R._COMPASS, key=R._COMPASS.get))          # s_h = (dx, dy) of heading h
_STEP_OF = tuple(R.STEPS.index(s) for s in HEADINGS)              # heading h drives along path_ref.STEPS[_STEP_OF[h]]
DRIVE, CCW, CW, AT_TARGET = 0, 1, 2, 255
TAU_MIN, TAU_MAX = 1.0, 1024.0


def size_ok(W, H):
    """The size guard: a Manhattan path plus at most eight turns bounds every state's cost below 2^24."""
    return (W + H) * (2 * max(H, 101) + 1) + 8 * 1024 < 2 ** 24


def _target_mask(shape, targets):
    return np.broadcast_to(R._target_mask(shape[1:], targets), shape)


def candidates(d, hmap, conn0, conn1, tau):
    """(drive, turn to h - 1, turn to h + 1), f32 [8][H][W] each; a drive off the frame is +inf."""
    _, H, W = d.shape
    h = hmap.astype(np.float32)
    lens = R._lengths(conn0, conn1)
    tau = np.float32(tau)
    drive = np.full(d.shape, INF, np.float32)
    for k, (dx, dy) in enumerate(HEADINGS):
        v, u = R._windows(H, W, dx, dy)
        drive[k][v] = (d[k][u] + lens[_STEP_OF[k]][v]) + np.abs(h[v] - h[u])
    ccw, cw = np.roll(d, 1, axis=0) + tau, np.roll(d, -1, axis=0) + tau      # from d[h - 1], from d[h + 1]
    assert drive.dtype == ccw.dtype == cw.dtype == np.float32
    return drive, ccw, cw


def jacobi(hmap, conn0, conn1, targets, tau):
    """Whole-grid sweeps over the eight layers to the fixed point; returns (d, sweeps)."""
    H, W = hmap.shape
    t = _target_mask((8, H, W), targets)
    d = np.where(t, np.float32(0), INF).astype(np.float32)
    sweeps = 0
    while True:
        new = np.minimum.reduce((d,) + candidates(d, hmap, conn0, conn1, tau))
        new[t] = 0
        sweeps += 1
        if np.array_equal(new, d):
            return d, sweeps
        d = new


def dijkstra(hmap, conn0, conn1, targets, tau):
    """Heap Dijkstra over (pixel, heading) from all targets in all headings; python floats that always hold f32 values. A settled
    state (u, h) relaxes the pixel that drives into it, (u - s_h, h), and its two turn neighbours (u, h - 1), (u, h + 1)."""
    H, W = hmap.shape
    n = H * W
    h = hmap.astype(np.float32).ravel().tolist()
    lens = [c.astype(np.float32).ravel().tolist() for c in R._lengths(conn0, conn1)]
    tau = R._f32(tau)
    d = [float("inf")] * (8 * n)
    heap = []
    for x, y in targets:
        for k in range(8):
            d[k * n + y * W + x] = 0.0
            heap.append((0.0, k * n + y * W + x))
    heapq.heapify(heap)
    done = [False] * (8 * n)
    while heap:
        du, s = heapq.heappop(heap)
        if done[s]:
            continue
        done[s] = True
        k, u = divmod(s, n)
        x, y = u % W, u // W
        dx, dy = HEADINGS[k]
        vx, vy = x - dx, y - dy
        if 0 <= vx < W and 0 <= vy < H:
            v = vy * W + vx
            cv = R._f32(R._f32(du + lens[_STEP_OF[k]][v]) + abs(h[v] - h[u]))
            if cv < d[k * n + v]:
                d[k * n + v] = cv
                heapq.heappush(heap, (cv, k * n + v))
        ct = R._f32(du + tau)
        for k2 in ((k - 1) % 8, (k + 1) % 8):
            if ct < d[k2 * n + u]:
                d[k2 * n + u] = ct
                heapq.heappush(heap, (ct, k2 * n + u))
    return np.array(d, np.float32).reshape(8, H, W)


def equation_residual(d, hmap, conn0, conn1, targets, tau):
    """States at which d does NOT satisfy its defining equations (0 at targets, the minimum candidate elsewhere), bitwise."""
    want = np.minimum.reduce(candidates(d, hmap, conn0, conn1, tau))
    want[_target_mask(d.shape, targets)] = 0
    return int((want.view(np.uint32) != d.view(np.uint32)).sum())


def actions(d, hmap, conn0, conn1, targets, tau):
    """act u8 [8][H][W]: 255 at targets, else the first of (drive, h - 1, h + 1) whose candidate equals d bitwise (3 if none does:
    not at a solution)."""
    act = np.full(d.shape, 3, np.uint8)
    for a, c in reversed(list(enumerate(candidates(d, hmap, conn0, conn1, tau)))):
        act[c.view(np.uint32) == d.view(np.uint32)] = a
    act[_target_mask(d.shape, targets)] = AT_TARGET
    return act


def walk(d, act, start, heading):
    """(path int32 [L][2], directions f32 [L - 1][2], turns int32 [L - 1]) from (start, heading) along act."""
    _, H, W = d.shape
    x, y, k = int(start[0]), int(start[1]), int(heading)
    path, dirs, turns = [(x, y)], [], []
    t = 0
    for _ in range(8 * W * H + 1):
        a = int(act[k, y, x])
        if a == AT_TARGET:
            break
        if a == DRIVE:
            dx, dy = HEADINGS[k]
            assert abs(t) <= 4
            dirs.append((d[k, y, x] - d[k, y + dy, x + dx], R.ROT[abs(t)]))
            turns.append(t)
            x, y, t = x + dx, y + dy, 0
            path.append((x, y))
        else:
            assert a in (CCW, CW), "not at a solution"
            k, t = (k + (1 if a == CW else -1)) % 8, t + (1 if a == CW else -1)
    else:
        raise AssertionError("the walk did not end within 8 W H actions")
    return (np.array(path, np.int32).reshape(-1, 2), np.array(dirs, np.float32).reshape(-1, 2), np.array(turns, np.int32))


def turning_steps(path):
    """Steps of a route (from the second on) whose heading differs from the step before, and the 45-degree steps between them in
    total - what a route of the pixel planners costs a drive base."""
    s = np.diff(np.asarray(path), axis=0)
    hd = [R._COMPASS[(int(a), int(b))] for a, b in s]
    k = [min((a - b) % 8, (b - a) % 8) for a, b in zip(hd[:-1], hd[1:])]
    return sum(1 for v in k if v), sum(k)
