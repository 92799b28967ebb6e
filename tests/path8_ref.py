"""What is specific to the diagonals (DESIGN.md §11 "Diagonals") in the CPU restatement for tests/test_scene_path8.py; the planner itself,
for either connectivity, is path_ref's: fields built from one length per edge, a synchronous emulation of the device solver's tile
rounds, and the constructed fields on which a solver without the corner rule stops early."""
import numpy as np

import path_ref as R

INF = R.INF


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
                new = np.minimum.reduce([loc] + R.candidates(loc, hmap[wy, wx], conn0[wy, wx], conn1[wy, wx], 8))
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
