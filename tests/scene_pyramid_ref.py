"""The scene memory's pyramid registration (DESIGN.md §11 "Scene memory: pyramid registration") restated in numpy from its
definition: the max-pooled levels, the level gathers, the descent of every base, the home hypothesis, the choice and the int32
conditions. The scores of a level are scene_register_ref's on that level's maps; everything after the choice is scene_memory_ref's.
Imports nothing from the library: the tests compare the library against this, and this against known answers worked out by hand."""
import numpy as np

import scene_memory_ref as R
import scene_register_ref as G

I32_MAX = G.I32_MAX
Q = G.Q


def pool(P):
    """the next level: ceil(W / 2) x ceil(H / 2), each cell the max of the up to four cells of P under it"""
    H, W = P.shape
    Z = np.zeros((2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), P.dtype)   # (u32: a zero outside changes no max)
    Z[:H, :W] = P
    return np.maximum(np.maximum(Z[0::2, 0::2], Z[0::2, 1::2]), np.maximum(Z[1::2, 0::2], Z[1::2, 1::2]))


def levels_of(P, levels):
    """[P_0 .. P_levels]"""
    out = [np.ascontiguousarray(P, np.uint32)]
    for _ in range(levels):
        out.append(pool(out[-1]))
    return out


def level_gather(g, lv):
    """the gather of level lv: the base carried to the centres of the coarse cells (Python integers, floor division)"""
    a, b, c, d, e, f = (int(t) for t in g)
    s = (1 << lv) - 1
    return (a, b, ((a + b - Q) * s + 2 * c) // (2 << lv), d, e, ((d + e - Q) * s + 2 * f) // (2 << lv))


def reach(levels, radius, refine):
    """[T_0 .. T_levels]: the largest total shift at each level"""
    T = [0] * (levels + 1)
    T[levels] = radius
    for lv in range(levels - 1, -1, -1):
        T[lv] = 2 * T[lv + 1] + refine
    return T


def bases_ok(gathers, carries, levels, radius, refine):
    """the int32 conditions: every level's shifted gather offsets, and the carry's with T_0 in place of the radius"""
    T = reach(levels, radius, refine)
    for g in gathers:
        for lv in range(levels + 1):
            q = level_gather(g, lv)
            if abs(q[2]) + T[lv] * Q > I32_MAX or abs(q[5]) + T[lv] * Q > I32_MAX:
                return False
    if carries is not None:
        for c in carries:
            c = [int(t) for t in c]
            if abs(c[2]) + T[0] * (abs(c[0]) + abs(c[1])) > I32_MAX or abs(c[5]) + T[0] * (abs(c[3]) + abs(c[4])) > I32_MAX:
                return False
    return True


def level_best(S, centre):
    """(U, V), total, of the best entry of one hypothesis' table S [2p+1][2p+1] around centre: the larger S, then the smaller
    U^2 + V^2 of the total shift, then the smaller V, then the smaller U"""
    p = (S.shape[0] - 1) // 2
    best = None
    for j in range(-p, p + 1):
        for i in range(-p, p + 1):
            U, V = centre[0] + i, centre[1] + j
            key = (-int(S[j + p, i + p]), U * U + V * V, V, U)
            if best is None or key < best:
                best = key
    return best[3], best[2]


def choose(S0, centres, n_rot):
    """(k, u, v, S) over every level-0 entry of all hypotheses (hypothesis n_rot counts as k = 0): the largest S, then the smaller
    u^2 + v^2, then the smaller k, then the smaller v, then the smaller u"""
    p = (S0.shape[1] - 1) // 2
    best = None
    for h in range(S0.shape[0]):
        k = 0 if h == n_rot else h
        for j in range(-p, p + 1):
            for i in range(-p, p + 1):
                u, v = centres[h][0] + i, centres[h][1] + j
                key = (-int(S0[h, j + p, i + p]), u * u + v * v, k, v, u)
                if best is None or key < best:
                    best = key
    return best[2], best[4], best[3], -best[0]


def search(N, M, gathers, carries, levels, radius, refine):
    """dict(chosen=(k, u, v), gather, carry, score=(S chosen, S(0, 0, 0), sum_n), pyr_n, pyr_m = levels 1 .. L, and per level
    lv = 0 .. L: centres[lv] i32 [hyp][2], tables[lv] u64 [hyp][2p+1][2p+1], sum_n[lv])"""
    n_rot = len(gathers)
    assert 1 <= n_rot <= 15 and 1 <= levels <= 3 and 0 <= radius <= 8 and 0 <= refine <= 8 and bases_ok(gathers, carries, levels, radius, refine)
    PN, PM = levels_of(N, levels), levels_of(M, levels)
    centres, tables, sums = [None] * (levels + 1), [None] * (levels + 1), [0] * (levels + 1)
    cen = [(0, 0)] * n_rot
    for lv in range(levels, -1, -1):
        p = radius if lv == levels else refine
        hyp = [(k, cen[k]) for k in range(n_rot)] + ([(0, (0, 0))] if lv == 0 else [])
        gs = []
        for k, (cx, cy) in hyp:
            a, b, c, d, e, f = level_gather(gathers[k], lv)
            gs.append((a, b, c + cx * Q, d, e, f + cy * Q))
        S, sums[lv] = G.scores(PN[lv], PM[lv], gs, p)
        centres[lv] = np.array([c for _, c in hyp], np.int32).reshape(len(hyp), 2)
        tables[lv] = S
        if lv:
            cen = []
            for k in range(n_rot):
                U, V = level_best(S[k], hyp[k][1])
                cen.append((2 * U, 2 * V))
    k, u, v, s = choose(tables[0], [tuple(int(t) for t in c) for c in centres[0]], n_rot)
    g, c = G.candidate(gathers[k], None if carries is None else carries[k], u, v)
    pr = refine
    return dict(chosen=(k, u, v), gather=g, carry=c, score=(s, int(tables[0][n_rot, pr, pr]), sums[0]),
                pyr_n=PN[1:], pyr_m=PM[1:], centres=centres, tables=tables, sum_n=sums)


class Memory(R.Memory):
    """scene_memory_ref.Memory with append_pyramid: yh_scene_append_memory_pyramid given the frame's stamps and balls"""

    def append_pyramid(self, N, frame_balls, gathers, carries, levels, radius, refine, keep=224, max_age=30):
        self.motion = search(N, self.M, gathers, carries, levels, radius, refine)
        return self.append(N, frame_balls, self.motion["gather"], self.motion["carry"], keep, max_age)
