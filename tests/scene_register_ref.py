"""The scene memory's registration (DESIGN.md §11 "Scene memory: registration") restated in numpy from its definition: the
candidates of a search, the score table, the choice and its tie rule, and the int32 conditions. Everything after the choice is
scene_memory_ref's. Imports nothing from the library: the tests compare the library against this, and this against known answers
worked out by hand."""
import numpy as np

import scene_memory_ref as R

I32_MAX = (1 << 31) - 1
Q = 65536


def candidate(gather_q16, carry_q16, u, v):
    """(gather, carry) of candidate (., u, v) of one base: the gather's source pixel moves by (u, v), the carry is the inverse moved
    the same way. Python integers; carry_q16 may be None (gather only)."""
    a, b, c, d, e, f = (int(t) for t in gather_q16)
    g = (a, b, c + u * Q, d, e, f + v * Q)
    if carry_q16 is None:
        return g, None
    A, B, Cc, D, E, Ff = (int(t) for t in carry_q16)
    return g, (A, B, Cc - (A * u + B * v), D, E, Ff - (D * u + E * v))


def bases_ok(gathers, carries, radius):
    """the int32 conditions, for every base; carries may be None"""
    for k, g in enumerate(gathers):
        g = [int(t) for t in g]
        if abs(g[2]) + radius * Q > I32_MAX or abs(g[5]) + radius * Q > I32_MAX:
            return False
        if carries is not None:
            c = [int(t) for t in carries[k]]
            if abs(c[2]) + radius * (abs(c[0]) + abs(c[1])) > I32_MAX or abs(c[5]) + radius * (abs(c[3]) + abs(c[4])) > I32_MAX:
                return False
    return True


def scores(N, M, gathers, radius):
    """(S u64 [n_rot][2R+1][2R+1] indexed [k][v + R][u + R], sum_n): S = sum over pixels of min(N, M at the base's source + (u, v)),
    0 where that lies outside the frame. int64 sources (|a x| < 2^31 * 2^13) and uint64 sums (< 2^32 * 2^26 pixels): exact."""
    H, W = N.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    n = 2 * radius + 1
    S = np.zeros((len(gathers), n, n), np.uint64)
    N64, M64 = N.astype(np.uint64), M.astype(np.uint64)
    for k, g in enumerate(gathers):
        sx, sy = R.affine(g, x, y)
        for v in range(-radius, radius + 1):
            for u in range(-radius, radius + 1):
                qx, qy = sx + u, sy + v
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                S[k, v + radius, u + radius] = np.minimum(N64[inside], M64[qy[inside], qx[inside]]).sum(dtype=np.uint64)
    return S, int(N64.sum(dtype=np.uint64))


def choose(S):
    """(k, u, v) of the largest S; ties: the smaller u^2 + v^2, then the smaller k, then the smaller v, then the smaller u"""
    n_rot, n, _ = S.shape
    radius = (n - 1) // 2
    best = None
    for k in range(n_rot):
        for v in range(-radius, radius + 1):
            for u in range(-radius, radius + 1):
                key = (-int(S[k, v + radius, u + radius]), u * u + v * v, k, v, u)
                if best is None or key < best:
                    best = key
    return best[2], best[4], best[3]


def strict(S):
    """whether the maximum of S is taken exactly once"""
    return int((S == S.max()).sum()) == 1


def search(N, M, gathers, carries, radius):
    """dict(chosen=(k, u, v), gather, carry, score=(S chosen, S prior, sum_n), scores) of one registration"""
    assert 1 <= len(gathers) <= 16 and 0 <= radius <= 8 and bases_ok(gathers, carries, radius)
    S, sum_n = scores(N, M, gathers, radius)
    k, u, v = choose(S)
    g, c = candidate(gathers[k], None if carries is None else carries[k], u, v)
    return dict(chosen=(k, u, v), gather=g, carry=c, score=(int(S[k, v + radius, u + radius]), int(S[0, radius, radius]), sum_n), scores=S)


class Memory(R.Memory):
    """scene_memory_ref.Memory with append_search: yh_scene_append_memory_search given the frame's stamps and balls"""

    def append_search(self, N, frame_balls, gathers, carries, radius, keep=224, max_age=30):
        self.motion = search(N, self.M, gathers, carries, radius)
        return self.append(N, frame_balls, self.motion["gather"], self.motion["carry"], keep, max_age)
