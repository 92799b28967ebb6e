"""The scene memory's normalised registration (DESIGN.md §11 "Scene memory: normalised registration") restated in numpy from its
definition: the three tables S, T, C of a search, the qualification, the choice by the ratio S / (T - S) in exact integers and its
tie rule. Candidates, int32 conditions and everything after the choice are scene_register_ref's and scene_memory_ref's. Imports
nothing from the library: the tests compare the library against this, and this against known answers worked out by hand."""
import numpy as np

import scene_memory_ref as R
import scene_register_ref as G


def tables(N, M, gathers, radius):
    """(S, T, C, sum_n): u64 [n_rot][2R+1][2R+1] each, indexed [k][v + R][u + R]. Over the frame pixels whose source (sx + u, sy + v)
    lies in the frame (int64 sources), Q = M there: S = sum of min(N, Q), T = sum of N + Q, C = their number. T < 2 * 2^32 * 2^26."""
    H, W = N.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    n = 2 * radius + 1
    S, T, C = (np.zeros((len(gathers), n, n), np.uint64) for _ in range(3))
    N64, M64 = N.astype(np.uint64), M.astype(np.uint64)
    for k, g in enumerate(gathers):
        sx, sy = R.affine(g, x, y)
        for v in range(-radius, radius + 1):
            for u in range(-radius, radius + 1):
                qx, qy = sx + u, sy + v
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                nn, qq = N64[inside], M64[qy[inside], qx[inside]]
                S[k, v + radius, u + radius] = np.minimum(nn, qq).sum(dtype=np.uint64)
                T[k, v + radius, u + radius] = nn.sum(dtype=np.uint64) + qq.sum(dtype=np.uint64)
                C[k, v + radius, u + radius] = int(inside.sum())
    return S, T, C, int(N64.sum(dtype=np.uint64))


def ratio_cmp(s1, u1, s2, u2):
    """the sign of s1 / u1 - s2 / u2 for u1, u2 > 0, by the cross products s1 u2 and s2 u1 in Python integers (up to 128 bits)"""
    a, b = int(s1) * int(u2), int(s2) * int(u1)
    return (a > b) - (a < b)


def choose(S, T, C, min_inside):
    """((k, u, v), qualified): among the candidates with C >= min_inside and U = T - S > 0 the largest S / U; ties: the smaller
    u^2 + v^2, then the smaller k, then the smaller v, then the smaller u. None qualified: ((0, 0, 0), False)."""
    n_rot, n, _ = S.shape
    radius = (n - 1) // 2
    best = None   # (s, u, tie key)
    for k in range(n_rot):
        for v in range(-radius, radius + 1):
            for u in range(-radius, radius + 1):
                s, t, c = (int(a[k, v + radius, u + radius]) for a in (S, T, C))
                if c < min_inside or t - s <= 0:
                    continue
                key = (u * u + v * v, k, v, u)
                if best is None:
                    best = (s, t - s, key)
                    continue
                sign = ratio_cmp(s, t - s, best[0], best[1])
                if sign > 0 or (sign == 0 and key < best[2]):
                    best = (s, t - s, key)
    if best is None:
        return (0, 0, 0), False
    return (best[2][1], best[2][3], best[2][2]), True


def search(N, M, gathers, carries, radius, min_inside):
    """scene_register_ref.search's dict of one normalised registration - chosen, gather, carry, score = (S chosen, S prior, sum_n),
    scores = S - and totals = T, inside = C, chosen_stc, prior_stc = (S, T, C) of the choice and of (0, 0, 0), qualified"""
    H, W = N.shape
    assert 1 <= len(gathers) <= 16 and 0 <= radius <= 8 and G.bases_ok(gathers, carries, radius) and 1 <= min_inside <= W * H
    S, T, C, sum_n = tables(N, M, gathers, radius)
    (k, u, v), qualified = choose(S, T, C, min_inside)
    g, c = G.candidate(gathers[k], None if carries is None else carries[k], u, v)
    at = lambda kk, uu, vv: tuple(int(a[kk, vv + radius, uu + radius]) for a in (S, T, C))
    return dict(chosen=(k, u, v), gather=g, carry=c, score=(at(k, u, v)[0], at(0, 0, 0)[0], sum_n), scores=S, totals=T, inside=C,
                chosen_stc=at(k, u, v), prior_stc=at(0, 0, 0), qualified=qualified)


class Memory(G.Memory):
    """scene_register_ref.Memory with append_search_norm: yh_scene_append_memory_search_norm given the frame's stamps and balls"""

    def append_search_norm(self, N, frame_balls, gathers, carries, radius, min_inside, keep=224, max_age=30):
        self.motion = search(N, self.M, gathers, carries, radius, min_inside)
        return self.append(N, frame_balls, self.motion["gather"], self.motion["carry"], keep, max_age)
