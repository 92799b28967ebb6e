"""The scene memory's normalised pyramid registration (DESIGN.md §11 "Scene memory: normalised pyramid registration") restated in
numpy from its definition: the pyramid registration's levels, level gathers, descent and home hypothesis (scene_pyramid_ref) with
every level decided by the normalised registration's tables and ratio (scene_register_norm_ref). Imports nothing from the library:
the tests compare the library against this, and this against known answers worked out by hand."""
import numpy as np

import scene_memory_ref as R
import scene_pyramid_ref as P
import scene_register_norm_ref as NR
import scene_register_ref as G

Q = G.Q


def level_min_inside(min_inside, lv):
    """m_lv: min_inside carried to level lv, rounded up (a cell of level lv covers up to 4^lv pixels)"""
    return (min_inside + 4 ** lv - 1) >> (2 * lv)


def _better(s, u, key, best):
    """whether qualified entry (s, u, key) beats best = (s, u, key) or None: the larger s / u, then the smaller key"""
    if best is None:
        return True
    sign = NR.ratio_cmp(s, u, best[0], best[1])
    return sign > 0 or (sign == 0 and key < best[2])


def level_best(S, T, C, centre, need):
    """((U, V), flag): the total shift of the best qualified entry of one hypothesis' tables [2p+1][2p+1] around centre - the largest
    S / (T - S), then the smaller U^2 + V^2 of the total shift, then the smaller V, then the smaller U - and 1; none qualified
    (C >= need and T - S > 0): the centre itself and 0"""
    p = (S.shape[0] - 1) // 2
    best = None
    for j in range(-p, p + 1):
        for i in range(-p, p + 1):
            s, t, c = (int(a[j + p, i + p]) for a in (S, T, C))
            if c < need or t - s <= 0:
                continue
            U, V = centre[0] + i, centre[1] + j
            key = (U * U + V * V, V, U)
            if _better(s, t - s, key, best):
                best = (s, t - s, key)
    if best is None:
        return (int(centre[0]), int(centre[1])), 0
    return (best[2][2], best[2][1]), 1


def choose(S0, T0, C0, centres, n_rot, need):
    """((k, u, v), (h, j, i) = where that entry lies in the level-0 tables, qualified, flags [hyp]) over every qualified level-0
    entry of all hypotheses (hypothesis n_rot counts as k = 0): the largest S / (T - S), then the smaller u^2 + v^2, then k, then v,
    then u. None qualified: (0, 0, 0) at the home hypothesis' centre, False."""
    p = (S0.shape[1] - 1) // 2
    best, at = None, None
    flags = [0] * S0.shape[0]
    for h in range(S0.shape[0]):
        k = 0 if h == n_rot else h
        for j in range(-p, p + 1):
            for i in range(-p, p + 1):
                s, t, c = (int(a[h, j + p, i + p]) for a in (S0, T0, C0))
                if c < need or t - s <= 0:
                    continue
                flags[h] = 1
                u, v = centres[h][0] + i, centres[h][1] + j
                key = (u * u + v * v, k, v, u)
                if _better(s, t - s, key, best):
                    best, at = (s, t - s, key), (h, j + p, i + p)
    if best is None:
        return (0, 0, 0), (n_rot, p, p), False, flags
    return (best[2][1], best[2][3], best[2][2]), at, True, flags


def search(N, M, gathers, carries, levels, radius, refine, min_inside):
    """scene_pyramid_ref.search's dict of one normalised pyramid registration - chosen, gather, carry, score = (S chosen, S(0, 0, 0)
    at the home hypothesis, level 0's sum_n), pyr_n, pyr_m, and per level centres, tables (S), sum_n - with totals (T), inside (C),
    flags (i32 [hyp]) and need (m_lv) per level, chosen_stc, prior_stc and qualified"""
    H, W = N.shape
    n_rot = len(gathers)
    assert 1 <= n_rot <= 15 and 1 <= levels <= 3 and 0 <= radius <= 8 and 0 <= refine <= 8 and P.bases_ok(gathers, carries, levels, radius, refine)
    assert 1 <= min_inside <= W * H
    PN, PM = P.levels_of(N, levels), P.levels_of(M, levels)
    n = levels + 1
    centres, tabs, tots, ins, sums, flags, need = ([None] * n for _ in range(7))
    cen = [(0, 0)] * n_rot
    for lv in range(levels, -1, -1):
        p = radius if lv == levels else refine
        hyp = [(k, cen[k]) for k in range(n_rot)] + ([(0, (0, 0))] if lv == 0 else [])
        gs = []
        for k, (cx, cy) in hyp:
            a, b, c, d, e, f = P.level_gather(gathers[k], lv)
            gs.append((a, b, c + cx * Q, d, e, f + cy * Q))
        S, T, C, sums[lv] = NR.tables(PN[lv], PM[lv], gs, p)
        centres[lv] = np.array([c for _, c in hyp], np.int32).reshape(len(hyp), 2)
        tabs[lv], tots[lv], ins[lv], need[lv] = S, T, C, level_min_inside(min_inside, lv)
        if lv:
            cen, flags[lv] = [], np.zeros(n_rot, np.int32)
            for k in range(n_rot):
                (U, V), flags[lv][k] = level_best(S[k], T[k], C[k], hyp[k][1], need[lv])
                cen.append((2 * U, 2 * V))
    (k, u, v), at, qualified, f0 = choose(tabs[0], tots[0], ins[0], [tuple(int(t) for t in c) for c in centres[0]], n_rot, need[0])
    flags[0] = np.array(f0, np.int32)
    g, c = G.candidate(gathers[k], None if carries is None else carries[k], u, v)
    stc = lambda h, j, i: tuple(int(a[h, j, i]) for a in (tabs[0], tots[0], ins[0]))
    chosen_stc, prior_stc = stc(*at), stc(n_rot, refine, refine)
    return dict(chosen=(k, u, v), gather=g, carry=c, score=(chosen_stc[0], prior_stc[0], sums[0]), pyr_n=PN[1:], pyr_m=PM[1:],
                centres=centres, tables=tabs, totals=tots, inside=ins, sum_n=sums, flags=flags, need=need,
                chosen_stc=chosen_stc, prior_stc=prior_stc, qualified=qualified)


class Memory(R.Memory):
    """scene_memory_ref.Memory with append_pyramid_norm: yh_scene_append_memory_pyramid_norm given the frame's stamps and balls"""

    def append_pyramid_norm(self, N, frame_balls, gathers, carries, levels, radius, refine, min_inside, keep=224, max_age=30):
        self.motion = search(N, self.M, gathers, carries, levels, radius, refine, min_inside)
        return self.append(N, frame_balls, self.motion["gather"], self.motion["carry"], keep, max_age)
