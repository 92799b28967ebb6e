"""The scene memory's normalised registration (DESIGN.md §11 "Scene memory: normalised registration"):
yh_scene_append_memory_search_norm ranks the plain search's candidates by S / U over the pixels both maps cover, among those that
keep min_inside pixels inside, so that a large true shift on a dense map does not lose to "no motion". CPU part: the numpy
restatement (tests/scene_register_norm_ref.py) against answers worked out by hand and a per-pixel loop, the exact comparison, the
tie rule, min_inside, and the recovery on dense terrain that the plain choice misses; the binding's surface. GPU part (-m gpu): the
three tables, the choice and every output of the library against the restatement, bit for bit."""
import inspect
import os
import re

import numpy as np
import pytest

import scene_memory_ref as R
import scene_register_ref as G
import scene_register_norm_ref as GN
from test_scene_memory import IDENT, shift, turn90, _stamps, _same, _same_memory, _DeviceFrame
from test_scene_register import I32_MAX, I32_MIN, Q, ROTATION, SHEARED, _bases, _edge, _lds_words, _maps, _window_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_HOOK = "yh_scene_memory_search_norm_time"


def _brute(N, M, g, radius):
    """(S, T, C) of one base as nested lists, one pixel and one shift at a time, in Python integers"""
    H, W = N.shape
    n = 2 * radius + 1
    S, T, C = ([[0] * n for _ in range(n)] for _ in range(3))
    for v in range(-radius, radius + 1):
        for u in range(-radius, radius + 1):
            for y in range(H):
                for x in range(W):
                    sx, sy = R.affine(g, x, y)
                    if 0 <= sx + u < W and 0 <= sy + v < H:
                        a, b = int(N[y, x]), int(M[sy + v, sx + u])
                        S[v + radius][u + radius] += min(a, b)
                        T[v + radius][u + radius] += a + b
                        C[v + radius][u + radius] += 1
    return S, T, C


def _table(n_rot, radius, entries, fill=(0, 10, 100)):
    """(S, T, C) with (S, U, C) = fill everywhere but at entries {(k, u, v): (S, U, C)}"""
    S, T, C = (np.zeros((n_rot, 2 * radius + 1, 2 * radius + 1), np.uint64) for _ in range(3))
    S[:], T[:], C[:] = fill[0], fill[0] + fill[1], fill[2]
    for (k, u, v), (s, uu, c) in entries.items():
        S[k, v + radius, u + radius], T[k, v + radius, u + radius], C[k, v + radius, u + radius] = s, s + uu, c
    return S, T, C


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------------

def test_tables_known_answers():
    M = (np.arange(16, dtype=np.uint32).reshape(4, 4) + 1) * 10
    N = np.zeros((4, 4), np.uint32)
    N[1, 1], N[2, 3] = 100, 35
    S, T, C, sum_n = GN.tables(N, M, [R.IDENTITY], 1)
    # by hand. C = (4 - |u|)(4 - |v|). T: N[1][1] is inside under every shift, N[2][3] only for u <= 0; the Q are M over the rectangle
    # the shifted frame covers: (0, 0) 135 + 1360; (1, 0) 100 + (1360 - column 0 = 280); (-1, -1) 135 + 10 (1 + 2 + 3 + 5 + 6 + 7 + 9 + 10 + 11)
    assert sum_n == 135 and C[0].tolist() == [[9, 12, 9], [12, 16, 12], [9, 12, 9]]
    assert S[0].tolist() == [[45, 55, 30], [85, 95, 70], [125, 135, 100]]
    assert (int(T[0, 1, 1]), int(T[0, 1, 2]), int(T[0, 0, 0])) == (1495, 1180, 675)
    assert (S[0].tolist(), T[0].tolist(), C[0].tolist()) == _brute(N, M, R.IDENTITY, 1)
    # 5 x 3, a map that moved one pixel to the right: column 0 of N has no source, so the truth covers ten pixels - and agrees on all
    M = np.array([[5, 1, 9], [2, 8, 3], [7, 4, 6], [1, 9, 2], [8, 3, 5]], np.uint32)
    N = np.zeros_like(M)
    N[:, 1:] = M[:, :2]
    g, c = shift(1, 0)
    S, T, C, sum_n = GN.tables(N, M, [g, R.IDENTITY], 1)
    assert sum_n == 48 and (int(S[0, 1, 1]), int(T[0, 1, 1]), int(C[0, 1, 1])) == (48, 96, 10)          # S = U: ratio 1
    assert (int(S[1, 1, 0]), int(T[1, 1, 0]), int(C[1, 1, 0])) == (48, 96, 10)                         # the identity moved one to the left: the same pixels
    assert (int(S[1, 1, 1]), int(T[1, 1, 1]), int(C[1, 1, 1])) == (24, 48 + 73, 15)                    # the identity: all fifteen, N's column 0 is 0
    for k, gk in enumerate((g, R.IDENTITY)):
        assert (S[k].tolist(), T[k].tolist(), C[k].tolist()) == _brute(N, M, gk, 1)
    out = GN.search(N, M, [g, R.IDENTITY], [c, R.IDENTITY], 1, 10)
    assert out["chosen"] == (0, 0, 0) and out["qualified"] and out["chosen_stc"] == out["prior_stc"] == (48, 96, 10) and out["score"] == (48, 48, 48)
    assert out["gather"] == tuple(g) and out["carry"] == tuple(c)
    # values up to 2^32 - 1, sources that are negative or read across the frame, coefficients on the int32 conditions
    rng = np.random.default_rng(3)
    N, M = (rng.integers(0, 1 << 32, (5, 3), dtype=np.uint64).astype(np.uint32) for _ in range(2))
    N[0, 0] = M[0, 0] = N[4, 2] = M[2, 1] = 0xFFFFFFFF
    for g in (R.IDENTITY, shift(-2, 1)[0], turn90(1, 2)[0], ROTATION[0], SHEARED[1], (I32_MAX, I32_MIN, 0, I32_MIN, I32_MAX, 0), _edge(2), _edge(2, -1)):
        S, T, C, _ = GN.tables(N, M, [g], 2)
        assert (S[0].tolist(), T[0].tolist(), C[0].tolist()) == _brute(N, M, g, 2), g
        assert np.array_equal(S, G.scores(N, M, [g], 2)[0])


def test_s_is_the_plain_score_table():
    for H, W, seed, radius in ((9, 11, 1, 3), (37, 53, 2, 2)):
        N, M = _maps(H, W, seed, top=1 << 32)
        gathers = _bases(H, W, radius)[:6]
        S, T, C, sum_n = GN.tables(N, M, gathers, radius)
        plain, plain_n = G.scores(N, M, gathers, radius)
        assert np.array_equal(S, plain) and sum_n == plain_n
        assert (T >= 2 * S).all() and (C <= H * W).all() and int(C[0, radius, radius]) == H * W and not C[5].any()   # min + max; the identity; every pixel outside


def test_the_ratio_is_compared_in_128_bits():
    # 2^33 / 1 against 1 / 2^31: the cross products are 2^64 - which wraps to 0 - and 1
    assert GN.ratio_cmp(1 << 33, 1, 1, 1 << 31) == 1 and ((1 << 33) * (1 << 31)) % (1 << 64) < 1
    big = (1 << 58) + 12345
    pairs = [((big, big + 1), (big - 1, big)),            # n / (n + 1) > (n - 1) / n, by 1 in 2^116
             ((1 << 57, (1 << 58) + 2), (1 << 56, (1 << 57) + 1)),   # equal ratios exactly
             ((3 << 10, (1 << 59) - 1), (2 << 10, (1 << 59) - 3))]
    for (s1, u1), (s2, u2) in pairs:
        want = (s1 * u2 > s2 * u1) - (s1 * u2 < s2 * u1)
        assert GN.ratio_cmp(s1, u1, s2, u2) == want == -GN.ratio_cmp(s2, u2, s1, u1)
        assert s1 * u2 >= 1 << 64 and s2 * u1 >= 1 << 64                                             # neither product fits 64 bits
    assert GN.ratio_cmp(*pairs[0][0], *pairs[0][1]) == 1 and GN.ratio_cmp(*pairs[1][0], *pairs[1][1]) == 0 and GN.ratio_cmp(*pairs[2][0], *pairs[2][1]) == 1
    # in the choice: u64 tables whose products pass 2^64
    S, T, C = _table(1, 1, {(0, 1, 1): (big, big + 1, 100), (0, -1, -1): (big - 1, big, 100)}, fill=(1 << 56, (1 << 57) + 1, 100))
    assert GN.choose(S, T, C, 1) == ((0, 1, 1), True)
    S, T, C = _table(1, 1, {(0, 1, 1): (1 << 33, 1, 100)}, fill=(1, 1 << 31, 100))
    assert GN.choose(S, T, C, 1) == ((0, 1, 1), True)


def test_every_tie_break_level():
    ch = lambda n_rot, entries, **kw: GN.choose(*_table(n_rot, 2, entries, **kw), 50)[0]
    assert ch(2, {(0, 0, 0): (5, 10, 100), (1, 2, 2): (6, 10, 100)}) == (1, 2, 2)                      # the larger ratio, however far
    assert ch(2, {(0, 0, 0): (6, 10, 100), (1, 2, 2): (5, 5, 100)}) == (1, 2, 2)                       # .. the ratio, not S
    assert ch(2, {(0, 2, 0): (6, 10, 100), (1, 1, 0): (3, 5, 100)}) == (1, 1, 0)                       # then the smaller u^2 + v^2, whatever k (6/10 = 3/5)
    assert ch(2, {(1, 0, -1): (6, 10, 100), (0, 1, 0): (6, 10, 100)}) == (0, 1, 0)                     # then the smaller k, whatever v
    assert ch(2, {(1, -1, 0): (6, 10, 100), (1, 0, -1): (6, 10, 100), (1, 0, 1): (6, 10, 100)}) == (1, 0, -1)   # then the smaller v
    assert ch(2, {(1, 1, 0): (6, 10, 100), (1, -1, 0): (6, 10, 100)}) == (1, -1, 0)                    # then the smaller u
    assert ch(3, {(0, 1, 2): (6, 10, 100), (0, 2, 1): (6, 10, 100), (0, -1, -2): (6, 10, 100), (0, -2, -1): (6, 10, 100), (0, 2, -1): (6, 10, 100)}) == (0, -1, -2)
    assert ch(3, {}, fill=(7, 9, 100)) == (0, 0, 0)


def test_min_inside_from_both_sides_and_none_qualified():
    # a sliver that agrees perfectly (ratio 1 on 49 pixels) against a good overlap (ratio 0.6 on 100)
    entries = {(0, 2, 2): (49, 49, 49), (0, 1, 0): (6, 10, 100)}
    fill = (1, 10, 100)
    assert GN.choose(*_table(1, 2, entries, fill=fill), 49) == ((0, 2, 2), True)
    assert GN.choose(*_table(1, 2, entries, fill=fill), 50) == ((0, 1, 0), True)
    assert GN.choose(*_table(1, 2, entries, fill=fill), 100) == ((0, 1, 0), True)
    assert GN.choose(*_table(1, 2, entries, fill=fill), 101) == ((0, 0, 0), False)                     # none qualified: the prior
    # U = 0 does not qualify either, whatever C: nothing on either map under that candidate
    assert GN.choose(*_table(2, 1, {(1, 1, 1): (0, 0, 100)}, fill=(0, 0, 100)), 1) == ((0, 0, 0), False)
    assert GN.choose(*_table(2, 1, {(1, 1, 1): (0, 5, 100)}, fill=(0, 0, 100)), 1) == ((1, 1, 1), True)
    N = np.full((6, 7), 9, np.uint32)
    out = GN.search(N, N, [(Q, 0, 20 * Q, 0, Q, 0)], [R.IDENTITY], 2, 1)                              # every pixel outside: C = 0 everywhere
    assert not out["inside"].any() and out["chosen"] == (0, 0, 0) and not out["qualified"] and out["chosen_stc"] == (0, 0, 0)
    out = GN.search(N, N, [R.IDENTITY], None, 2, 6 * 7)                                               # only the unshifted candidate keeps all 42
    assert out["chosen"] == (0, 0, 0) and out["qualified"] and out["chosen_stc"] == (42 * 9, 2 * 42 * 9, 42)


def test_empty_maps_choose_the_prior():
    rng = np.random.default_rng(5)
    H, W = 9, 11
    full = rng.integers(1, 500, (H, W)).astype(np.uint32)
    zero = np.zeros((H, W), np.uint32)
    bases = [R.IDENTITY, shift(1, 0)[0], ROTATION[0]]
    out = GN.search(zero, zero, bases, None, 3, 1)                                                    # both empty: U = 0, none qualified
    assert out["chosen"] == (0, 0, 0) and not out["qualified"] and not out["totals"].any() and out["inside"][0, 3, 3] == H * W
    out = GN.search(full, zero, bases, None, 3, 1)                                                    # an empty memory: every ratio 0, the tie rule
    assert out["chosen"] == (0, 0, 0) and out["qualified"] and not out["scores"].any() and out["chosen_stc"] == (0, int(full.sum()), H * W)
    out = GN.search(zero, full, bases, None, 3, 1)                                                    # an empty frame: likewise
    assert out["chosen"] == (0, 0, 0) and out["qualified"] and not out["scores"].any() and out["chosen_stc"] == (0, int(full.sum()), H * W)
    out = GN.search(full, zero, [shift(1, 0)[0], R.IDENTITY], None, 0, 1)
    assert out["chosen"] == (0, 0, 0) and out["gather"] == tuple(shift(1, 0)[0])


# the dense terrain the plain score goes wrong on: twelve low-frequency sines, 200 .. 7200, no zeros; M a window of the field, N the
# window moved by the true shift (N(x, y) = M(x + u, y + v) wherever both see it), optionally with uniform noise of +-300 on N
_TERRAIN = {}
# Seeds 1 .. 6 were tried on every case below (48 in all). The normalised choice recovers the truth on all 48, strictly on the 24
# without noise. The plain choice misses on 43; on seeds 3, 4 and 6 it finds the truth in five noise-free cases, so those seeds do not
# show the difference in every case; 1, 2 and 5 do.
TERRAIN_SEED = 1


def _terrain(H, W, true, noise, seed=TERRAIN_SEED):
    key = (H, W, true, noise, seed)
    if key not in _TERRAIN:
        rng = np.random.default_rng(seed)
        pad = 8
        yy, xx = np.mgrid[0:H + 2 * pad, 0:W + 2 * pad].astype(np.float64)
        f = np.zeros_like(yy)
        for _ in range(12):
            fx, fy, amp, ph = rng.uniform(-0.06, 0.06), rng.uniform(-0.06, 0.06), rng.uniform(0.3, 1.0), rng.uniform(0, 2 * np.pi)
            f += amp * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
        F = np.rint(200 + (f - f.min()) / (f.max() - f.min()) * 7000).astype(np.int64)
        u, v = true
        M = F[pad:pad + H, pad:pad + W]
        N = F[pad + v:pad + v + H, pad + u:pad + u + W]
        if noise:
            N = N + rng.integers(-noise, noise + 1, N.shape)
            N = np.maximum(N, 1)                                                                      # (no zeros, and nothing below zero)
        assert N.min() > 0 and M.min() >= 200 and M.max() <= 7200
        N, M = N.astype(np.uint32), M.astype(np.uint32)
        _TERRAIN[key] = (N, M, GN.search(N, M, [R.IDENTITY], [R.IDENTITY], 8, (W * H) // 4))
    return _TERRAIN[key]


TERRAIN_CASES = [(37, 53, (5, -3)), (37, 53, (8, 8)), (37, 53, (-7, 2)), (65, 130, (6, -8))]


def _check_recovery(out, true, noise, min_inside):
    u, v = true
    S, T = out["scores"], out["totals"]
    assert G.choose(S) != (0, u, v)                                                                   # the plain choice misses it
    assert out["chosen"] == (0, u, v) and out["qualified"]
    ok = (out["inside"] >= min_inside) & (T > S)                                                      # the qualified candidates
    assert ok[0, v + 8, u + 8]
    if not noise:
        s, t, _ = out["chosen_stc"]
        assert t - s == s > 0                                                                         # S = U at the truth
        U = (T - S).astype(object)
        strictly = [(vi, ui) for vi in range(17) for ui in range(17) if ok[0, vi, ui] and (vi, ui) != (v + 8, u + 8) and int(S[0, vi, ui]) >= int(U[0, vi, ui])]
        assert not strictly, strictly                                                                 # S < U at every other qualified candidate


@pytest.mark.parametrize("noise", [0, 300])
@pytest.mark.parametrize("H,W,true", TERRAIN_CASES)
def test_recovery_on_dense_terrain(H, W, true, noise):
    N, M, out = _terrain(H, W, true, noise)
    assert out["inside"][0, 8, 8] == H * W
    _check_recovery(out, true, noise, (W * H) // 4)
    want = G.candidate(R.IDENTITY, R.IDENTITY, *true)
    assert (out["gather"], out["carry"]) == want


def test_surface(built):
    from yolact_amd import capi
    import yolact_amd as ya
    L = capi.load_library()
    pub = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read()
    protos = dict((s[0], s) for s in capi.SYMBOLS)
    _i, _vp, _fp = capi.C.c_int32, capi.C.c_void_p, capi.C.POINTER(capi.C.c_float)
    assert protos["yh_scene_append_memory_search_norm"][1:] == (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i])
    assert protos["yh_scene_motion_norm_read"][1:] == (_i, [_vp, _vp, _vp, _vp, _vp, _vp])
    assert protos["yh_scene_op_register_norm"][1:] == (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp])
    assert protos["yh_scene_memory_search_norm_time"][1:] == (_i, [_vp, _i, _fp, _fp])
    for name in ("yh_scene_append_memory_search_norm", "yh_scene_motion_norm_read"):
        assert hasattr(L, name) and re.search(r"\bint %s\(yh_scene\* h" % name, pub) and name not in re.sub(r"/\*.*?\*/", "", dbg, flags=re.S), name
    for name in ("yh_scene_op_register_norm", "yh_scene_memory_search_norm_time"):
        assert hasattr(L, name) and name not in pub and re.search(r"\bint %s\(yh_scene\* h" % name, dbg), name
    assert re.search(r"int yh_scene_append_memory_search_norm\(yh_scene\* h, const uint16_t\* depth_host, const uint32_t\* frame, int32_t frame_on_device, int32_t n_rot,\s*"
                     r"const int32_t\* gather_q16 /\* \[n_rot\]\[6\] \*/, const int32_t\* carry_q16 /\* \[n_rot\]\[6\] \*/, int32_t radius,\s*"
                     r"int32_t min_inside, int32_t keep, int32_t ball_max_age\);", pub)
    assert re.search(r"int yh_scene_motion_norm_read\(yh_scene\* h, uint64_t\* totals [^,]*, uint64_t\* inside [^,]*,\s*"
                     r"uint64_t\* chosen_stc /\* \[3\] = S, T, C \*/, uint64_t\* prior_stc /\* \[3\] \*/, int32_t\* qualified\);", pub)
    assert re.search(r"int yh_scene_memory_search_norm_time\(yh_scene\* h, int32_t reps, float\* ms_per_frame, float\* ms_search\);", dbg)
    assert "#define YH_ABI_VERSION 4" in pub and "Scene memory: normalised registration" in pub
    assert pub.index("int yh_scene_append_memory_search(") < pub.index("int yh_scene_append_memory_search_norm(") < pub.index("---- scene batch")
    sig = inspect.signature(capi.Scene.append_memory_search_norm)
    assert list(sig.parameters) == ["self", "depth", "frame_u32", "frame_dev_ptr", "cls_id", "candidates", "radius", "min_inside", "keep", "ball_max_age"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, None, None, None, 4, None, 224, 30]
    assert list(inspect.signature(capi.Scene.read_motion_norm).parameters) == ["self"]
    assert list(inspect.signature(capi.Scene.op_register_norm).parameters) == ["self", "n", "m", "gathers", "radius", "min_inside"]
    assert inspect.signature(capi.Scene.memory_search_norm_time).parameters["reps"].default == 20
    assert ya.Scene is capi.Scene
    cfg = capi.Config()
    L.yh_default_config(cfg)
    assert cfg.abi_version == 4
    # no tuning field, no new environment variable, the plain search's files as they were: the new kernels live in files of their own
    csrc = os.path.join(ROOT, "tiny-object-detection_amd", "csrc")
    assert "register_norm" not in open(os.path.join(csrc, "scene_register.hip")).read() + open(os.path.join(csrc, "scene_register_dev.h")).read()
    assert "scene_register_norm.o" in open(os.path.join(ROOT, "tiny-object-detection_amd", "Makefile")).read()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def _check_norm(sc, N, M, gathers, radius, min_insides, what):
    """op_register_norm against the restatement at every min_inside given - or, a function, that it makes of the table C - (the
    tables once); returns the restatement's tables"""
    S, T, C, sum_n = GN.tables(N, M, gathers, radius)
    if callable(min_insides):
        min_insides = min_insides(C)
    for mi in min_insides:
        chosen, qualified = GN.choose(S, T, C, mi)
        got = sc.op_register_norm(N, M, gathers, radius, mi)
        for name, want in (("scores", S), ("totals", T), ("inside", C)):
            assert got[name].dtype == np.uint64 and got[name].shape == want.shape, (what, name)
            assert np.array_equal(got[name], want), (what, name, mi, np.argwhere(got[name] != want)[:5].tolist())
        assert (got["chosen"], got["qualified"], got["sum_n"]) == (chosen, qualified, sum_n), (what, mi, got["chosen"], got["qualified"], chosen, qualified)
    return S, T, C


@pytest.mark.gpu
@pytest.mark.parametrize("radius,n_rot,first", [(0, 1, 0), (1, 3, 0), (3, 3, 3), (8, 16, 0)])
@pytest.mark.parametrize("H,W", [(3, 3), (8, 8), (37, 53), (100, 9), (65, 130)])
def test_op_register_norm_matches_the_restatement(built, H, W, radius, n_rot, first):
    import yolact_amd as ya
    N, M = _maps(H, W, 100 * H + W)                                                                  # (the first tile of N is empty where there are several)
    gathers = _bases(H, W, radius)[first:first + n_rot]
    sc = ya.Scene(W, H)
    # min_inside at 1, at the default, at W H, and one above the largest C (where that is allowed): none qualified
    S, T, C = _check_norm(sc, N, M, gathers, radius, lambda C: (1, max((W * H) // 4, 1), W * H, min(int(C.max()) + 1, W * H)), (H, W, radius, n_rot))
    assert T.max() > 0 and C.max() > 0
    if (H, W) == (65, 130):
        assert not N[:16, :64].any() and M[:16, :64].any()                                            # the tile the plain kernel leaves early: its Q and pixels count
        if any(tuple(g) == SHEARED[1] for g in gathers):                                              # the magnifying shear ran the global fallback
            assert _window_words(SHEARED[1], H, W, radius) > _lds_words()
    sc.close()


@pytest.mark.gpu
def test_op_register_norm_none_qualified_when_every_pixel_is_outside(built):
    import yolact_amd as ya
    H, W = 37, 53
    N, M = _maps(H, W, 9)
    sc = ya.Scene(W, H)
    S, T, C = _check_norm(sc, N, M, [(Q, 0, 2 * W * Q, 0, Q, 0), (Q, 0, 0, 0, Q, -3 * H * Q)], 3, (1, W * H), "outside")
    assert not C.any() and not T.any()
    zero = np.zeros((H, W), np.uint32)
    _check_norm(sc, zero, zero, [R.IDENTITY, shift(1, 0)[0]], 2, (1,), "both empty")
    _check_norm(sc, N, zero, [R.IDENTITY, shift(1, 0)[0]], 2, (1,), "empty memory")
    _check_norm(sc, zero, M, [R.IDENTITY, shift(1, 0)[0]], 2, (1,), "empty frame")
    sc.close()


@pytest.mark.gpu
def test_op_register_norm_full_range_values_and_edge_coefficients(built):
    import yolact_amd as ya
    H, W = 65, 130
    N, M = _maps(H, W, 7, top=1 << 32)
    N[20:40, 70:120] = 0xFFFFFFFF; M[18:44, 66:124] = 0xFFFFFFFF                                      # a thousand pixels of 2^32 - 1 that meet under small shifts
    sc = ya.Scene(W, H)
    S, T, C = _check_norm(sc, N, M, [R.IDENTITY, shift(3, -2)[0], SHEARED[1], _edge(3), _edge(3, -1), (I32_MAX, I32_MIN, 0, I32_MIN, I32_MAX, 0)], 3,
                          (1, (W * H) // 4), "full range")
    assert S.max() > 1 << 41 and T.max() > 1 << 43                                                    # cross products far past 64 bits
    sc.close()


@pytest.mark.gpu
def test_op_register_norm_at_the_camera_size(built):
    import yolact_amd as ya
    H, W = 480, 640
    N, M = _maps(H, W, 8)
    sc = ya.Scene(W, H)
    _check_norm(sc, N, M, [ROTATION[0], R.IDENTITY, SHEARED[1]], 2, ((W * H) // 4,), "640 x 480")
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("noise", [0, 300])
@pytest.mark.parametrize("H,W,true", TERRAIN_CASES)
def test_op_register_norm_recovers_the_shift_on_dense_terrain(built, H, W, true, noise):
    import yolact_amd as ya
    N, M, want = _terrain(H, W, true, noise)
    sc = ya.Scene(W, H)
    got = sc.op_register_norm(N, M, [R.IDENTITY], 8, (W * H) // 4)
    for a, b in (("scores", "scores"), ("totals", "totals"), ("inside", "inside")):
        assert np.array_equal(got[a], want[b]), a
    assert got["chosen"] == (0,) + true == want["chosen"] and got["qualified"] and got["sum_n"] == want["score"][2]
    plain, chosen, _ = sc.op_register(N, M, [R.IDENTITY], 8)                                          # the S table is the plain kernel's; its choice misses
    assert np.array_equal(plain, got["scores"]) and chosen != (0,) + true
    sc.close()


@pytest.mark.gpu
def test_the_s_table_is_op_registers(built):
    import yolact_amd as ya
    H, W = 65, 130
    N, M = _maps(H, W, 21, top=1 << 32)
    gathers = _bases(H, W, 4)[:8]
    sc = ya.Scene(W, H)
    plain, _, sum_n = sc.op_register(N, M, gathers, 4)
    got = sc.op_register_norm(N, M, gathers, 4, 1)
    assert np.array_equal(got["scores"], plain) and got["sum_n"] == sum_n
    sc.close()


def _same_motion(sc, want, what):
    got = sc.read_motion(scores=True)
    assert tuple(got["chosen"].tolist()) == want["chosen"] and tuple(got["gather"].tolist()) == want["gather"] and tuple(got["carry"].tolist()) == want["carry"], (what, got, want["chosen"])
    assert tuple(int(v) for v in got["score"]) == want["score"] and np.array_equal(got["scores"], want["scores"]), what
    ext = sc.read_motion_norm()
    assert np.array_equal(ext["totals"], want["totals"]) and np.array_equal(ext["inside"], want["inside"]), what
    assert tuple(int(v) for v in ext["chosen_stc"]) == want["chosen_stc"] and tuple(int(v) for v in ext["prior_stc"]) == want["prior_stc"], (what, ext, want["chosen_stc"])
    assert ext["qualified"] == want["qualified"], what
    return got


def _candidates(H, W):
    """per frame of a sequence: (gathers, carries), radius, min_inside"""
    return [(([IDENT[0]], [IDENT[1]]), 2, 1),
            (([shift(1, 0)[0], IDENT[0], ROTATION[0]], [shift(1, 0)[1], IDENT[1], ROTATION[1]]), 2, (W * H) // 4),
            (([ROTATION[0], shift(-2, 1)[0]], [ROTATION[1], shift(-2, 1)[1]]), 3, (W * H) // 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (37, 53), (100, 9)])
def test_norm_sequences_match_the_restatement_and_append_memory(built, oracle, H, W):
    import yolact_amd as ya
    sc, mem, ref = ya.Scene(W, H), ya.Scene(W, H), GN.Memory(W, H)
    for t, ((gs, cs), radius, mi) in enumerate(_candidates(H, W)):
        depth, ci, o = _stamps(oracle, H, W, 10 * H + W + t, balls=t != 1)                            # the second frame has no ball: those of the first are remembered
        keep = (256, 224, 200)[t]
        sc.append_memory_search_norm(depth, cls_id=ci, candidates=(gs, cs), radius=radius, min_inside=mi, keep=keep, ball_max_age=5)
        want = ref.append_search_norm(o["map"], o["balls"], gs, cs, radius, mi, keep, 5)
        got = _same_motion(sc, ref.motion, (H, W, t))
        _same(sc.read(), want, ("norm", H, W, t))
        _same_memory(sc, ref, ("norm", H, W, t))
        # a second handle given the twelve integers read back
        mem.append_memory(depth, cls_id=ci, motion=(got["gather"].tolist(), got["carry"].tolist()), keep=keep, ball_max_age=5)
        _same(mem.read(), want, ("append_memory", H, W, t))
        _same_memory(mem, ref, ("append_memory", H, W, t))
    assert ref.motion["score"][2] > 0
    sc.close(); mem.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (37, 53)])
def test_one_candidate_is_append_memory_and_an_empty_memory_a_plain_append(built, oracle, H, W):
    import yolact_amd as ya
    d0, c0, _ = _stamps(oracle, H, W, 1)
    d1, c1, _ = _stamps(oracle, H, W, 2)
    srch, mem, plain = ya.Scene(W, H), ya.Scene(W, H), ya.Scene(W, H)
    srch.append_memory_search_norm(d0, cls_id=c0, candidates=([IDENT[0], ROTATION[0]], [IDENT[1], ROTATION[1]]), radius=8, min_inside=1, keep=256, ball_max_age=255)
    plain.append_classified(d0, frame_u32=ya.SceneBatch.pack(c0), mode=ya.COMPAT_SANE)               # an empty memory: every ratio 0, the prior, nothing to carry
    _same(srch.read(), plain.read(), ("empty", H, W))
    ext = srch.read_motion_norm()
    assert tuple(srch.read_motion()["chosen"].tolist()) == (0, 0, 0) and ext["qualified"] and int(ext["chosen_stc"][0]) == 0 and int(ext["chosen_stc"][2]) == W * H
    mem.append_memory(d0, cls_id=c0, motion=IDENT, keep=256, ball_max_age=255)
    for t, motion in enumerate((ROTATION, shift(2, -1))):
        srch.append_memory_search_norm(d1, cls_id=c1, candidates=([motion[0]], [motion[1]]), radius=0, min_inside=W * H, keep=200, ball_max_age=9)
        mem.append_memory(d1, cls_id=c1, motion=motion, keep=200, ball_max_age=9)                     # (qualified or not: there is one candidate)
        _same(srch.read(), mem.read(), ("n_rot 1, R 0", H, W, t))
        a, b = srch.read_memory(), mem.read_memory()
        assert np.array_equal(a["map"], b["map"]) and np.array_equal(a["balls"], b["balls"])
        got = srch.read_motion(scores=True)
        assert (tuple(got["gather"].tolist()), tuple(got["carry"].tolist())) == motion and got["scores"].shape == (1, 1, 1) and got["scores"][0, 0, 0] == got["score"][0] == got["score"][1]
    assert plain.read()["map"].max() > 0
    srch.close(); mem.close(); plain.close()


@pytest.mark.gpu
def test_a_remembered_ball_is_carried_by_the_chosen_carry(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    d, c, o = _stamps(oracle, H, W, 61)
    _, c_none, o_none = _stamps(oracle, H, W, 61, balls=False)                                        # the same depth image, the balls not seen
    sc, ref = ya.Scene(W, H), GN.Memory(W, H)
    sc.append_memory_search_norm(d, cls_id=c, radius=0)
    ref.append_search_norm(o["map"], o["balls"], [R.IDENTITY], [R.IDENTITY], 0, (W * H) // 4)
    seen = ref.B.copy()
    g, cr = shift(2, 1)                                                                               # the prior says the map moved; it did not
    sc.append_memory_search_norm(d, cls_id=c_none, candidates=([g], [cr]), radius=3, keep=256, ball_max_age=5)
    want = ref.append_search_norm(o_none["map"], o_none["balls"], [g], [cr], 3, (W * H) // 4, 256, 5)
    s, t, _ = ref.motion["chosen_stc"]
    assert ref.motion["chosen"] == (0, 2, 1) and ref.motion["carry"] == R.IDENTITY and t - s == s > 0   # the maps agree on all of the frame
    _same_motion(sc, ref.motion, "ball")
    _same(sc.read(), want, ("ball",))
    _same_memory(sc, ref, "ball")
    ids = np.flatnonzero(seen[:, 2] > 0)
    assert len(ids) == 2 and not o_none["balls"].any()
    mem = sc.read_memory()["balls"]
    for k in ids:                                                                                     # where it was, not two pixels right and one down
        assert mem[k].tolist() == [seen[k, 0], seen[k, 1], seen[k, 2], 1] and sc.read()["balls"][k].tolist() == [seen[k, 0], seen[k, 1], seen[k, 2], 0]
    sc.close()


@pytest.mark.gpu
def test_a_planner_runs_on_the_fused_frame(built, oracle):
    import yolact_amd as ya
    H, W = 33, 65
    start = ((W * 5) // 8, H - 1)
    d0, c0, _ = _stamps(oracle, H, W, 31)
    d1, c1, o1 = _stamps(oracle, H, W, 32, balls=False)
    sc, other = ya.Scene(W, H), ya.Scene(W, H)
    sc.append_memory_search_norm(d0, cls_id=c0, radius=1)
    sc.append_memory_search_norm(d1, cls_id=c1, candidates=([shift(2, -1)[0], IDENT[0]], [shift(2, -1)[1], IDENT[1]]), radius=2, keep=240)
    f = sc.read()
    assert not o1["balls"].any() and (f["balls"][:, 2] > 0).sum() >= 1 and (f["map"] > o1["map"]).any()          # balls only remembered, map fused
    remembered = [(int(b[0]), int(b[1])) for b in f["balls"] if b[2] > 0]
    other.set_fields(f["map"], f["conn0"], f["conn1"])
    sc.plan(None, n_targets=3, start=start, connectivity=8)
    other.plan(remembered[:3], start=start, connectivity=8)
    a, b = sc.read_plan(), other.read_plan()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    sc.close(); other.close()


def _estate(call, names=None):
    import yolact_amd as ya
    with pytest.raises(ya.YhError) as e:
        call()
    assert e.value.code == ya.capi.ESTATE and (names is None or names in str(e.value)), str(e.value)


@pytest.mark.gpu
def test_norm_time_commits_nothing_and_the_other_hooks_name_it(built, oracle):
    import ctypes as C
    import yolact_amd as ya
    H, W = 37, 53
    d0, c0, _ = _stamps(oracle, H, W, 41)
    d1, c1, _ = _stamps(oracle, H, W, 42)
    sc = ya.Scene(W, H)
    cands = ([shift(1, 0)[0], ROTATION[0]], [shift(1, 0)[1], ROTATION[1]])
    sc.append_memory_search_norm(d0, cls_id=c0, radius=1)
    sc.append_memory_search_norm(d1, cls_id=c1, candidates=cands, radius=3, keep=250)
    before, mem, motion, ext = sc.read(), sc.read_memory(), sc.read_motion(scores=True), sc.read_motion_norm()
    ms, ms_search = sc.memory_search_norm_time(3)
    assert ms > 0 and 0 < ms_search < ms
    _same(sc.read(), before, ("norm time",))
    after, again, ext2 = sc.read_memory(), sc.read_motion(scores=True), sc.read_motion_norm()
    assert np.array_equal(after["map"], mem["map"]) and np.array_equal(after["balls"], mem["balls"])
    assert all(np.array_equal(again[k], motion[k]) for k in motion) and all(np.array_equal(ext2[k], ext[k]) for k in ext)
    for call in (lambda: sc.time(2), lambda: sc.memory_time(2), lambda: sc.memory_search_time(2), lambda: sc.memory_pyramid_time(2)):
        _estate(call, NORM_HOOK)
    f = C.c_float()
    assert sc.L.yh_scene_memory_search_norm_time(sc.h, 0, C.byref(f), C.byref(f)) == ya.capi.EINVAL
    assert sc.L.yh_scene_memory_search_norm_time(sc.h, 1, None, C.byref(f)) == ya.capi.EINVAL and sc.L.yh_scene_memory_search_norm_time(sc.h, 1, C.byref(f), None) == ya.capi.EINVAL
    assert sc.L.yh_scene_memory_search_norm_time(None, 1, C.byref(f), C.byref(f)) == ya.capi.EINVAL
    sc.close()


@pytest.mark.gpu
def test_motion_reads_in_every_state(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    d, c, _ = _stamps(oracle, H, W, 43)
    cands = ([shift(1, 0)[0], IDENT[0]], [shift(1, 0)[1], IDENT[1]])
    sc = ya.Scene(W, H)
    _estate(sc.read_motion_norm); _estate(sc.read_motion); _estate(lambda: sc.memory_search_norm_time(2))           # no memory append yet
    sc.append_classified(d, frame_u32=ya.SceneBatch.pack(c), mode=ya.COMPAT_SANE)
    _estate(sc.read_motion_norm); _estate(lambda: sc.memory_search_norm_time(2))
    sc.append_memory(d, cls_id=c)                                                                     # a plain memory append
    _estate(sc.read_motion_norm); _estate(sc.read_motion); _estate(lambda: sc.memory_search_norm_time(2))
    assert sc.memory_time(2) > 0
    sc.append_memory_search(d, cls_id=c, candidates=cands, radius=2)                                  # a plain search: its own reads and hook, as before
    plain = sc.read_motion(scores=True)
    _estate(sc.read_motion_norm); _estate(lambda: sc.memory_search_norm_time(2))
    assert sc.memory_search_time(2)[0] > 0
    _estate(lambda: sc.time(2), "yh_scene_memory_search_time"); _estate(lambda: sc.memory_time(2), "yh_scene_memory_search_time")
    sc.append_memory_search_norm(d, cls_id=c, candidates=cands, radius=2)                             # the normalised search: both reads
    got, ext = sc.read_motion(scores=True), sc.read_motion_norm()
    assert got["scores"].shape == plain["scores"].shape == ext["totals"].shape == ext["inside"].shape == (2, 5, 5)
    assert int(got["score"][0]) == int(ext["chosen_stc"][0]) and int(got["score"][1]) == int(ext["prior_stc"][0]) == int(got["scores"][0, 2, 2])
    assert sc.L.yh_scene_motion_norm_read(sc.h, None, None, None, None, None) == ya.capi.OK and sc.L.yh_scene_motion_norm_read(None, None, None, None, None, None) == ya.capi.EINVAL
    sc.plan(None, start=((W * 5) // 8, H - 1))                                                        # plans and plain appends do not end it
    sc.append_classified(d, frame_u32=ya.SceneBatch.pack(c), mode=ya.COMPAT_SANE)
    assert all(np.array_equal(sc.read_motion_norm()[k], ext[k]) for k in ext)
    _estate(lambda: sc.memory_search_norm_time(2))                                                    # .. but the last frame is no longer that append
    assert sc.time(2) > 0
    sc.append_memory_search_norm(d, cls_id=c, candidates=cands, radius=2)
    sc.append_memory_pyramid(d, cls_id=c, candidates=cands, levels=2, radius=2, refine=1)             # a pyramid append: its own state, as before
    _estate(sc.read_motion_norm); _estate(lambda: sc.memory_search_norm_time(2))
    assert sc.memory_pyramid_time(2)[0] > 0 and sc.read_motion()["chosen"].shape == (3,)
    _estate(lambda: sc.memory_search_time(2), "yh_scene_memory_pyramid_time")
    sc.append_memory_search_norm(d, cls_id=c, candidates=cands, radius=2)
    sc.memory_reset()                                                                                 # a reset ends it
    _estate(sc.read_motion_norm); _estate(sc.read_motion); _estate(lambda: sc.memory_search_norm_time(2))
    sc.close()


@pytest.mark.gpu
def test_refusals_touch_nothing(built, oracle):
    import yolact_amd as ya
    from yolact_amd.capi import _p
    H, W = 37, 53
    start = ((W * 5) // 8, H - 1)
    d0, c0, _ = _stamps(oracle, H, W, 51)
    d1, c1, _ = _stamps(oracle, H, W, 52)
    sc = ya.Scene(W, H)
    sc.append_memory_search_norm(d0, cls_id=c0, candidates=([shift(1, 0)[0]], [shift(1, 0)[1]]), radius=2)
    sc.plan(None, start=start)
    before, mem, plan, motion, ext = sc.read(), sc.read_memory(), sc.read_plan(), sc.read_motion(scores=True), sc.read_motion_norm()
    ok = ([IDENT[0]], [IDENT[1]])
    top = I32_MAX - 2 * Q
    bad = [dict(candidates=ok, radius=-1), dict(candidates=ok, radius=9), dict(candidates=ok, radius=2, keep=-1), dict(candidates=ok, radius=2, keep=257),
           dict(candidates=ok, radius=2, ball_max_age=-1), dict(candidates=ok, radius=2, ball_max_age=256),
           dict(candidates=ok, radius=2, min_inside=0), dict(candidates=ok, radius=2, min_inside=-1), dict(candidates=ok, radius=2, min_inside=W * H + 1),
           dict(candidates=([IDENT[0]] * 17, [IDENT[1]] * 17), radius=2),
           dict(candidates=([IDENT[0], (Q, 0, top + 1, 0, Q, 0)], [IDENT[1]] * 2), radius=2),
           dict(candidates=([IDENT[0], (Q, 0, 0, 0, Q, -top - 1)], [IDENT[1]] * 2), radius=2),
           dict(candidates=([IDENT[0]] * 2, [IDENT[1], (Q, Q, top + 1 - 2 * Q, 0, Q, 0)]), radius=2),
           dict(candidates=([IDENT[0]] * 2, [IDENT[1], (Q, 0, 0, -Q, 2 * Q, -(top + 1 - 4 * Q))]), radius=2)]
    for kw in bad:
        with pytest.raises(ya.YhError) as e:
            sc.append_memory_search_norm(d1, cls_id=c1, **kw)
        assert e.value.code == ya.capi.EINVAL, kw
    # the same offsets one step inside the conditions, and min_inside on both of its ends, are taken (on another handle)
    edge = ya.Scene(W, H)
    edge.append_memory_search_norm(d1, cls_id=c1, candidates=([IDENT[0], (Q, 0, top, 0, Q, -top)], [IDENT[1], (Q, Q, top - 2 * Q, -Q, 2 * Q, -(top - 4 * Q))]), radius=2, min_inside=1)
    assert tuple(edge.read_motion()["chosen"].tolist()) == (0, 0, 0)
    edge.append_memory_search_norm(d1, cls_id=c1, candidates=ok, radius=2, min_inside=W * H)
    assert tuple(edge.read_motion()["chosen"].tolist()) == (0, 0, 0) and edge.read_motion_norm()["qualified"]
    edge.close()
    frame, g = ya.SceneBatch.pack(c1), np.array(R.IDENTITY, np.int32)
    full = [sc.h, _p(d1), _p(frame), 0, 1, _p(g), _p(g), 2, 100, 224, 30]
    for hole in (0, 1, 2, 5, 6):
        args = list(full)
        args[hole] = None
        assert sc.L.yh_scene_append_memory_search_norm(*args) == ya.capi.EINVAL, hole
    assert sc.L.yh_scene_append_memory_search_norm(*(full[:4] + [0] + full[5:])) == ya.capi.EINVAL
    N = np.ones((H, W), np.uint32)
    for args in ((None, _p(N), 1, _p(g), 1, 1), (_p(N), None, 1, _p(g), 1, 1), (_p(N), _p(N), 1, None, 1, 1), (_p(N), _p(N), 0, _p(g), 1, 1), (_p(N), _p(N), 17, _p(g), 1, 1),
                 (_p(N), _p(N), 1, _p(g), 9, 1), (_p(N), _p(N), 1, _p(g), 1, 0), (_p(N), _p(N), 1, _p(g), 1, W * H + 1),
                 (_p(N), _p(N), 1, _p(np.array((Q, 0, I32_MAX - Q + 1, 0, Q, 0), np.int32)), 1, 1)):
        assert sc.L.yh_scene_op_register_norm(sc.h, args[0], args[1], args[2], args[3], args[4], args[5], None, None, None, None, None, None) == ya.capi.EINVAL, args[2:]
    got = sc.op_register_norm(N, N, [R.IDENTITY], 1, W * H)                                           # the hook itself commits nothing either
    assert (got["chosen"], got["qualified"], got["sum_n"]) == ((0, 0, 0), True, H * W)
    _same(sc.read(), before, ("refused",))
    after, again, still, ext2 = sc.read_memory(), sc.read_plan(), sc.read_motion(scores=True), sc.read_motion_norm()
    assert np.array_equal(after["map"], mem["map"]) and np.array_equal(after["balls"], mem["balls"])
    assert all(np.array_equal(again[k], plan[k]) for k in plan) and all(np.array_equal(still[k], motion[k]) for k in motion)
    assert all(np.array_equal(ext2[k], ext[k]) for k in ext)
    sc.close()


@pytest.mark.gpu
def test_frame_from_a_device_pointer_and_from_the_host(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    host, dev, ref = ya.Scene(W, H), ya.Scene(W, H), GN.Memory(W, H)
    gs, cs = [shift(2, 1)[0], IDENT[0]], [shift(2, 1)[1], IDENT[1]]
    for t in range(2):
        depth, ci, o = _stamps(oracle, H, W, 20 + t)
        frame = ya.SceneBatch.pack(ci)
        on_dev = _DeviceFrame(frame)
        host.append_memory_search_norm(depth, frame_u32=frame, candidates=(gs, cs), radius=2)
        dev.append_memory_search_norm(depth, frame_dev_ptr=on_dev.ptr.value, candidates=(gs, cs), radius=2)
        want = ref.append_search_norm(o["map"], o["balls"], gs, cs, 2, (W * H) // 4)
        for name, s in (("host", host), ("device", dev)):
            _same(s.read(), want, (name, t))
            _same_motion(s, ref.motion, (name, t))
            _same_memory(s, ref, (name, t))
        assert dev.memory_search_norm_time(2)[0] > 0                                                  # the replay reads the device frame again: still valid
        _same(dev.read(), want, ("device, replayed", t))
        on_dev.free()
    host.close(); dev.close()


@pytest.mark.gpu
def test_the_normalised_registration_costs_what_its_sums_cost(built):
    """At 640 x 480, on the terrain-only and the robots + balls frame of tools/time_scene.py, in this process: the normalised
    registration alone (yh_scene_memory_search_norm_time's second figure) against the plain registration alone
    (yh_scene_memory_search_time's) at (n_rot, R) = (5, 4) with the same candidates, alternated, one warm-up each, the median of
    five runs of 30 replays.
    Ceiling 1.996, each term read from profiles/scene_register_norm_timings.txt (2026-10-20, the two runs at its head): the largest
    ratio of its four (5, 4) rows, 1.921, plus the largest spread of the plain registration in any row of those runs, 4.5 %,
    plus the 3 % by which the pool's boxes differ. The other grids are recorded there and in DESIGN.md, not bounded here."""
    import yolact_amd as ya
    H, W = 480, 640
    depth = np.random.default_rng(0).integers(200, 4000, (H, W)).astype(np.uint16)
    srch, norm = ya.Scene(W, H), ya.Scene(W, H)
    prior = (3.0, -2.0, 0.05)
    motion = ya.scene_motion(*prior)
    cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=2)
    for name, robots in (("terrain only", False), ("robots + balls", True)):
        ci = np.zeros((H, W, 2), np.uint8)
        if robots:
            ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
        for sc in (srch, norm):
            sc.memory_reset()
            sc.append_memory(depth, cls_id=ci, motion=motion)
        srch.append_memory_search(depth, cls_id=ci, candidates=cands, radius=4)
        norm.append_memory_search_norm(depth, cls_id=ci, candidates=cands, radius=4)
        srch.memory_search_time(30); norm.memory_search_norm_time(30)
        tr, tq = [], []
        for _ in range(5):
            tr.append(srch.memory_search_time(30)[1]); tq.append(norm.memory_search_norm_time(30)[1])
        ratio = float(np.median(tq) / np.median(tr))
        print(f"scene 640x480, {name}: plain registration {np.median(tr):.4f} ms, normalised {np.median(tq):.4f} ms, ratio {ratio:.3f}")
        assert ratio <= 1.996, (name, tr, tq)
    srch.close(); norm.close()
