"""The scene memory's pyramid registration (DESIGN.md §11 "Scene memory: pyramid registration"): yh_scene_append_memory_pyramid
searches the candidates of yh_scene_append_memory_search coarse to fine over max-pooled levels of the frame's stamps and the memory.
CPU part: the numpy restatement (tests/scene_pyramid_ref.py) against answers worked out by hand - the pooling, the level gathers,
the tie rules, the home hypothesis, the int32 conditions -, its floor against the plain search, recovery of motions the plain search
cannot reach; the binding's surface. GPU part (-m gpu): the levels, every level's centres and tables, the choice and every output of
the library against the restatement, bit for bit."""
import inspect
import os
import re

import numpy as np
import pytest

import scene_memory_ref as R
import scene_pyramid_ref as P
import scene_register_ref as G
from test_scene_memory import IDENT, shift, turn90, _stamps, _same, _same_memory, _DeviceFrame
from test_scene_register import ROTATION, SHEARED, _maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
Q = 65536
# a gather that level 0 takes (on its condition) and level 1 refuses, at levels 1, radius 8, refine 0
COARSE_ALONE = (I32_MIN, I32_MIN, -(I32_MAX - 16 * Q), Q, 0, 0)
# (d, the first level that refuses (I32_MIN, I32_MIN, -(I32_MAX - 64 * Q) + d, ..) at levels 3, radius 8, refine 0): both sides of
# each level's condition
COARSE_LEVELS = ((0, 1), (32768, 1), (32769, 2), (98306, 2), (98307, 3), (229382, 3), (229383, None))


def _first_refusing_level(g, levels, radius, refine):
    """the lowest level at which gather g misses its int32 condition, or None"""
    T = P.reach(levels, radius, refine)
    for lv in range(levels + 1):
        q = P.level_gather(g, lv)
        if abs(q[2]) + T[lv] * Q > I32_MAX or abs(q[5]) + T[lv] * Q > I32_MAX:
            return lv
    return None


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------------

def test_pooling_by_hand():
    a = np.array([[1, 9, 2], [3, 4, 8], [7, 0, 5]], np.uint32)
    assert P.pool(a).tolist() == [[9, 8], [7, 5]] and P.pool(P.pool(a)).tolist() == [[9]]
    b = np.array([[1, 2, 3, 4, 0xFFFFFFFF], [6, 5, 0, 0, 7]], np.uint32)                       # 5 x 2: the last column stands alone
    assert P.pool(b).tolist() == [[6, 4, 0xFFFFFFFF]] and P.pool(b).dtype == np.uint32
    assert P.pool(np.array([[5]], np.uint32)).tolist() == [[5]]
    lv = P.levels_of(a, 3)
    assert [t.shape for t in lv] == [(3, 3), (2, 2), (1, 1), (1, 1)] and lv[3].tolist() == [[9]]
    big = np.arange(37 * 53, dtype=np.uint32).reshape(37, 53)
    assert [t.shape for t in P.levels_of(big, 3)] == [(37, 53), (19, 27), (10, 14), (5, 7)]
    assert P.levels_of(big, 3)[3][4, 6] == big.max() and P.levels_of(big, 2)[2][0, 0] == big[3, 3]


def test_level_gathers_by_hand():
    assert all(P.level_gather(R.IDENTITY, lv) == R.IDENTITY for lv in range(4))
    # a shift halves, floored: sources (3, -2) pixels away are (1.5, -1) coarse pixels away at level 1: 2 c / 4
    g = shift(-3, 2)[0]
    assert g == (Q, 0, 3 * Q, 0, Q, -2 * Q)
    assert P.level_gather(g, 0) == g and P.level_gather(g, 1) == (Q, 0, 3 * Q // 2, 0, Q, -Q) and P.level_gather(g, 2) == (Q, 0, 3 * Q // 4, 0, Q, -Q // 2)
    assert P.level_gather((Q, 0, -1, 0, Q, -3), 1) == (Q, 0, -1, 0, Q, -2)                     # floor, not truncation: -2 / 4, -6 / 4
    # the quarter turn x' = px + py - y, y' = py - px + x: a + b - 65536 = -2 * 65536 in the first row, 0 in the second. At level 1
    # c_1 = (-2 + 2 (px + py)) / 4 pixels, f_1 = 2 (py - px) / 4; at level 3 c_3 = (-2 * 7 + 2 (px + py)) / 16
    px, py = 20, 30
    t = turn90(px, py)[1]
    assert t == (0, -Q, (px + py) * Q, Q, 0, (py - px) * Q)
    assert P.level_gather(t, 1) == (0, -Q, 49 * Q // 2, Q, 0, 5 * Q) and P.level_gather(t, 3) == (0, -Q, 86 * Q // 16, Q, 0, 20 * Q // 16)
    # what the formula is for: the centre of coarse cell (X, Y), x = s X + (s - 1) / 2 with s = 2^l, goes under the base to
    # (a x + b y + c) / 65536, which in coarse units is that minus (s - 1) / 2, over s. Doubled and times s it is an integer, and the
    # level gather on (X, Y) is its floor
    for g in (t, turn90(px, py)[0], shift(-3, 2)[0], ROTATION[0], SHEARED[1]):
        for lv in (1, 2, 3):
            s = 1 << lv
            for row in (0, 3):
                a, b, c = P.level_gather(g, lv)[row:row + 3]
                for X, Y in ((0, 0), (5, 3), (17, 40)):
                    exact = g[row] * (2 * s * X + s - 1) + g[row + 1] * (2 * s * Y + s - 1) + 2 * g[row + 2] - Q * (s - 1)
                    assert 0 <= exact - 2 * s * (a * X + b * Y + c) < 2 * s, (g, lv, X, Y)


def test_reach_and_int32_conditions_from_both_sides():
    assert P.reach(3, 8, 1) == [71, 35, 17, 8] and P.reach(1, 0, 0) == [0, 0] and P.reach(3, 8, 8) == [120, 56, 24, 8] and P.reach(2, 2, 1) == [11, 5, 2]
    for levels, radius, refine in ((1, 8, 1), (3, 8, 1), (3, 8, 8), (2, 0, 3)):
        T = P.reach(levels, radius, refine)
        # a pure shift: c_l = floor(c / 2^l), and level 0 is the tight one
        top0 = I32_MAX - T[0] * Q
        for s in (1, -1):
            assert P.bases_ok([(Q, 0, s * top0, 0, Q, -s * top0)], None, levels, radius, refine)
            assert not P.bases_ok([(Q, 0, s * (top0 + 1), 0, Q, 0)], None, levels, radius, refine)
            assert not P.bases_ok([R.IDENTITY, (Q, 0, 0, 0, Q, s * (top0 + 1))], None, levels, radius, refine)
        # the carry's offsets move by A u + B v with |u|, |v| <= T_0
        A, B = 3 * Q, -2 * Q
        topc = I32_MAX - T[0] * (abs(A) + abs(B))
        for s in (1, -1):
            assert P.bases_ok([R.IDENTITY], [(A, B, s * topc, B, A, -s * topc)], levels, radius, refine)
            if T[0]:
                assert not P.bases_ok([R.IDENTITY], [(A, B, s * (topc + 1), B, A, 0)], levels, radius, refine)
                assert not P.bases_ok([R.IDENTITY] * 2, [R.IDENTITY, (A, B, 0, B, A, s * (topc + 1))], levels, radius, refine)
    # a coarse level alone refuses only where refine = 0 and a + b is as negative as it gets: |c_l| + T_l 65536 is then at most
    # 2^31 + 65536 (s - 1) (1 - 2 refine) / (2 s), s = 2^l. Levels 1, radius 8, refine 0: |c_0| + 16 * 65536 = INT32_MAX exactly,
    # c_1 = floor((-2^32 - 65536 - 2 (INT32_MAX - 16 * 65536)) / 4) = -2^31 + 507904, and 507904 < 8 * 65536
    g = COARSE_ALONE
    assert abs(P.level_gather(g, 0)[2]) + 16 * Q == I32_MAX and P.level_gather(g, 1)[2] == I32_MIN + 507904 and not P.bases_ok([g], None, 1, 8, 0)
    assert P.bases_ok([g], None, 1, 7, 0) and P.bases_ok([g], None, 1, 8, 1) is False       # (refine 1: level 0 refuses, T_0 = 17)
    inside = g[:2] + (g[2] + 32770,) + g[3:]                                                  # c_1 moves by half of it: 16385 back inside
    assert P.level_gather(inside, 1)[2] == I32_MIN + 507904 + 16385 and P.bases_ok([inside], None, 1, 8, 0)
    assert not P.bases_ok([g[:2] + (g[2] + 32768,) + g[3:]], None, 1, 8, 0)
    # each coarse level alone, at levels 3, radius 8, refine 0 (T = 64, 32, 16, 8): the excess of level l over INT32_MAX is about
    # 65536 (s - 1) / (2 s) - d / s for an offset d inside level 0's condition, s = 2^l: 16384 - d / 2, 24576 - d / 4, 28672 - d / 8
    for d, level in COARSE_LEVELS:
        g = (I32_MIN, I32_MIN, -(I32_MAX - 64 * Q) + d, Q, 0, 0)
        assert _first_refusing_level(g, 3, 8, 0) == level and P.bases_ok([g], None, 3, 8, 0) == (level is None), (d, level)
        assert _first_refusing_level(g[3:] + g[:3], 3, 8, 0) == level                          # the second row's f_l likewise


def _tables(n_hyp, p, entries, fill=0):
    S = np.full((n_hyp, 2 * p + 1, 2 * p + 1), fill, np.uint64)
    for (h, i, j), s in entries.items():
        S[h, j + p, i + p] = s
    return S


def test_every_tie_break_level():
    # within a level, one hypothesis around centre (cx, cy): the total shift counts
    S = _tables(1, 1, {(0, 1, 1): 6, (0, -1, -1): 5})[0]
    assert P.level_best(S, (0, 0)) == (1, 1) and P.level_best(S, (4, -2)) == (5, -1)          # the larger S
    S = _tables(1, 1, {(0, 1, 0): 6, (0, -1, 0): 6})[0]
    assert P.level_best(S, (0, 0)) == (-1, 0)                                                  # a tie at equal distance: the smaller U
    assert P.level_best(S, (2, 0)) == (1, 0) and P.level_best(S, (-2, 0)) == (-1, 0)          # the smaller U^2 + V^2 of the TOTAL shift
    S = _tables(1, 1, {(0, 0, 1): 6, (0, 1, 0): 6, (0, 0, -1): 6})[0]
    assert P.level_best(S, (0, 0)) == (0, -1)                                                  # then the smaller V
    assert P.level_best(_tables(1, 2, {}, fill=3)[0], (0, 0)) == (0, 0) and P.level_best(_tables(1, 2, {}, fill=3)[0], (3, 1)) == (1, 0)
    # the choice over all level-0 entries: hypothesis 2 of n_rot = 2 is the home one and counts as k = 0
    cen = [(4, 0), (0, 2), (0, 0)]
    assert P.choose(_tables(3, 1, {(0, 1, 1): 9, (2, 0, 0): 8}), cen, 2)[:3] == (0, 5, 1)       # the larger S, however far
    assert P.choose(_tables(3, 1, {(0, -1, 0): 9, (1, 0, -1): 9}), cen, 2)[:3] == (1, 0, 1)     # then the smaller u^2 + v^2, whatever k
    assert P.choose(_tables(3, 1, {(1, 1, -1): 9, (2, 1, 1): 9}), cen, 2)[:3] == (0, 1, 1)      # then the smaller k: home is 0
    assert P.choose(_tables(3, 1, {(1, 1, -1): 9, (1, -1, -1): 9}), cen, 2)[:3] == (1, -1, 1)   # then the smaller u
    assert P.choose(_tables(3, 1, {(2, 0, 1): 9, (2, 1, 0): 9, (2, 0, -1): 9}), cen, 2)[:3] == (0, 0, -1)   # the smaller v before the smaller u
    assert P.choose(_tables(3, 1, {}, fill=4), cen, 2) == (0, 0, 0, 4)
    # a duplicated candidate - the same (k, u, v) reached by base 0's descent and by the home hypothesis - carries the same S
    assert P.choose(_tables(2, 1, {(0, -1, 0): 7, (1, 0, 0): 7}), [(1, 0), (0, 0)], 1) == (0, 0, 0, 7)


def test_the_home_hypothesis_wins_where_the_descent_ends_elsewhere():
    """16 x 16, L = 2, R = 1, r = 0. N and M share one strong pixel, (6, 6): the prior (no shift) scores 900. A field of
    single pixels around it is pooled into coarse cells that all fill at level 2, where shifting by one coarse cell (four pixels)
    matches more of them, so the descent of base 0 goes to (4, 0) - where at full size almost nothing meets."""
    N, M = np.zeros((16, 16), np.uint32), np.zeros((16, 16), np.uint32)
    N[6, 6] = M[6, 6] = 900
    for Y in range(4):                                                                        # level 2 sees N full in columns 0 .. 2, M in columns 1 .. 3
        for X in range(3):
            N[4 * Y + 1, 4 * X + 1] = max(N[4 * Y + 1, 4 * X + 1], 1000)
            M[4 * Y + 2, 4 * (X + 1) + 3] = max(M[4 * Y + 2, 4 * (X + 1) + 3], 1000)
    out = P.search(N, M, [R.IDENTITY], [R.IDENTITY], 2, 1, 0)
    assert [tuple(c) for c in out["centres"][1].tolist()] == [(2, 0)] and [tuple(c) for c in out["centres"][0].tolist()] == [(4, 0), (0, 0)]
    assert out["tables"][2][0, 1, 2] > out["tables"][2][0, 1, 1]                               # level 2 prefers one cell to the right
    assert int(out["tables"][0][0, 0, 0]) == 0 and int(out["tables"][0][1, 0, 0]) == 900       # the descended base ends on nothing, home on the pixel
    assert out["chosen"] == (0, 0, 0) and out["score"][:2] == (900, 900) and out["gather"] == R.IDENTITY
    assert G.search(N, M, [R.IDENTITY], [R.IDENTITY], 0)["score"][0] == 900


def test_empty_maps_choose_the_prior():
    rng = np.random.default_rng(5)
    H, W = 19, 23
    full = rng.integers(1, 500, (H, W)).astype(np.uint32)
    zero = np.zeros((H, W), np.uint32)
    bases = [shift(1, 0)[0], R.IDENTITY, ROTATION[0]]
    for N, M in ((full, zero), (zero, full), (zero, zero)):
        for levels, radius, refine in ((1, 2, 1), (3, 8, 1), (2, 0, 0)):
            out = P.search(N, M, bases, None, levels, radius, refine)
            assert out["chosen"] == (0, 0, 0) and out["gather"] == tuple(bases[0]) and out["score"][:2] == (0, 0)
            assert out["score"][2] == int(N.astype(np.uint64).sum())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_chosen_score_is_the_plain_one_and_never_below_base_0_at_radius_r(seed):
    H, W = 23 + seed, 41 - seed
    N, M = _maps(H, W, 50 + seed)
    bases = [shift(1, -1)[0], R.IDENTITY, ROTATION[0], turn90(20, 15)[0]][:1 + seed]
    for levels, radius, refine in ((1, 1, 1), (2, 2, 1), (3, 8, 1), (3, 2, 2), (2, 3, 0)):
        out = P.search(N, M, bases, None, levels, radius, refine)
        k, u, v = out["chosen"]
        one, _ = G.scores(N, M, [G.candidate(bases[k], None, u, v)[0]], 0)                    # S(k, u, v) of the plain definition
        assert int(one[0, 0, 0]) == out["score"][0]
        floor, _ = G.scores(N, M, bases[:1], refine)
        assert out["score"][0] >= int(floor.max()) >= out["score"][1] == int(floor[0, refine, refine])
        assert max(abs(u), abs(v)) <= P.reach(levels, radius, refine)[0]
        assert out["score"][0] == int(out["tables"][0].max())


def _bumps(H, W, seed):
    """a sparse synthetic map: Gaussian bumps on a zero background, one per 700 pixels"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    M = np.zeros((H, W))
    for _ in range(max(6, H * W // 700)):
        cx, cy, s, a = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(1.5, 4.0), rng.uniform(500, 5000)
        M = np.maximum(M, a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s)))
    M[M < 20] = 0
    return M.astype(np.uint32)


# name: H, W, levels, the true candidate (k, u, v), the step of the five bases' turns (None: the identity alone). Shifts of at most a
# quarter of the smaller side. Seeds 1 .. 6 were tried for each case on the restatement; all six pass all three assertions; 1 is used.
_CASES = {"L1": (65, 130, 1, (0, 13, -11), None), "L2": (65, 130, 2, (0, 16, -13), None), "L3": (120, 160, 3, (0, 29, -22), None),
          "turn": (120, 160, 3, (3, 29, -22), 0.02)}                                         # row 3 of five: the prior turned by 0.04 rad
_RECOVERY = {}


def _recovery(name):
    """(N, M, gathers, carries, levels, the true candidate, the restatement's result, the plain search's at R = 8): N[p] =
    M[gather_true(p)] of a sparse M, the candidates built around the prior "it did not move". Computed once."""
    if name not in _RECOVERY:
        from yolact_amd import scene_motion_candidates
        H, W, levels, true, step = _CASES[name]
        M = _bumps(H, W, 1)
        gs, cs = ([list(R.IDENTITY)], [list(R.IDENTITY)]) if step is None else scene_motion_candidates(prior=(0.0, 0.0, 0.0), dtheta_step=step, n_side=2, size=(W, H))
        N = R.carry_map(M, G.candidate(gs[true[0]], cs[true[0]], true[1], true[2])[0], 256)
        _RECOVERY[name] = (N, M, gs, cs, levels, true, P.search(N, M, gs, cs, levels, 8, 1), G.search(N, M, gs, cs, 8))
    return _RECOVERY[name]


def _entries_at_the_top(out, n_rot):
    """the candidates (k, u, v) that hold the largest level-0 entry"""
    S, cen = out["tables"][0], out["centres"][0]
    p = (S.shape[1] - 1) // 2
    return {(0 if h == n_rot else h, int(cen[h][0]) + i - p, int(cen[h][1]) + j - p) for h, j, i in np.argwhere(S == S.max()).tolist()}


@pytest.mark.parametrize("name", list(_CASES))
def test_recovery_of_a_motion_the_plain_search_cannot_reach(name):
    N, M, gs, cs, levels, true, out, plain = _recovery(name)
    assert max(abs(true[1]), abs(true[2])) > 8 and 4 * max(abs(true[1]), abs(true[2])) <= min(N.shape) + 3
    assert plain["chosen"] != true and plain["score"][0] < plain["score"][2]                  # the plain search at R = 8 chooses something else
    assert out["chosen"] == true and out["score"][0] == out["score"][2] > out["score"][1]      # the pyramid chooses the truth: every stamp explained
    assert _entries_at_the_top(out, len(gs)) == {true}                                        # and strictly: no other candidate ties with it
    assert out["gather"] == G.candidate(gs[true[0]], cs[true[0]], true[1], true[2])[0]


def test_surface_and_abi(built):
    import yolact_amd as ya
    from yolact_amd import capi
    L = capi.load_library()
    pub = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read()
    protos = dict((s[0], s) for s in capi.SYMBOLS)
    _i, _vp, _fp = capi.C.c_int32, capi.C.c_void_p, capi.C.POINTER(capi.C.c_float)
    assert protos["yh_scene_append_memory_pyramid"][1:] == (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i])
    assert protos["yh_scene_pyramid_read"][1:] == (_i, [_vp, _i, _vp, _vp, _vp])
    assert protos["yh_scene_memory_pyramid_time"][1:] == (_i, [_vp, _i, _fp, _fp])
    assert protos["yh_scene_op_pyramid"][1:] == (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp])
    pub_code, dbg_code = (re.sub(r"/\*.*?\*/", "", t, flags=re.S) for t in (pub, dbg))
    for name in ("yh_scene_append_memory_pyramid", "yh_scene_pyramid_read"):
        assert hasattr(L, name) and re.search(r"\bint %s\(yh_scene\* h" % name, pub_code) and name not in dbg_code, name
    for name in ("yh_scene_op_pyramid", "yh_scene_memory_pyramid_time"):
        assert hasattr(L, name) and re.search(r"\bint %s\(yh_scene\* h" % name, dbg_code) and name not in pub_code, name
    assert re.search(r"int yh_scene_append_memory_pyramid\(yh_scene\* h, const uint16_t\* depth_host, const uint32_t\* frame, int32_t frame_on_device, int32_t n_rot,\s*"
                     r"const int32_t\* gather_q16 , const int32_t\* carry_q16 , int32_t levels,\s*int32_t radius, int32_t refine, int32_t keep, int32_t ball_max_age\);", pub_code)
    assert re.search(r"int yh_scene_pyramid_read\(yh_scene\* h, int32_t level, int32_t\* centres , uint64_t\* scores , uint64_t\* sum_n\);", pub_code)
    # after yh_scene_motion_read, before the scene batch, under its comment line
    a, b, c = pub.index("int yh_scene_motion_read("), pub.index("int yh_scene_append_memory_pyramid("), pub.index("/* ---- scene batch")
    assert a < pub.index("Scene memory: pyramid registration") < b < pub.index("int yh_scene_pyramid_read(") < c
    sig = inspect.signature(capi.Scene.append_memory_pyramid)
    assert list(sig.parameters) == ["self", "depth", "frame_u32", "frame_dev_ptr", "cls_id", "candidates", "levels", "radius", "refine", "keep", "ball_max_age"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, None, None, None, 3, 8, 1, 224, 30]
    assert list(inspect.signature(capi.Scene.read_pyramid).parameters) == ["self", "level"]
    assert list(inspect.signature(capi.Scene.op_pyramid).parameters) == ["self", "n", "m", "gathers", "levels", "radius", "refine"]
    assert inspect.signature(capi.Scene.memory_pyramid_time).parameters["reps"].default == 20
    assert ya.Scene is capi.Scene
    cfg = capi.Config()
    L.yh_default_config(cfg)
    assert cfg.abi_version == 4 and "#define YH_ABI_VERSION 4" in pub


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def _bases(H, W):
    """fifteen gathers: every kind the definition allows, the first ones the plainest"""
    px, py = (W * 5) // 8, H - 1
    top = I32_MAX - 120 * Q                                                                    # on the level-0 condition at the widest reach
    return [R.IDENTITY, shift(3, -2)[0], ROTATION[0],
            turn90(px, py)[0], SHEARED[1], (Q, 0, 2 * W * Q, 0, Q, 0),                        # a quarter turn, a magnifying shear, every pixel outside
            SHEARED[0], (Q, 0, top, 0, Q, -top), (Q, 0, -top, 0, Q, top), (4 * Q, 0, 0, 0, 4 * Q, 0),
            shift(-W // 2, H // 2)[0], turn90(px // 2, py // 2)[0], (Q, Q // 8, -Q, -Q // 8, Q, 3 * Q), shift(1, 0)[0], shift(-5, 7)[0]]


def _check_op(sc, N, M, gathers, levels, radius, refine, what):
    want = P.search(N, M, gathers, None, levels, radius, refine)
    got = sc.op_pyramid(N, M, gathers, levels, radius, refine)
    for name in ("pyr_n", "pyr_m"):
        assert len(got[name]) == levels
        for lv in range(levels):
            assert got[name][lv].dtype == np.uint32 and np.array_equal(got[name][lv], want[name][lv]), (what, name, lv + 1)
    for lv in range(levels, -1, -1):
        assert np.array_equal(got["centres"][lv], want["centres"][lv]), (what, "centres", lv, got["centres"][lv].tolist(), want["centres"][lv].tolist())
        assert got["scores"][lv].dtype == np.uint64 and np.array_equal(got["scores"][lv], want["tables"][lv]), (what, "tables", lv, np.argwhere(got["scores"][lv] != want["tables"][lv])[:5].tolist())
    assert got["chosen"] == want["chosen"] and tuple(int(v) for v in got["score"]) == want["score"], (what, got["chosen"], want["chosen"], got["score"], want["score"])
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("levels,radius,refine,n_rot,first", [(1, 0, 0, 1, 0), (2, 2, 1, 3, 0), (3, 8, 1, 5, 1), (3, 8, 8, 15, 0)])
@pytest.mark.parametrize("H,W", [(3, 3), (8, 8), (37, 53), (100, 9), (65, 130)])
def test_op_pyramid_matches_the_restatement(built, H, W, levels, radius, refine, n_rot, first):
    import yolact_amd as ya
    N, M = _maps(H, W, 100 * H + W)
    gathers = _bases(H, W)[first:first + n_rot]                                               # (3, 8, 1, 5): shift, rotation, quarter turn, shear, all outside
    assert P.bases_ok(gathers, None, levels, radius, refine)
    sc = ya.Scene(W, H)
    want = _check_op(sc, N, M, gathers, levels, radius, refine, (H, W, levels, radius, refine, n_rot))
    assert want["score"][2] > 0 and want["tables"][0].max() > 0
    sc.close()


@pytest.mark.gpu
def test_op_pyramid_full_range_values_and_coefficients_on_the_conditions(built):
    import yolact_amd as ya
    H, W = 65, 130
    N, M = _maps(H, W, 7, top=1 << 32)
    N[20:40, 70:120] = 0xFFFFFFFF; M[18:44, 66:124] = 0xFFFFFFFF                             # a thousand pixels of 2^32 - 1 that meet under small shifts
    sc = ya.Scene(W, H)
    want = _check_op(sc, N, M, [R.IDENTITY, shift(3, -2)[0], SHEARED[1]], 3, 3, 2, "full range")
    assert want["tables"][0].max() > 1 << 41 and want["score"][2] > 1 << 42 and want["pyr_n"][2].max() == 0xFFFFFFFF
    # offsets exactly on the int32 conditions, at level 0 and - through a + b - at the top level
    for levels, radius, refine in ((1, 8, 1), (3, 8, 1), (2, 2, 8)):
        T = P.reach(levels, radius, refine)
        top = I32_MAX - T[0] * Q
        edge = [R.IDENTITY, (Q, 0, top, 0, Q, -top), (Q, 0, -top, 0, Q, top), (I32_MAX, I32_MAX, 0, I32_MIN, I32_MIN, 0)]
        assert P.bases_ok(edge, None, levels, radius, refine)
        _check_op(sc, N, M, edge, levels, radius, refine, ("edge", levels))
        for bad in ((Q, 0, top + 1, 0, Q, 0), (Q, 0, 0, 0, Q, -top - 1)):
            with pytest.raises(ya.YhError) as e:
                sc.op_pyramid(N, M, [R.IDENTITY, bad], levels, radius, refine)
            assert e.value.code == ya.capi.EINVAL and "base 1" in str(e.value), bad
    # the one kind of gather a coarse level alone refuses, and the same 32770 further in, which every level takes
    inside = COARSE_ALONE[:2] + (COARSE_ALONE[2] + 32770,) + COARSE_ALONE[3:]
    _check_op(sc, N, M, [R.IDENTITY, inside], 1, 8, 0, "coarse edge")
    with pytest.raises(ya.YhError) as e:
        sc.op_pyramid(N, M, [R.IDENTITY, COARSE_ALONE], 1, 8, 0)
    assert e.value.code == ya.capi.EINVAL and "base 1" in str(e.value) and "level 1" in str(e.value)
    for d, level in COARSE_LEVELS:                                                            # each coarse level alone, from both sides
        g = (I32_MIN, I32_MIN, -(I32_MAX - 64 * Q) + d, Q, 0, 0)
        if level is None:
            _check_op(sc, N, M, [R.IDENTITY, g], 3, 8, 0, ("coarse edge", d))
            continue
        with pytest.raises(ya.YhError) as e:
            sc.op_pyramid(N, M, [R.IDENTITY, g], 3, 8, 0)
        assert e.value.code == ya.capi.EINVAL and "base 1" in str(e.value) and "level %d" % level in str(e.value), (d, level, str(e.value))
    sc.close()


@pytest.mark.gpu
def test_op_pyramid_at_the_camera_size(built):
    import yolact_amd as ya
    H, W = 480, 640
    N, M = _maps(H, W, 8)
    sc = ya.Scene(W, H)
    _check_op(sc, N, M, [ROTATION[0], R.IDENTITY, SHEARED[1]], 3, 2, 1, "640 x 480")
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_CASES))
def test_op_pyramid_recovers_what_the_plain_search_cannot(built, name):
    import yolact_amd as ya
    N, M, gs, cs, levels, true, out, plain = _recovery(name)
    sc = ya.Scene(N.shape[1], N.shape[0])
    want = _check_op(sc, N, M, gs, levels, 8, 1, name)
    assert want["chosen"] == true
    _, chosen, _ = sc.op_register(N, M, gs, 8)
    assert chosen == plain["chosen"] != true
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,levels,radius,refine", [(37, 53, 2, 1, 1), (65, 130, 3, 0, 1), (100, 9, 1, 4, 0)])
def test_the_chosen_score_is_op_registers(built, H, W, levels, radius, refine):
    import yolact_amd as ya
    N, M = _maps(H, W, 9 * H + W)
    gathers = [shift(1, -1)[0], R.IDENTITY, ROTATION[0]]
    sc = ya.Scene(W, H)
    got = sc.op_pyramid(N, M, gathers, levels, radius, refine)
    k, u, v = got["chosen"]
    assert max(abs(u), abs(v)) <= P.reach(levels, radius, refine)[0] <= 8                     # (the cases are chosen so: op_register reaches 8)
    scores, _, sum_n = sc.op_register(N, M, gathers, 8)
    assert int(scores[k, v + 8, u + 8]) == int(got["score"][0]) and sum_n == int(got["score"][2]) and int(scores[0, 8, 8]) == int(got["score"][1])
    floor, _, _ = sc.op_register(N, M, gathers[:1], refine)
    assert int(got["score"][0]) >= int(floor.max())
    sc.close()


def _same_motion(sc, want, levels, what):
    got = sc.read_motion()
    assert tuple(got["chosen"].tolist()) == want["chosen"] and tuple(got["gather"].tolist()) == want["gather"] and tuple(got["carry"].tolist()) == want["carry"], (what, got, want["chosen"])
    assert tuple(int(v) for v in got["score"]) == want["score"], what
    for lv in range(levels + 1):
        t = sc.read_pyramid(lv)
        assert np.array_equal(t["centres"], want["centres"][lv]) and np.array_equal(t["scores"], want["tables"][lv]) and t["sum_n"] == want["sum_n"][lv], (what, lv)
    return got


def _candidates():
    """per frame of a sequence: (gathers, carries), levels, radius, refine"""
    return [(([IDENT[0]], [IDENT[1]]), 1, 2, 1),
            (([shift(1, 0)[0], IDENT[0], ROTATION[0]], [shift(1, 0)[1], IDENT[1], ROTATION[1]]), 2, 2, 1),
            (([ROTATION[0], shift(-2, 1)[0]], [ROTATION[1], shift(-2, 1)[1]]), 3, 8, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (37, 53), (100, 9)])
def test_pyramid_sequences_match_the_restatement_and_append_memory(built, oracle, H, W):
    import yolact_amd as ya
    sc, mem, ref = ya.Scene(W, H), ya.Scene(W, H), P.Memory(W, H)
    for t, ((gs, cs), levels, radius, refine) in enumerate(_candidates()):
        depth, ci, o = _stamps(oracle, H, W, 10 * H + W + t, balls=t != 1)                    # the second frame has no ball: those of the first are remembered
        keep = (256, 224, 200)[t]
        sc.append_memory_pyramid(depth, cls_id=ci, candidates=(gs, cs), levels=levels, radius=radius, refine=refine, keep=keep, ball_max_age=5)
        want = ref.append_pyramid(o["map"], o["balls"], gs, cs, levels, radius, refine, keep, 5)
        got = _same_motion(sc, ref.motion, levels, (H, W, t))
        _same(sc.read(), want, ("pyramid", H, W, t))
        _same_memory(sc, ref, ("pyramid", H, W, t))
        # the same append on a second handle, handed the twelve integers read back
        mem.append_memory(depth, cls_id=ci, motion=(tuple(got["gather"].tolist()), tuple(got["carry"].tolist())), keep=keep, ball_max_age=5)
        _same(sc.read(), mem.read(), ("append_memory", H, W, t))
        a, b = sc.read_memory(), mem.read_memory()
        assert np.array_equal(a["map"], b["map"]) and np.array_equal(a["balls"], b["balls"])
    assert ref.motion["score"][2] > 0
    sc.close(); mem.close()


@pytest.mark.gpu
def test_a_wrong_prior_far_off_is_corrected(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    d, c, o = _stamps(oracle, H, W, 2)
    g, cr = shift(11, -9)                                                                     # the prior says the map moved far; it did not
    want = P.search(o["map"], o["map"], [g], [cr], 2, 3, 1)                                   # the memory after frame A alone IS its stamps
    assert want["chosen"] == (0, 11, -9) and want["gather"] == R.IDENTITY and want["carry"] == R.IDENTITY
    assert want["score"][0] == want["score"][2] > want["score"][1] and G.search(o["map"], o["map"], [g], [cr], 8)["chosen"] != (0, 11, -9)
    sc, twice = ya.Scene(W, H), ya.Scene(W, H)
    for s in (sc, twice):
        s.append_memory(d, cls_id=c, keep=256)
    sc.append_memory_pyramid(d, cls_id=c, candidates=([g], [cr]), levels=2, radius=3, refine=1, keep=256)
    twice.append_memory(d, cls_id=c, keep=256)
    _same_motion(sc, want, 2, "wrong prior")
    _same(sc.read(), twice.read(), ("wrong prior",))
    a, b = sc.read_memory(), twice.read_memory()
    assert np.array_equal(a["map"], b["map"]) and np.array_equal(a["balls"], b["balls"]) and np.array_equal(a["map"], o["map"])
    sc.close(); twice.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (37, 53)])
def test_an_empty_memory_is_a_plain_append(built, oracle, H, W):
    import yolact_amd as ya
    d0, c0, _ = _stamps(oracle, H, W, 1)
    pyr, plain = ya.Scene(W, H), ya.Scene(W, H)
    pyr.append_memory_pyramid(d0, cls_id=c0, candidates=([shift(1, 1)[0], ROTATION[0]], [shift(1, 1)[1], ROTATION[1]]), levels=3, radius=8, refine=1, keep=256, ball_max_age=255)
    plain.append_classified(d0, frame_u32=ya.SceneBatch.pack(c0), mode=ya.COMPAT_SANE)     # an empty memory: the prior, and nothing to carry
    _same(pyr.read(), plain.read(), ("empty", H, W))
    m = pyr.read_motion()
    assert tuple(m["chosen"].tolist()) == (0, 0, 0) and tuple(m["gather"].tolist()) == shift(1, 1)[0] and tuple(m["carry"].tolist()) == shift(1, 1)[1]
    assert m["score"][0] == m["score"][1] == 0 and m["score"][2] > 0 and plain.read()["map"].max() > 0
    pyr.close(); plain.close()


@pytest.mark.gpu
def test_a_remembered_ball_is_carried_by_the_chosen_carry(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    d, c, o = _stamps(oracle, H, W, 61)
    _, c_none, o_none = _stamps(oracle, H, W, 61, balls=False)                                # the same depth image, the balls not seen
    sc, ref = ya.Scene(W, H), P.Memory(W, H)
    sc.append_memory_pyramid(d, cls_id=c, levels=1, radius=0, refine=0)
    ref.append_pyramid(o["map"], o["balls"], [R.IDENTITY], [R.IDENTITY], 1, 0, 0)
    seen = ref.B.copy()
    g, cr = shift(10, 7)                                                                      # the prior says the map moved; it did not
    sc.append_memory_pyramid(d, cls_id=c_none, candidates=([g], [cr]), levels=2, radius=3, refine=1, keep=256, ball_max_age=5)
    want = ref.append_pyramid(o_none["map"], o_none["balls"], [g], [cr], 2, 3, 1, 256, 5)
    assert ref.motion["chosen"] == (0, 10, 7) and ref.motion["carry"] == R.IDENTITY
    _same_motion(sc, ref.motion, 2, "ball")
    _same(sc.read(), want, ("ball",))
    _same_memory(sc, ref, "ball")
    ids = np.flatnonzero(seen[:, 2] > 0)
    assert len(ids) == 2 and not o_none["balls"].any()
    mem = sc.read_memory()["balls"]
    for k in ids:                                                                             # where it was, not ten pixels right and seven down
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
    sc.append_memory_pyramid(d0, cls_id=c0, levels=1, radius=1, refine=1)
    sc.append_memory_pyramid(d1, cls_id=c1, candidates=([shift(2, -1)[0], IDENT[0]], [shift(2, -1)[1], IDENT[1]]), levels=2, radius=2, refine=1, keep=240)
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


def _levels_of(sc, levels):
    return [sc.read_pyramid(lv) for lv in range(levels + 1)]


def _same_levels(a, b):
    return all(np.array_equal(x[k], y[k]) if k != "sum_n" else x[k] == y[k] for x, y in zip(a, b) for k in x)


@pytest.mark.gpu
def test_pyramid_time_commits_nothing_and_the_other_hooks_name_it(built, oracle):
    import ctypes as C
    import yolact_amd as ya
    H, W = 37, 53
    d0, c0, _ = _stamps(oracle, H, W, 41)
    d1, c1, _ = _stamps(oracle, H, W, 42)
    sc = ya.Scene(W, H)
    with pytest.raises(ya.YhError) as e:                                                      # before any memory append
        sc.read_pyramid(0)
    assert e.value.code == ya.capi.ESTATE
    cands = ([shift(1, 0)[0], ROTATION[0]], [shift(1, 0)[1], ROTATION[1]])
    sc.append_memory_pyramid(d0, cls_id=c0, levels=1, radius=1, refine=1)
    sc.append_memory_pyramid(d1, cls_id=c1, candidates=cands, levels=3, radius=3, refine=1, keep=250)
    before, mem, motion, tables = sc.read(), sc.read_memory(), sc.read_motion(), _levels_of(sc, 3)
    ms, ms_search = sc.memory_pyramid_time(3)
    assert ms > 0 and 0 < ms_search < ms
    _same(sc.read(), before, ("pyramid time",))
    after, again = sc.read_memory(), sc.read_motion()
    assert np.array_equal(after["map"], mem["map"]) and np.array_equal(after["balls"], mem["balls"])
    assert all(np.array_equal(again[k], motion[k]) for k in motion) and _same_levels(_levels_of(sc, 3), tables)
    for call in (lambda: sc.time(2), lambda: sc.memory_time(2), lambda: sc.memory_search_time(2)):
        with pytest.raises(ya.YhError) as e:
            call()
        assert e.value.code == ya.capi.ESTATE and "yh_scene_memory_pyramid_time" in str(e.value)
    with pytest.raises(ya.YhError) as e:                                                      # the table's shape differs: the level tables have a call of their own
        sc.read_motion(scores=True)
    assert e.value.code == ya.capi.EINVAL and "yh_scene_pyramid_read" in str(e.value)
    for level in (-1, 4):
        with pytest.raises(ya.YhError) as e:
            sc.read_pyramid(level)
        assert e.value.code == ya.capi.EINVAL
    f = C.c_float()
    assert sc.L.yh_scene_memory_pyramid_time(sc.h, 0, C.byref(f), C.byref(f)) == ya.capi.EINVAL
    assert sc.L.yh_scene_memory_pyramid_time(sc.h, 1, None, C.byref(f)) == ya.capi.EINVAL and sc.L.yh_scene_memory_pyramid_time(sc.h, 1, C.byref(f), None) == ya.capi.EINVAL
    assert sc.L.yh_scene_pyramid_read(None, 0, None, None, None) == ya.capi.EINVAL and sc.L.yh_scene_pyramid_read(sc.h, 0, None, None, None) == ya.capi.OK
    # every other memory append ends the state: a search append, a plain memory append, a reset
    sc.append_memory_search(d1, cls_id=c1, candidates=cands, radius=2)
    assert sc.memory_search_time(2)[0] > 0 and sc.read_motion(scores=True)["scores"].shape == (2, 5, 5)
    for call in (lambda: sc.memory_pyramid_time(2), lambda: sc.read_pyramid(0)):
        with pytest.raises(ya.YhError) as e:
            call()
        assert e.value.code == ya.capi.ESTATE
    sc.append_memory_pyramid(d1, cls_id=c1, candidates=cands, levels=1, radius=1, refine=0)
    assert sc.read_pyramid(1)["scores"].shape == (2, 3, 3) and sc.read_pyramid(0)["scores"].shape == (3, 1, 1)
    sc.append_memory(d1, cls_id=c1)
    assert sc.memory_time(2) > 0
    for call in (lambda: sc.memory_pyramid_time(2), lambda: sc.read_pyramid(0), lambda: sc.read_motion()):
        with pytest.raises(ya.YhError) as e:
            call()
        assert e.value.code == ya.capi.ESTATE
    sc.append_memory_pyramid(d1, cls_id=c1, levels=1, radius=1, refine=0)
    sc.append(d1, c1, ya.COMPAT_SANE)                                                         # a plain append: the motion stays readable, nothing to replay
    assert sc.read_pyramid(0)["scores"].shape == (2, 1, 1) and sc.time(2) > 0
    with pytest.raises(ya.YhError) as e:
        sc.memory_pyramid_time(2)
    assert e.value.code == ya.capi.ESTATE
    sc.memory_reset()
    for call in (lambda: sc.read_pyramid(0), lambda: sc.read_motion()):
        with pytest.raises(ya.YhError) as e:
            call()
        assert e.value.code == ya.capi.ESTATE
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
    sc.append_memory_pyramid(d0, cls_id=c0, candidates=([shift(1, 0)[0]], [shift(1, 0)[1]]), levels=2, radius=2, refine=1)
    sc.plan(None, start=start)
    before, mem, plan, motion, tables = sc.read(), sc.read_memory(), sc.read_plan(), sc.read_motion(), _levels_of(sc, 2)
    ok = ([IDENT[0]], [IDENT[1]])
    lrr = dict(levels=2, radius=2, refine=1)
    T0 = P.reach(2, 2, 1)[0]
    top = I32_MAX - T0 * Q
    bad = [dict(candidates=ok, levels=0, radius=2, refine=1), dict(candidates=ok, levels=4, radius=2, refine=1), dict(candidates=ok, levels=2, radius=-1, refine=1),
           dict(candidates=ok, levels=2, radius=9, refine=1), dict(candidates=ok, levels=2, radius=2, refine=-1), dict(candidates=ok, levels=2, radius=2, refine=9),
           dict(candidates=ok, keep=-1, **lrr), dict(candidates=ok, keep=257, **lrr), dict(candidates=ok, ball_max_age=-1, **lrr), dict(candidates=ok, ball_max_age=256, **lrr),
           dict(candidates=([IDENT[0]] * 16, [IDENT[1]] * 16), **lrr)]
    named = [dict(candidates=([IDENT[0], (Q, 0, top + 1, 0, Q, 0)], [IDENT[1]] * 2), **lrr),
             dict(candidates=([IDENT[0], (Q, 0, 0, 0, Q, -top - 1)], [IDENT[1]] * 2), **lrr),
             dict(candidates=([IDENT[0], COARSE_ALONE], [IDENT[1]] * 2), levels=1, radius=8, refine=0),     # a coarse level alone refuses
             dict(candidates=([IDENT[0]] * 2, [IDENT[1], (Q, Q, I32_MAX - 2 * T0 * Q + 1, 0, Q, 0)]), **lrr),
             dict(candidates=([IDENT[0]] * 2, [IDENT[1], (Q, 0, 0, -Q, 2 * Q, -(I32_MAX - 3 * T0 * Q + 1))]), **lrr)]
    for kw in bad + named:
        assert kw in bad or not P.bases_ok(kw["candidates"][0], kw["candidates"][1], kw["levels"], kw["radius"], kw["refine"])
        with pytest.raises(ya.YhError) as e:
            sc.append_memory_pyramid(d1, cls_id=c1, **kw)
        assert e.value.code == ya.capi.EINVAL and (kw in bad or "base 1" in str(e.value)), kw
    # the same offsets one step inside the conditions are taken (on another handle: this one stays as it is)
    edge = ya.Scene(W, H)
    inside = ([IDENT[0], (Q, 0, top, 0, Q, -top)], [IDENT[1], (Q, Q, I32_MAX - 2 * T0 * Q, -Q, 2 * Q, -(I32_MAX - 3 * T0 * Q))])
    assert P.bases_ok(inside[0], inside[1], 2, 2, 1)
    edge.append_memory_pyramid(d1, cls_id=c1, candidates=inside, **lrr)
    assert tuple(edge.read_motion()["chosen"].tolist()) == (0, 0, 0)
    edge.close()
    frame, g = ya.SceneBatch.pack(c1), np.array(R.IDENTITY, np.int32)
    full = [sc.h, _p(d1), _p(frame), 0, 1, _p(g), _p(g), 2, 2, 1, 224, 30]
    for hole in (0, 1, 2, 5, 6):
        args = list(full)
        args[hole] = None
        assert sc.L.yh_scene_append_memory_pyramid(*args) == ya.capi.EINVAL, hole
    assert sc.L.yh_scene_append_memory_pyramid(*(full[:4] + [0] + full[5:])) == ya.capi.EINVAL
    N = np.ones((H, W), np.uint32)
    tail = [None] * 6
    for args in ((None, _p(N), 1, _p(g), 1, 1, 1), (_p(N), None, 1, _p(g), 1, 1, 1), (_p(N), _p(N), 1, None, 1, 1, 1), (_p(N), _p(N), 0, _p(g), 1, 1, 1),
                 (_p(N), _p(N), 16, _p(g), 1, 1, 1), (_p(N), _p(N), 1, _p(g), 0, 1, 1), (_p(N), _p(N), 1, _p(g), 4, 1, 1), (_p(N), _p(N), 1, _p(g), 1, 9, 1),
                 (_p(N), _p(N), 1, _p(g), 1, 1, 9), (_p(N), _p(N), 1, _p(np.array((Q, 0, I32_MAX - 3 * Q + 1, 0, Q, 0), np.int32)), 1, 1, 1)):
        assert sc.L.yh_scene_op_pyramid(sc.h, *args, *tail) == ya.capi.EINVAL, args[2:]
    got = sc.op_pyramid(N, N, [R.IDENTITY], 2, 1, 1)                                          # the hook itself commits nothing either
    assert got["chosen"] == (0, 0, 0) and int(got["score"][0]) == H * W
    _same(sc.read(), before, ("refused",))
    after, again, still = sc.read_memory(), sc.read_plan(), sc.read_motion()
    assert np.array_equal(after["map"], mem["map"]) and np.array_equal(after["balls"], mem["balls"])
    assert all(np.array_equal(again[k], plan[k]) for k in plan) and all(np.array_equal(still[k], motion[k]) for k in motion)
    assert _same_levels(_levels_of(sc, 2), tables)
    sc.close()


@pytest.mark.gpu
def test_frame_from_a_device_pointer_and_from_the_host(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    host, dev, ref = ya.Scene(W, H), ya.Scene(W, H), P.Memory(W, H)
    gs, cs = [shift(2, 1)[0], IDENT[0]], [shift(2, 1)[1], IDENT[1]]
    for t in range(2):
        depth, ci, o = _stamps(oracle, H, W, 20 + t)
        frame = ya.SceneBatch.pack(ci)
        on_dev = _DeviceFrame(frame)
        host.append_memory_pyramid(depth, frame_u32=frame, candidates=(gs, cs), levels=2, radius=2, refine=1)
        dev.append_memory_pyramid(depth, frame_dev_ptr=on_dev.ptr.value, candidates=(gs, cs), levels=2, radius=2, refine=1)
        want = ref.append_pyramid(o["map"], o["balls"], gs, cs, 2, 2, 1)
        for name, s in (("host", host), ("device", dev)):
            _same(s.read(), want, (name, t))
            _same_motion(s, ref.motion, 2, (name, t))
            _same_memory(s, ref, (name, t))
        assert dev.memory_pyramid_time(2)[0] > 0                                              # the replay reads the device frame again: still valid
        _same(dev.read(), want, ("device, replayed", t))
        on_dev.free()
    host.close(); dev.close()


@pytest.mark.gpu
def test_the_pyramid_registration_costs_no_more_than_the_plain_search_it_outreaches(built):
    """At 640 x 480, on the terrain-only and the robots + balls frame of tools/time_scene.py, in this process: the registration
    launches alone of the pyramid append at (n_rot, L, R, r) = (5, 3, 8, 1) (yh_scene_memory_pyramid_time's second figure: reach
    71 pixels) against those of the plain search append at (n_rot, R) = (5, 8) (yh_scene_memory_search_time's: reach 8), alternated,
    one warm-up each, the median of five runs of 30 replays.
    Ceiling 1.013, each term read from profiles/scene_pyramid_timings.txt (2026-10-20, the two runs at its head): the larger ratio
    of the two runs' (5, 3, 8, 1) rows, 0.973, plus the plain registration's largest spread in any row of those runs, 1.0 %, plus
    the 3 % by which the pool's boxes differ. The measured ratio is below 1, but barely: the pyramid is bound by its ten launches.
    The other grids are recorded there and in DESIGN.md, not bounded here."""
    import yolact_amd as ya
    H, W = 480, 640
    depth = np.random.default_rng(0).integers(200, 4000, (H, W)).astype(np.uint16)
    srch, pyr = ya.Scene(W, H), ya.Scene(W, H)
    prior = (3.0, -2.0, 0.05)
    motion = ya.scene_motion(*prior)
    cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=2)
    for name, robots in (("terrain only", False), ("robots + balls", True)):
        ci = np.zeros((H, W, 2), np.uint8)
        if robots:
            ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
        for sc in (srch, pyr):
            sc.memory_reset()
            sc.append_memory(depth, cls_id=ci, motion=motion)
        srch.append_memory_search(depth, cls_id=ci, candidates=cands, radius=8)
        pyr.append_memory_pyramid(depth, cls_id=ci, candidates=cands, levels=3, radius=8, refine=1)
        srch.memory_search_time(30); pyr.memory_pyramid_time(30)
        ts, tp = [], []
        for _ in range(5):
            ts.append(srch.memory_search_time(30)[1]); tp.append(pyr.memory_pyramid_time(30)[1])
        ratio = float(np.median(tp) / np.median(ts))
        print(f"scene 640x480, {name}: plain (5, 8) registration {np.median(ts):.4f} ms, pyramid (5, 3, 8, 1) {np.median(tp):.4f} ms, ratio {ratio:.3f}")
        assert ratio <= 1.013, (name, ts, tp)
    srch.close(); pyr.close()
