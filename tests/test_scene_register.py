"""The scene memory's registration (DESIGN.md §11 "Scene memory: registration"): yh_scene_append_memory_search scores the frame's
stamps against the memory over a grid of candidate motions, chooses the best on the device and appends with it. CPU part: the numpy
restatement (tests/scene_register_ref.py) against known answers worked out by hand and a per-pixel loop, the tie rule, the int32
conditions, recovery of a known motion; the binding's surface. GPU part (-m gpu): the score table, the choice and every output of
the library against the restatement, bit for bit."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import scene_memory_ref as R
import scene_register_ref as G
from test_scene import _frame
from test_scene_memory import IDENT, shift, turn90, _stamps, _same, _same_memory, _DeviceFrame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
Q = 65536
# about 0.1 rad and a translation, and a shear that halves (gather) / doubles (carry): the pairs of tests/test_scene_memory.py
ROTATION = ((65209, 6543, -40000, -6543, 65209, 90000), (65209, -6543, 48785, 6543, 65209, -85560))
SHEARED = ((Q // 2, Q // 4, 0, 0, Q // 2, Q), (2 * Q, -Q, 2 * Q, 0, 2 * Q, -2 * Q))


def _brute(N, M, g, radius):
    """the score table of one base, one pixel and one shift at a time, in Python integers"""
    H, W = N.shape
    n = 2 * radius + 1
    S = [[0] * n for _ in range(n)]
    for v in range(-radius, radius + 1):
        for u in range(-radius, radius + 1):
            for y in range(H):
                for x in range(W):
                    sx, sy = R.affine(g, x, y)
                    if 0 <= sx + u < W and 0 <= sy + v < H:
                        S[v + radius][u + radius] += min(int(N[y, x]), int(M[sy + v, sx + u]))
    return S


def _edge(radius, sign=1):
    """a gather whose offsets sit exactly on the int32 conditions for this radius"""
    return (Q, 0, sign * (I32_MAX - radius * Q), 0, Q, -sign * (I32_MAX - radius * Q))


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------------

def test_score_tables_known_answers():
    M = (np.arange(16, dtype=np.uint32).reshape(4, 4) + 1) * 10
    N = np.zeros((4, 4), np.uint32)
    N[1, 1], N[2, 3] = 100, 35
    S, sum_n = G.scores(N, M, [R.IDENTITY], 1)
    # by hand: min(100, M[1 + v][1 + u]) + min(35, M[2 + v][3 + u]), the second term 0 where 3 + u leaves the frame
    assert S[0].tolist() == [[45, 55, 30], [85, 95, 70], [125, 135, 100]] and sum_n == 135
    assert G.choose(S) == (0, 0, 1) and S[0].tolist() == _brute(N, M, R.IDENTITY, 1)
    out = G.search(N, M, [R.IDENTITY], [R.IDENTITY], 1)
    assert out["chosen"] == (0, 0, 1) and out["score"] == (135, 95, 135)
    assert out["gather"] == (Q, 0, 0, 0, Q, Q) and out["carry"] == (Q, 0, 0, 0, Q, -Q)
    # 5 x 3, a map that moved one pixel to the right: column 0 of N has no source (sx = -1)
    M = np.array([[5, 1, 9], [2, 8, 3], [7, 4, 6], [1, 9, 2], [8, 3, 5]], np.uint32)
    N = np.zeros_like(M)
    N[:, 1:] = M[:, :2]
    g, c = shift(1, 0)
    S, sum_n = G.scores(N, M, [g, R.IDENTITY], 1)
    # the shift itself and the identity moved one to the left read the same pixels: everything; one to the right of the shift is the
    # identity: min(5, 1) + min(1, 9) + min(2, 8) + min(8, 3) + ..
    assert sum_n == 48 and S[0, 1, 1] == 48 and S[1, 1, 0] == 48 and S[0, 1, 2] == S[1, 1, 1] == 2 + 5 + 8 + 3 + 6
    assert G.strict(S[0]) and not G.strict(S) and G.choose(S) == (0, 0, 0)
    assert S[0].tolist() == _brute(N, M, g, 1) and S[1].tolist() == _brute(N, M, R.IDENTITY, 1)
    # values up to 2^32 - 1 and bases that read across the frame: the vectorised sums are the loop's
    rng = np.random.default_rng(3)
    N, M = (rng.integers(0, 1 << 32, (5, 3), dtype=np.uint64).astype(np.uint32) for _ in range(2))
    N[0, 0] = M[0, 0] = 0xFFFFFFFF
    for g in (R.IDENTITY, turn90(1, 2)[0], ROTATION[0], SHEARED[1], (I32_MAX, I32_MIN, 0, I32_MIN, I32_MAX, 0), _edge(2)):
        assert G.scores(N, M, [g], 2)[0][0].tolist() == _brute(N, M, g, 2), g


def test_shift_identity_and_carry_rule():
    rng = np.random.default_rng(4)
    pts = [(int(x), int(y)) for x, y in rng.integers(-50, 700, (40, 2))] + [(0, 0), (-1, -1), (8191, 8191)]
    bases = [R.IDENTITY, shift(3, -2)[0], shift(-700, 900)[0], turn90(400, 479)[0], ROTATION[0], SHEARED[0], SHEARED[1],
             (I32_MAX, I32_MIN, 0, I32_MIN, I32_MAX, 0), _edge(8), _edge(8, -1), (I32_MIN, I32_MAX, -(I32_MAX - 8 * Q), I32_MAX, I32_MIN, I32_MAX - 8 * Q)]
    for g in bases:
        assert G.bases_ok([g], None, 8)
        for u, v in ((0, 0), (1, 0), (0, -1), (-8, 8), (8, 8), (-8, -8), (3, -5)):
            gc, _ = G.candidate(g, None, u, v)
            assert all(I32_MIN <= t <= I32_MAX for t in gc)
            for x, y in pts:
                sx, sy = R.affine(g, x, y)
                assert R.affine(gc, x, y) == (sx + u, sy + v), (g, u, v, x, y)
    # the carry is the inverse moved the same way: back within a pixel (exactly, for whole-pixel motions)
    for (g, c), exact in ((shift(3, -2), True), (turn90(20, 30), True), (ROTATION, False)):
        for u, v in ((0, 0), (4, -3), (-8, 8), (8, 7)):
            gc, cc = G.candidate(g, c, u, v)
            assert G.bases_ok([g], [c], 8) and all(I32_MIN <= t <= I32_MAX for t in cc) and cc[:2] == tuple(c[:2]) and cc[3:5] == tuple(c[3:5])
            for x, y in pts:
                bx, by = R.affine(cc, *R.affine(gc, x, y))
                assert (bx, by) == (x, y) if exact else abs(bx - x) <= 1 and abs(by - y) <= 1, (g, u, v, x, y)


def test_every_tie_break_level():
    def table(n_rot, radius, entries, fill=0):
        S = np.full((n_rot, 2 * radius + 1, 2 * radius + 1), fill, np.uint64)
        for (k, u, v), s in entries.items():
            S[k, v + radius, u + radius] = s
        return S
    assert G.choose(table(2, 2, {(0, 0, 0): 5, (1, 2, 2): 6})) == (1, 2, 2)                   # the larger S, however far
    assert G.choose(table(2, 2, {(0, 2, 0): 6, (1, 1, 0): 6})) == (1, 1, 0)                   # then the smaller u^2 + v^2, whatever k
    assert G.choose(table(2, 2, {(1, 0, -1): 6, (0, 1, 0): 6})) == (0, 1, 0)                  # then the smaller k, whatever v
    assert G.choose(table(2, 2, {(1, -1, 0): 6, (1, 0, -1): 6, (1, 0, 1): 6})) == (1, 0, -1)  # then the smaller v
    assert G.choose(table(2, 2, {(1, 1, 0): 6, (1, -1, 0): 6})) == (1, -1, 0)                 # then the smaller u
    assert G.choose(table(3, 2, {(0, 1, 2): 6, (0, 2, 1): 6, (0, -1, -2): 6, (0, -2, -1): 6, (0, 2, -1): 6})) == (0, -1, -2)
    assert G.choose(table(3, 1, {}, fill=7)) == (0, 0, 0) and not G.strict(table(3, 1, {}, fill=7)) and G.strict(table(1, 1, {(0, 1, 1): 1}))


def test_empty_and_featureless_maps_choose_the_prior():
    rng = np.random.default_rng(5)
    H, W = 9, 11
    full = rng.integers(1, 500, (H, W)).astype(np.uint32)
    zero = np.zeros((H, W), np.uint32)
    bases = [shift(1, 0)[0], R.IDENTITY, ROTATION[0]]
    for N, M in ((full, zero), (zero, full), (full, np.full((H, W), 300, np.uint32)), (zero, zero)):
        # (a constant map still has an edge: a prior that reads across it loses those pixels, so there the prior is the identity)
        for gs in ([[R.IDENTITY] + bases] if M.any() and N.any() else [bases, [R.IDENTITY] + bases]):
            out = G.search(N, M, gs, None, 3)
            assert out["chosen"] == (0, 0, 0) and out["gather"] == tuple(gs[0])


def test_int32_conditions_from_both_sides():
    for radius in (0, 1, 8):
        top = I32_MAX - radius * Q
        for s in (1, -1):
            assert G.bases_ok([(Q, 0, s * top, 0, Q, -s * top)], None, radius)
            assert not G.bases_ok([(Q, 0, s * (top + 1), 0, Q, 0)], None, radius)
            assert not G.bases_ok([R.IDENTITY, (Q, 0, 0, 0, Q, s * (top + 1))], None, radius)
        # the carry's offsets move by A u + B v: |Cc| + R (|A| + |B|)
        A, B = 3 * Q, -2 * Q
        top = I32_MAX - radius * (abs(A) + abs(B))
        for s in (1, -1):
            assert G.bases_ok([R.IDENTITY], [(A, B, s * top, B, A, -s * top)], radius)
            if radius:
                assert not G.bases_ok([R.IDENTITY], [(A, B, s * (top + 1), B, A, 0)], radius)
                assert not G.bases_ok([R.IDENTITY, R.IDENTITY], [R.IDENTITY, (A, B, 0, B, A, s * (top + 1))], radius)
            for u, v in ((radius, -radius), (-radius, radius), (radius, radius), (-radius, -radius)):
                assert all(I32_MIN <= t <= I32_MAX for t in G.candidate(R.IDENTITY, (A, B, s * top, B, A, -s * top), u, v)[1])
    assert G.bases_ok([(I32_MIN, I32_MAX, 0, I32_MAX, I32_MIN, 0)], [(I32_MIN, I32_MAX, I32_MAX, I32_MAX, I32_MIN, I32_MIN + 1)], 0)
    assert not G.bases_ok([R.IDENTITY], [(I32_MIN, 0, 0, 0, Q, 0)], 1)                        # R |A| alone is past int32


_RECOVERY = {}


def _recovery(name):
    """(N, M, gathers, carries, radius, the true candidate) of a recovery case: N[p] = M[gather_true(p)] of a random sparse M, the
    candidates built around a wrong prior. Computed once."""
    if name in _RECOVERY:
        return _RECOVERY[name]
    from yolact_amd import scene_motion_candidates
    if name == "shift":
        H, W, seed, radius, true = 37, 53, 11, 4, (0, -3, 2)
        gathers, carries = [list(R.IDENTITY)], [list(R.IDENTITY)]                              # the prior says: no motion; it was shift (3, -2)
    else:
        H, W, seed, radius, true = 65, 130, 12, 4, (1, 2, -3)
        # the prior says 0.03 rad; it was 0.05 rad about the start pixel, and a shift (row 1 of +1, -1, +2, -2 steps of 0.02 rad)
        gathers, carries = scene_motion_candidates(prior=(1.0, 2.0, 0.03), dtheta_step=0.02, n_side=2, size=(W, H))
    rng = np.random.default_rng(seed)
    M = np.where(rng.random((H, W)) < 0.3, rng.integers(1, 5000, (H, W)), 0).astype(np.uint32)
    g_true, _ = G.candidate(gathers[true[0]], carries[true[0]], true[1], true[2])
    if name == "shift":
        assert g_true == shift(3, -2)[0]
    N = R.carry_map(M, g_true, 256)
    _RECOVERY[name] = (N, M, gathers, carries, radius, true)
    return _RECOVERY[name]


@pytest.mark.parametrize("name", ["shift", "rotation"])
def test_recovery_of_a_known_motion(name):
    N, M, gathers, carries, radius, true = _recovery(name)
    out = G.search(N, M, gathers, carries, radius)
    S, sum_n = out["scores"], out["score"][2]
    k, u, v = true
    assert sum_n > 0 and int(S[k, v + radius, u + radius]) == sum_n and out["chosen"] == true
    assert G.strict(S) and int(np.sort(S.ravel())[-2]) < sum_n                                # strictly less everywhere else: no tie to blame
    assert out["score"][1] < sum_n                                                            # the prior itself was wrong


def test_scene_motion_candidates():
    from yolact_amd import scene_motion, scene_motion_candidates
    gs, cs = scene_motion_candidates()
    assert len(gs) == len(cs) == 5 and (gs[0], cs[0]) == scene_motion()
    for n_side in (0, 1, 3):
        gs, cs = scene_motion_candidates(prior=(3.0, -2.0, 0.05), dtheta_step=0.02, n_side=n_side, pivot=(30, 40))
        assert len(gs) == len(cs) == 2 * n_side + 1 and (gs[0], cs[0]) == scene_motion(3.0, -2.0, 0.05, pivot=(30, 40))
        steps = [0] + [s * j for j in range(1, n_side + 1) for s in (1, -1)]                  # row 0 the prior, then +1, -1, +2, -2, ..
        assert steps[:3] == [0, 1, -1][:len(steps)]
        for row, s in enumerate(steps):
            assert (gs[row], cs[row]) == scene_motion(3.0, -2.0, 0.05 + s * 0.02, pivot=(30, 40)), (n_side, row)
    assert scene_motion_candidates(size=(64, 32), n_side=1)[0][1] == scene_motion(0, 0, 0.01, size=(64, 32))[0]
    assert G.bases_ok(gs, cs, 8)


def test_surface(built):
    from yolact_amd import capi
    import yolact_amd as ya
    L = capi.load_library()
    pub = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read()
    protos = dict((s[0], s) for s in capi.SYMBOLS)
    _i, _vp, _fp = capi.C.c_int32, capi.C.c_void_p, capi.C.POINTER(capi.C.c_float)
    assert protos["yh_scene_append_memory_search"][1:] == (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i])
    assert protos["yh_scene_motion_read"][1:] == (_i, [_vp, _vp, _vp, _vp, _vp, _vp])
    assert protos["yh_scene_op_register"][1:] == (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp])
    assert protos["yh_scene_memory_search_time"][1:] == (_i, [_vp, _i, _fp, _fp])
    for name in ("yh_scene_append_memory_search", "yh_scene_motion_read"):
        assert hasattr(L, name) and re.search(r"\bint %s\(yh_scene\* h" % name, pub) and name not in re.sub(r"/\*.*?\*/", "", dbg, flags=re.S), name
    for name in ("yh_scene_op_register", "yh_scene_memory_search_time"):
        assert hasattr(L, name) and name not in pub and re.search(r"\bint %s\(yh_scene\* h" % name, dbg), name
    assert re.search(r"int yh_scene_append_memory_search\(yh_scene\* h, const uint16_t\* depth_host, const uint32_t\* frame, int32_t frame_on_device, int32_t n_rot,\s*"
                     r"const int32_t\* gather_q16 /\* \[n_rot\]\[6\] \*/, const int32_t\* carry_q16 /\* \[n_rot\]\[6\] \*/, int32_t radius,\s*int32_t keep, int32_t ball_max_age\);", pub)
    assert re.search(r"int yh_scene_motion_read\(yh_scene\* h, int32_t\* gather_q16 /\* \[6\] \*/, int32_t\* carry_q16 /\* \[6\] \*/, int32_t\* chosen /\* \[3\] = k, u, v \*/,\s*"
                     r"uint64_t\* score /\* \[3\] = S chosen, S prior, sum_n \*/, uint64_t\* scores /\* \[n_rot\]\[2R\+1\]\[2R\+1\] or NULL \*/\);", pub)
    assert re.search(r"int yh_scene_memory_search_time\(yh_scene\* h, int32_t reps, float\* ms_per_frame, float\* ms_search\);", dbg)
    assert "Scene memory: registration" in pub and pub.index("int yh_scene_append_memory(") < pub.index("int yh_scene_append_memory_search(") < pub.index("---- scene batch")
    sig = inspect.signature(capi.Scene.append_memory_search)
    assert list(sig.parameters) == ["self", "depth", "frame_u32", "frame_dev_ptr", "cls_id", "candidates", "radius", "keep", "ball_max_age"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, None, None, None, 4, 224, 30]
    assert list(inspect.signature(capi.Scene.read_motion).parameters) == ["self", "scores"] and inspect.signature(capi.Scene.read_motion).parameters["scores"].default is False
    assert list(inspect.signature(capi.Scene.op_register).parameters) == ["self", "n", "m", "gathers", "radius"]
    assert inspect.signature(capi.Scene.memory_search_time).parameters["reps"].default == 20
    sig = inspect.signature(capi.scene_motion_candidates)
    assert list(sig.parameters) == ["prior", "dtheta_step", "n_side", "pivot", "size"]
    assert [p.default for p in sig.parameters.values()] == [(0.0, 0.0, 0.0), 0.01, 2, None, (640, 480)]
    assert ya.scene_motion_candidates is capi.scene_motion_candidates
    cfg = capi.Config()
    L.yh_default_config(cfg)
    assert cfg.abi_version == 4


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def _lds_words():
    src = open(os.path.join(ROOT, "tiny-object-detection_amd", "csrc", "scene_register_dev.h")).read()
    return int(re.search(r"#define SR_LDS_WORDS (\d+)", src).group(1))


def _window_words(g, H, W, radius):
    """the largest window of M a 64 x 16 tile of an H x W frame can read under gather g, in LDS words as the kernel lays it out
    (the box of the four corner sources, dilated by the radius, the row pitch made odd)"""
    worst = 0
    for y0 in range(0, H, 16):
        for x0 in range(0, W, 64):
            x1, y1 = min(x0 + 64, W) - 1, min(y0 + 16, H) - 1
            src = [R.affine(g, x, y) for x in (x0, x1) for y in (y0, y1)]
            ww = max(s[0] for s in src) - min(s[0] for s in src) + 1 + 2 * radius
            wh = max(s[1] for s in src) - min(s[1] for s in src) + 1 + 2 * radius
            worst = max(worst, (ww | 1) * wh)
    return worst


def _maps(H, W, seed, top=1 << 16):
    """(N, M): random sparse u32 maps with values below `top`; where the frame has more than one tile, the first tile of N is empty"""
    rng = np.random.default_rng(seed)
    N, M = (np.where(rng.random((H, W)) < 0.6, rng.integers(0, top, (H, W), dtype=np.uint64), 0).astype(np.uint32) for _ in range(2))
    if W > 64 or H > 16:
        N[:16, :64] = 0
    return N, M


def _bases(H, W, radius):
    """sixteen gathers: every kind the definition allows, the first ones the plainest"""
    px, py = (W * 5) // 8, H - 1
    return [R.IDENTITY, shift(3, -2)[0], ROTATION[0],
            turn90(px, py)[0], SHEARED[1], (Q, 0, 2 * W * Q, 0, Q, 0),                        # a quarter turn, a magnifying shear, every pixel outside
            SHEARED[0], _edge(radius), _edge(radius, -1), (I32_MAX, I32_MIN, 0, I32_MIN, I32_MAX, 0),
            (4 * Q, 0, 0, 0, 4 * Q, 0), shift(-W // 2, H // 2)[0], turn90(px // 2, py // 2)[0], (Q, Q // 8, -Q, -Q // 8, Q, 3 * Q),
            (I32_MIN, I32_MAX, -(I32_MAX - radius * Q), I32_MAX, I32_MIN, I32_MAX - radius * Q), shift(1, 0)[0]]


def _check_register(sc, N, M, gathers, radius, what):
    want = G.search(N, M, gathers, None, radius)
    scores, chosen, sum_n = sc.op_register(N, M, gathers, radius)
    assert scores.dtype == np.uint64 and scores.shape == want["scores"].shape, what
    assert np.array_equal(scores, want["scores"]), (what, np.argwhere(scores != want["scores"])[:5].tolist())
    assert chosen == want["chosen"] and sum_n == want["score"][2], (what, chosen, want["chosen"], sum_n)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("radius,n_rot,first", [(0, 1, 0), (1, 3, 0), (3, 3, 3), (8, 16, 0)])
@pytest.mark.parametrize("H,W", [(3, 3), (8, 8), (37, 53), (100, 9), (65, 130)])
def test_op_register_matches_the_restatement(built, H, W, radius, n_rot, first):
    import yolact_amd as ya
    N, M = _maps(H, W, 100 * H + W)
    gathers = _bases(H, W, radius)[first:first + n_rot]
    sc = ya.Scene(W, H)
    want = _check_register(sc, N, M, gathers, radius, (H, W, radius, n_rot))
    assert want["score"][2] > 0 and want["scores"].max() > 0
    if (H, W) == (65, 130) and any(tuple(g) == SHEARED[1] for g in gathers):
        # the magnifying shear's window does not fit the LDS budget (the fallback ran), the rotation's and the quarter turn's do
        assert _window_words(SHEARED[1], H, W, radius) > _lds_words() >= max(_window_words(g, H, W, radius) for g in (ROTATION[0], _bases(H, W, radius)[3]))
    sc.close()


@pytest.mark.gpu
def test_op_register_full_range_values_show_a_narrow_accumulator(built):
    import yolact_amd as ya
    H, W = 65, 130
    N, M = _maps(H, W, 7, top=1 << 32)
    N[20:40, 70:120] = 0xFFFFFFFF; M[18:44, 66:124] = 0xFFFFFFFF                           # a thousand pixels of 2^32 - 1 that meet under small shifts
    sc = ya.Scene(W, H)
    want = _check_register(sc, N, M, [R.IDENTITY, shift(3, -2)[0], SHEARED[1]], 3, "full range")
    assert want["scores"].max() > 1 << 41 and want["score"][2] > 1 << 42                      # past 32 bits in a tile, past 2^40 in all
    sc.close()


@pytest.mark.gpu
def test_op_register_at_the_camera_size(built):
    import yolact_amd as ya
    H, W = 480, 640
    N, M = _maps(H, W, 8)
    sc = ya.Scene(W, H)
    _check_register(sc, N, M, [ROTATION[0], R.IDENTITY, SHEARED[1]], 2, "640 x 480")
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shift", "rotation"])
def test_op_register_recovers_the_known_motion(built, name):
    import yolact_amd as ya
    N, M, gathers, carries, radius, true = _recovery(name)
    sc = ya.Scene(N.shape[1], N.shape[0])
    want = _check_register(sc, N, M, gathers, radius, name)
    assert want["chosen"] == true and G.strict(want["scores"])
    sc.close()


def _same_motion(sc, want, what):
    got = sc.read_motion(scores=True)
    assert tuple(got["chosen"].tolist()) == want["chosen"] and tuple(got["gather"].tolist()) == want["gather"] and tuple(got["carry"].tolist()) == want["carry"], (what, got, want["chosen"])
    assert tuple(int(v) for v in got["score"]) == want["score"] and np.array_equal(got["scores"], want["scores"]), what
    return got


def _candidates(H, W):
    """per frame of a sequence: (gathers, carries), radius"""
    return [(([IDENT[0]], [IDENT[1]]), 2),
            (([shift(1, 0)[0], IDENT[0], ROTATION[0]], [shift(1, 0)[1], IDENT[1], ROTATION[1]]), 2),
            (([ROTATION[0], shift(-2, 1)[0]], [ROTATION[1], shift(-2, 1)[1]]), 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (37, 53), (100, 9)])
def test_search_sequences_match_the_restatement(built, oracle, H, W):
    import yolact_amd as ya
    sc, ref = ya.Scene(W, H), G.Memory(W, H)
    for t, ((gs, cs), radius) in enumerate(_candidates(H, W)):
        depth, ci, o = _stamps(oracle, H, W, 10 * H + W + t, balls=t != 1)                    # the second frame has no ball: those of the first are remembered
        keep = (256, 224, 200)[t]
        sc.append_memory_search(depth, cls_id=ci, candidates=(gs, cs), radius=radius, keep=keep, ball_max_age=5)
        want = ref.append_search(o["map"], o["balls"], gs, cs, radius, keep, 5)
        _same_motion(sc, ref.motion, (H, W, t))
        _same(sc.read(), want, ("search", H, W, t))
        _same_memory(sc, ref, ("search", H, W, t))
    assert ref.motion["score"][2] > 0
    sc.close()


@pytest.mark.gpu
def test_a_wrong_prior_is_corrected_to_the_identity(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    d, c, o = _stamps(oracle, H, W, 2)
    g, cr = shift(3, -2)
    want = G.search(o["map"], o["map"], [g], [cr], 4)                                         # the memory after frame A alone IS its stamps
    assert want["chosen"] == (0, 3, -2) and want["gather"] == R.IDENTITY and want["carry"] == R.IDENTITY
    assert G.strict(want["scores"]) and want["score"][0] == want["score"][2] > want["score"][1]
    sc, twice = ya.Scene(W, H), ya.Scene(W, H)
    for s in (sc, twice):
        s.append_memory(d, cls_id=c, keep=256)
    sc.append_memory_search(d, cls_id=c, candidates=([g], [cr]), radius=4, keep=256)
    twice.append_memory(d, cls_id=c, keep=256)
    _same_motion(sc, want, "wrong prior")
    _same(sc.read(), twice.read(), ("wrong prior",))
    a, b = sc.read_memory(), twice.read_memory()
    assert np.array_equal(a["map"], b["map"]) and np.array_equal(a["balls"], b["balls"]) and np.array_equal(a["map"], o["map"])
    sc.close(); twice.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(8, 8), (37, 53)])
def test_one_candidate_is_append_memory_and_an_empty_memory_a_plain_append(built, oracle, H, W):
    import yolact_amd as ya
    d0, c0, _ = _stamps(oracle, H, W, 1)
    d1, c1, _ = _stamps(oracle, H, W, 2)
    srch, mem, plain = ya.Scene(W, H), ya.Scene(W, H), ya.Scene(W, H)
    srch.append_memory_search(d0, cls_id=c0, candidates=([shift(1, 1)[0], ROTATION[0]], [shift(1, 1)[1], ROTATION[1]]), radius=8, keep=256, ball_max_age=255)
    plain.append_classified(d0, frame_u32=ya.SceneBatch.pack(c0), mode=ya.COMPAT_SANE)     # an empty memory: the prior, and nothing to carry
    _same(srch.read(), plain.read(), ("empty", H, W))
    assert tuple(srch.read_motion()["chosen"].tolist()) == (0, 0, 0) and tuple(srch.read_motion()["gather"].tolist()) == shift(1, 1)[0]
    mem.append_memory(d0, cls_id=c0, motion=shift(1, 1), keep=256, ball_max_age=255)
    for t, motion in enumerate((ROTATION, shift(2, -1))):
        srch.append_memory_search(d1, cls_id=c1, candidates=([motion[0]], [motion[1]]), radius=0, keep=200, ball_max_age=9)
        mem.append_memory(d1, cls_id=c1, motion=motion, keep=200, ball_max_age=9)
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
    _, c_none, o_none = _stamps(oracle, H, W, 61, balls=False)                                # the same depth image, the balls not seen
    sc, ref = ya.Scene(W, H), G.Memory(W, H)
    sc.append_memory_search(d, cls_id=c, radius=0)
    ref.append_search(o["map"], o["balls"], [R.IDENTITY], [R.IDENTITY], 0)
    seen = ref.B.copy()
    g, cr = shift(2, 1)                                                                       # the prior says the map moved; it did not
    sc.append_memory_search(d, cls_id=c_none, candidates=([g], [cr]), radius=3, keep=256, ball_max_age=5)
    want = ref.append_search(o_none["map"], o_none["balls"], [g], [cr], 3, 256, 5)
    assert ref.motion["chosen"] == (0, 2, 1) and ref.motion["carry"] == R.IDENTITY and G.strict(ref.motion["scores"])
    _same_motion(sc, ref.motion, "ball")
    _same(sc.read(), want, ("ball",))
    _same_memory(sc, ref, "ball")
    ids = np.flatnonzero(seen[:, 2] > 0)
    assert len(ids) == 2 and not o_none["balls"].any()
    mem = sc.read_memory()["balls"]
    for k in ids:                                                                             # where it was, not two pixels right and one down
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
    sc.append_memory_search(d0, cls_id=c0, radius=1)
    sc.append_memory_search(d1, cls_id=c1, candidates=([shift(2, -1)[0], IDENT[0]], [shift(2, -1)[1], IDENT[1]]), radius=2, keep=240)
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


@pytest.mark.gpu
def test_search_time_commits_nothing_and_the_other_hooks_name_it(built, oracle):
    import ctypes as C
    import yolact_amd as ya
    H, W = 37, 53
    d0, c0, _ = _stamps(oracle, H, W, 41)
    d1, c1, _ = _stamps(oracle, H, W, 42)
    sc = ya.Scene(W, H)
    cands = ([shift(1, 0)[0], ROTATION[0]], [shift(1, 0)[1], ROTATION[1]])
    sc.append_memory_search(d0, cls_id=c0, radius=1)
    sc.append_memory_search(d1, cls_id=c1, candidates=cands, radius=3, keep=250)
    before, mem, motion = sc.read(), sc.read_memory(), sc.read_motion(scores=True)
    ms, ms_search = sc.memory_search_time(3)
    assert ms > 0 and 0 < ms_search < ms
    _same(sc.read(), before, ("search time",))
    after, again = sc.read_memory(), sc.read_motion(scores=True)
    assert np.array_equal(after["map"], mem["map"]) and np.array_equal(after["balls"], mem["balls"])
    assert all(np.array_equal(again[k], motion[k]) for k in motion)
    for call in (lambda: sc.time(2), lambda: sc.memory_time(2)):
        with pytest.raises(ya.YhError) as e:
            call()
        assert e.value.code == ya.capi.ESTATE and "yh_scene_memory_search_time" in str(e.value)
    f = C.c_float()
    assert sc.L.yh_scene_memory_search_time(sc.h, 0, C.byref(f), C.byref(f)) == ya.capi.EINVAL
    assert sc.L.yh_scene_memory_search_time(sc.h, 1, None, C.byref(f)) == ya.capi.EINVAL and sc.L.yh_scene_memory_search_time(sc.h, 1, C.byref(f), None) == ya.capi.EINVAL
    sc.append_memory(d1, cls_id=c1)                                                          # a plain memory append: its own hook again, not this one
    assert sc.memory_time(2) > 0
    for call in (lambda: sc.memory_search_time(2), lambda: sc.read_motion()):
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
    with pytest.raises(ya.YhError) as e:                                                      # before any memory append
        sc.read_motion()
    assert e.value.code == ya.capi.ESTATE
    sc.append_memory_search(d0, cls_id=c0, candidates=([shift(1, 0)[0]], [shift(1, 0)[1]]), radius=2)
    sc.plan(None, start=start)
    before, mem, plan, motion = sc.read(), sc.read_memory(), sc.read_plan(), sc.read_motion(scores=True)
    ok = ([IDENT[0]], [IDENT[1]])
    top = I32_MAX - 2 * Q
    bad = [dict(candidates=ok, radius=-1), dict(candidates=ok, radius=9), dict(candidates=ok, radius=2, keep=-1), dict(candidates=ok, radius=2, keep=257),
           dict(candidates=ok, radius=2, ball_max_age=-1), dict(candidates=ok, radius=2, ball_max_age=256),
           dict(candidates=([IDENT[0]] * 17, [IDENT[1]] * 17), radius=2),
           dict(candidates=([IDENT[0], (Q, 0, top + 1, 0, Q, 0)], [IDENT[1]] * 2), radius=2),
           dict(candidates=([IDENT[0], (Q, 0, 0, 0, Q, -top - 1)], [IDENT[1]] * 2), radius=2),
           dict(candidates=([IDENT[0]] * 2, [IDENT[1], (Q, Q, top + 1 - 2 * Q, 0, Q, 0)]), radius=2),
           dict(candidates=([IDENT[0]] * 2, [IDENT[1], (Q, 0, 0, -Q, 2 * Q, -(top + 1 - 4 * Q))]), radius=2)]
    for kw in bad:
        with pytest.raises(ya.YhError) as e:
            sc.append_memory_search(d1, cls_id=c1, **kw)
        assert e.value.code == ya.capi.EINVAL, kw
    # the same offsets one step inside the conditions are taken (on another handle: this one stays as it is)
    edge = ya.Scene(W, H)
    edge.append_memory_search(d1, cls_id=c1, candidates=([IDENT[0], (Q, 0, top, 0, Q, -top)], [IDENT[1], (Q, Q, top - 2 * Q, -Q, 2 * Q, -(top - 4 * Q))]), radius=2)
    assert tuple(edge.read_motion()["chosen"].tolist()) == (0, 0, 0)
    edge.close()
    frame, g = ya.SceneBatch.pack(c1), np.array(R.IDENTITY, np.int32)
    full = [sc.h, _p(d1), _p(frame), 0, 1, _p(g), _p(g), 2, 224, 30]
    for hole in (0, 1, 2, 5, 6):
        args = list(full)
        args[hole] = None
        assert sc.L.yh_scene_append_memory_search(*args) == ya.capi.EINVAL, hole
    assert sc.L.yh_scene_append_memory_search(*(full[:4] + [0] + full[5:])) == ya.capi.EINVAL
    assert sc.L.yh_scene_motion_read(None, None, None, None, None, None) == ya.capi.EINVAL
    N = np.ones((H, W), np.uint32)
    for args in ((None, _p(N), 1, _p(g), 1), (_p(N), None, 1, _p(g), 1), (_p(N), _p(N), 1, None, 1), (_p(N), _p(N), 0, _p(g), 1), (_p(N), _p(N), 17, _p(g), 1),
                 (_p(N), _p(N), 1, _p(g), 9), (_p(N), _p(N), 1, _p(np.array((Q, 0, I32_MAX - Q + 1, 0, Q, 0), np.int32)), 1)):
        assert sc.L.yh_scene_op_register(sc.h, args[0], args[1], args[2], args[3], args[4], None, None, None) == ya.capi.EINVAL, args[2:]
    assert sc.op_register(N, N, [R.IDENTITY], 1)[1:] == ((0, 0, 0), H * W)                    # the hook itself commits nothing either
    _same(sc.read(), before, ("refused",))
    after, again, still = sc.read_memory(), sc.read_plan(), sc.read_motion(scores=True)
    assert np.array_equal(after["map"], mem["map"]) and np.array_equal(after["balls"], mem["balls"])
    assert all(np.array_equal(again[k], plan[k]) for k in plan) and all(np.array_equal(still[k], motion[k]) for k in motion)
    sc.close()


@pytest.mark.gpu
def test_frame_from_a_device_pointer_and_from_the_host(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    host, dev, ref = ya.Scene(W, H), ya.Scene(W, H), G.Memory(W, H)
    gs, cs = [shift(2, 1)[0], IDENT[0]], [shift(2, 1)[1], IDENT[1]]
    for t in range(2):
        depth, ci, o = _stamps(oracle, H, W, 20 + t)
        frame = ya.SceneBatch.pack(ci)
        on_dev = _DeviceFrame(frame)
        host.append_memory_search(depth, frame_u32=frame, candidates=(gs, cs), radius=2)
        dev.append_memory_search(depth, frame_dev_ptr=on_dev.ptr.value, candidates=(gs, cs), radius=2)
        want = ref.append_search(o["map"], o["balls"], gs, cs, 2)
        for name, s in (("host", host), ("device", dev)):
            _same(s.read(), want, (name, t))
            _same_motion(s, ref.motion, (name, t))
            _same_memory(s, ref, (name, t))
        assert dev.memory_search_time(2)[0] > 0                                               # the replay reads the device frame again: still valid
        _same(dev.read(), want, ("device, replayed", t))
        on_dev.free()
    host.close(); dev.close()


@pytest.mark.gpu
def test_a_search_of_one_candidate_costs_what_its_launches_cost(built):
    """At 640 x 480, on the terrain-only and the robots + balls frame of tools/time_scene.py, in this process: the search append with
    n_rot = 1 and radius 0 (yh_scene_memory_search_time) against the memory append (yh_scene_memory_time), alternated, one warm-up
    each, the median of five runs of 30 frames.
    Ceiling 1.152, each term read from profiles/scene_register_timings.txt (2026-10-20, the two runs at its head): the largest
    ratio of its four (1, 0) rows, 1.115, plus the largest spread of the memory append in any row of those runs, 0.7 %, plus the
    3 % by which the pool's boxes differ. The larger grids are recorded there and in DESIGN.md, not bounded here."""
    import yolact_amd as ya
    H, W = 480, 640
    depth = np.random.default_rng(0).integers(200, 4000, (H, W)).astype(np.uint16)
    mem, srch = ya.Scene(W, H), ya.Scene(W, H)
    motion = ya.scene_motion(3.0, -2.0, 0.05)
    for name, robots in (("terrain only", False), ("robots + balls", True)):
        ci = np.zeros((H, W, 2), np.uint8)
        if robots:
            ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
        for sc in (mem, srch):
            sc.memory_reset()
            sc.append_memory(depth, cls_id=ci, motion=motion)
        mem.append_memory(depth, cls_id=ci, motion=motion)                       # replayed: this frame fused into a filled memory
        srch.append_memory_search(depth, cls_id=ci, candidates=([motion[0]], [motion[1]]), radius=0)
        mem.memory_time(30); srch.memory_search_time(30)
        tm, ts = [], []
        for _ in range(5):
            tm.append(mem.memory_time(30)); ts.append(srch.memory_search_time(30)[0])
        ratio = float(np.median(ts) / np.median(tm))
        print(f"scene 640x480, {name}: memory {np.median(tm):.4f} ms, search (1, 0) {np.median(ts):.4f} ms, ratio {ratio:.3f}")
        assert ratio <= 1.152, (name, tm, ts)
    mem.close(); srch.close()
