"""The scene batch's pyramid registration (DESIGN.md §11 "Scene batch: pyramid registration"): yh_scene_batch_append_memory_pyramid is
n yh_scene_append_memory_pyramid calls in batch order, frame b on the memory of streams[b] - so a stream's later frame is registered,
coarse to fine, against what its earlier frame has just fused. CPU part: the surface, and the restated bank
(tests/scene_batch_pyramid_ref.py) against answers worked out by hand and on priors wrong by more than the plain search reaches. GPU
part (-m gpu): every output, table, memory, motion and level table bit for bit against the restatement fed the oracle's SANE stamps AND
against real Scene handles, one per stream, driven with append_memory_pyramid in batch order; the planners on the fused frames; the
replay hook; every refusal; and the cost per frame against the single handle's pyramid append."""
import inspect
import os
import re

import numpy as np
import pytest

import scene_batch_memory_ref as BR
import scene_batch_pyramid_ref as BP
import scene_batch_register_ref as BG
import scene_memory_ref as R
import scene_pyramid_ref as P
import scene_register_ref as G
from test_scene_batch_memory import N, PATTERNS, _call_frames, _code, _packed, _same
from test_scene_batch_register import OUTSIDE, THREE, _close
from test_scene_memory import IDENT, _DeviceFrame, _stamps, shift
from test_scene_pyramid import COARSE_ALONE, I32_MAX, Q, _bases
from test_scene_register import ROTATION, SHEARED, _lds_words, _window_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# case 1: the same frame in every slot of one stream, each prior wrong by a known shift - further than the plain search reaches (FAR, at
# (levels, radius, refine) = (2, 3, 1): reach 15) or, on the two shapes too small for that, as far as they allow (NEAR, at (1, 2, 1))
FAR_SHAPES, NEAR_SHAPES = [(37, 53), (65, 130), (100, 9), (9, 130)], [(3, 3), (8, 8)]
FAR = ([IDENT, shift(11, -9), shift(-10, 12), shift(9, 9)], (2, 3, 1), [(0, 0, 0), (0, 11, -9), (0, -10, 12), (0, 9, 9)])
NEAR = ([IDENT, shift(3, -2), shift(-1, 4), shift(2, 2)], (1, 2, 1), [(0, 0, 0), (0, 3, -2), (0, -1, 4), (0, 2, 2)])
DECL_APPEND = ("int yh_scene_batch_append_memory_pyramid(yh_scene_batch* h, int32_t n_frames, const int32_t* streams, int32_t n_rot, "
               "const int32_t* gather_q16, const int32_t* carry_q16, int32_t levels, int32_t radius, int32_t refine, int32_t keep, int32_t ball_max_age);")
DECL_READ = "int yh_scene_batch_pyramid_read(yh_scene_batch* h, int32_t frame, int32_t level, int32_t* centres, uint64_t* scores, uint64_t* sum_n);"
DECL_TIME = "int yh_scene_batch_memory_pyramid_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, float* ms_search);"


def _case(H, W):
    return NEAR if (H, W) in NEAR_SHAPES else FAR


# ---- CPU: the surface and the restated bank ----------------------------------------------------------------------------------------

def _code_of(text):
    """a header without its comments, white space folded, none before a comma or a closing parenthesis"""
    return re.sub(r" ([,)])", r"\1", re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_surface():
    import yolact_amd as ya
    from yolact_amd import capi
    pub = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "yolact_hip_debug.h")).read()
    pub_code, dbg_code = _code_of(pub), _code_of(dbg)
    for decl in (DECL_APPEND, DECL_READ):
        assert re.search(r"(?<![\w])" + re.escape(decl), pub_code), decl
    assert re.search(r"(?<![\w])" + re.escape(DECL_TIME), dbg_code)
    for name in ("yh_scene_batch_append_memory_pyramid", "yh_scene_batch_pyramid_read"):
        assert name not in dbg_code, name
    assert "yh_scene_batch_memory_pyramid_time" not in pub
    # a section of its own, the last of the scene batch's, under its comment line
    marks = ["---- scene batch: memory", "int yh_scene_batch_append_memory(", "---- scene batch: registration", "int yh_scene_batch_append_memory_search(",
             "int yh_scene_batch_motion_read(", "---- scene batch: pyramid registration (DESIGN.md section 11 \"Scene batch: pyramid registration\")",
             "int yh_scene_batch_append_memory_pyramid(", "int yh_scene_batch_pyramid_read("]
    at = [pub.index(m) for m in marks]
    assert at == sorted(at) and pub.rindex("---- scene batch") == at[5]
    protos = dict((s[0], s) for s in capi.SYMBOLS)
    _i, _vp, _fp = capi.C.c_int32, capi.C.c_void_p, capi.C.POINTER(capi.C.c_float)
    assert protos["yh_scene_batch_append_memory_pyramid"][1:] == (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i])
    assert protos["yh_scene_batch_pyramid_read"][1:] == (_i, [_vp, _i, _i, _vp, _vp, _vp])
    assert protos["yh_scene_batch_memory_pyramid_time"][1:] == (_i, [_vp, _i, _fp, _fp])
    sig = inspect.signature(capi.SceneBatch.append_memory_pyramid)
    assert list(sig.parameters) == ["self", "n", "candidates", "streams", "levels", "radius", "refine", "keep", "ball_max_age"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, None, 3, 8, 1, 224, 30]
    assert list(inspect.signature(capi.SceneBatch.read_pyramid).parameters) == ["self", "frame", "level"]
    sig = inspect.signature(capi.SceneBatch.memory_pyramid_time)
    assert list(sig.parameters) == ["self", "reps"] and sig.parameters["reps"].default == 20
    assert "#define YH_ABI_VERSION 4" in pub and BP.STREAMS_MAX == capi.SCENE_STREAMS_MAX == ya.SCENE_STREAMS_MAX


def test_restated_bank_registers_a_chained_frame_against_its_predecessors_map():
    W, H = 4, 3
    Z = np.zeros((H, W), np.uint32)
    A = Z.copy(); A[1, 1] = 100; A[0, 3] = 7
    B = Z.copy(); B[2, 2] = 50
    A1 = Z.copy(); A1[1, 2] = 100                                                                    # A's peak one to the right: the map moved by (1, 0)
    none = np.zeros((100, 4), np.float32)
    seen = none.copy(); seen[7] = (1.5, 2.5, 4, 0)
    one = ([R.IDENTITY], [R.IDENTITY])
    bank = BP.Bank(W, H)
    # frames 0 and 2 on stream 0, frames 1 and 3 on stream 1. Both streams start empty, so against the call-start memory every score of
    # frames 2 and 3 would be 0 and the choice (0, 0, 0): only against frame 0's fused map does frame 2 find its shift.
    out, tabs, mot = bank.append_pyramid([A, B, A1, B], [seen, none, none, none], [0, 1, 0, 1], [one] * 4, 1, 1, 1, 128, 2)
    assert mot[0]["chosen"] == mot[1]["chosen"] == (0, 0, 0) and mot[0]["score"] == (0, 0, 107) and not any(t.any() for t in mot[1]["tables"])
    # by hand. Level 1 (2 x 2): N has 100 in cell (1, 0), M = A pooled is [[100, 7], [0, 0]]: S(U, V) = min(100, M1[V][1 + U]), 100 at
    # U = -1, 7 at U = 0, both V = 0. The centre below is twice (-1, 0).
    m = mot[2]
    top = np.zeros((1, 3, 3), np.uint64); top[0, 1, 0] = 100; top[0, 1, 1] = 7
    assert np.array_equal(m["tables"][1], top) and m["centres"][1].tolist() == [[0, 0]] and m["centres"][0].tolist() == [[-2, 0], [0, 0]]
    # level 0: S(u, v) = min(100, A[1 + v][2 + u]). Around (-2, 0) only u = -1, v = 0 meets A's peak; the home hypothesis around (0, 0)
    # meets it too, and A's corner pixel at u = 1, v = -1
    low = np.zeros((2, 3, 3), np.uint64); low[0, 1, 2] = 100; low[1, 1, 0] = 100; low[1, 0, 2] = 7
    assert np.array_equal(m["tables"][0], low) and m["sum_n"] == [100, 100]
    assert m["chosen"] == (0, -1, 0) and m["score"] == (100, 0, 100) and m["gather"] == shift(1, 0)[0] and m["carry"] == shift(1, 0)[1]
    # frame 3 is frame 1 again, against frame 1's own map: the identity, S = sum_n, the stream-0 frames between them nothing to it
    assert mot[3]["chosen"] == (0, 0, 0) and mot[3]["score"] == (50, 50, 50)
    f2 = Z.copy(); f2[1, 2] = 100                                                                    # A moved right (its corner pixel leaves), halved: 50 < 100
    assert np.array_equal(out[2]["map"], f2) and np.array_equal(bank.mem[0].M, f2) and np.array_equal(bank.mem[1].M, B)
    assert tabs[2][7].tolist() == [2, 2, 4, 1] and out[2]["balls"][7].tolist() == [2, 2, 4, 0]     # the ball carried by the CHOSEN carry, one to the right
    # the next call continues the streams: frame A1 again on stream 0 now sits where the memory has it; reset empties
    out, tabs, mot = bank.append_pyramid([A1], [none], [0], [one], 1, 1, 1, 256, 2)
    assert mot[0]["chosen"] == (0, 0, 0) and mot[0]["score"] == (100, 100, 100) and tabs[0][7].tolist() == [2, 2, 4, 2]
    bank.reset(0)
    assert not bank.mem[0].M.any() and not bank.mem[0].B.any() and bank.mem[1].M.any()
    bank.reset()
    assert not bank.mem[1].M.any()


def test_restated_bank_with_one_candidate_and_no_search_is_the_plain_bank():
    rng = np.random.default_rng(9)
    W, H = 4, 3
    stamps = [rng.integers(0, 300, (H, W)).astype(np.uint32) for _ in range(5)]
    balls = [np.zeros((100, 4), np.float32) for _ in range(5)]
    balls[0][3] = (2.5, 1.5, 6, 0)
    motions = [IDENT, shift(1, 0), shift(0, 1), IDENT, shift(-1, 1)]
    streams = [2, 0, 2, 2, 0]
    a, b = BP.Bank(W, H), BR.Bank(W, H)
    for keep in (224, 200):
        got, tabs, mot = a.append_pyramid(stamps, balls, streams, [([g], [c]) for g, c in motions], 1, 0, 0, keep, 3)
        want, wtabs = b.append(stamps, balls, streams, motions, keep, 3)
        for i in range(5):
            _same(got[i], want[i], ("plain", keep, i))
            assert np.array_equal(tabs[i], wtabs[i]) and mot[i]["chosen"] == (0, 0, 0) and (mot[i]["gather"], mot[i]["carry"]) == motions[i]
        for s in (0, 2):
            assert np.array_equal(a.mem[s].M, b.mem[s].M) and np.array_equal(a.mem[s].B, b.mem[s].B)
    assert a.mem[2].M.any() and a.mem[2].B[3, 2] == 6


_WRONG = {}


def _wrong_priors(oracle, H, W):
    """case 1 on the restatement, computed once per shape: (the frames, (per-frame outputs, tables, motions), the bank)"""
    if (H, W) not in _WRONG:
        priors, (levels, radius, refine), _ = _case(H, W)
        frames = _packed([_stamps(oracle, H, W, 2)] * 4)
        bank = BP.Bank(W, H)
        o = frames[2][0]
        out = bank.append_pyramid([o["map"]] * 4, [o["balls"]] * 4, None, [([g], [c]) for g, c in priors], levels, radius, refine, 256, 30)
        _WRONG[H, W] = (frames, out, bank)
    return _WRONG[H, W]


def _wrong_priors_hold(mot, H, W):
    priors, _, chosen = _case(H, W)
    assert [m["chosen"] for m in mot] == chosen and mot[0]["gather"] == R.IDENTITY
    for m in mot[1:]:
        assert m["gather"] == R.IDENTITY and m["carry"] == R.IDENTITY and m["score"][0] == m["score"][2]
        assert G.strict(m["tables"][0])                                                              # exactly one level-0 entry holds the maximum


@pytest.mark.parametrize("H,W", FAR_SHAPES + NEAR_SHAPES)
def test_same_frame_far_wrong_priors_restated(oracle, H, W):
    """Frame 0 meets an empty memory; every later frame is the frame its predecessor fused (keep = 256: the memory IS the frame's
    stamps), so its wrong prior is corrected to the identity - which the call-start memory, empty, could never tell it, and which on
    the FAR shapes the plain search at its widest, radius 8, cannot reach: it stops at the corner of its grid."""
    frames, (_, _, mot), _ = _wrong_priors(oracle, H, W)
    _wrong_priors_hold(mot, H, W)
    if (H, W) in FAR_SHAPES:
        stamps = frames[2][0]["map"]
        for (g, c), (_, u, v) in list(zip(FAR[0], FAR[2]))[1:]:
            assert max(abs(u), abs(v)) > 8 and G.search(stamps, stamps, [g], [c], 8)["chosen"] == (0, 8 * np.sign(u), 8 * np.sign(v)), (u, v)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def _same_motion(motion, tables, want, what):
    """read_motion's dict and read_pyramid's per level against what scene_pyramid_ref.search returns"""
    assert motion["gather"].dtype == motion["carry"].dtype == motion["chosen"].dtype == np.int32 and motion["score"].dtype == np.uint64, what
    assert tuple(motion["chosen"].tolist()) == want["chosen"] and tuple(motion["gather"].tolist()) == want["gather"] and tuple(motion["carry"].tolist()) == want["carry"], (what, motion["chosen"], want["chosen"])
    assert tuple(int(v) for v in motion["score"]) == want["score"], what
    assert len(tables) == len(want["tables"])
    for lv, t in enumerate(tables):
        assert t["centres"].dtype == np.int32 and t["scores"].dtype == np.uint64 and t["scores"].shape == want["tables"][lv].shape, what + (lv,)
        assert np.array_equal(t["centres"], want["centres"][lv]) and np.array_equal(t["scores"], want["tables"][lv]) and t["sum_n"] == want["sum_n"][lv], what + (lv,)


def _levels_of(sb, b, levels):
    return [sb.read_pyramid(b, lv) for lv in range(levels + 1)]


def _same_levels(a, b):
    return len(a) == len(b) and all(np.array_equal(x[k], y[k]) if k != "sum_n" else x[k] == y[k] for x, y in zip(a, b) for k in x)


def _run_call(sb, bank, scenes, frames, streams, cands, lrr, keep, max_age, what, restated=None):
    """One batched pyramid call against the restated bank (or its result, if computed before) and against Scene handles, one per
    stream, driven with append_memory_pyramid in batch order; returns (the batch's per-frame outputs, the restated motions)."""
    import yolact_amd as ya
    depths, packed, ora = frames
    n, H, W = len(ora), sb.H, sb.W
    levels, radius, refine = lrr
    sb.stage_frames(0, depths, frames_u32=packed)
    sb.append_memory_pyramid(n, candidates=cands, streams=streams, levels=levels, radius=radius, refine=refine, keep=keep, ball_max_age=max_age)
    want, tables, motions = restated or bank.append_pyramid([o["map"] for o in ora], [o["balls"] for o in ora], streams, cands, levels, radius, refine, keep, max_age)
    got = []
    for b in range(n):
        s = 0 if streams is None else streams[b]
        got.append(sb.read(b))
        _same(got[b], want[b], what + ("ref", b))
        tab = sb.read_frame_memory_balls(b)
        assert tab.dtype == np.int32 and np.array_equal(tab, tables[b]), what + ("table", b)
        motion, lvs = sb.read_motion(b), _levels_of(sb, b, levels)
        _same_motion(motion, lvs, motions[b], what + ("motion", b))
        if scenes is not None:
            if s not in scenes:
                scenes[s] = ya.Scene(W, H)
            sc = scenes[s]
            sc.append_memory_pyramid(depths[b], frame_u32=packed[b], candidates=cands[b] if cands else None, levels=levels, radius=radius, refine=refine, keep=keep,
                                     ball_max_age=max_age)
            _same(got[b], sc.read(), what + ("scene", b))
            assert np.array_equal(tab, sc.read_memory()["balls"]), what + ("scene table", b)
            single = sc.read_motion()
            assert motion.keys() == single.keys() and all(np.array_equal(motion[k], single[k]) for k in single), what + ("scene motion", b)
            assert _same_levels(lvs, [sc.read_pyramid(lv) for lv in range(levels + 1)]), what + ("scene levels", b)
    for s in set([0] if streams is None else streams):
        mem = sb.read_memory(s)
        assert mem["map"].dtype == np.uint32 and np.array_equal(mem["map"], bank.mem[s].M) and np.array_equal(mem["balls"], bank.mem[s].B), what + ("bank", s)
        if scenes is not None:
            _same(mem, scenes[s].read_memory(), what + ("scene bank", s))
    return got, motions


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", FAR_SHAPES + NEAR_SHAPES)
def test_same_frame_far_wrong_priors(built, oracle, H, W):
    """Case 1. An implementation that pools or scores the call-start (empty) memory for a chained frame, or hands a frame another frame's
    table or record, cannot pass: the three corrections differ and none is (0, 0, 0). One that falls back to the plain search cannot
    either: on the FAR shapes every correction lies beyond radius 8."""
    import yolact_amd as ya
    frames, restated, bank = _wrong_priors(oracle, H, W)
    priors, lrr, _ = _case(H, W)
    _wrong_priors_hold(restated[2], H, W)
    sb, scenes = ya.SceneBatch(W, H, 4), {}
    _run_call(sb, bank, scenes, frames, None, [([g], [c]) for g, c in priors], lrr, 256, 30, ("wrong priors", H, W), restated=restated)
    _close(sb, scenes)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("H,W", [(37, 53), (100, 9), (9, 130)])
def test_distinct_frames_equal_the_restatement_and_one_scene_per_stream(built, oracle, H, W, pattern):
    """Case 2: two calls of six distinct frames over the stream patterns of test_scene_batch_memory.py (the second continues every
    stream of the first), three bases per frame, (levels, radius, refine) = (2, 2, 1), keep 224 then 200. With all frames on one
    stream, some frame of rank >= 2 of the second call has a level-0 table against its predecessor's map that differs from its table
    against the call-start memory."""
    import yolact_amd as ya
    streams = PATTERNS[pattern]
    sb, bank, scenes = ya.SceneBatch(W, H, N), BP.Bank(W, H), {}
    for k, keep in enumerate((224, 200)):
        start = bank.mem[9].M.copy()
        frames = _call_frames(oracle, H, W, k)
        _, mot = _run_call(sb, bank, scenes, frames, streams, [THREE] * N, (2, 2, 1), keep, 5, (pattern, H, W, k))
        if pattern == "one" and k == 1:
            assert start.any() and any(not np.array_equal(P.search(frames[2][b]["map"], start, THREE[0], THREE[1], 2, 2, 1)["tables"][0], mot[b]["tables"][0]) for b in range(2, N))
    assert any(m["score"][0] > 0 for m in mot) and len(scenes) == len(set(streams or [0]))
    _close(sb, scenes)


@pytest.mark.gpu
def test_the_largest_grid(built, oracle):
    """(levels, radius, refine) = (3, 8, 8), n_rot 15: fifteen bases of every kind the definition allows, on filled memories, three
    frames over two streams, two of them chained."""
    import yolact_amd as ya
    H, W = 37, 53
    sb, bank, scenes = ya.SceneBatch(W, H, 3), BP.Bank(W, H), {}
    _run_call(sb, bank, scenes, _call_frames(oracle, H, W, 0, 2), [0, 1], None, (1, 0, 0), 256, 5, ("fill",))
    gathers = [tuple(g) for g in _bases(H, W)]
    assert len(gathers) == 15 and P.bases_ok(gathers, [R.IDENTITY] * 15, 3, 8, 8)
    _, mot = _run_call(sb, bank, scenes, _call_frames(oracle, H, W, 1, 3), [0, 0, 1], [(gathers, [R.IDENTITY] * 15)] * 3, (3, 8, 8), 224, 5, ("(3, 8, 8)",))
    assert all(m["tables"][0].shape == (16, 17, 17) and m["tables"][3].shape == (15, 17, 17) and m["tables"][0].max() > 0 for m in mot)
    _close(sb, scenes)


@pytest.mark.gpu
def test_edge_bases_and_the_global_memory_fallback_per_frame(built, oracle):
    """At 9 x 130 on filled memories, four frames over two streams, refine 6 - so level 0 runs at radius 6: the magnifying shear, whose
    window of M overflows the LDS budget there (so the score kernel's global-memory path runs, per frame of a batch), a motion that
    sends every pixel outside, and offsets exactly on the int32 conditions of the reach. The bases of cases 1 and 2 never overflow."""
    import yolact_amd as ya
    H, W, lrr = 9, 130, (1, 2, 6)
    T0 = P.reach(*lrr)[0]
    lds = _lds_words()
    assert T0 == 10 and _window_words(SHEARED[1], H, W, 6) > lds == 4096 >= _window_words(SHEARED[1], H, W, 5)
    sb, bank, scenes = ya.SceneBatch(W, H, 4), BP.Bank(W, H), {}
    _run_call(sb, bank, scenes, _call_frames(oracle, H, W, 0, 2), [0, 1], None, (1, 0, 0), 256, 5, ("fill",))
    top = I32_MAX - T0 * Q
    gathers = [SHEARED[1], OUTSIDE(W), (Q, 0, top, 0, Q, -top), (Q, 0, -top, 0, Q, top)]
    carries = [SHEARED[0], R.IDENTITY, (Q, Q, I32_MAX - 2 * T0 * Q, -Q, 2 * Q, -(I32_MAX - 3 * T0 * Q)), R.IDENTITY]
    assert P.bases_ok(gathers, carries, *lrr) and not P.bases_ok(gathers[:2] + [(Q, 0, top + 1, 0, Q, 0)], carries[:3], *lrr)
    _, mot = _run_call(sb, bank, scenes, _call_frames(oracle, H, W, 1, 4), [0, 1, 0, 1], [(gathers, carries)] * 4, lrr, 224, 5, ("edges",))
    assert all(m["tables"][0][0].max() > 0 and not m["tables"][0][1].any() and m["tables"][0].shape == (5, 13, 13) for m in mot)   # the shear reads the memory, the motion outside nothing
    # every pixel outside as the only base: nothing to score, the prior stands, nothing is gathered
    frames = _call_frames(oracle, H, W, 2, 2)
    got, mot = _run_call(sb, bank, scenes, frames, [1, 1], [([OUTSIDE(W)], [OUTSIDE(-W)])] * 2, lrr, 224, 5, ("outside",))
    assert all(m["chosen"] == (0, 0, 0) and m["score"][:2] == (0, 0) for m in mot) and np.array_equal(got[1]["map"], frames[2][1]["map"])
    _close(sb, scenes)


@pytest.mark.gpu
def test_at_the_camera_size(built, oracle):
    """The three frames of test_scene_memory.py's camera-size sequence (the oracle's stamps are computed once for all): two on stream 1,
    the ball-less one between them on stream 0."""
    import yolact_amd as ya
    H, W = 480, 640
    frames = _packed([_stamps(oracle, H, W, 10 * H + W + t, balls=t != 1) for t in range(3)])
    sb, bank, scenes = ya.SceneBatch(W, H, 3), BP.Bank(W, H), {}
    cands = ([ROTATION[0], IDENT[0]], [ROTATION[1], IDENT[1]])
    _, mot = _run_call(sb, bank, scenes, frames, [1, 0, 1], [cands] * 3, (3, 2, 1), 224, 5, ("camera",))
    assert mot[2]["score"][0] > 0 and not any(t.any() for t in mot[1]["tables"])                    # frame 2 met frame 0's map, frame 1 an empty stream
    _close(sb, scenes)


@pytest.mark.gpu
def test_one_slot_batches_and_fewer_frames_than_slots(built, oracle):
    import yolact_amd as ya
    H, W, lrr = 37, 53, (2, 2, 1)
    sb, bank, scenes = ya.SceneBatch(W, H, 1), BP.Bank(W, H), {}
    for k in range(3):                                                                                # max_frames = 1: the chain runs through the bank
        _run_call(sb, bank, scenes, _call_frames(oracle, H, W, k, 1), [5], [THREE], lrr, 230, 4, ("one slot", k))
    assert _code(lambda: sb.append_memory_pyramid(2, candidates=[THREE] * 2)) == ya.capi.EINVAL
    _close(sb, scenes)
    sb, bank, scenes = ya.SceneBatch(W, H, 4), BP.Bank(W, H), {}
    depths, packed, _ = _call_frames(oracle, H, W, 0, 3)
    sb.stage_frames(0, depths, frames_u32=packed)
    with pytest.raises(ya.YhError) as e:                                                              # slot 3 was never staged
        sb.append_memory_pyramid(4, candidates=[THREE] * 4)
    assert e.value.code == ya.capi.ESTATE and "slot 3" in str(e.value)
    _run_call(sb, bank, scenes, _call_frames(oracle, H, W, 0, 4), [0, 1, 2, 0], [THREE] * 4, lrr, 240, 9, ("first",))
    before = sb.read_memory(1)
    _run_call(sb, bank, scenes, _call_frames(oracle, H, W, 1, 2), [0, 2], [THREE] * 2, (3, 1, 2), 240, 9, ("n < max_frames",))
    _same(sb.read_memory(1), before, ("absent stream",))
    assert before["map"].any() and _code(lambda: sb.read(2)) == ya.capi.EINVAL and _code(lambda: sb.read_motion(2)) == ya.capi.EINVAL
    assert _code(lambda: sb.read_pyramid(2, 0)) == ya.capi.EINVAL
    _close(sb, scenes)


@pytest.mark.gpu
def test_no_search_is_append_memory_and_an_empty_bank_the_plain_sane_append(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    pyr, mem, plain = ya.SceneBatch(W, H, 3), ya.SceneBatch(W, H, 3), ya.SceneBatch(W, H, 3)
    # an empty bank, a stream per frame: every frame chooses the prior, and nothing is carried
    depths, packed, _ = _call_frames(oracle, H, W, 0, 3)
    for sb in (pyr, mem, plain):
        sb.stage_frames(0, depths, frames_u32=packed)
    pyr.append_memory_pyramid(3, candidates=[THREE] * 3, streams=[4, 5, 6], levels=3, radius=8, refine=1, keep=256, ball_max_age=255)
    plain.append(3, ya.COMPAT_SANE)
    mem.append_memory(3, motions=[shift(1, 0)] * 3, streams=[4, 5, 6], keep=256, ball_max_age=255)
    for b in range(3):
        _same(pyr.read(b), plain.read(b), ("empty bank", b))
        m = pyr.read_motion(b)
        assert tuple(m["chosen"].tolist()) == (0, 0, 0) and tuple(m["gather"].tolist()) == THREE[0][0] and tuple(m["carry"].tolist()) == THREE[1][0]
    # n_rot = 1, levels 1, radius 0, refine 0: yh_scene_batch_append_memory with the same motions, two calls on chained streams
    for k in (1, 2):
        depths, packed, _ = _call_frames(oracle, H, W, k, 3)
        motions = [ROTATION, shift(2, -1), shift(-1, 1)]
        for sb in (pyr, mem):
            sb.stage_frames(0, depths, frames_u32=packed)
        pyr.append_memory_pyramid(3, candidates=[([g], [c]) for g, c in motions], streams=[4, 4, 6], levels=1, radius=0, refine=0, keep=200, ball_max_age=9)
        mem.append_memory(3, motions=motions, streams=[4, 4, 6], keep=200, ball_max_age=9)
        for b in range(3):
            _same(pyr.read(b), mem.read(b), ("(1, 1, 0, 0)", k, b))
            assert np.array_equal(pyr.read_frame_memory_balls(b), mem.read_frame_memory_balls(b))
            got, low = pyr.read_motion(b), pyr.read_pyramid(b, 0)
            assert (tuple(got["gather"].tolist()), tuple(got["carry"].tolist())) == motions[b] and low["scores"].shape == (2, 1, 1)
            assert low["scores"][0, 0, 0] == low["scores"][1, 0, 0] == got["score"][0] == got["score"][1]
        for s in (4, 5, 6):
            _same(pyr.read_memory(s), mem.read_memory(s), ("(1, 1, 0, 0) bank", k, s))
    assert pyr.read_memory(4)["map"].any() and plain.read(0)["map"].max() > 0
    _close(pyr, mem, plain)


@pytest.mark.gpu
def test_frames_staged_from_a_device_pointer_and_from_the_host(built, oracle):
    import yolact_amd as ya
    H, W = 37, 53
    host, dev = ya.SceneBatch(W, H, 3), ya.SceneBatch(W, H, 3)
    for k in range(2):
        depths, packed, _ = _call_frames(oracle, H, W, k, 3)
        on_dev = _DeviceFrame(packed)
        host.stage_frames(0, depths, frames_u32=packed)
        dev.stage_frames(0, depths, frames_dev_ptr=on_dev.ptr.value)
        on_dev.free()                                                                                # staged: the caller's frames are free again
        for sb in (host, dev):
            sb.append_memory_pyramid(3, candidates=[THREE] * 3, streams=[1, 0, 1], levels=2, radius=2, refine=1)
        for b in range(3):
            _same(dev.read(b), host.read(b), ("device", k, b))
            a, h = dev.read_motion(b), host.read_motion(b)
            assert all(np.array_equal(a[key], h[key]) for key in h) and np.array_equal(dev.read_frame_memory_balls(b), host.read_frame_memory_balls(b))
            assert _same_levels(_levels_of(dev, b, 2), _levels_of(host, b, 2))
        for s in (0, 1):
            _same(dev.read_memory(s), host.read_memory(s), ("device bank", k, s))
    assert dev.read_motion(2)["score"][0] > 0
    _close(host, dev)


@pytest.mark.gpu
def test_remembered_balls_are_carried_by_the_chosen_carry_of_their_own_frame(built, oracle):
    """test_scene_pyramid.py's construction on two streams in ONE call: each stream sees its balls, then the same depth image without
    them under a prior that says the map moved far - by a different shift per stream, both beyond the plain search's reach. Each
    correction is its own frame's; the balls stay where they were, not where either prior would put them."""
    import yolact_amd as ya
    H, W, lrr = 37, 53, (2, 3, 1)
    with_balls = [_stamps(oracle, H, W, seed) for seed in (61, 62)]
    without = [_stamps(oracle, H, W, seed, balls=False) for seed in (61, 62)]
    sb, bank, scenes = ya.SceneBatch(W, H, 4), BP.Bank(W, H), {}
    priors = [shift(10, 7), shift(-9, 11)]
    cands = [([IDENT[0]], [IDENT[1]])] * 2 + [([g], [c]) for g, c in priors]
    got, mot = _run_call(sb, bank, scenes, _packed(with_balls + without), [3, 8, 3, 8], cands, lrr, 256, 5, ("balls",))
    assert [m["chosen"] for m in mot] == [(0, 0, 0), (0, 0, 0), (0, 10, 7), (0, -9, 11)]                # both corrected, on the restatement
    assert all(m["carry"] == R.IDENTITY and m["gather"] == R.IDENTITY and G.strict(m["tables"][0]) for m in mot[2:])
    for b, s in ((2, 3), (3, 8)):
        seen = sb.read_frame_memory_balls(b - 2)
        ids = np.flatnonzero(seen[:, 2] > 0)
        assert len(ids) >= 1 and not without[b - 2][2]["balls"].any()
        tab, mem = sb.read_frame_memory_balls(b), sb.read_memory(s)["balls"]
        for k in ids:
            assert tab[k].tolist() == mem[k].tolist() == [seen[k, 0], seen[k, 1], seen[k, 2], 1] and got[b]["balls"][k].tolist() == [seen[k, 0], seen[k, 1], seen[k, 2], 0]
    _close(sb, scenes)


@pytest.mark.gpu
def test_planners_run_on_the_fused_frames(built, oracle):
    """One plan and one turn plan with targets=None, against the per-stream Scenes after the same appends: two frames on one stream,
    the second sees no ball and plans to the ones remembered; a third on another stream."""
    import yolact_amd as ya
    H, W = 33, 65
    start = ((W * 5) // 8, H - 1)
    fr = [_stamps(oracle, H, W, 31), _stamps(oracle, H, W, 32, balls=False), _stamps(oracle, H, W, 33)]
    depths, packed, ora = _packed(fr)
    streams = [2, 2, 0]
    cands = [([shift(2, -1)[0], IDENT[0]], [shift(2, -1)[1], IDENT[1]])] * 3
    kw = dict(levels=2, radius=2, refine=1, keep=240)
    sb, scenes = ya.SceneBatch(W, H, 3), {s: ya.Scene(W, H) for s in (0, 2)}
    sb.stage_frames(0, depths, frames_u32=packed)
    sb.append_memory_pyramid(3, candidates=cands, streams=streams, **kw)
    f1 = sb.read(1)
    assert not ora[1]["balls"].any() and (f1["balls"][:, 2] > 0).sum() >= 1 and (f1["map"] > ora[1]["map"]).any()        # balls only remembered, map fused
    want = []
    for b, s in enumerate(streams):
        sc = scenes[s]
        sc.append_memory_pyramid(depths[b], frame_u32=packed[b], candidates=cands[b], **kw)
        sc.plan(None, n_targets=3, start=start, connectivity=8)
        w = dict(plan=sc.read_plan())
        sc.plan_turn(None, n_targets=3, start=start, heading=6, turn_price=2.0)
        w["turn"] = sc.read_turn()
        want.append(w)
    assert sb.plan(None, n_targets=3, starts=[start] * 3, connectivity=8) == [0, 0, 0]
    for b in range(3):
        _same(sb.read_plan(b), want[b]["plan"], ("plan", b))
    assert sb.plan_turn(None, n_targets=3, starts=[start] * 3, headings=6, turn_price=2.0) == [0, 0, 0]
    for b in range(3):
        _same(sb.read_turn(b), want[b]["turn"], ("turn", b))
    _close(sb, scenes)


def _raises(fn, code, text=None):
    import yolact_amd as ya
    with pytest.raises(ya.YhError) as e:
        fn()
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)


@pytest.mark.gpu
def test_pyramid_time_commits_nothing_and_the_state_rules(built, oracle):
    import ctypes as C
    import yolact_amd as ya
    from yolact_amd.capi import EINVAL, ESTATE, OK
    H, W = 37, 53
    sb, scenes = ya.SceneBatch(W, H, 4), {s: ya.Scene(W, H) for s in (1, 2)}
    assert _code(lambda: sb.read_pyramid(0, 0)) == ESTATE and _code(lambda: sb.memory_pyramid_time(1)) == ESTATE     # before any memory append
    depths, packed, _ = _call_frames(oracle, H, W, 0, 4)
    sb.stage_frames(0, depths, frames_u32=packed)
    sb.append_memory(4, motions=[IDENT] * 4, streams=[1, 2, 1, 1])
    assert _code(lambda: sb.read_pyramid(0, 0)) == ESTATE and _code(lambda: sb.memory_pyramid_time(1)) == ESTATE     # a plain batched memory append
    assert sb.memory_time(1) > 0
    for b, s in enumerate([1, 2, 1, 1]):
        scenes[s].append_memory(depths[b], frame_u32=packed[b])
    depths, packed, _ = _call_frames(oracle, H, W, 1, 4)
    sb.stage_frames(0, depths, frames_u32=packed)
    streams, kw = [1, 2, 1], dict(levels=3, radius=3, refine=1, keep=250)
    sb.append_memory_pyramid(3, candidates=[THREE] * 3, streams=streams, **kw)
    for b, s in enumerate(streams):
        scenes[s].append_memory_pyramid(depths[b], frame_u32=packed[b], candidates=THREE, **kw)
    frames = [sb.read(b) for b in range(3)]
    mems = {s: sb.read_memory(s) for s in (1, 2)}
    motions, tabs, levels = [sb.read_motion(b) for b in range(3)], [sb.read_frame_memory_balls(b) for b in range(3)], [_levels_of(sb, b, 3) for b in range(3)]
    assert motions[2]["score"][0] > 0 and levels[2][3]["scores"].shape == (3, 7, 7) and levels[2][0]["scores"].shape == (4, 3, 3)
    ms, ms_search = sb.memory_pyramid_time(3)
    assert ms > 0 and 0 < ms_search < ms
    for b in range(3):
        _same(sb.read(b), frames[b], ("pyramid time", b))
        again = sb.read_motion(b)
        assert all(np.array_equal(again[k], motions[b][k]) for k in again) and np.array_equal(sb.read_frame_memory_balls(b), tabs[b])
        assert _same_levels(_levels_of(sb, b, 3), levels[b])
    for s in (1, 2):
        _same(sb.read_memory(s), mems[s], ("pyramid time bank", s))
    for call in (lambda: sb.time(2), lambda: sb.memory_time(2), lambda: sb.memory_search_time(2)):
        _raises(call, ESTATE, "yh_scene_batch_memory_pyramid_time")
    _raises(lambda: sb.read_motion(0, scores=True), EINVAL, "yh_scene_batch_pyramid_read")          # the level tables have a call of their own
    for frame, level in ((0, -1), (0, 4), (3, 0), (-1, 0)):
        assert _code(lambda: sb.read_pyramid(frame, level)) == EINVAL, (frame, level)
    f = C.c_float()
    L = sb.L
    assert L.yh_scene_batch_memory_pyramid_time(sb.h, 0, C.byref(f), C.byref(f)) == EINVAL and L.yh_scene_batch_memory_pyramid_time(None, 1, C.byref(f), C.byref(f)) == EINVAL
    assert L.yh_scene_batch_memory_pyramid_time(sb.h, 1, None, C.byref(f)) == EINVAL and L.yh_scene_batch_memory_pyramid_time(sb.h, 1, C.byref(f), None) == EINVAL
    assert L.yh_scene_batch_pyramid_read(None, 0, 0, None, None, None) == EINVAL and L.yh_scene_batch_pyramid_read(sb.h, 0, 0, None, None, None) == OK
    # a search call after a pyramid call continues the same streams' memories
    sb.append_memory_search(3, candidates=[THREE] * 3, streams=streams, radius=2)
    for b, s in enumerate(streams):
        scenes[s].append_memory_search(depths[b], frame_u32=packed[b], candidates=THREE, radius=2)
    for s in (1, 2):
        _same(sb.read_memory(s), scenes[s].read_memory(), ("search after pyramid", s))
    assert sb.memory_search_time(1)[0] > 0 and sb.read_motion(2, scores=True)["scores"].shape == (3, 5, 5)
    assert _code(lambda: sb.read_pyramid(0, 0)) == ESTATE and _code(lambda: sb.memory_pyramid_time(1)) == ESTATE     # a search append ends the state
    # refused as yh_scene_batch_memory_search_time refuses: a slot staged since, a memory reset since; the tables stay readable until a reset
    sb.append_memory_pyramid(3, candidates=[THREE] * 3, streams=streams, levels=1, radius=1, refine=0)
    assert sb.memory_pyramid_time(1)[0] > 0 and sb.read_pyramid(1, 1)["scores"].shape == (3, 3, 3) and sb.read_pyramid(1, 0)["scores"].shape == (4, 1, 1)
    chosen = sb.read_motion(1)["chosen"]
    sb.stage_frames(0, depths, frames_u32=packed)
    assert _code(lambda: sb.memory_pyramid_time(1)) == ESTATE and np.array_equal(sb.read_motion(1)["chosen"], chosen) and sb.read_pyramid(1, 0)["sum_n"] > 0
    sb.append_memory_pyramid(3, candidates=[THREE] * 3, streams=streams, levels=1, radius=1, refine=0)
    sb.memory_reset(2)
    assert _code(lambda: sb.memory_pyramid_time(1)) == ESTATE and _code(lambda: sb.read_pyramid(0, 0)) == ESTATE
    sb.append_memory_pyramid(3, candidates=[THREE] * 3, streams=streams, levels=1, radius=1, refine=0)
    sb.append(3, ya.COMPAT_SANE)                                                                     # a plain append: its own hook again, no motions or tables
    assert sb.time(2) > 0 and _code(lambda: sb.read_motion(0)) == ESTATE and _code(lambda: sb.memory_pyramid_time(1)) == ESTATE and _code(lambda: sb.read_pyramid(0, 0)) == ESTATE
    _close(sb, scenes)


@pytest.mark.gpu
def test_refusals_touch_nothing(built, oracle):
    import yolact_amd as ya
    from yolact_amd.capi import EINVAL, ESTATE, _p
    H, W = 37, 53
    start = ((W * 5) // 8, H - 1)
    sb = ya.SceneBatch(W, H, 3)
    L, h = sb.L, sb.h
    depths, packed, _ = _call_frames(oracle, H, W, 0, 2)
    sb.stage_frames(0, depths, frames_u32=packed)
    sb.append_memory_pyramid(2, candidates=[THREE] * 2, streams=[7, 2], levels=2, radius=2, refine=1)
    sb.append_memory_pyramid(2, candidates=[THREE] * 2, streams=[2, 7], levels=2, radius=2, refine=1)   # frame 1 on stream 7 remembers frame 0's balls of the first call
    assert sb.plan(None, starts=[start] * 2) == [0, 0]
    frames, plans = [sb.read(b) for b in range(2)], [sb.read_plan(b) for b in range(2)]
    mems, tabs = [sb.read_memory(s) for s in (2, 7)], [sb.read_frame_memory_balls(b) for b in range(2)]
    motions, levels = [sb.read_motion(b) for b in range(2)], [_levels_of(sb, b, 2) for b in range(2)]
    g = np.tile(np.array(R.IDENTITY, np.int32), (3, 2, 1))                                          # [3 frames][2 bases][6]
    st = np.array([2, 7, 0], np.int32)
    call = lambda hh=h, n=2, s=st, n_rot=2, gg=g, cc=g, lv=2, radius=2, refine=1, keep=224, age=30: L.yh_scene_batch_append_memory_pyramid(
        hh, n, None if s is None else _p(s), n_rot, None if gg is None else _p(gg), None if cc is None else _p(cc), lv, radius, refine, keep, age)
    err = lambda: L.yh_scene_batch_last_error(h)
    assert call(hh=None) == EINVAL and call(gg=None) == EINVAL and call(cc=None) == EINVAL
    assert call(n=0) == EINVAL and call(n=4) == EINVAL and call(n=-1) == EINVAL
    assert call(n_rot=0) == EINVAL and call(n_rot=16) == EINVAL and call(n_rot=-1) == EINVAL and call(lv=0) == EINVAL and call(lv=4) == EINVAL
    assert call(radius=-1) == EINVAL and call(radius=9) == EINVAL and call(refine=-1) == EINVAL and call(refine=9) == EINVAL
    assert call(keep=-1) == EINVAL and call(keep=257) == EINVAL and call(age=-1) == EINVAL and call(age=256) == EINVAL
    for bad in (-1, 64):
        assert call(s=np.array([2, bad, 0], np.int32)) == EINVAL and b"frame 1" in err()
    assert call(n=3) == ESTATE and b"slot 2" in err()                                                # slot 2 was never staged
    # an int32 condition broken in the last frame's last base only: each of the four, the text naming frame and base
    T0 = P.reach(2, 2, 1)[0]
    top = I32_MAX - T0 * Q
    for which, row in (("g", (Q, 0, top + 1, 0, Q, 0)), ("g", (Q, 0, 0, 0, Q, -top - 1)), ("c", (Q, Q, I32_MAX - 2 * T0 * Q + 1, 0, Q, 0)),
                       ("c", (Q, 0, 0, -Q, 2 * Q, -(I32_MAX - 3 * T0 * Q + 1)))):
        bad = g.copy()
        bad[1, 1] = row
        assert not P.bases_ok([tuple(r) for r in (bad if which == "g" else g)[1].tolist()], [tuple(r) for r in (bad if which == "c" else g)[1].tolist()], 2, 2, 1)
        assert (call(gg=bad) if which == "g" else call(cc=bad)) == EINVAL and b"frame 1" in err() and b"base 1" in err(), row
    # a coarse level alone refuses: frame, base and level are named; the same 32770 further in is taken by every level
    coarse, coarse_in = g.copy(), g.copy()
    coarse[1, 1], coarse_in[1, 1] = COARSE_ALONE, COARSE_ALONE[:2] + (COARSE_ALONE[2] + 32770,) + COARSE_ALONE[3:]
    assert call(gg=coarse, lv=1, radius=8, refine=0) == EINVAL and b"frame 1" in err() and b"base 1" in err() and b"level 1" in err()
    inside_g, inside_c = g.copy(), g.copy()                                                         # the same offsets one step inside: taken (below)
    inside_g[1, 1], inside_c[1, 1] = (Q, 0, top, 0, Q, -top), (Q, Q, I32_MAX - 2 * T0 * Q, -Q, 2 * Q, -(I32_MAX - 3 * T0 * Q))
    for b in range(2):
        _same(sb.read(b), frames[b], ("refused", b))
        _same(sb.read_plan(b), plans[b], ("refused plan", b))                                       # not a new frame generation: the plan is still readable
        assert np.array_equal(sb.read_frame_memory_balls(b), tabs[b])
        again = sb.read_motion(b)
        assert all(np.array_equal(again[k], motions[b][k]) for k in again) and _same_levels(_levels_of(sb, b, 2), levels[b])
    for s, m in zip((2, 7), mems):
        _same(sb.read_memory(s), m, ("refused memory", s))
    assert not sb.read_memory(0)["map"].any()
    assert call(gg=inside_g, cc=inside_c) == 0 and _code(lambda: sb.read_plan(0)) == ESTATE          # a new frame generation: the plan is of earlier frames
    assert tuple(sb.read_motion(1)["chosen"].tolist()) == (0, 0, 0)                                 # (the edge base reads nothing: the identity's tie wins)
    assert call(gg=coarse_in, lv=1, radius=8, refine=0) == 0 and tuple(sb.read_motion(1)["chosen"].tolist())[0] == 0
    sb.close()


# the ceiling of the cost test, from the single handle alone (see the test): 1.0 + its own spread, 0.22 %, + the 3 % between boxes
CEILING = 1.032


@pytest.mark.gpu
def test_batched_pyramid_costs_no_more_per_frame_than_the_single_handle(built):
    """At 640 x 480 and n = 8, (n_rot, levels, radius, refine) = (5, 3, 8, 1), the robots + balls frame of tools/time_scene.py in every
    slot, memories filled, the tool's prior with bases 0.01 rad apart, in this process: yh_scene_batch_memory_pyramid_time per frame
    against yh_scene_memory_pyramid_time's first figure on a single handle, alternated, one warm-up each, the median of five runs of
    30 replays, in both columns: a stream per frame (the frames share every launch) and all frames on one stream (eight rounds of ten
    launches). The batch must not cost more per frame than the single handle.
    Ceiling 1.032 = 1.0 + the single handle's own run-to-run spread in that measurement, 0.22 % ((max - min) / median of its five
    runs, profiles/scene_batch_pyramid_timings.txt, 2026-10-20) + the 3 % by which the pool's boxes differ - the derivation of
    test_batched_search_costs_no_more_per_frame_than_the_single_handle: nothing here comes from the batch's own figures. Measured
    there: 0.2084 / 0.3258 ms per frame against 0.4145, ratios 0.503 / 0.786 - both columns meet it, so both are bounded. The other
    batch sizes are recorded there and in DESIGN.md, not bounded here."""
    import yolact_amd as ya
    H, W, n = 480, 640, 8
    depth = np.random.default_rng(0).integers(200, 4000, (H, W)).astype(np.uint16)
    ci = np.zeros((H, W, 2), np.uint8)
    ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
    prior = (3.0, -2.0, 0.05)
    motion = ya.scene_motion(*prior)
    cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=2)
    kw = dict(levels=3, radius=8, refine=1)
    single = ya.Scene(W, H)
    single.append_memory(depth, cls_id=ci, motion=motion)
    single.append_memory_pyramid(depth, cls_id=ci, candidates=cands, **kw)
    for name, streams in (("a stream per frame", list(range(n))), ("all on one stream", None)):
        sb = ya.SceneBatch(W, H, n)
        sb.stage_frames(0, np.stack([depth] * n), frames_u32=np.stack([ya.SceneBatch.pack(ci)] * n))
        sb.append_memory(n, motions=[motion] * n, streams=streams)
        sb.append_memory_pyramid(n, candidates=[cands] * n, streams=streams, **kw)
        single.memory_pyramid_time(30); sb.memory_pyramid_time(30)
        ts, tb, tr = [], [], []
        for _ in range(5):
            ts.append(single.memory_pyramid_time(30)[0])
            a, b = sb.memory_pyramid_time(30)
            tb.append(a / n); tr.append(b / n)
        ratio = float(np.median(tb) / np.median(ts))
        print(f"scene pyramid 640x480, n = {n}, (5, 3, 8, 1), {name}: single {np.median(ts):.4f} ms, batch {np.median(tb):.4f} ms per frame (registration alone {np.median(tr):.4f}), "
              f"ratio {ratio:.3f}, spread of the single handle {100 * (max(ts) - min(ts)) / np.median(ts):.2f} %")
        assert ratio <= CEILING, (name, ts, tb)
        sb.close()
    single.close()
