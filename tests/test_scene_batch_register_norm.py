"""The scene batch's normalised registration (DESIGN.md §11 "Scene batch: normalised registration"):
yh_scene_batch_append_memory_search_norm is n yh_scene_append_memory_search_norm calls in batch order, frame b on the memory of
streams[b] - so a stream's later frame is scored, by the normalised score, against what its earlier frame has just fused. CPU part:
the surface, the restated bank (tests/scene_batch_register_norm_ref.py) against answers worked out by hand, and chained sequences over
dense terrain which the normalised bank registers and the plain bank does not. GPU part (-m gpu): every output, table, memory, motion,
T and C table and record bit for bit against the restatement fed the oracle's SANE stamps AND against real Scene handles, one per
stream, driven with append_memory_search_norm in batch order; the planners on the fused frames; the replay hook and the state matrix of
the reads and hooks; every refusal; and the cost per frame against the single handle's normalised search append.
The helpers here take a FORM - how one of the two normalised batched appends is called, restated and read - and serve
test_scene_batch_pyramid_norm.py too."""
import inspect
import os
import re

import numpy as np
import pytest

import scene_batch_memory_ref as BR
import scene_batch_register_norm_ref as BN
import scene_batch_register_ref as BG
import scene_memory_ref as R
import scene_register_norm_ref as GN
import scene_register_ref as G
from test_scene_batch_memory import N, PATTERNS, _call_frames, _code, _packed, _same
from test_scene_batch_register import OUTSIDE, PRIORS, SHAPES, THREE, _close
from test_scene_memory import IDENT, _DeviceFrame, _stamps, shift
from test_scene_register import I32_MAX, Q, ROTATION, SHEARED, _bases, _edge, _lds_words, _window_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS_PUBLIC = [
    "int yh_scene_batch_append_memory_search_norm(yh_scene_batch* h, int32_t n_frames, const int32_t* streams, int32_t n_rot, const int32_t* gather_q16, "
    "const int32_t* carry_q16, int32_t radius, int32_t min_inside, int32_t keep, int32_t ball_max_age);",
    "int yh_scene_batch_motion_norm_read(yh_scene_batch* h, int32_t frame, uint64_t* totals, uint64_t* inside, uint64_t* chosen_stc, uint64_t* prior_stc, int32_t* qualified);",
    "int yh_scene_batch_append_memory_pyramid_norm(yh_scene_batch* h, int32_t n_frames, const int32_t* streams, int32_t n_rot, const int32_t* gather_q16, "
    "const int32_t* carry_q16, int32_t levels, int32_t radius, int32_t refine, int32_t min_inside, int32_t keep, int32_t ball_max_age);",
    "int yh_scene_batch_pyramid_norm_read(yh_scene_batch* h, int32_t frame, int32_t level, int32_t* centres, uint64_t* scores, uint64_t* totals, uint64_t* inside, "
    "uint64_t* sum_n, int32_t* level_min_inside, int32_t* qualified);"]
DECLS_DEBUG = ["int yh_scene_batch_memory_search_norm_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, float* ms_search);",
               "int yh_scene_batch_memory_pyramid_norm_time(yh_scene_batch* h, int32_t reps, float* ms_per_batch, float* ms_search);"]
HOOK, PYRAMID_HOOK = "yh_scene_batch_memory_search_norm_time", "yh_scene_batch_memory_pyramid_norm_time"


class Flat:
    """the flat form: params = radius"""
    name, hook, largest = "search_norm", HOOK, 8
    Bank = BN.Bank

    @staticmethod
    def append(sb, n, cands, streams, params, mi, keep=224, age=30):
        sb.append_memory_search_norm(n, candidates=cands, streams=streams, radius=params, min_inside=mi, keep=keep, ball_max_age=age)

    @staticmethod
    def restate(bank, stamps, balls, streams, cands, params, mi, keep=224, age=30):
        return bank.append_search_norm(stamps, balls, streams, cands, params, mi, keep, age)

    @staticmethod
    def single(sc, depth, packed, cands, params, mi, keep=224, age=30):
        sc.append_memory_search_norm(depth, frame_u32=packed, candidates=cands, radius=params, min_inside=mi, keep=keep, ball_max_age=age)

    @staticmethod
    def read(h, b=None):
        """everything the reads return for frame b of a batch (b None: of a Scene), a flat dict"""
        at = () if b is None else (b,)
        out = dict(h.read_motion(*at, scores=True))
        out.update(h.read_motion_norm(*at))
        return out

    @staticmethod
    def check(got, want, what):
        """the reads against what scene_register_norm_ref.search returns"""
        assert got["gather"].dtype == got["carry"].dtype == got["chosen"].dtype == np.int32, what
        assert all(got[k].dtype == np.uint64 for k in ("score", "scores", "totals", "inside", "chosen_stc", "prior_stc")), what
        assert tuple(got["chosen"].tolist()) == want["chosen"] and tuple(got["gather"].tolist()) == want["gather"] and tuple(got["carry"].tolist()) == want["carry"], (what, got["chosen"], want["chosen"])
        assert tuple(int(v) for v in got["score"]) == want["score"], what
        for k in ("scores", "totals", "inside"):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), what + (k,)
        assert tuple(int(v) for v in got["chosen_stc"]) == want["chosen_stc"] and tuple(int(v) for v in got["prior_stc"]) == want["prior_stc"], what
        assert got["qualified"] is want["qualified"], what

    @staticmethod
    def table0(m):
        return m["scores"]

    @staticmethod
    def time(h, reps):
        return h.memory_search_norm_time(reps)


def _equal(a, b):
    """two dicts of reads, bit for bit"""
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def _run_call(form, sb, bank, scenes, frames, streams, cands, params, mi, keep, max_age, what, restated=None):
    """One batched normalised call against the restated bank (or its result, if computed before) and against Scene handles, one per
    stream, driven with the single normalised append in batch order; returns (the batch's per-frame outputs, the restated motions)."""
    import yolact_amd as ya
    depths, packed, ora = frames
    n, H, W = len(ora), sb.H, sb.W
    sb.stage_frames(0, depths, frames_u32=packed)
    form.append(sb, n, cands, streams, params, mi, keep, max_age)
    want, tables, motions = restated or form.restate(bank, [o["map"] for o in ora], [o["balls"] for o in ora], streams, cands, params, mi, keep, max_age)
    got = []
    for b in range(n):
        s = 0 if streams is None else streams[b]
        got.append(sb.read(b))
        _same(got[b], want[b], what + ("ref", b))
        tab = sb.read_frame_memory_balls(b)
        assert tab.dtype == np.int32 and np.array_equal(tab, tables[b]), what + ("table", b)
        motion = form.read(sb, b)
        form.check(motion, motions[b], what + ("motion", b))
        if scenes is not None:
            if s not in scenes:
                scenes[s] = ya.Scene(W, H)
            sc = scenes[s]
            form.single(sc, depths[b], packed[b], cands[b] if cands else None, params, mi, keep, max_age)
            _same(got[b], sc.read(), what + ("scene", b))
            assert np.array_equal(tab, sc.read_memory()["balls"]), what + ("scene table", b)
            assert _equal(motion, form.read(sc)), what + ("scene motion", b)
    for s in set([0] if streams is None else streams):
        mem = sb.read_memory(s)
        assert mem["map"].dtype == np.uint32 and np.array_equal(mem["map"], bank.mem[s].M) and np.array_equal(mem["balls"], bank.mem[s].B), what + ("bank", s)
        if scenes is not None:
            _same(mem, scenes[s].read_memory(), what + ("scene bank", s))
    return got, motions


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
    for decl in DECLS_PUBLIC:
        assert re.search(r"(?<![\w])" + re.escape(decl), pub_code), decl
        assert decl.split("(")[0].split()[-1] + "(" not in dbg_code, decl
    for decl in DECLS_DEBUG:
        assert re.search(r"(?<![\w])" + re.escape(decl), dbg_code), decl
        assert decl.split("(")[0].split()[-1] not in pub, decl
    # sections of their own behind the scene batch's, under their comment lines
    marks = ["int yh_scene_batch_pyramid_read(", "---- batched normalised registration (DESIGN.md section 11 \"Scene batch: normalised registration\")",
             "int yh_scene_batch_append_memory_search_norm(", "int yh_scene_batch_motion_norm_read(",
             "---- batched normalised pyramid registration (DESIGN.md section 11 \"Scene batch: normalised pyramid registration\")",
             "int yh_scene_batch_append_memory_pyramid_norm(", "int yh_scene_batch_pyramid_norm_read("]
    at = [pub.index(m) for m in marks]
    assert at == sorted(at)
    protos = dict((s[0], s) for s in capi.SYMBOLS)
    _i, _vp, _fp = capi.C.c_int32, capi.C.c_void_p, capi.C.POINTER(capi.C.c_float)
    assert protos["yh_scene_batch_append_memory_search_norm"][1:] == (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i])
    assert protos["yh_scene_batch_motion_norm_read"][1:] == (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp])
    assert protos["yh_scene_batch_append_memory_pyramid_norm"][1:] == (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i])
    assert protos["yh_scene_batch_pyramid_norm_read"][1:] == (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
    for name in (HOOK, PYRAMID_HOOK):
        assert protos[name][1:] == (_i, [_vp, _i, _fp, _fp])
    sig = inspect.signature(capi.SceneBatch.append_memory_search_norm)
    assert list(sig.parameters) == ["self", "n", "candidates", "streams", "radius", "min_inside", "keep", "ball_max_age"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, None, 4, None, 224, 30]
    sig = inspect.signature(capi.SceneBatch.append_memory_pyramid_norm)
    assert list(sig.parameters) == ["self", "n", "candidates", "streams", "levels", "radius", "refine", "min_inside", "keep", "ball_max_age"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, None, 3, 8, 1, None, 224, 30]
    assert list(inspect.signature(capi.SceneBatch.read_motion_norm).parameters) == ["self", "frame"]
    assert list(inspect.signature(capi.SceneBatch.read_pyramid_norm).parameters) == ["self", "frame", "level"]
    for hook in (capi.SceneBatch.memory_search_norm_time, capi.SceneBatch.memory_pyramid_norm_time):
        sig = inspect.signature(hook)
        assert list(sig.parameters) == ["self", "reps"] and sig.parameters["reps"].default == 20
    assert all(hasattr(ya.SceneBatch, k) for k in ("append_memory_search_norm", "read_motion_norm", "append_memory_pyramid_norm", "read_pyramid_norm"))
    assert "#define YH_ABI_VERSION 4" in pub and BN.STREAMS_MAX == capi.SCENE_STREAMS_MAX == ya.SCENE_STREAMS_MAX


def _hand_frames():
    W, H = 4, 3
    Z = np.zeros((H, W), np.uint32)
    A = Z.copy(); A[1, 1] = 100; A[0, 3] = 7
    B = Z.copy(); B[2, 2] = 50
    A1 = Z.copy(); A1[1, 2] = 100                                                                    # A's peak one to the right: the map moved by (1, 0)
    none = np.zeros((100, 4), np.float32)
    seen = none.copy(); seen[7] = (1.5, 2.5, 4, 0)
    return W, H, Z, A, B, A1, none, seen


def test_restated_bank_scores_a_chained_frame_against_its_predecessors_map():
    W, H, Z, A, B, A1, none, seen = _hand_frames()
    one = ([R.IDENTITY], [R.IDENTITY])
    bank = BN.Bank(W, H)
    # frames 0 and 2 on stream 0, frames 1 and 3 on stream 1, min_inside 6. Both streams start empty: against the call-start memory
    # S would be 0 everywhere for frames 2 and 3 and the choice (0, 0, 0); only against frame 0's fused map does frame 2 find its shift.
    out, tabs, mot = bank.append_search_norm([A, B, A1, B], [seen, none, none, none], [0, 1, 0, 1], [one] * 4, 1, 6, 128, 2)
    # an empty memory: S = 0, T = the frame's own sum over the inside pixels, every ratio 0: the nearest qualified candidate, (0, 0, 0)
    assert mot[0]["chosen"] == mot[1]["chosen"] == (0, 0, 0) and mot[0]["score"] == (0, 0, 107) and mot[0]["qualified"] and not mot[1]["scores"].any()
    assert mot[0]["chosen_stc"] == mot[0]["prior_stc"] == (0, 107, 12) and mot[1]["chosen_stc"] == (0, 50, 12)
    # by hand. N has 100 at (2, 1): S(u, v) = min(100, A[1 + v][2 + u]) - 100 at (-1, 0), 7 at (1, -1). C(u, v) = (4 - |u|)(3 - |v|).
    # At (-1, 0) the inside pixels are columns 1 .. 3, their sources columns 0 .. 2 of A: T = 100 + 100, U = 100 = S - ratio 1.
    # At (1, -1): columns 0 .. 2 of rows 1 .. 2, sources columns 1 .. 3 of rows 0 .. 1: T = 100 + 107. At (0, 0): T = 100 + 107, S = 0.
    m = mot[2]
    S = np.zeros((1, 3, 3), np.uint64); S[0, 1, 0] = 100; S[0, 0, 2] = 7
    assert np.array_equal(m["scores"], S) and np.array_equal(m["inside"][0], np.array([[6, 8, 6], [9, 12, 9], [6, 8, 6]], np.uint64))
    assert m["totals"][0, 1, 0] == 200 and m["totals"][0, 0, 2] == 207 and m["totals"][0, 1, 1] == 207
    assert m["chosen"] == (0, -1, 0) and m["score"] == (100, 0, 100) and m["chosen_stc"] == (100, 200, 9) and m["prior_stc"] == (0, 207, 12) and m["qualified"]
    assert m["gather"] == shift(1, 0)[0] and m["carry"] == shift(1, 0)[1]
    # frame 3 is frame 1 again, against frame 1's own map: the identity at ratio 1, the stream-0 frames between them nothing to it
    assert mot[3]["chosen"] == (0, 0, 0) and mot[3]["score"] == (50, 50, 50) and mot[3]["chosen_stc"] == (50, 100, 12)
    f2 = Z.copy(); f2[1, 2] = 100                                                                    # A moved right (its corner pixel leaves), halved: 50 < 100
    assert np.array_equal(out[2]["map"], f2) and np.array_equal(bank.mem[0].M, f2) and np.array_equal(bank.mem[1].M, B)
    assert tabs[2][7].tolist() == [2, 2, 4, 1] and out[2]["balls"][7].tolist() == [2, 2, 4, 0]     # the ball carried by the CHOSEN carry, one to the right
    # min_inside from both sides of C(-1, 0) = 9, per call: at 9 the shift qualifies, at 10 only (0, 0, 0) does (C = 12) and is chosen
    for mi, chosen in ((9, (0, -1, 0)), (10, (0, 0, 0))):
        other = BN.Bank(W, H)
        _, _, mo = other.append_search_norm([A, A1], [none, none], [3, 3], [one] * 2, 1, mi, 128, 2)
        assert mo[1]["chosen"] == chosen and mo[1]["qualified"], mi
    other = BN.Bank(W, H)                                                                            # nothing qualifies: the prior, qualified False
    _, _, mo = other.append_search_norm([A, A1], [none, none], [3, 3], [([shift(-1, 0)[0]], [shift(-1, 0)[1]])] * 2, 0, 10, 128, 2)
    assert mo[1]["chosen"] == (0, 0, 0) and not mo[1]["qualified"] and mo[1]["chosen_stc"][2] == 9
    # the next call continues the streams: frame A1 again on stream 0 now sits where the memory has it; reset empties
    out, tabs, mot = bank.append_search_norm([A1], [none], [0], [one], 1, 6, 256, 2)
    assert mot[0]["chosen"] == (0, 0, 0) and mot[0]["score"] == (100, 100, 100) and tabs[0][7].tolist() == [2, 2, 4, 2]
    bank.reset(0)
    assert not bank.mem[0].M.any() and not bank.mem[0].B.any() and bank.mem[1].M.any()
    bank.reset()
    assert not bank.mem[1].M.any()


def _plain_bank_case(form, params):
    rng = np.random.default_rng(9)
    W, H = 4, 3
    stamps = [rng.integers(0, 300, (H, W)).astype(np.uint32) for _ in range(5)]
    balls = [np.zeros((100, 4), np.float32) for _ in range(5)]
    balls[0][3] = (2.5, 1.5, 6, 0)
    motions = [IDENT, shift(1, 0), shift(0, 1), IDENT, shift(-1, 1)]
    streams = [2, 0, 2, 2, 0]
    a, b = form.Bank(W, H), BR.Bank(W, H)
    for keep, mi in ((224, 1), (200, 12)):                                                           # (whether the one candidate qualifies changes nothing)
        got, tabs, mot = form.restate(a, stamps, balls, streams, [([g], [c]) for g, c in motions], params, mi, keep, 3)
        want, wtabs = b.append(stamps, balls, streams, motions, keep, 3)
        for i in range(5):
            _same(got[i], want[i], ("plain", keep, i))
            assert np.array_equal(tabs[i], wtabs[i]) and mot[i]["chosen"] == (0, 0, 0) and (mot[i]["gather"], mot[i]["carry"]) == motions[i]
        for s in (0, 2):
            assert np.array_equal(a.mem[s].M, b.mem[s].M) and np.array_equal(a.mem[s].B, b.mem[s].B)
    assert a.mem[2].M.any() and a.mem[2].B[3, 2] == 6


def test_restated_bank_with_one_candidate_and_no_search_is_the_plain_bank():
    _plain_bank_case(Flat, 0)


# dense terrain, chained: the twelve-sinusoid field of test_scene_pyramid_norm.py's _dense with a pad of 48, four windows at cumulative
# offsets fed to one stream in order; noise per frame from default_rng(100 + seed)
_CHAIN = {}


def _chain(H, W, steps, seed, noise):
    key = (H, W, tuple(steps), seed, noise)
    if key not in _CHAIN:
        rng = np.random.default_rng(seed)
        pad = 48
        yy, xx = np.mgrid[0:H + 2 * pad, 0:W + 2 * pad].astype(np.float64)
        f = np.zeros_like(yy)
        for _ in range(12):
            fx, fy, amp, ph = rng.uniform(-0.06, 0.06), rng.uniform(-0.06, 0.06), rng.uniform(0.3, 1.0), rng.uniform(0, 2 * np.pi)
            f += amp * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph)
        F = np.rint(200 + (f - f.min()) / (f.max() - f.min()) * 7000).astype(np.int64)
        jitter = np.random.default_rng(100 + seed)
        frames, x, y = [], 0, 0
        for u, v in [(0, 0)] + list(steps):
            x, y = x + u, y + v
            assert max(abs(x), abs(y)) <= pad
            n = F[pad + y:pad + y + H, pad + x:pad + x + W]
            if noise:
                n = np.maximum(n + jitter.integers(-noise, noise + 1, n.shape), 1)
            frames.append(n.astype(np.uint32))
        _CHAIN[key] = frames
    return _CHAIN[key]


FLAT_STEPS = {(65, 130): [(5, -7), (-8, 6), (7, 7)], (53, 37): [(-4, 8), (6, -5), (3, 3)]}
NO_BALLS = [np.zeros((100, 4), np.float32)] * 4


@pytest.mark.parametrize("noise", [0, 300])
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("H,W", list(FLAT_STEPS))
def test_dense_chained_sequences_are_registered_by_the_normalised_bank_alone(H, W, seed, noise):
    """keep = 256, identity prior, radius 8, min_inside = W H // 4: the normalised bank chooses every step of all 12 sequences. The
    plain bank finds all three steps in one of them only (65 x 130, seed 1, no noise) and none at 53 x 37 or under noise: its miss is
    asserted on those rows."""
    steps = FLAT_STEPS[H, W]
    frames = _chain(H, W, steps, seed, noise)
    _, _, mot = BN.Bank(W, H).append_search_norm(frames, NO_BALLS, None, None, 8, None, 256, 30)
    assert [m["chosen"] for m in mot[1:]] == [(0,) + s for s in steps] and all(m["qualified"] for m in mot)
    if (H, W) == (53, 37) or noise:
        _, _, plain = BG.Bank(W, H).append_search(frames, NO_BALLS, None, None, 8, 256, 30)
        assert all(p["chosen"] != (0,) + s for p, s in zip(plain[1:], steps)), [p["chosen"] for p in plain]


_WRONG = {}


def _wrong_priors(form, oracle, H, W, priors, params):
    """case 1 on the restatement, computed once per form and shape: (the frames, (per-frame outputs, tables, motions), the bank)"""
    if (form.name, H, W) not in _WRONG:
        frames = _packed([_stamps(oracle, H, W, 2)] * 4)
        bank = form.Bank(W, H)
        o = frames[2][0]
        out = form.restate(bank, [o["map"]] * 4, [o["balls"]] * 4, None, [([g], [c]) for g, c in priors], params, None, 256, 30)
        _WRONG[form.name, H, W] = (frames, out, bank)
    return _WRONG[form.name, H, W]


WRONG_CHOSEN = [(0, 0, 0), (0, 3, -2), (0, -1, 4), (0, 2, 2)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_same_frame_wrong_priors_restated(oracle, H, W):
    """Frame 0 meets an empty memory; every later frame is the frame its predecessor fused (keep = 256: the memory IS the frame's
    stamps), so its wrong prior is corrected to the identity, at S = U - which the call-start memory, empty, could never tell it."""
    _, (_, _, mot), _ = _wrong_priors(Flat, oracle, H, W, PRIORS, 4)
    assert [m["chosen"] for m in mot] == WRONG_CHOSEN and mot[0]["score"][2] > 0 and not mot[0]["scores"].any()
    for m in mot[1:]:
        s, t, c = m["chosen_stc"]
        assert m["gather"] == R.IDENTITY and m["carry"] == R.IDENTITY and m["qualified"] and t - s == s > 0 and c == W * H


_CASE2 = {}


def _case2(form, oracle, H, W, params, plain):
    """case 2 with all frames on one stream, on the restatement and on the plain bank: the two calls' (motions, plain motions, the
    map the call started from)"""
    if (form.name, H, W) not in _CASE2:
        bank, calls = form.Bank(W, H), []
        for k, keep in enumerate((224, 200)):
            start = bank.mem[9].M.copy()
            ora = _call_frames(oracle, H, W, k)[2]
            stamps, balls = [o["map"] for o in ora], [o["balls"] for o in ora]
            _, _, mot = form.restate(bank, stamps, balls, PATTERNS["one"], [THREE] * N, params, None, keep, 5)
            calls.append((mot, plain(k, stamps, balls, keep), start))
        _CASE2[form.name, H, W] = calls
    return _CASE2[form.name, H, W]


_PLAIN2 = {}


def _plain_search_bank(k, stamps, balls, keep):
    bank = _PLAIN2.setdefault("flat", BG.Bank(9, 100))
    return bank.append_search(stamps, balls, PATTERNS["one"], [THREE] * N, 2, keep, 5)[2]


def test_case_2_on_one_stream_the_normalised_bank_chooses_otherwise_than_the_plain_bank(oracle):
    """On the frames of case 2 at 100 x 9, all on one stream: some chained frame (rank >= 1 in its call) is registered otherwise by
    the normalised bank than by the plain one - the batched normalised append is not the plain one under another name. (At 37 x 53
    and 9 x 130 the two agree on these frames, for the seeds of this case and for eleven further sets tried.)"""
    calls = _case2(Flat, oracle, 100, 9, 2, _plain_search_bank)
    assert any(m["chosen"] != p["chosen"] for mot, plain, _ in calls for m, p in list(zip(mot, plain))[1:])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def wrong_priors_on_the_device(form, oracle, H, W, priors, params, chosen):
    import yolact_amd as ya
    frames, restated, bank = _wrong_priors(form, oracle, H, W, priors, params)
    assert chosen is None or ([m["chosen"] for m in restated[2]] == chosen and all(m["gather"] == R.IDENTITY for m in restated[2][1:]))
    sb, scenes = ya.SceneBatch(W, H, 4), {}
    _run_call(form, sb, bank, scenes, frames, None, [([g], [c]) for g, c in priors], params, None, 256, 30, ("wrong priors", H, W), restated=restated)
    _close(sb, scenes)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
def test_same_frame_wrong_priors(built, oracle, H, W):
    """Case 1. An implementation that scores a chained frame against the call-start (empty) memory, or hands a frame another frame's
    tables or records, cannot pass: the three corrections differ and none is (0, 0, 0)."""
    wrong_priors_on_the_device(Flat, oracle, H, W, PRIORS, 4, WRONG_CHOSEN)


def distinct_frames_on_the_device(form, oracle, H, W, pattern, params, against_start):
    import yolact_amd as ya
    streams = PATTERNS[pattern]
    sb, bank, scenes = ya.SceneBatch(W, H, N), form.Bank(W, H), {}
    for k, keep in enumerate((224, 200)):
        start = bank.mem[9].M.copy()
        frames = _call_frames(oracle, H, W, k)
        _, mot = _run_call(form, sb, bank, scenes, frames, streams, [THREE] * N, params, None, keep, 5, (pattern, H, W, k))
        if pattern == "one" and k == 1:
            assert start.any() and any(not np.array_equal(against_start(frames[2][b]["map"], start), form.table0(mot[b])) for b in range(2, N))
    assert any(m["score"][0] > 0 for m in mot) and len(scenes) == len(set(streams or [0]))
    _close(sb, scenes)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("H,W", [(37, 53), (100, 9), (9, 130)])
def test_distinct_frames_equal_the_restatement_and_one_scene_per_stream(built, oracle, H, W, pattern):
    """Case 2: two calls of six distinct frames over the stream patterns of test_scene_batch_memory.py (the second continues every
    stream of the first), three bases per frame, radius 2, keep 224 then 200. With all frames on one stream, some frame of rank >= 2 of
    the second call has an S table against its predecessor's map that differs from its table against the call-start memory."""
    distinct_frames_on_the_device(Flat, oracle, H, W, pattern, 2, lambda n, start: GN.tables(n, start, THREE[0], 2)[0])


@pytest.mark.gpu
def test_the_largest_grid(built, oracle):
    """(radius, n_rot) = (8, 16): sixteen bases of every kind the definition allows, on filled memories, two frames chained."""
    import yolact_amd as ya
    H, W = 37, 53
    sb, bank, scenes = ya.SceneBatch(W, H, 3), BN.Bank(W, H), {}
    _run_call(Flat, sb, bank, scenes, _call_frames(oracle, H, W, 0, 2), [0, 1], None, 0, None, 256, 5, ("fill",))
    gathers = [tuple(g) for g in _bases(H, W, 8)]
    assert len(gathers) == 16 and G.bases_ok(gathers, [R.IDENTITY] * 16, 8)
    _, mot = _run_call(Flat, sb, bank, scenes, _call_frames(oracle, H, W, 1, 3), [0, 0, 1], [(gathers, [R.IDENTITY] * 16)] * 3, 8, None, 224, 5, ("(8, 16)",))
    assert all(m["scores"].shape == (16, 17, 17) and m["scores"].max() > 0 and m["inside"].max() == W * H for m in mot)
    _close(sb, scenes)


@pytest.mark.gpu
def test_edge_bases_and_the_global_memory_fallback_per_frame(built, oracle):
    """At 9 x 130 on filled memories, four frames over two streams: the magnifying shear, whose window of M overflows the LDS budget
    (so the score kernel's global-memory path runs, per frame of a batch), a motion that sends every pixel outside, and coefficients
    on the int32 conditions."""
    import yolact_amd as ya
    H, W, radius = 9, 130, 6                                                                         # (a tile is nine rows here: at radius 5 the shear still fits)
    lds = _lds_words()
    assert _window_words(SHEARED[1], H, W, radius) > lds == 4096 >= _window_words(SHEARED[1], H, W, 5)
    sb, bank, scenes = ya.SceneBatch(W, H, 4), BN.Bank(W, H), {}
    _run_call(Flat, sb, bank, scenes, _call_frames(oracle, H, W, 0, 2), [0, 1], None, 0, None, 256, 5, ("fill",))
    gathers = [SHEARED[1], OUTSIDE(W), _edge(radius), _edge(radius, -1), (I32_MAX, -I32_MAX - 1, 0, -I32_MAX - 1, I32_MAX, 0)]
    carries = [SHEARED[0]] + [R.IDENTITY] * 4
    assert G.bases_ok(gathers, carries, radius)
    _, mot = _run_call(Flat, sb, bank, scenes, _call_frames(oracle, H, W, 1, 4), [0, 1, 0, 1], [(gathers, carries)] * 4, radius, 64, 224, 5, ("edges",))
    assert all(m["scores"][0].max() > 0 and not m["inside"][1].any() for m in mot)                  # the shear reads the memory, the motion outside nothing
    # every pixel outside as the only base: nothing qualifies, the prior stands, nothing is gathered
    frames = _call_frames(oracle, H, W, 2, 2)
    got, mot = _run_call(Flat, sb, bank, scenes, frames, [1, 1], [([OUTSIDE(W)], [OUTSIDE(-W)])] * 2, 1, 1, 224, 5, ("outside",))
    assert all(m["chosen"] == (0, 0, 0) and not m["qualified"] and m["score"][:2] == (0, 0) for m in mot) and np.array_equal(got[1]["map"], frames[2][1]["map"])
    _close(sb, scenes)


def _two_shifts(H, W):
    """two bases at radius 0 that keep (W - 2) H and W (H - 1) pixels inside"""
    return ([shift(2, 0)[0], shift(0, 1)[0]], [shift(2, 0)[1], shift(0, 1)[1]]), (W - 2) * H, W * (H - 1)


def qualification_on_the_device(form, oracle, params):
    """Within one round: a frame none of whose candidates qualifies (every pixel outside: the prior, qualified 0) beside one that
    qualifies; then min_inside exactly at, and one above, the larger of two candidates' C."""
    import yolact_amd as ya
    H, W = 37, 53
    sb, bank, scenes = ya.SceneBatch(W, H, 3), form.Bank(W, H), {}
    _run_call(form, sb, bank, scenes, _call_frames(oracle, H, W, 0, 2), [0, 1], None, params, None, 256, 5, ("fill",))
    outside, inside = ([OUTSIDE(W)] * 2, [OUTSIDE(-W)] * 2), ([IDENT[0], shift(1, 0)[0]], [IDENT[1], shift(1, 0)[1]])
    _, mot = _run_call(form, sb, bank, scenes, _call_frames(oracle, H, W, 1, 3), [0, 1, 0], [outside, inside, inside], params, 100, 224, 5, ("one round",))
    assert not mot[0]["qualified"] and mot[0]["chosen"] == (0, 0, 0) and mot[1]["qualified"] and mot[2]["qualified"]
    two, c0, c1 = _two_shifts(H, W)
    assert c0 < c1
    for k, (mi, qualified) in enumerate(((c0, True), (c1, True), (c1 + 1, False))):
        _, mot = _run_call(form, sb, bank, scenes, _call_frames(oracle, H, W, 2 + k, 2), [0, 0], [two] * 2, params, mi, 224, 5, ("min_inside", mi))
        assert all(m["qualified"] is qualified for m in mot) and (qualified or all(m["chosen"] == (0, 0, 0) for m in mot))
        if mi == c1:
            assert all(m["chosen"][0] == 1 for m in mot)                                              # base 0, one pixel column short, is out
    _close(sb, scenes)


@pytest.mark.gpu
def test_qualification_per_frame_within_one_round(built, oracle):
    qualification_on_the_device(Flat, oracle, 0)


@pytest.mark.gpu
def test_at_the_camera_size(built, oracle):
    """The three frames of test_scene_memory.py's camera-size sequence (the oracle's stamps are computed once for all): two on stream 1,
    the ball-less one between them on stream 0."""
    import yolact_amd as ya
    H, W = 480, 640
    frames = _packed([_stamps(oracle, H, W, 10 * H + W + t, balls=t != 1) for t in range(3)])
    sb, bank, scenes = ya.SceneBatch(W, H, 3), BN.Bank(W, H), {}
    cands = ([ROTATION[0], IDENT[0]], [ROTATION[1], IDENT[1]])
    _, mot = _run_call(Flat, sb, bank, scenes, frames, [1, 0, 1], [cands] * 3, 1, None, 224, 5, ("camera",))
    assert mot[2]["score"][0] > 0 and not mot[1]["scores"].any()                                     # frame 2 met frame 0's map, frame 1 an empty stream
    _close(sb, scenes)


def one_slot_and_fewer_frames_on_the_device(form, oracle, params, other):
    import yolact_amd as ya
    H, W = 37, 53
    sb, bank, scenes = ya.SceneBatch(W, H, 1), form.Bank(W, H), {}
    for k in range(3):                                                                                # max_frames = 1: the chain runs through the bank
        _run_call(form, sb, bank, scenes, _call_frames(oracle, H, W, k, 1), [5], [THREE], params, None, 230, 4, ("one slot", k))
    assert _code(lambda: form.append(sb, 2, [THREE] * 2, None, params, None)) == ya.capi.EINVAL
    _close(sb, scenes)
    sb, bank, scenes = ya.SceneBatch(W, H, 4), form.Bank(W, H), {}
    depths, packed, _ = _call_frames(oracle, H, W, 0, 3)
    sb.stage_frames(0, depths, frames_u32=packed)
    with pytest.raises(ya.YhError) as e:                                                              # slot 3 was never staged
        form.append(sb, 4, [THREE] * 4, None, params, None)
    assert e.value.code == ya.capi.ESTATE and "slot 3" in str(e.value)
    _run_call(form, sb, bank, scenes, _call_frames(oracle, H, W, 0, 4), [0, 1, 2, 0], [THREE] * 4, params, None, 240, 9, ("first",))
    before = sb.read_memory(1)
    _run_call(form, sb, bank, scenes, _call_frames(oracle, H, W, 1, 2), [0, 2], [THREE] * 2, other, 300, 240, 9, ("n < max_frames",))
    _same(sb.read_memory(1), before, ("absent stream",))
    assert before["map"].any() and _code(lambda: sb.read(2)) == ya.capi.EINVAL and _code(lambda: sb.read_motion(2)) == ya.capi.EINVAL
    assert _code(lambda: sb.read_motion_norm(2)) == ya.capi.EINVAL
    _close(sb, scenes)


@pytest.mark.gpu
def test_one_slot_batches_and_fewer_frames_than_slots(built, oracle):
    one_slot_and_fewer_frames_on_the_device(Flat, oracle, 2, 3)


def degenerate_forms_on_the_device(form, oracle, wide, none):
    """wide: parameters of a real search; none: the degenerate ones (no search at all)"""
    import yolact_amd as ya
    H, W = 37, 53
    srch, mem, plain = ya.SceneBatch(W, H, 3), ya.SceneBatch(W, H, 3), ya.SceneBatch(W, H, 3)
    # an empty bank, a stream per frame: nothing is carried, whatever is chosen (S = 0 everywhere: the nearest qualified candidate of base 0)
    depths, packed, _ = _call_frames(oracle, H, W, 0, 3)
    for sb in (srch, mem, plain):
        sb.stage_frames(0, depths, frames_u32=packed)
    form.append(srch, 3, [THREE] * 3, [4, 5, 6], wide, None, 256, 255)
    plain.append(3, ya.COMPAT_SANE)
    for b in range(3):
        _same(srch.read(b), plain.read(b), ("empty bank", b))
        assert tuple(srch.read_motion(b)["score"][:2].tolist()) == (0, 0)
    # one base and no search: yh_scene_batch_append_memory with the same motions, two calls on chained streams
    mem.append_memory(3, motions=[(tuple(srch.read_motion(b)["gather"].tolist()), tuple(srch.read_motion(b)["carry"].tolist())) for b in range(3)], streams=[4, 5, 6],
                      keep=256, ball_max_age=255)
    for k in (1, 2):
        depths, packed, _ = _call_frames(oracle, H, W, k, 3)
        motions = [ROTATION, shift(2, -1), shift(-1, 1)]
        for sb in (srch, mem):
            sb.stage_frames(0, depths, frames_u32=packed)
        form.append(srch, 3, [([g], [c]) for g, c in motions], [4, 4, 6], none, 1 if k == 1 else W * H, 200, 9)
        mem.append_memory(3, motions=motions, streams=[4, 4, 6], keep=200, ball_max_age=9)
        for b in range(3):
            _same(srch.read(b), mem.read(b), ("no search", k, b))
            assert np.array_equal(srch.read_frame_memory_balls(b), mem.read_frame_memory_balls(b))
            got = srch.read_motion(b)
            assert (tuple(got["gather"].tolist()), tuple(got["carry"].tolist())) == motions[b] and got["score"][0] == got["score"][1]
        for s in (4, 5, 6):
            _same(srch.read_memory(s), mem.read_memory(s), ("no search bank", k, s))
    assert srch.read_memory(4)["map"].any() and plain.read(0)["map"].max() > 0
    _close(srch, mem, plain)


@pytest.mark.gpu
def test_no_search_is_append_memory_and_an_empty_bank_the_plain_sane_append(built, oracle):
    degenerate_forms_on_the_device(Flat, oracle, 8, 0)


def device_pointer_on_the_device(form, oracle, params):
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
            form.append(sb, 3, [THREE] * 3, [1, 0, 1], params, None)
        for b in range(3):
            _same(dev.read(b), host.read(b), ("device", k, b))
            assert _equal(form.read(dev, b), form.read(host, b)) and np.array_equal(dev.read_frame_memory_balls(b), host.read_frame_memory_balls(b))
        for s in (0, 1):
            _same(dev.read_memory(s), host.read_memory(s), ("device bank", k, s))
    assert dev.read_motion(2)["score"][0] > 0
    _close(host, dev)


@pytest.mark.gpu
def test_frames_staged_from_a_device_pointer_and_from_the_host(built, oracle):
    device_pointer_on_the_device(Flat, oracle, 2)


def balls_on_the_device(form, oracle, params, priors, chosen):
    """Two streams in ONE call: each stream sees its balls, then the same depth image without them under a prior that says the map
    moved - by a different shift per stream. Each correction is its own frame's; the balls stay where they were."""
    import yolact_amd as ya
    H, W = 37, 53
    with_balls = [_stamps(oracle, H, W, seed) for seed in (61, 62)]
    without = [_stamps(oracle, H, W, seed, balls=False) for seed in (61, 62)]
    sb, bank, scenes = ya.SceneBatch(W, H, 4), form.Bank(W, H), {}
    cands = [([IDENT[0]], [IDENT[1]])] * 2 + [([g], [c]) for g, c in priors]
    got, mot = _run_call(form, sb, bank, scenes, _packed(with_balls + without), [3, 8, 3, 8], cands, params, None, 256, 5, ("balls",))
    assert [m["chosen"] for m in mot] == [(0, 0, 0), (0, 0, 0)] + chosen                             # both corrected, on the restatement
    assert all(m["carry"] == R.IDENTITY and m["gather"] == R.IDENTITY for m in mot[2:])
    for b, s in ((2, 3), (3, 8)):
        seen = sb.read_frame_memory_balls(b - 2)
        ids = np.flatnonzero(seen[:, 2] > 0)
        assert len(ids) >= 1 and not without[b - 2][2]["balls"].any()
        tab, mem = sb.read_frame_memory_balls(b), sb.read_memory(s)["balls"]
        for k in ids:
            assert tab[k].tolist() == mem[k].tolist() == [seen[k, 0], seen[k, 1], seen[k, 2], 1] and got[b]["balls"][k].tolist() == [seen[k, 0], seen[k, 1], seen[k, 2], 0]
    _close(sb, scenes)


@pytest.mark.gpu
def test_remembered_balls_are_carried_by_the_chosen_carry_of_their_own_frame(built, oracle):
    balls_on_the_device(Flat, oracle, 3, [shift(2, 1), shift(-1, 2)], [(0, 2, 1), (0, -1, 2)])


def planners_on_the_device(form, oracle, params):
    """One plan and one turn plan with targets=None, against the per-stream Scenes after the same appends: two frames on one stream,
    the second sees no ball and plans to the ones remembered; a third on another stream."""
    import yolact_amd as ya
    H, W = 33, 65
    start = ((W * 5) // 8, H - 1)
    fr = [_stamps(oracle, H, W, 31), _stamps(oracle, H, W, 32, balls=False), _stamps(oracle, H, W, 33)]
    depths, packed, ora = _packed(fr)
    streams = [2, 2, 0]
    cands = [([shift(2, -1)[0], IDENT[0]], [shift(2, -1)[1], IDENT[1]])] * 3
    sb, scenes = ya.SceneBatch(W, H, 3), {s: ya.Scene(W, H) for s in (0, 2)}
    sb.stage_frames(0, depths, frames_u32=packed)
    form.append(sb, 3, cands, streams, params, None, 240)
    f1 = sb.read(1)
    assert not ora[1]["balls"].any() and (f1["balls"][:, 2] > 0).sum() >= 1 and (f1["map"] > ora[1]["map"]).any()        # balls only remembered, map fused
    want = []
    for b, s in enumerate(streams):
        sc = scenes[s]
        form.single(sc, depths[b], packed[b], cands[b], params, None, 240)
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


@pytest.mark.gpu
def test_planners_run_on_the_fused_frames(built, oracle):
    planners_on_the_device(Flat, oracle, 2)


def _raises(fn, code, text=None):
    import yolact_amd as ya
    with pytest.raises(ya.YhError) as e:
        fn()
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)


def state_matrix_on_the_device(oracle):
    """Every read and every hook of the batch after each of the five memory appends and a plain append, a staged slot and a reset."""
    import yolact_amd as ya
    from yolact_amd.capi import EINVAL, ESTATE
    H, W = 37, 53
    sb = ya.SceneBatch(W, H, 3)
    depths, packed, _ = _call_frames(oracle, H, W, 0, 3)
    streams = [1, 2, 1]
    reads = dict(motion=lambda: sb.read_motion(0), scores=lambda: sb.read_motion(0, scores=True), pyramid=lambda: sb.read_pyramid(0, 0),
                 norm=lambda: sb.read_motion_norm(0), pyramid_norm=lambda: sb.read_pyramid_norm(0, 0))
    hooks = dict(time=lambda: sb.time(1), memory=lambda: sb.memory_time(1), search=lambda: sb.memory_search_time(1), pyramid=lambda: sb.memory_pyramid_time(1),
                 search_norm=lambda: sb.memory_search_norm_time(1), pyramid_norm=lambda: sb.memory_pyramid_norm_time(1))
    appends = dict(plain=lambda: sb.append(3, ya.COMPAT_SANE), memory=lambda: sb.append_memory(3, streams=streams),
                   search=lambda: sb.append_memory_search(3, candidates=[THREE] * 3, streams=streams, radius=2),
                   pyramid=lambda: sb.append_memory_pyramid(3, candidates=[THREE] * 3, streams=streams, levels=2, radius=2, refine=1),
                   search_norm=lambda: sb.append_memory_search_norm(3, candidates=[THREE] * 3, streams=streams, radius=2),
                   pyramid_norm=lambda: sb.append_memory_pyramid_norm(3, candidates=[THREE] * 3, streams=streams, levels=2, radius=2, refine=1))
    # which reads work after which append (everything else: YH_ESTATE, but scores after either pyramid form: YH_EINVAL naming the read)
    works = dict(plain=[], memory=[], search=["motion", "scores"], pyramid=["motion", "pyramid"], search_norm=["motion", "scores", "norm"],
                 pyramid_norm=["motion", "pyramid", "norm", "pyramid_norm"])
    hook_of = dict(plain="time", memory="memory", search="search", pyramid="pyramid", search_norm="search_norm", pyramid_norm="pyramid_norm")
    named = dict(search_norm=HOOK, pyramid_norm=PYRAMID_HOOK)
    for r in reads.values():
        assert _code(r) == ESTATE
    for k in ("search_norm", "pyramid_norm"):
        assert _code(hooks[k]) == ESTATE                                                             # before any append
    sb.stage_frames(0, depths, frames_u32=packed)
    sb.append(3, ya.COMPAT_SANE)                                                                     # (yh_scene_batch_time replays the last plain append, whatever came since)
    for name in ("memory", "search_norm", "search", "pyramid_norm", "pyramid", "search_norm", "plain", "pyramid_norm"):
        appends[name]()
        for r, read in reads.items():
            if r in works[name]:
                read()
            elif r == "scores" and name in ("pyramid", "pyramid_norm"):
                _raises(read, EINVAL, "yh_scene_batch_pyramid_read")
            else:
                assert _code(read) == ESTATE, (name, r)
        for k, hook in hooks.items():
            if k == hook_of[name]:
                hook()
            elif name in named and k in ("time", "memory", "search", "pyramid"):
                _raises(hook, ESTATE, named[name])                                                   # the existing hooks name the new one
            else:
                assert _code(hook) == ESTATE, (name, k)
    # after the normalised pyramid: the flat tables have a call of their own
    spare = np.zeros(3 * 5 * 5, np.uint64)
    for totals, inside in ((spare, None), (None, spare)):
        assert sb.L.yh_scene_batch_motion_norm_read(sb.h, 0, None if totals is None else ya.capi._p(totals), None if inside is None else ya.capi._p(inside), None, None, None) == EINVAL
        assert b"yh_scene_batch_pyramid_norm_read" in sb.L.yh_scene_batch_last_error(sb.h) and not spare.any()
    for frame, level in ((0, -1), (0, 3), (3, 0), (-1, 0)):
        assert _code(lambda: sb.read_pyramid_norm(frame, level)) == EINVAL and _code(lambda: sb.read_pyramid(frame, level)) == EINVAL, (frame, level)
    assert _code(lambda: sb.read_motion_norm(3)) == EINVAL and _code(lambda: sb.read_motion_norm(-1)) == EINVAL
    # a slot staged since: no replay, the reads stay; a memory reset since: no replay and no level tables, the records stay
    for name, hook in (("search_norm", hooks["search_norm"]), ("pyramid_norm", hooks["pyramid_norm"])):
        appends[name]()
        chosen = sb.read_motion(1)["chosen"]
        sb.stage_frames(0, depths, frames_u32=packed)
        assert _code(hook) == ESTATE and np.array_equal(sb.read_motion(1)["chosen"], chosen) and "qualified" in sb.read_motion_norm(1)
        appends[name]()
        sb.memory_reset(2)
        assert _code(hook) == ESTATE and "qualified" in sb.read_motion_norm(1)
        if name == "pyramid_norm":
            assert _code(lambda: sb.read_pyramid_norm(0, 0)) == ESTATE and _code(lambda: sb.read_pyramid(0, 0)) == ESTATE
    sb.close()


@pytest.mark.gpu
def test_the_state_matrix_of_the_reads_and_the_hooks(built, oracle):
    state_matrix_on_the_device(oracle)


def time_hook_on_the_device(form, oracle, params):
    import ctypes as C
    import yolact_amd as ya
    from yolact_amd.capi import EINVAL
    H, W = 37, 53
    sb, scenes = ya.SceneBatch(W, H, 4), {s: ya.Scene(W, H) for s in (1, 2)}
    depths, packed, _ = _call_frames(oracle, H, W, 0, 4)
    sb.stage_frames(0, depths, frames_u32=packed)
    sb.append_memory(4, motions=[IDENT] * 4, streams=[1, 2, 1, 1])
    for b, s in enumerate([1, 2, 1, 1]):
        scenes[s].append_memory(depths[b], frame_u32=packed[b])
    depths, packed, _ = _call_frames(oracle, H, W, 1, 4)
    sb.stage_frames(0, depths, frames_u32=packed)
    streams = [1, 2, 1]
    form.append(sb, 3, [THREE] * 3, streams, params, None, 250)
    for b, s in enumerate(streams):
        form.single(scenes[s], depths[b], packed[b], THREE, params, None, 250)
    frames, mems = [sb.read(b) for b in range(3)], {s: sb.read_memory(s) for s in (1, 2)}
    motions, tabs = [form.read(sb, b) for b in range(3)], [sb.read_frame_memory_balls(b) for b in range(3)]
    assert motions[2]["score"][0] > 0
    ms, ms_search = form.time(sb, 3)
    assert ms > 0 and 0 < ms_search < ms
    for b in range(3):
        _same(sb.read(b), frames[b], ("time", b))
        assert _equal(form.read(sb, b), motions[b]) and np.array_equal(sb.read_frame_memory_balls(b), tabs[b])
    for s in (1, 2):
        _same(sb.read_memory(s), mems[s], ("time bank", s))
        _same(mems[s], scenes[s].read_memory(), ("time scene bank", s))
    f = C.c_float()
    hook = getattr(sb.L, form.hook)
    assert hook(sb.h, 0, C.byref(f), C.byref(f)) == EINVAL and hook(None, 1, C.byref(f), C.byref(f)) == EINVAL
    assert hook(sb.h, 1, None, C.byref(f)) == EINVAL and hook(sb.h, 1, C.byref(f), None) == EINVAL
    # a plain search call after it continues the same streams' memories
    sb.append_memory_search(3, candidates=[THREE] * 3, streams=streams, radius=2)
    for b, s in enumerate(streams):
        scenes[s].append_memory_search(depths[b], frame_u32=packed[b], candidates=THREE, radius=2)
    for s in (1, 2):
        _same(sb.read_memory(s), scenes[s].read_memory(), ("search after it", s))
    _close(sb, scenes)


@pytest.mark.gpu
def test_norm_time_commits_nothing(built, oracle):
    time_hook_on_the_device(Flat, oracle, 3)


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
    Flat.append(sb, 2, [THREE] * 2, [7, 2], 2, None)
    Flat.append(sb, 2, [THREE] * 2, [2, 7], 2, None)                                                 # frame 1 on stream 7 remembers frame 0's balls of the first call
    assert sb.plan(None, starts=[start] * 2) == [0, 0]
    frames, plans = [sb.read(b) for b in range(2)], [sb.read_plan(b) for b in range(2)]
    mems, tabs = [sb.read_memory(s) for s in (2, 7)], [sb.read_frame_memory_balls(b) for b in range(2)]
    motions = [Flat.read(sb, b) for b in range(2)]
    g = np.tile(np.array(R.IDENTITY, np.int32), (3, 2, 1))                                          # [3 frames][2 bases][6]
    st = np.array([2, 7, 0], np.int32)
    call = lambda hh=h, n=2, s=st, n_rot=2, gg=g, cc=g, radius=2, mi=100, keep=224, age=30: L.yh_scene_batch_append_memory_search_norm(
        hh, n, None if s is None else _p(s), n_rot, None if gg is None else _p(gg), None if cc is None else _p(cc), radius, mi, keep, age)
    err = lambda: L.yh_scene_batch_last_error(h)
    assert call(hh=None) == EINVAL and call(gg=None) == EINVAL and call(cc=None) == EINVAL
    assert call(n=0) == EINVAL and call(n=4) == EINVAL and call(n=-1) == EINVAL
    assert call(n_rot=0) == EINVAL and call(n_rot=17) == EINVAL and call(radius=-1) == EINVAL and call(radius=9) == EINVAL
    assert call(mi=0) == EINVAL and b"min_inside" in err() and call(mi=W * H + 1) == EINVAL and call(mi=-1) == EINVAL
    assert call(keep=-1) == EINVAL and call(keep=257) == EINVAL and call(age=-1) == EINVAL and call(age=256) == EINVAL
    for bad in (-1, 64):
        assert call(s=np.array([2, bad, 0], np.int32)) == EINVAL and b"frame 1" in err()
    assert call(n=3) == ESTATE and b"slot 2" in err()                                                # slot 2 was never staged
    # an int32 condition broken in the last frame's last base only: the text names frame and base
    for which, row in (("g", _edge(2)[:2] + (_edge(2)[2] + Q,) + _edge(2)[3:]), ("c", (Q, Q, I32_MAX, 0, Q, 0))):
        bad = g.copy()
        bad[1, 1] = row
        assert not G.bases_ok([tuple(r) for r in (bad if which == "g" else g)[1].tolist()], [tuple(r) for r in (bad if which == "c" else g)[1].tolist()], 2)
        assert (call(gg=bad) if which == "g" else call(cc=bad)) == EINVAL and b"frame 1" in err() and b"base 1" in err(), row
    for b in range(2):
        _same(sb.read(b), frames[b], ("refused", b))
        _same(sb.read_plan(b), plans[b], ("refused plan", b))                                       # not a new frame generation: the plan is still readable
        assert np.array_equal(sb.read_frame_memory_balls(b), tabs[b]) and _equal(Flat.read(sb, b), motions[b])
    for s, m in zip((2, 7), mems):
        _same(sb.read_memory(s), m, ("refused memory", s))
    assert not sb.read_memory(0)["map"].any()
    assert call(mi=W * H) == 0 and _code(lambda: sb.read_plan(0)) == ESTATE                          # a new frame generation: the plan is of earlier frames
    assert call(mi=1) == 0
    sb.close()


def cost_on_the_device(form, n_rot_side, params, ceiling, what):
    import yolact_amd as ya
    H, W, n = 480, 640, 8
    depth = np.random.default_rng(0).integers(200, 4000, (H, W)).astype(np.uint16)
    ci = np.zeros((H, W, 2), np.uint8)
    ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
    prior = (3.0, -2.0, 0.05)
    motion = ya.scene_motion(*prior)
    cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=n_rot_side)
    single = ya.Scene(W, H)
    single.append_memory(depth, cls_id=ci, motion=motion)
    form.single(single, depth, ya.SceneBatch.pack(ci), cands, params, None)
    ratios = {}
    for name, streams in (("a stream per frame", list(range(n))), ("all on one stream", None)):
        sb = ya.SceneBatch(W, H, n)
        sb.stage_frames(0, np.stack([depth] * n), frames_u32=np.stack([ya.SceneBatch.pack(ci)] * n))
        sb.append_memory(n, motions=[motion] * n, streams=streams)
        form.append(sb, n, [cands] * n, streams, params, None)
        form.time(single, 30); form.time(sb, 30)
        ts, tb, tr = [], [], []
        for _ in range(5):
            ts.append(form.time(single, 30)[0])
            a, b = form.time(sb, 30)
            tb.append(a / n); tr.append(b / n)
        ratio = float(np.median(tb) / np.median(ts))
        spread = (max(ts) - min(ts)) / np.median(ts)
        print(f"scene {what} 640x480, n = {n}, {name}: single {np.median(ts):.4f} ms, batch {np.median(tb):.4f} ms per frame (registration alone {np.median(tr):.4f}), "
              f"ratio {ratio:.3f}, spread of the single handle {100 * spread:.2f} %")
        ratios[name] = (ratio, ts, tb)
        sb.close()
    single.close()
    for name, (ratio, ts, tb) in ratios.items():
        assert ratio <= ceiling, (name, ts, tb)


# the ceiling of the cost test, from the single handle alone (see the test): 1.0 + its own spread, 0.44 %, + the 3 % between boxes
CEILING = 1.034


@pytest.mark.gpu
def test_batched_normalised_search_costs_no_more_per_frame_than_the_single_handle(built):
    """At 640 x 480 and n = 8, (n_rot, radius) = (5, 4), min_inside W H // 4, the robots + balls frame of tools/time_scene.py in every
    slot, memories filled, the tool's prior with bases 0.01 rad apart, in this process: yh_scene_batch_memory_search_norm_time per
    frame against yh_scene_memory_search_norm_time's first figure on a single handle, alternated, one warm-up each, the median of five
    runs of 30 replays, in both columns: a stream per frame (the frames share every launch) and all frames on one stream (eight rounds
    of three launches). The batch must not cost more per frame than the single handle.
    Ceiling 1.034 = 1.0 + the single handle's own run-to-run spread in that measurement, 0.44 % ((max - min) / median of its five
    runs, profiles/scene_batch_register_norm_timings.txt, 2026-10-20) + the 3 % by which the pool's boxes differ - the derivation of
    CEILING in test_scene_batch_pyramid.py: nothing here comes from the batch's own figures. Measured there: 0.2691 / 0.3283 ms per
    frame against 0.4150, ratios 0.649 / 0.791 - both columns meet it, so both are bounded. The other batch sizes are recorded
    there and in DESIGN.md, not bounded here."""
    cost_on_the_device(Flat, 2, 4, CEILING, "normalised search, (5, 4),")
