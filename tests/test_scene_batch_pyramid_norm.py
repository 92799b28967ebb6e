"""The scene batch's normalised pyramid registration (DESIGN.md §11 "Scene batch: normalised pyramid registration"):
yh_scene_batch_append_memory_pyramid_norm is n yh_scene_append_memory_pyramid_norm calls in batch order, frame b on the memory of
streams[b] - so a stream's later frame is registered, coarse to fine and by the normalised score at every level, against what its
earlier frame has just fused. CPU part: the restated bank (tests/scene_batch_pyramid_norm_ref.py) against answers worked out by hand
and on chained sequences over dense terrain whose steps lie beyond the flat search's reach, which the plain pyramid bank never finds.
GPU part (-m gpu): every output, table, memory, motion, level table (S, T, C), threshold, flag and record bit for bit against the
restatement fed the oracle's SANE stamps AND against real Scene handles, one per stream, driven with append_memory_pyramid_norm in
batch order; the planners on the fused frames; the replay hook; every refusal; and the cost per frame against the single handle's
normalised pyramid append. The cases and their helpers are those of test_scene_batch_register_norm.py, given the pyramid FORM."""
import numpy as np
import pytest

import scene_batch_pyramid_norm_ref as BPN
import scene_batch_pyramid_ref as BP
import scene_memory_ref as R
import scene_pyramid_norm_ref as PN
import scene_pyramid_ref as P
import scene_register_norm_ref as GN
import test_scene_batch_register_norm as T
from test_scene_batch_memory import N, PATTERNS, _call_frames, _code, _packed, _same
from test_scene_batch_pyramid import FAR, FAR_SHAPES, NEAR_SHAPES, _case
from test_scene_batch_register import OUTSIDE, THREE, _close
from test_scene_memory import IDENT, _stamps, shift
from test_scene_pyramid import COARSE_ALONE, I32_MAX, Q, _bases
from test_scene_register import ROTATION, SHEARED, _lds_words, _window_words


class Pyr:
    """the pyramid form: params = (levels, radius, refine)"""
    name, hook = "pyramid_norm", T.PYRAMID_HOOK
    Bank = BPN.Bank

    @staticmethod
    def append(sb, n, cands, streams, params, mi, keep=224, age=30):
        sb.append_memory_pyramid_norm(n, candidates=cands, streams=streams, levels=params[0], radius=params[1], refine=params[2], min_inside=mi, keep=keep, ball_max_age=age)

    @staticmethod
    def restate(bank, stamps, balls, streams, cands, params, mi, keep=224, age=30):
        return bank.append_pyramid_norm(stamps, balls, streams, cands, params[0], params[1], params[2], mi, keep, age)

    @staticmethod
    def single(sc, depth, packed, cands, params, mi, keep=224, age=30):
        sc.append_memory_pyramid_norm(depth, frame_u32=packed, candidates=cands, levels=params[0], radius=params[1], refine=params[2], min_inside=mi, keep=keep, ball_max_age=age)

    @staticmethod
    def read(h, b=None):
        """everything the four reads return for frame b of a batch (b None: of a Scene), a flat dict"""
        at = () if b is None else (b,)
        out = dict(h.read_motion(*at))
        out.update(h.read_motion_norm(*at))
        for lv in range(h._pyramid[1] + 1):
            for k, v in h.read_pyramid_norm(*at, lv).items():
                out[f"{k} {lv}"] = v
            for k, v in h.read_pyramid(*at, lv).items():
                out[f"plain {k} {lv}"] = v
        return out

    @staticmethod
    def check(got, want, what):
        """the reads against what scene_pyramid_norm_ref.search returns"""
        assert got["gather"].dtype == got["carry"].dtype == got["chosen"].dtype == np.int32 and got["score"].dtype == np.uint64, what
        assert tuple(got["chosen"].tolist()) == want["chosen"] and tuple(got["gather"].tolist()) == want["gather"] and tuple(got["carry"].tolist()) == want["carry"], (what, got["chosen"], want["chosen"])
        assert tuple(int(v) for v in got["score"]) == want["score"], what
        assert tuple(int(v) for v in got["chosen_stc"]) == want["chosen_stc"] and tuple(int(v) for v in got["prior_stc"]) == want["prior_stc"], what
        assert got["qualified"] is want["qualified"] and "totals" not in got and "inside" not in got, what
        for lv in range(len(want["tables"])):
            for k, w in (("scores", want["tables"][lv]), ("totals", want["totals"][lv]), ("inside", want["inside"][lv])):
                t = got[f"{k} {lv}"]
                assert t.dtype == np.uint64 and t.shape == w.shape and np.array_equal(t, w), what + (k, lv)
            assert got[f"centres {lv}"].dtype == got[f"qualified {lv}"].dtype == np.int32, what + (lv,)
            assert np.array_equal(got[f"centres {lv}"], want["centres"][lv]) and np.array_equal(got[f"qualified {lv}"], want["flags"][lv]), what + ("centres, flags", lv)
            assert got[f"sum_n {lv}"] == want["sum_n"][lv] and got[f"min_inside {lv}"] == want["need"][lv], what + ("sum_n, threshold", lv)
            # yh_scene_batch_pyramid_read after the normalised append: the centres, the S tables and sum_n again
            assert np.array_equal(got[f"plain centres {lv}"], want["centres"][lv]) and np.array_equal(got[f"plain scores {lv}"], want["tables"][lv]), what + ("plain read", lv)
            assert got[f"plain sum_n {lv}"] == want["sum_n"][lv], what + ("plain read", lv)

    @staticmethod
    def table0(m):
        return m["tables"][0]

    @staticmethod
    def time(h, reps):
        return h.memory_pyramid_norm_time(reps)


# ---- CPU: the restated bank --------------------------------------------------------------------------------------------------------

def test_restated_bank_registers_a_chained_frame_against_its_predecessors_map():
    W, H, Z, A, B, A1, none, seen = T._hand_frames()
    one = ([R.IDENTITY], [R.IDENTITY])
    bank = BPN.Bank(W, H)
    # frames 0 and 2 on stream 0, frames 1 and 3 on stream 1; (levels, radius, refine) = (1, 1, 1), min_inside 6: m_1 = 2
    out, tabs, mot = bank.append_pyramid_norm([A, B, A1, B], [seen, none, none, none], [0, 1, 0, 1], [one] * 4, 1, 1, 1, 6, 128, 2)
    assert mot[0]["chosen"] == mot[1]["chosen"] == (0, 0, 0) and mot[0]["score"] == (0, 0, 107) and mot[0]["qualified"] and not any(t.any() for t in mot[1]["tables"])
    # by hand. Level 1 (2 x 2): N has 100 in cell (1, 0), M = A pooled is [[100, 7], [0, 0]]: S(U, V) = min(100, M1[V][1 + U]), 100 at
    # U = -1, 7 at U = 0, both V = 0. At (-1, 0) column 1 is inside (C = 2 = m_1), its sources column 0: T = 100 + 100, ratio 1; at (0, 0)
    # T = 100 + 107, ratio 7 / 200. The centre below is twice (-1, 0).
    m = mot[2]
    top = np.zeros((1, 3, 3), np.uint64); top[0, 1, 0] = 100; top[0, 1, 1] = 7
    assert np.array_equal(m["tables"][1], top) and m["totals"][1][0, 1, 0] == 200 and m["totals"][1][0, 1, 1] == 207
    assert m["inside"][1][0].tolist() == [[1, 2, 1], [2, 4, 2], [1, 2, 1]] and m["need"] == [6, 2] and m["flags"][1].tolist() == [1]
    assert m["centres"][1].tolist() == [[0, 0]] and m["centres"][0].tolist() == [[-2, 0], [0, 0]]
    # level 0: S(u, v) = min(100, A[1 + v][2 + u]). Around (-2, 0) only u = -1, v = 0 meets A's peak (C = 9, T = 200: ratio 1); the home
    # hypothesis around (0, 0) meets it too, and A's corner pixel at u = 1, v = -1. (-2, 0) itself: C = 6 = m_0, S = 0.
    low = np.zeros((2, 3, 3), np.uint64); low[0, 1, 2] = 100; low[1, 1, 0] = 100; low[1, 0, 2] = 7
    assert np.array_equal(m["tables"][0], low) and m["sum_n"] == [100, 100] and m["flags"][0].tolist() == [1, 1]
    assert m["inside"][0][0, 1].tolist() == [3, 6, 9] and m["totals"][0][0, 1, 2] == m["totals"][0][1, 1, 0] == 200
    assert m["chosen"] == (0, -1, 0) and m["score"] == (100, 0, 100) and m["chosen_stc"] == (100, 200, 9) and m["prior_stc"] == (0, 207, 12) and m["qualified"]
    assert m["gather"] == shift(1, 0)[0] and m["carry"] == shift(1, 0)[1]
    # frame 3 is frame 1 again, against frame 1's own map: the identity at ratio 1, the stream-0 frames between them nothing to it
    assert mot[3]["chosen"] == (0, 0, 0) and mot[3]["score"] == (50, 50, 50) and mot[3]["chosen_stc"] == (50, 100, 12)
    f2 = Z.copy(); f2[1, 2] = 100                                                                    # A moved right (its corner pixel leaves), halved: 50 < 100
    assert np.array_equal(out[2]["map"], f2) and np.array_equal(bank.mem[0].M, f2) and np.array_equal(bank.mem[1].M, B)
    assert tabs[2][7].tolist() == [2, 2, 4, 1] and out[2]["balls"][7].tolist() == [2, 2, 4, 0]     # the ball carried by the CHOSEN carry, one to the right
    # min_inside 12: m_1 = 3 leaves level 1 its centre entry alone (C = 4), m_0 = 12 level 0 the two (0, 0) entries: the prior, qualified
    other = BPN.Bank(W, H)
    _, _, mo = other.append_pyramid_norm([A, A1], [none, none], [3, 3], [one] * 2, 1, 1, 1, 12, 128, 2)
    assert mo[1]["chosen"] == (0, 0, 0) and mo[1]["qualified"] and mo[1]["centres"][0].tolist() == [[0, 0], [0, 0]] and mo[1]["need"] == [12, 3]
    out, tabs, mot = bank.append_pyramid_norm([A1], [none], [0], [one], 1, 1, 1, 6, 256, 2)           # the next call continues the streams
    assert mot[0]["chosen"] == (0, 0, 0) and mot[0]["score"] == (100, 100, 100) and tabs[0][7].tolist() == [2, 2, 4, 2]
    bank.reset(0)
    assert not bank.mem[0].M.any() and not bank.mem[0].B.any() and bank.mem[1].M.any()
    bank.reset()
    assert not bank.mem[1].M.any()


def test_restated_bank_with_one_candidate_and_no_search_is_the_plain_bank():
    T._plain_bank_case(Pyr, (1, 0, 0))


PYRAMID_STEPS = {(65, 130): [(13, -11), (-16, 13), (9, 10)], (53, 37): [(-9, 12), (10, -9), (9, 9)]}


@pytest.mark.parametrize("noise", [0, 300])
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("H,W", list(PYRAMID_STEPS))
def test_dense_chained_sequences_are_registered_by_the_normalised_pyramid_bank_alone(H, W, seed, noise):
    """keep = 256, identity prior, (levels, radius, refine) = (2, 8, 1), min_inside = W H // 4, every step beyond radius 8: the
    normalised pyramid bank chooses every step of all 12 sequences exactly, the plain pyramid bank none of the 36, and the flat
    normalised bank at radius 8 stops at the edge of its grid."""
    steps = PYRAMID_STEPS[H, W]
    assert all(8 < max(abs(u), abs(v)) <= P.reach(2, 8, 1)[0] for u, v in steps)
    frames = T._chain(H, W, steps, seed, noise)
    _, _, mot = BPN.Bank(W, H).append_pyramid_norm(frames, T.NO_BALLS, None, None, 2, 8, 1, None, 256, 30)
    assert [m["chosen"] for m in mot[1:]] == [(0,) + s for s in steps] and all(m["qualified"] for m in mot)
    _, _, plain = BP.Bank(W, H).append_pyramid(frames, T.NO_BALLS, None, None, 2, 8, 1, 256, 30)
    assert all(p["chosen"] != (0,) + s for p, s in zip(plain[1:], steps)), [p["chosen"] for p in plain]
    _, _, flat = T.BN.Bank(W, H).append_search_norm(frames, T.NO_BALLS, None, None, 8, None, 256, 30)
    assert max(abs(t) for t in flat[1]["chosen"][1:]) == 8 and flat[1]["chosen"] != (0,) + steps[0]


# On two of the shapes the oracle's stamps are too flat for case 1 to end AT the identity: 9 x 130 and 8 x 8 are a few rows of one
# terrain band, a pooled level of such a map is the same under many shifts, every one of them has S = U, and the tie goes to the
# smallest total shift - the normalised score is made not to tell such shifts apart (the single handle chooses the same, bit for bit).
# There the case asserts what chaining still shows: a choice that is not (0, 0, 0) at S > 0, which an empty memory cannot give.
FLAT_BANDS = [(9, 130), (8, 8)]


@pytest.mark.parametrize("H,W", FAR_SHAPES + NEAR_SHAPES)
def test_same_frame_far_wrong_priors_restated(oracle, H, W):
    """Frame 0 meets an empty memory; every later frame is the frame its predecessor fused (keep = 256), so its wrong prior is
    corrected to the identity at S = U - which the call-start memory, empty, could never tell it, and which on the FAR shapes the flat
    normalised search at its widest, radius 8, cannot reach."""
    priors, lrr, chosen = _case(H, W)
    frames, (_, _, mot), _ = T._wrong_priors(Pyr, oracle, H, W, priors, lrr)
    assert mot[0]["chosen"] == (0, 0, 0) and mot[0]["gather"] == R.IDENTITY and not any(t.any() for t in mot[0]["tables"])
    if (H, W) in FLAT_BANDS:
        assert all(m["chosen"] != (0, 0, 0) and m["score"][0] > 0 and m["qualified"] for m in mot[1:]) and len(set(m["chosen"] for m in mot[1:])) >= 2
        return
    assert [m["chosen"] for m in mot] == chosen
    for m in mot[1:]:
        s, t, c = m["chosen_stc"]
        assert m["gather"] == R.IDENTITY and m["carry"] == R.IDENTITY and m["qualified"] and t - s == s > 0 and c == W * H
    if (H, W) in FAR_SHAPES:
        stamps = frames[2][0]["map"]
        for (g, c), (_, u, v) in list(zip(FAR[0], FAR[2]))[1:]:
            assert max(abs(u), abs(v)) > 8 and GN.search(stamps, stamps, [g], [c], 8, (W * H) // 4)["chosen"] != (0, u, v), (u, v)


def _plain_pyramid_bank(k, stamps, balls, keep):
    bank = T._PLAIN2.setdefault("pyramid", BP.Bank(9, 100))
    return bank.append_pyramid(stamps, balls, PATTERNS["one"], [THREE] * N, 2, 2, 1, keep, 5)[2]


def test_case_2_on_one_stream_the_normalised_bank_chooses_otherwise_than_the_plain_bank(oracle):
    """On the frames of case 2 at 100 x 9, all on one stream: some chained frame (rank >= 1 in its call) is registered otherwise by
    the normalised pyramid bank than by the plain pyramid bank."""
    calls = T._case2(Pyr, oracle, 100, 9, (2, 2, 1), _plain_pyramid_bank)
    assert any(m["chosen"] != p["chosen"] for mot, plain, _ in calls for m, p in list(zip(mot, plain))[1:])


COARSE_BASE = (Q, 0, 3 * Q, 0, Q, 0)
COARSE_CALLS = [([4], None, None), ([4, 4], [([COARSE_BASE], [R.IDENTITY])] * 2, 40)]           # (streams, candidates, min_inside) at (1, 0, 0), keep 256


def _coarse_frames(oracle):
    """test_op_pyramid_norm_where_the_coarsest_level_disqualifies_everything_and_level_0_does_not's construction through a chained
    append at 8 x 8: a base three pixels to the side keeps 5 x 8 = 40 pixels inside at level 0 and, one and a half cells to the side,
    fewer than the 10 cells min_inside = 40 asks of level 1. The first call fills the memory; the second chains two frames on it."""
    return [_call_frames(oracle, 8, 8, 0, 1), _call_frames(oracle, 8, 8, 1, 2)]


def _coarse_holds(mot):
    for m in mot:
        # 40 pixels inside at level 0 = min_inside; level 1 asks 10 cells and the base keeps fewer: the descent falls back to its centre
        assert m["need"] == [40, 10] and int(m["inside"][1].max()) < 10 and m["flags"][1].tolist() == [0] and m["centres"][0].tolist() == [[0, 0], [0, 0]]
        assert m["flags"][0].tolist() == [1, 1] and m["qualified"] and int(m["inside"][0][0, 0, 0]) == 40


def test_the_coarsest_level_disqualifies_everything_and_level_0_does_not_restated(oracle):
    bank = BPN.Bank(8, 8)
    for frames, (streams, cands, mi) in zip(_coarse_frames(oracle), COARSE_CALLS):
        _, _, mot = Pyr.restate(bank, [o["map"] for o in frames[2]], [o["balls"] for o in frames[2]], streams, cands, (1, 0, 0), mi, 256, 5)
    _coarse_holds(mot)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("H,W", FAR_SHAPES + NEAR_SHAPES)
def test_same_frame_far_wrong_priors(built, oracle, H, W):
    """Case 1. An implementation that pools or scores the call-start (empty) memory for a chained frame, or hands a frame another frame's
    table or record, cannot pass: the three corrections differ and none is (0, 0, 0). One that falls back to a flat search cannot
    either: on the FAR shapes every correction lies beyond radius 8."""
    priors, lrr, chosen = _case(H, W)
    T.wrong_priors_on_the_device(Pyr, oracle, H, W, priors, lrr, None if (H, W) in FLAT_BANDS else chosen)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("H,W", [(37, 53), (100, 9), (9, 130)])
def test_distinct_frames_equal_the_restatement_and_one_scene_per_stream(built, oracle, H, W, pattern):
    """Case 2: two calls of six distinct frames over the stream patterns of test_scene_batch_memory.py, three bases per frame,
    (levels, radius, refine) = (2, 2, 1), keep 224 then 200. With all frames on one stream, some frame of rank >= 2 of the second call
    has level-0 S tables against its predecessor's map that differ from those against the call-start memory."""
    T.distinct_frames_on_the_device(Pyr, oracle, H, W, pattern, (2, 2, 1),
                                    lambda n, start: PN.search(n, start, THREE[0], THREE[1], 2, 2, 1, (W * H) // 4)["tables"][0])


@pytest.mark.gpu
def test_the_largest_grid(built, oracle):
    """(levels, radius, refine) = (3, 8, 8), n_rot 15: fifteen bases of every kind the definition allows, on filled memories, three
    frames over two streams, two of them chained. The coarsest level runs at radius 8: seventeen rows of shifts."""
    import yolact_amd as ya
    H, W = 37, 53
    sb, bank, scenes = ya.SceneBatch(W, H, 3), BPN.Bank(W, H), {}
    T._run_call(Pyr, sb, bank, scenes, _call_frames(oracle, H, W, 0, 2), [0, 1], None, (1, 0, 0), None, 256, 5, ("fill",))
    gathers = [tuple(g) for g in _bases(H, W)]
    assert len(gathers) == 15 and P.bases_ok(gathers, [R.IDENTITY] * 15, 3, 8, 8)
    _, mot = T._run_call(Pyr, sb, bank, scenes, _call_frames(oracle, H, W, 1, 3), [0, 0, 1], [(gathers, [R.IDENTITY] * 15)] * 3, (3, 8, 8), 64, 224, 5, ("(3, 8, 8)",))
    assert all(m["tables"][0].shape == (16, 17, 17) and m["tables"][3].shape == (15, 17, 17) and m["tables"][0].max() > 0 for m in mot)
    _close(sb, scenes)


@pytest.mark.gpu
def test_edge_bases_and_the_global_memory_fallback_per_frame(built, oracle):
    """At 9 x 130 on filled memories, four frames over two streams, refine 6 - so level 0 runs at radius 6: the magnifying shear, whose
    window of M overflows the LDS budget there (so the score kernel's global-memory path runs, per frame of a batch), a motion that
    sends every pixel outside, and offsets exactly on the int32 conditions of the reach."""
    import yolact_amd as ya
    H, W, lrr = 9, 130, (1, 2, 6)
    T0 = P.reach(*lrr)[0]
    lds = _lds_words()
    assert T0 == 10 and _window_words(SHEARED[1], H, W, 6) > lds == 4096 >= _window_words(SHEARED[1], H, W, 5)
    sb, bank, scenes = ya.SceneBatch(W, H, 4), BPN.Bank(W, H), {}
    T._run_call(Pyr, sb, bank, scenes, _call_frames(oracle, H, W, 0, 2), [0, 1], None, (1, 0, 0), None, 256, 5, ("fill",))
    top = I32_MAX - T0 * Q
    gathers = [SHEARED[1], OUTSIDE(W), (Q, 0, top, 0, Q, -top), (Q, 0, -top, 0, Q, top)]
    carries = [SHEARED[0], R.IDENTITY, (Q, Q, I32_MAX - 2 * T0 * Q, -Q, 2 * Q, -(I32_MAX - 3 * T0 * Q)), R.IDENTITY]
    assert P.bases_ok(gathers, carries, *lrr) and not P.bases_ok(gathers[:2] + [(Q, 0, top + 1, 0, Q, 0)], carries[:3], *lrr)
    _, mot = T._run_call(Pyr, sb, bank, scenes, _call_frames(oracle, H, W, 1, 4), [0, 1, 0, 1], [(gathers, carries)] * 4, lrr, 64, 224, 5, ("edges",))
    assert all(m["tables"][0][0].max() > 0 and not m["inside"][0][1].any() and m["tables"][0].shape == (5, 13, 13) for m in mot)   # the shear reads the memory, the motion outside nothing
    # every pixel outside as the only base: nothing qualifies at any level, the prior stands, nothing is gathered
    frames = _call_frames(oracle, H, W, 2, 2)
    got, mot = T._run_call(Pyr, sb, bank, scenes, frames, [1, 1], [([OUTSIDE(W)], [OUTSIDE(-W)])] * 2, lrr, 1, 224, 5, ("outside",))
    assert all(m["chosen"] == (0, 0, 0) and not m["qualified"] and not any(f.any() for f in m["flags"]) for m in mot) and np.array_equal(got[1]["map"], frames[2][1]["map"])
    _close(sb, scenes)


@pytest.mark.gpu
def test_qualification_per_frame_within_one_round(built, oracle):
    T.qualification_on_the_device(Pyr, oracle, (1, 0, 0))


@pytest.mark.gpu
def test_the_coarsest_level_disqualifies_everything_and_level_0_does_not(built, oracle):
    import yolact_amd as ya
    sb, bank, scenes = ya.SceneBatch(8, 8, 2), BPN.Bank(8, 8), {}
    for frames, (streams, cands, mi) in zip(_coarse_frames(oracle), COARSE_CALLS):
        _, mot = T._run_call(Pyr, sb, bank, scenes, frames, streams, cands, (1, 0, 0), mi, 256, 5, ("coarsest", len(streams)))
    _coarse_holds(mot)
    assert sb.read_pyramid_norm(1, 1)["qualified"].tolist() == [0] and sb.read_pyramid_norm(1, 0)["qualified"].tolist() == [1, 1]
    _close(sb, scenes)


@pytest.mark.gpu
def test_at_the_camera_size(built, oracle):
    """The three frames of test_scene_memory.py's camera-size sequence: two on stream 1, the ball-less one between them on stream 0;
    (levels, radius, refine) = (3, 2, 1) and two bases."""
    import yolact_amd as ya
    H, W = 480, 640
    frames = _packed([_stamps(oracle, H, W, 10 * H + W + t, balls=t != 1) for t in range(3)])
    sb, bank, scenes = ya.SceneBatch(W, H, 3), BPN.Bank(W, H), {}
    cands = ([ROTATION[0], IDENT[0]], [ROTATION[1], IDENT[1]])
    _, mot = T._run_call(Pyr, sb, bank, scenes, frames, [1, 0, 1], [cands] * 3, (3, 2, 1), None, 224, 5, ("camera",))
    assert mot[2]["score"][0] > 0 and not any(t.any() for t in mot[1]["tables"])                    # frame 2 met frame 0's map, frame 1 an empty stream
    _close(sb, scenes)


@pytest.mark.gpu
def test_one_slot_batches_and_fewer_frames_than_slots(built, oracle):
    T.one_slot_and_fewer_frames_on_the_device(Pyr, oracle, (2, 2, 1), (3, 1, 2))


@pytest.mark.gpu
def test_no_search_is_append_memory_and_an_empty_bank_the_plain_sane_append(built, oracle):
    T.degenerate_forms_on_the_device(Pyr, oracle, (3, 8, 1), (1, 0, 0))


@pytest.mark.gpu
def test_frames_staged_from_a_device_pointer_and_from_the_host(built, oracle):
    T.device_pointer_on_the_device(Pyr, oracle, (2, 2, 1))


@pytest.mark.gpu
def test_remembered_balls_are_carried_by_the_chosen_carry_of_their_own_frame(built, oracle):
    """both priors wrong by more than the flat search reaches"""
    T.balls_on_the_device(Pyr, oracle, (2, 3, 1), [shift(10, 7), shift(-9, 11)], [(0, 10, 7), (0, -9, 11)])


@pytest.mark.gpu
def test_planners_run_on_the_fused_frames(built, oracle):
    T.planners_on_the_device(Pyr, oracle, (2, 2, 1))


@pytest.mark.gpu
def test_pyramid_norm_time_commits_nothing(built, oracle):
    T.time_hook_on_the_device(Pyr, oracle, (3, 3, 1))


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
    Pyr.append(sb, 2, [THREE] * 2, [7, 2], (2, 2, 1), None)
    Pyr.append(sb, 2, [THREE] * 2, [2, 7], (2, 2, 1), None)                                          # frame 1 on stream 7 remembers frame 0's balls of the first call
    assert sb.plan(None, starts=[start] * 2) == [0, 0]
    frames, plans = [sb.read(b) for b in range(2)], [sb.read_plan(b) for b in range(2)]
    mems, tabs = [sb.read_memory(s) for s in (2, 7)], [sb.read_frame_memory_balls(b) for b in range(2)]
    motions = [Pyr.read(sb, b) for b in range(2)]
    g = np.tile(np.array(R.IDENTITY, np.int32), (3, 2, 1))                                          # [3 frames][2 bases][6]
    st = np.array([2, 7, 0], np.int32)
    call = lambda hh=h, n=2, s=st, n_rot=2, gg=g, cc=g, lv=2, radius=2, refine=1, mi=100, keep=224, age=30: L.yh_scene_batch_append_memory_pyramid_norm(
        hh, n, None if s is None else _p(s), n_rot, None if gg is None else _p(gg), None if cc is None else _p(cc), lv, radius, refine, mi, keep, age)
    err = lambda: L.yh_scene_batch_last_error(h)
    assert call(hh=None) == EINVAL and call(gg=None) == EINVAL and call(cc=None) == EINVAL
    assert call(n=0) == EINVAL and call(n=4) == EINVAL and call(n=-1) == EINVAL
    assert call(n_rot=0) == EINVAL and call(n_rot=16) == EINVAL and call(n_rot=-1) == EINVAL and call(lv=0) == EINVAL and call(lv=4) == EINVAL
    assert call(radius=-1) == EINVAL and call(radius=9) == EINVAL and call(refine=-1) == EINVAL and call(refine=9) == EINVAL
    assert call(mi=0) == EINVAL and b"min_inside" in err() and call(mi=W * H + 1) == EINVAL and call(mi=-1) == EINVAL
    assert call(keep=-1) == EINVAL and call(keep=257) == EINVAL and call(age=-1) == EINVAL and call(age=256) == EINVAL
    for bad in (-1, 64):
        assert call(s=np.array([2, bad, 0], np.int32)) == EINVAL and b"frame 1" in err()
    assert call(n=3) == ESTATE and b"slot 2" in err()                                                # slot 2 was never staged
    # an int32 condition broken in the last frame's last base only: the text names frame and base
    T0 = P.reach(2, 2, 1)[0]
    top = I32_MAX - T0 * Q
    for which, row in (("g", (Q, 0, top + 1, 0, Q, 0)), ("g", (Q, 0, 0, 0, Q, -top - 1)), ("c", (Q, Q, I32_MAX - 2 * T0 * Q + 1, 0, Q, 0)),
                       ("c", (Q, 0, 0, -Q, 2 * Q, -(I32_MAX - 3 * T0 * Q + 1)))):
        bad = g.copy()
        bad[1, 1] = row
        assert not P.bases_ok([tuple(r) for r in (bad if which == "g" else g)[1].tolist()], [tuple(r) for r in (bad if which == "c" else g)[1].tolist()], 2, 2, 1)
        assert (call(gg=bad) if which == "g" else call(cc=bad)) == EINVAL and b"frame 1" in err() and b"base 1" in err(), row
    # a coarse level alone refuses: frame, base and level are named
    coarse = g.copy()
    coarse[1, 1] = COARSE_ALONE
    assert call(gg=coarse, lv=1, radius=8, refine=0) == EINVAL and b"frame 1" in err() and b"base 1" in err() and b"level 1" in err()
    for b in range(2):
        _same(sb.read(b), frames[b], ("refused", b))
        _same(sb.read_plan(b), plans[b], ("refused plan", b))                                       # not a new frame generation: the plan is still readable
        assert np.array_equal(sb.read_frame_memory_balls(b), tabs[b]) and T._equal(Pyr.read(sb, b), motions[b])
    for s, m in zip((2, 7), mems):
        _same(sb.read_memory(s), m, ("refused memory", s))
    assert not sb.read_memory(0)["map"].any()
    assert call(mi=W * H) == 0 and _code(lambda: sb.read_plan(0)) == ESTATE                          # a new frame generation: the plan is of earlier frames
    assert call(mi=1) == 0
    sb.close()


# the ceiling of the cost test, from the single handle alone (see the test): 1.0 + its own spread, 0.31 %, + the 3 % between boxes
CEILING = 1.033


@pytest.mark.gpu
def test_batched_normalised_pyramid_costs_no_more_per_frame_than_the_single_handle(built):
    """At 640 x 480 and n = 8, (n_rot, levels, radius, refine) = (5, 3, 8, 1), min_inside W H // 4, the robots + balls frame of
    tools/time_scene.py in every slot, memories filled, the tool's prior with bases 0.01 rad apart, in this process:
    yh_scene_batch_memory_pyramid_norm_time per frame against yh_scene_memory_pyramid_norm_time's first figure on a single handle,
    alternated, one warm-up each, the median of five runs of 30 replays, in both columns: a stream per frame (the frames share every
    launch) and all frames on one stream (eight rounds of ten launches). The batch must not cost more per frame than the single handle.
    Ceiling 1.033 = 1.0 + the single handle's own run-to-run spread in that measurement, 0.31 % ((max - min) / median of its five
    runs, profiles/scene_batch_pyramid_norm_timings.txt, 2026-10-20) + the 3 % by which the pool's boxes differ - the derivation of
    CEILING in test_scene_batch_pyramid.py: nothing here comes from the batch's own figures. Measured there: 0.2372 / 0.3314 ms per
    frame against 0.4185, ratios 0.567 / 0.792 - both columns meet it, so both are bounded. The other batch sizes are recorded
    there and in DESIGN.md, not bounded here."""
    T.cost_on_the_device(Pyr, 2, (3, 8, 1), CEILING, "normalised pyramid, (5, 3, 8, 1),")
