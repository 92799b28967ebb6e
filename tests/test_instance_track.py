"""Instance tracks (yh_instance_track, yh_instance_tracks_read, yh_instance_track_reset, yh_op_instance_track; DESIGN.md §11
"Instance tracks"). CPU part: the restatement (tests/track_ref.py) on hand cases - the purpose (ids follow the masks, not the
ranks), the threshold, the tie order, the greedy match, the memory, the room - and the new symbols. GPU part (-m gpu): the HIP
kernels array_equal to the restatement after every call of a sequence through the single-op hook at tiny and full shapes, and
through the engine on its own detections, the join with the scene, every refusal, the life cycle and a floor on time."""
import ctypes as C
import inspect
import os
import re
import time

import numpy as np
import pytest

import instance_ref as I
import track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RED, BLUE, BALL = 1 << 24, 2 << 24, 3 << 24


def _disc(hp, wp, cx, cy, r):
    yy, xx = np.mgrid[0:hp, 0:wp]
    return ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r).astype(np.uint8)


def _box(hp, wp, y0, y1, x0, x1):
    m = np.zeros((hp, wp), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def _balls(tr, masks, W=4, H=4, **kw):
    """A tracked call of the restatement on balls in the order given (scores descending)."""
    masks = np.stack(masks) if len(masks) else np.zeros((0,) + tr.shape, np.uint8)
    return tr.track(masks, [2] * len(masks), np.linspace(0.9, 0.5, len(masks)), W, H, **kw)


# ---------------------------------------------------------------- CPU

def test_two_discs_move_and_their_ids_follow_the_masks_not_the_ranks():
    """What the feature is for. Two balls at 0.91 and 0.90 each move one pixel: matched, ids kept. Then their scores cross - the
    same masks in the other rank order: every mask keeps its id, where yh_instance_frame's rule swaps them."""
    a0, b0, a1, b1 = _disc(12, 12, 3, 3, 2), _disc(12, 12, 8, 8, 2), _disc(12, 12, 4, 3, 2), _disc(12, 12, 8, 9, 2)
    tr = T.Tracker()
    f0, tab, trk = tr.track(np.stack([a0, b0]), [2, 2], [0.91, 0.90], 12, 12)
    assert tab[:, :3].tolist() == [[0, 3, 0], [1, 3, 1]] and trk.tolist() == [[0, 3, 0, 0, 13, 0], [1, 3, 1, 0, 13, 1]]
    f1, tab, trk = tr.track(np.stack([a1, b1]), [2, 2], [0.91, 0.90], 12, 12)
    assert tab[:, :3].tolist() == [[0, 3, 0], [1, 3, 1]] and trk.tolist() == [[0, 3, 0, 0, 13, 0], [1, 3, 1, 0, 13, 1]]
    assert (f1[a1 != 0] == BALL).all() and (f1[b1 != 0] == BALL | 1 << 16).all() and np.count_nonzero(f1) == 26
    f2, tab, trk = tr.track(np.stack([b1, a1]), [2, 2], [0.91, 0.90], 12, 12)
    assert tab[:, :3].tolist() == [[0, 3, 1], [1, 3, 0]] and trk.tolist() == [[0, 3, 0, 0, 13, 1], [1, 3, 1, 0, 13, 0]]
    assert np.array_equal(f2, f1)
    g, gtab = I.instance_frame(np.stack([b1, a1]), [2, 2], [0.91, 0.90], 12, 12)                       # the per-frame rule
    assert (g[a1 != 0] == BALL | 1 << 16).all() and (g[b1 != 0] == BALL).all() and gtab[:, :3].tolist() == [[0, 3, 0], [1, 3, 1]]


def test_overlap_union_and_the_threshold_at_equality_by_hand():
    """4x4: the slot's mask is row 0 (4 pixels), the detection 3 pixels of which 2 lie on it: I = 2, U = 4 + 3 - 2 = 5. At 400 per
    mille 1000 I == 400 U: a match. At 401 it is not: the slot ages, the detection is born in slot 1 with id 1."""
    t, c = _box(4, 4, 0, 1, 0, 4), _box(4, 4, 0, 1, 2, 4)
    c[1, 2] = 1
    assert T.overlap(t[None] != 0, c[None] != 0).tolist() == [[2]]
    one, yes = np.array([3]), np.array([True])
    assert T.candidates(np.array([[2]]), one, np.array([4]), one, np.array([3]), yes, yes, 400) == [(0, 0, 2, 5)]
    assert T.candidates(np.array([[2]]), one, np.array([4]), one, np.array([3]), yes, yes, 401) == []
    assert T.candidates(np.array([[0]]), one, np.array([4]), one, np.array([3]), yes, yes, 1) == []      # I > 0 is required
    tr = T.Tracker()
    _balls(tr, [t])
    _, tab, trk = _balls(tr, [c], iou_permille=400)
    assert tab[:, :3].tolist() == [[0, 3, 0]] and trk.tolist() == [[0, 3, 0, 0, 3, 0]]
    tr = T.Tracker()
    _balls(tr, [t])
    _, tab, trk = _balls(tr, [c], iou_permille=401)
    assert tab[:, :3].tolist() == [[0, 3, 1]] and trk.tolist() == [[0, 3, 0, 1, 4, -1], [1, 3, 1, 0, 3, 0]]


def test_another_class_with_full_overlap_does_not_match():
    t = _box(4, 4, 0, 2, 0, 4)
    tr = T.Tracker()
    tr.track(t[None], [2], [0.9], 4, 4)
    f, tab, trk = tr.track(t[None], [0], [0.9], 4, 4)                            # the same pixels, now a red robot
    assert tab.tolist() == [[0, 1, 0, 8]] and trk.tolist() == [[0, 3, 0, 1, 8, -1], [1, 1, 0, 0, 8, 0]]
    assert (f[:2] == RED).all() and not f[2:].any()


def test_equal_ratios_are_resolved_by_age_then_rank_then_slot():
    age = np.array([1, 0, 0, 0])
    assert T.better((0, 0, 3, 4), (1, 0, 2, 3), age) and not T.better((1, 0, 2, 3), (0, 0, 3, 4), age)   # 3/4 > 2/3 despite the age
    assert T.greedy([(0, 0, 1, 2), (1, 0, 2, 4)], age) == {0: 1}                # 1/2 == 2/4: slot 1 is younger
    assert T.greedy([(1, 1, 2, 4), (1, 0, 1, 2)], age) == {0: 1}                # equal ages: the smaller rank
    assert T.greedy([(2, 0, 1, 2), (1, 0, 1, 2)], age) == {0: 1}                # equal age and rank: the smaller slot
    assert list(T.greedy([(1, 1, 1, 2), (2, 0, 1, 2), (2, 1, 1, 2)], age).items()) == [(0, 2), (1, 1)]   # rank before slot
    assert list(T.greedy([(0, 0, 1, 2), (1, 1, 1, 2)], age).items()) == [(1, 1), (0, 0)]                 # age before rank
    # on masks: two slots hold the same pixels (ids 0 and 1). One detection there: equal ratios, ages and rank, so slot 0 has it.
    # Then both are lost; with the larger slot made the younger one the detection goes to slot 1: the age comes before the slot.
    m = _box(4, 4, 0, 2, 0, 2)
    tr = T.Tracker()
    _balls(tr, [m, m])
    _, tab, trk = _balls(tr, [m])
    assert tab[:, :3].tolist() == [[0, 3, 0]] and trk[:, :4].tolist() == [[0, 3, 0, 0], [1, 3, 1, 1]]
    _balls(tr, [_box(4, 4, 3, 4, 3, 4)])                                        # elsewhere: both age (slot 0 to 1, slot 1 to 2)
    tr.age[[0, 1]] = tr.age[[1, 0]]                                              # (make the larger slot the younger one)
    _, tab, trk = _balls(tr, [m], max_age=5)
    assert tab[:, :3].tolist() == [[0, 3, 1]] and trk[:, :4].tolist() == [[0, 3, 0, 3], [1, 3, 1, 0], [2, 3, 2, 1]]


def test_the_best_pair_blocks_the_second_best_that_shares_its_slot():
    """The slot holds rows 0-1 (8 pixels). Rank 0 is row 0 (I/U = 4/8), rank 1 seven of the eight pixels (7/8): rank 1 takes the
    slot and its id although rank 0 comes first; rank 0 is born with the next id."""
    t, c0, c1 = _box(4, 4, 0, 2, 0, 4), _box(4, 4, 0, 1, 0, 4), _box(4, 4, 0, 2, 0, 4)
    c1[1, 3] = 0
    tr = T.Tracker()
    _balls(tr, [t])
    f, tab, trk = _balls(tr, [c0, c1])
    assert tab.tolist() == [[0, 3, 1, 4], [1, 3, 0, 3]] and trk.tolist() == [[0, 3, 0, 0, 7, 1], [1, 3, 1, 0, 4, 0]]
    assert (f[0] == BALL | 1 << 16).all() and f[1].tolist() == [BALL, BALL, BALL, 0]


def test_memory_a_lost_track_keeps_its_id_for_max_age_calls():
    A, B, N = _box(4, 4, 0, 2, 0, 2), _box(4, 4, 2, 4, 2, 4), _box(4, 4, 0, 2, 2, 4)
    tr = T.Tracker()                                                             # missing for max_age = 2 calls: the id comes back
    _balls(tr, [A, B])
    _, _, trk = _balls(tr, [A])
    assert trk.tolist() == [[0, 3, 0, 0, 4, 0], [1, 3, 1, 1, 4, -1]]
    _, _, trk = _balls(tr, [A])
    assert trk.tolist() == [[0, 3, 0, 0, 4, 0], [1, 3, 1, 2, 4, -1]]
    _, tab, trk = _balls(tr, [B, A])
    assert tab[:, :3].tolist() == [[0, 3, 1], [1, 3, 0]] and trk.tolist() == [[0, 3, 0, 0, 4, 1], [1, 3, 1, 0, 4, 0]]
    tr = T.Tracker()                                                             # a newcomer during the gap does not take the held id
    _balls(tr, [A, B])
    _, tab, trk = _balls(tr, [N, A])
    assert tab[:, :3].tolist() == [[0, 3, 2], [1, 3, 0]] and trk[:, :4].tolist() == [[0, 3, 0, 0], [1, 3, 1, 1], [2, 3, 2, 0]]
    _, tab, _ = _balls(tr, [B, N, A])
    assert tab[:, :3].tolist() == [[0, 3, 1], [1, 3, 2], [2, 3, 0]]
    tr = T.Tracker()                                                             # missing for max_age + 1 calls: dead, then reborn
    _balls(tr, [A, B])
    for k in range(3):
        _, _, trk = _balls(tr, [A])
    assert trk.tolist() == [[0, 3, 0, 0, 4, 0]]
    _, tab, trk = _balls(tr, [N, A])                                             # the smallest free id is 1 again: the newcomer has it
    assert tab[:, :3].tolist() == [[0, 3, 1], [1, 3, 0]] and trk[:, :3].tolist() == [[0, 3, 0], [1, 3, 1]]
    _, tab, _ = _balls(tr, [B, N, A])
    assert tab[:, :3].tolist() == [[0, 3, 2], [1, 3, 1], [2, 3, 0]]
    tr = T.Tracker()                                                             # max_age = 0: alive only while matched every call
    _balls(tr, [A, B], max_age=0)
    _, _, trk = _balls(tr, [A], max_age=0)
    assert trk.tolist() == [[0, 3, 0, 0, 4, 0]]
    _, tab, _ = _balls(tr, [N, A], max_age=0)
    assert tab[:, :3].tolist() == [[0, 3, 1], [1, 3, 0]]
    _, _, trk = _balls(tr, [], max_age=0)
    assert trk.shape == (0, 6)


def test_room_the_oldest_lost_tracks_die_first_then_the_largest_slots():
    """128 single-pixel balls fill the tracker. Slots 0-63 are seen once more, then nobody is: ages 2 (slots 0-63) and 3 (64-127)
    when 100 new balls arrive. No slot is free: the 64 of age 3 die, then the 36 largest slots of age 2 (63 ... 28). The new balls
    take slots 28 ... 127 in rank order and the ids no live ball holds; with 128 new balls every lost track dies."""
    def px(k):
        m = np.zeros((16, 16), np.uint8)
        m.flat[k] = 1
        return m
    for new in (100, 128):
        tr = T.Tracker()
        _balls(tr, [px(k) for k in range(128)], max_age=5)
        _balls(tr, [px(k) for k in range(64)], max_age=5)
        _, _, trk = _balls(tr, [], max_age=5)
        assert trk[:, 3].tolist() == [1] * 64 + [2] * 64
        _, tab, trk = _balls(tr, [px(128 + k) for k in range(new)], max_age=5)
        keep = 128 - new
        assert trk[:keep].tolist() == [[s, 3, s, 2, 1, -1] for s in range(keep)]
        assert trk[keep:].tolist() == [[s, 3, s, 0, 1, s - keep] for s in range(keep, 128)]
        assert tab[:, :3].tolist() == [[c, 3, keep + c] for c in range(new)]


def test_first_call_is_the_instance_frame_the_same_input_is_a_fixed_point_and_reset():
    rng = np.random.default_rng(4)
    masks = I.disc_masks(rng, 20, 10, 12)
    ids, sc = rng.choice((0, 1, 2, 5), 20), np.sort(rng.random(20).astype(np.float32))[::-1]
    want, wtable = I.instance_frame(masks, ids, sc, 17, 9, min_score=float(sc[15]))
    tr = T.Tracker()
    f, tab, trk = tr.track(masks, ids, sc, 17, 9, min_score=float(sc[15]))
    assert np.array_equal(f, want) and np.array_equal(tab, wtable) and len(tab) == len(trk) > 5
    assert np.array_equal(trk[:, 5], tab[:, 0]) and np.array_equal(trk[:, 1:3], tab[:, 1:3]) and not trk[:, 3].any()
    f2, tab2, trk2 = tr.track(masks, ids, sc, 17, 9, min_score=float(sc[15]))
    assert np.array_equal(f2, f) and np.array_equal(tab2, tab) and np.array_equal(trk2, trk)
    perm = rng.permutation(20)                                                   # other ranks, the same masks: every mask keeps its id
    f3, tab3, _ = tr.track(masks[perm], ids[perm], sc, 17, 9)
    old = {int(r[0]): (int(r[1]), int(r[2])) for r in tab}
    assert all((int(r[1]), int(r[2])) == old[int(perm[r[0]])] for r in tab3 if int(perm[r[0]]) in old)
    tr.reset()
    assert tr.table().shape == (0, 6)
    f4, tab4, _ = tr.track(masks, ids, sc, 17, 9, min_score=float(sc[15]))
    assert np.array_equal(f4, want) and np.array_equal(tab4, wtable)


def test_track_symbols_are_declared_and_bound(built):
    from yolact_amd import capi
    L = capi.load_library()
    bound = {s[0]: s for s in capi.SYMBOLS}
    strip = lambda f: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", f)).read(), flags=re.S)
    pub, dbg = strip("yolact_hip.h"), strip("yolact_hip_debug.h")
    for name, src, nargs in (("yh_instance_track", pub, 9), ("yh_instance_tracks_read", pub, 4), ("yh_instance_track_reset", pub, 1),
                             ("yh_op_instance_track", dbg, 17)):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(L, name), name
        assert len(bound[name][2]) == nargs, name
    assert "yh_op_instance_track" not in pub and "#define YH_ABI_VERSION 4" in pub
    sig = inspect.signature(capi.Engine.instance_track).parameters
    assert list(sig)[1:8] == ["frame", "width", "height", "class_map", "min_score", "min_iou", "max_age"]
    assert sig["class_map"].default is None and sig["min_score"].default == 0.0
    assert sig["min_iou"].default == 0.3 and sig["max_age"].default == 2
    assert capi.Engine._permille(0.3) == 300 and capi.Engine._permille(0.0004) == 0 and capi.Engine._permille(1.0) == 1000
    for m in ("tracks", "track_reset", "op_instance_track"):
        assert callable(getattr(capi.Engine, m))


# ---------------------------------------------------------------- GPU, through yh_op_instance_track

@pytest.fixture(scope="module")
def op_eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=1, max_dets=128, use_graph=False)    # no weights: the hook needs none
    yield e
    e.close()


@pytest.fixture
def pair(op_eng):
    """The engine with an empty tracker and an empty restatement beside it."""
    op_eng.track_reset()
    return op_eng, T.Tracker()


def _dets(rng, n, classes=(0, 1, 2, 5)):
    """class ids and strictly descending scores for n detections."""
    return rng.choice(classes, n).astype(np.int32), np.sort(rng.random(n).astype(np.float32))[::-1].copy()


def _step(eng, ref, masks, ids, sc, W, H, permille=300, max_age=2, **kw):
    """One call on both sides: frame, instance table and track table equal."""
    got, table = eng.op_instance_track(masks, ids, sc, W, H, min_iou=permille / 1000, max_age=max_age, **kw)
    want, wtable, wtracks = ref.track(masks, ids, sc, W, H, iou_permille=permille, max_age=max_age, **kw)
    assert np.array_equal(got, want)
    assert np.array_equal(table, wtable) and np.array_equal(eng.instances(), wtable)
    tracks = eng.tracks()
    assert np.array_equal(tracks, wtracks), (tracks.tolist(), wtracks.tolist())
    assert table[:, 3].sum() == np.count_nonzero(got)
    return got, table, tracks


def _device_u32(ptr, n):
    """n uint32 from device memory (the instance frame's device pointer)."""
    path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), "libamdhip64.so")
    hip = C.CDLL(path)
    out = np.zeros(n, np.uint32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0   # hipMemcpyDeviceToHost
    return out


@pytest.mark.gpu
def test_five_by_five_drifting_discs_equal_the_restatement(pair):
    """5x5 -> 7x3: px is no multiple of four (inst_pack's byte path) and less than one wave of inst_overlap."""
    eng, ref = pair
    rng = np.random.default_rng(55)
    masks = I.disc_masks(rng, 12, 5, 5)
    ids, sc = _dets(rng, 12)
    first, table, _ = _step(eng, ref, masks, ids, sc, 7, 3)
    want, wtable = I.instance_frame(masks, ids, sc, 7, 3)
    assert np.array_equal(first, want) and np.array_equal(table, wtable)         # an empty tracker: yh_instance_frame's ids
    _step(eng, ref, masks, ids, sc, 7, 3)                                        # a fixed point
    for k in range(1, 4):
        perm = rng.permutation(12)
        _step(eng, ref, np.roll(masks, k, axis=2)[perm], ids[perm], sc, 7, 3, permille=200)


@pytest.mark.gpu
@pytest.mark.parametrize("classes", [(2,), (0, 1, 2)])
def test_all_masks_full_every_overlap_equal_the_whole_tie_order(pair, classes):
    """8x8, 128 full masks: every entry of I is 64 and every I / U is 1 - the densest walk and nothing but ties: age, rank, slot.
    After the births and the fixed point only ranks 0-63 come (slots 64-127 age), then all 128 again: the younger slots go first."""
    eng, ref = pair
    masks = np.ones((128, 8, 8), np.uint8)
    ids = np.array([classes[k % len(classes)] for k in range(128)], np.int32)
    sc = np.linspace(0.9, 0.1, 128).astype(np.float32)
    _step(eng, ref, masks, ids, sc, 8, 8, permille=1000)
    _, table, tracks = _step(eng, ref, masks, ids, sc, 8, 8, permille=1000)
    assert len(tracks) == 128 and np.array_equal(tracks[:, 5], np.arange(128)) and not tracks[:, 3].any()
    _, _, tracks = _step(eng, ref, masks[:64], ids[64:], sc[:64], 8, 8, permille=1000)
    assert sorted(tracks[:, 3].tolist()) == [0] * 64 + [1] * 64
    _, _, tracks = _step(eng, ref, masks, ids, sc, 8, 8, permille=1000)
    assert len(tracks) == 128 and not tracks[:, 3].any()


@pytest.mark.gpu
def test_full_size_drift_with_private_squares_at_the_word_boundaries(pair):
    """138x138 -> 64x48, 100 discs drifting over four calls in changing rank order: 75 workgroups of inst_overlap merge into one
    matrix. The detections at ranks 31, 32, 63, 64 and 99 of every call each own a square no other mask covers."""
    eng, ref = pair
    rng = np.random.default_rng(7)
    n, own = 100, (31, 32, 63, 64, 99)
    base = I.disc_masks(rng, n, 138, 138, rmax=40)
    base[:, 4:10, :] = 0
    ids, sc = _dets(rng, n, classes=(0, 1, 2))
    order = np.arange(n)
    for call in range(4):
        masks = np.roll(base, 2 * call, axis=2)[order]
        for k, d in enumerate(own):
            masks[d, 4:10, 20 * k + 4:20 * k + 10] = 1
        got, table, tracks = _step(eng, ref, masks, ids[order], sc, 64, 48)
        assert len(table) == n and len(tracks) >= n
        for k, d in enumerate(own):
            assert table[d, 0] == d and table[d, 3] > 0
            assert got[2, int((20 * k + 7) * 64 / 138)] == (int(table[d, 1]) << 24) | (int(table[d, 2]) << 16)
        order = rng.permutation(n)
    assert set(tracks[tracks[:, 5] >= 0][:, 0].tolist()) & {31, 32, 63, 64, 96}, "slots on both sides of the word boundaries are in use"


@pytest.mark.gpu
@pytest.mark.parametrize("max_age", [0, 2])
def test_none_then_max_dets_a_drop_out_and_a_return(pair, max_age):
    eng, ref = pair
    assert eng.cfg.max_dets == 128
    rng = np.random.default_rng(12)
    masks = I.disc_masks(rng, 128, 12, 16, rmax=3)
    ids, sc = _dets(rng, 128, classes=(0, 1, 2))
    _step(eng, ref, masks[:30], ids[:30], sc[:30], 40, 30, max_age=max_age)
    got, table, tracks = _step(eng, ref, masks[:0], ids[:0], sc[:0], 40, 30, max_age=max_age)          # n = 0: everything ages
    assert not got.any() and len(table) == 0 and len(tracks) == (30 if max_age else 0)
    keep = np.r_[0:10, 20:30]
    _step(eng, ref, masks[keep], ids[keep], sc[:20], 40, 30, max_age=max_age)                           # ten stay away
    _step(eng, ref, masks[:30], ids[:30], sc[:30], 40, 30, max_age=max_age)                             # and return
    _, table, tracks = _step(eng, ref, masks, ids, sc, 40, 30, max_age=max_age)                         # n = max_dets
    assert len(table) == 128 and len(tracks) == 128


@pytest.mark.gpu
def test_another_prototype_size_starts_from_an_empty_tracker(pair):
    eng, ref = pair
    rng = np.random.default_rng(9)
    ids, sc = _dets(rng, 10, classes=(2,))
    a, b = I.disc_masks(rng, 10, 6, 4), I.disc_masks(rng, 10, 9, 11)
    _step(eng, ref, a, ids, sc, 17, 9)
    _step(eng, ref, a[::-1], ids, sc, 17, 9)
    _, table, tracks = _step(eng, ref, b, ids, sc, 17, 9)                        # grows the track image; ids from 0 in rank order
    assert table[:, 2].tolist() == list(range(10)) and tracks[:, 0].tolist() == list(range(10))
    _step(eng, ref, b[::-1], ids, sc, 17, 9)
    _, table, _ = _step(eng, ref, a, ids, sc, 17, 9)                             # and back: empty again
    assert table[:, 2].tolist() == list(range(10))


@pytest.mark.gpu
def test_a_rank_permutation_of_the_same_masks_keeps_every_id(pair):
    eng, ref = pair
    rng = np.random.default_rng(21)
    masks = I.disc_masks(rng, 40, 9, 11, rmax=2)
    masks[np.arange(40), np.arange(40) // 11, np.arange(40) % 11] = 1           # (no empty mask, every one distinguishable)
    ids, sc = _dets(rng, 40, classes=(0, 1, 2))
    _, t0, _ = _step(eng, ref, masks, ids, sc, 33, 21, permille=1000)
    perm = rng.permutation(40)
    _, t1, _ = _step(eng, ref, masks[perm], ids[perm], sc, 33, 21, permille=1000)
    same = [k for k in range(40) if not any(np.array_equal(masks[k], masks[j]) and ids[k] == ids[j] for j in range(40) if j != k)]
    assert len(same) >= 20
    for r in t1:
        if perm[r[0]] in same:
            assert r[1:3].tolist() == t0[perm[r[0]], 1:3].tolist()


@pytest.mark.gpu
def test_every_refusal_of_the_hook_leaves_frame_tables_and_tracker_as_they_were(pair):
    import yolact_amd as ya
    eng, ref = pair
    rng = np.random.default_rng(3)
    masks = I.disc_masks(rng, 12, 9, 11)
    ids, sc = _dets(rng, 12, classes=(0, 2, 5, 9))
    cm = np.zeros(80, np.uint8)
    cm[[0, 5, 9]] = (2, 3, 1)
    _step(eng, ref, masks, ids, sc, 33, 21, class_map=cm)
    want, table, tracks = _step(eng, ref, np.roll(masks, 1, axis=1), ids, sc, 33, 21, class_map=cm, min_score=float(sc[9]))
    ptr = eng.instance_device_frame()
    bad = cm.copy()
    bad[0] = 4
    z = np.zeros(129)
    for fn in (lambda: eng.op_instance_track(masks, ids, sc, 0, 21), lambda: eng.op_instance_track(masks, ids, sc, 33, 4097),
               lambda: eng.op_instance_track(masks, ids, sc, 33, 21, class_map=bad),
               lambda: eng.op_instance_track(masks, ids, sc, 33, 21, min_score=float("nan")),
               lambda: eng.op_instance_track(np.zeros((129, 2, 2), np.uint8), z, z, 4, 4),
               lambda: eng.op_instance_track(masks, np.full(12, 80), sc, 33, 21),
               lambda: eng.op_instance_track(masks, ids, sc, 33, 21, min_iou=0.0004),
               lambda: eng.op_instance_track(masks, ids, sc, 33, 21, min_iou=1.001),
               lambda: eng.op_instance_track(masks, ids, sc, 33, 21, max_age=-1),
               lambda: eng.op_instance_track(masks, ids, sc, 33, 21, max_age=256)):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == ya.capi.EINVAL
        assert eng.instance_device_frame() == ptr and np.array_equal(_device_u32(ptr, 33 * 21).reshape(21, 33), want)
        assert np.array_equal(eng.instances(), table) and np.array_equal(eng.tracks(), tracks)
    n = C.c_int32(-1)
    small = np.zeros((1, 6), np.int32)
    assert eng.L.yh_instance_tracks_read(eng.h, C.byref(n), small.ctypes.data_as(C.c_void_p), 1) == ya.capi.EOVERFLOW
    assert n.value == len(tracks) > 1 and not small.any()
    _step(eng, ref, np.roll(masks, 2, axis=1), ids, sc, 33, 21, class_map=cm, permille=1, max_age=255)  # the tracker itself is intact
    _step(eng, ref, masks, ids, sc, 33, 21, class_map=cm, permille=1000, max_age=0)                     # (the bounds are accepted)


# ---------------------------------------------------------------- GPU, through the engine

W0, H0 = 640, 480
WS, HS = 64, 48


@pytest.fixture(scope="module")
def evaluated(built):
    """550 R50, seeded weights, a batch of two noise frames evaluated; both frames' detections and a class map over the classes
    they hold, in the order of their first appearance: ball, red robot, blue robot, ball, ... A class one of whose detections has
    an empty mask (with seeded weights a box crop can leave one) stays unmapped: an empty mask overlaps nothing (I > 0 is
    required), so its track is never matched and "the same detections twice change no id" would not hold for it."""
    import yolact_amd as ya
    eng = ya.Engine(input_size=550, backbone=50, max_batch=2, use_graph=True)
    eng.load_weights(eng.generate_weights(seed=1))
    frames = np.random.default_rng(5).integers(0, 256, (2, 550, 550, 3), dtype=np.uint8)
    eng.set_input(frames)
    eng.evaluate()
    dets = []
    for b in range(2):
        d, masks = eng.detections(b)
        dets.append((masks, np.array([x["class_id"] for x in d], np.int32), np.array([x["score"] for x in d], np.float32)))
    ids = np.concatenate([dets[0][1], dets[1][1]])
    empty = set(ids[~np.concatenate([dets[0][0], dets[1][0]]).any((1, 2))].tolist())
    held = [k for k in dict.fromkeys(ids.tolist()) if k not in empty]
    kept = [int(np.isin(d[1], held).sum()) for d in dets]
    print(f"detections {len(dets[0][1])} / {len(dets[1][1])}, classes with an empty mask {sorted(empty)}, mapped classes {held}, eligible {kept}")
    assert min(kept) >= 20 and len(held) >= 3
    cm = np.zeros(80, np.uint8)
    for i, k in enumerate(held):
        cm[k] = (3, 1, 2)[i % 3]
    yield dict(eng=eng, frames=frames, dets=dets, cm=cm)
    eng.close()


def _engine_step(ev, ref, b, W=WS, H=HS, **kw):
    eng, cm = ev["eng"], ev["cm"]
    got = eng.instance_track(b, W, H, class_map=cm, **kw)
    want, wtable, wtracks = ref.track(*ev["dets"][b], W, H, class_map=cm)
    assert np.array_equal(got, want) and np.array_equal(eng.instances(), wtable) and np.array_equal(eng.tracks(), wtracks)
    assert np.array_equal(_device_u32(eng.instance_device_frame(), W * H).reshape(H, W), want)
    return got, wtable, wtracks


@pytest.mark.gpu
def test_engine_sequence_equals_the_restatement_and_the_untracked_call_leaves_the_tracker_alone(evaluated):
    eng, cm = evaluated["eng"], evaluated["cm"]
    eng.track_reset()
    ref = T.Tracker()
    first, table, tracks = _engine_step(evaluated, ref, 0)
    assert np.array_equal(first, eng.instance_frame(0, WS, HS, class_map=cm)) and np.array_equal(eng.instances(), table)
    assert len(tracks) == len(table) == int((cm[evaluated["dets"][0][1]] != 0).sum()) >= 20
    again, table2, tracks2 = _engine_step(evaluated, ref, 0)                     # frame 0 again: ids unchanged, every age 0
    assert np.array_equal(again, first) and np.array_equal(table2, table) and np.array_equal(tracks2, tracks) and not tracks2[:, 3].any()
    _engine_step(evaluated, ref, 1)
    before = eng.tracks()
    untracked = eng.instance_frame(1, WS, HS, class_map=cm)                      # between two tracked calls
    want1, wtable1 = I.instance_frame(*evaluated["dets"][1], WS, HS, class_map=cm)
    assert np.array_equal(untracked, want1) and np.array_equal(eng.instances(), wtable1) and np.array_equal(eng.tracks(), before)
    _engine_step(evaluated, ref, 0)


@pytest.mark.gpu
def test_device_frame_into_the_scene_puts_the_balls_where_the_restatement_does(evaluated):
    """evaluate -> instance_track -> scene with the class image never on the host: every output of Scene.read(), the ball
    centroids among them, has the bits of a scene fed the restatement's class image from the host."""
    import yolact_amd as ya
    from test_scene import _frame
    eng, cm = evaluated["eng"], evaluated["cm"]
    eng.track_reset()
    ref = T.Tracker()
    ref.track(*evaluated["dets"][0], 8, 8, class_map=cm)                         # (the tracker does not depend on the target size)
    want, wtable, _ = ref.track(*evaluated["dets"][1], W0, H0, class_map=cm)
    assert eng.instance_track(0, 8, 8, class_map=cm, read=False) is None
    assert eng.instance_track(1, W0, H0, class_map=cm, read=False) is None
    assert np.array_equal(eng.instances(), wtable)
    depth, _ = _frame(np.random.default_rng(11), H0, W0)
    a, b = ya.Scene(W0, H0), ya.Scene(W0, H0)
    a.append_classified(depth, frame_dev_ptr=eng.instance_device_frame(), mode=ya.COMPAT_SANE)
    b.append(depth, I.class_image(want), ya.COMPAT_SANE)
    fa, fb = a.read(), b.read()
    for k in fb:
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert (wtable[:, 1] == 3).sum() >= 1 and fa["balls"][:, 2].max() > 0
    a.close(); b.close()


@pytest.mark.gpu
def test_life_cycle_before_any_evaluate_reset_and_destroy_after_a_tracked_call(built):
    import yolact_amd as ya
    eng = ya.Engine(input_size=128, max_batch=1, use_graph=False, conf_thresh=0.005)
    eng.track_reset()                                                            # valid before the first tracked call
    for fn in (lambda: eng.instance_track(0, 8, 8), eng.tracks):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == ya.capi.ESTATE
    eng.load_weights(eng.generate_weights(seed=1))
    eng.set_input(np.random.default_rng(0).integers(0, 256, (1, 128, 128, 3), dtype=np.uint8))
    eng.invoke()
    with pytest.raises(ya.YhError) as e:                                         # yh_invoke only
        eng.instance_track(0, 8, 8)
    assert e.value.code == ya.capi.ESTATE
    eng.evaluate()
    dets, masks = eng.detections(0)
    assert len(dets) > 0
    ids, sc = [d["class_id"] for d in dets], [d["score"] for d in dets]
    cm = np.zeros(80, np.uint8)
    cm[ids[0]] = 3
    with pytest.raises(ya.YhError) as e:
        eng.instance_track(0, 8, 8, class_map=cm, max_age=256)
    assert e.value.code == ya.capi.EINVAL and not eng.instance_device_frame()
    ref = T.Tracker()
    for w, h in ((50, 20), (31, 7)):
        want, wtable, wtracks = ref.track(masks, ids, sc, w, h, class_map=cm)
        assert np.array_equal(eng.instance_track(0, w, h, class_map=cm), want)
        assert np.array_equal(eng.instances(), wtable) and np.array_equal(eng.tracks(), wtracks)
    eng.track_reset()
    assert eng.tracks().shape == (0, 6) and np.array_equal(eng.instances(), wtable)                     # the frame is not touched
    ref.reset()
    want, wtable, wtracks = ref.track(masks, ids, sc, 31, 7, class_map=cm)
    assert np.array_equal(eng.instance_track(0, 31, 7, class_map=cm), want) and np.array_equal(eng.tracks(), wtracks)
    eng.close()


@pytest.mark.gpu
def test_tracked_call_beats_the_numpy_restatement(evaluated):
    """A condition, not a measurement: a tracked call at 138x138 -> 640x480, host copy included, every detection matched to a
    track, must take less than the restatement's cheapest call (its first: births only) on the same detections timed here
    (tools/time_instance.py --track measures the call)."""
    eng, cm = evaluated["eng"], evaluated["cm"]
    eng.track_reset()
    ref = T.Tracker()
    t0 = time.perf_counter()
    want, _, _ = ref.track(*evaluated["dets"][1], W0, H0, class_map=cm)
    took = time.perf_counter() - t0
    runs = []
    for _ in range(6):                                                           # (the first: allocations, warm-up, births)
        t0 = time.perf_counter()
        got = eng.instance_track(1, W0, H0, class_map=cm)
        runs.append(time.perf_counter() - t0)
    dev = sorted(runs[1:])[2]
    print(f"tracked call 640x480, {len(evaluated['dets'][1][1])} detections: {dev * 1e3:.3f} ms with the host copy; numpy restatement {took * 1e3:.1f} ms")
    assert np.array_equal(got, want) and not eng.tracks()[:, 3].any() and dev < took
