"""The instance track batch (yh_instance_track_batch, yh_instance_track_batch_read, yh_instance_track_reset_stream,
yh_op_instance_track_batch; DESIGN.md §11 "Instance track batch"): the frames of a step tracked per camera stream with one wait.
There is no new arithmetic: the batch is exactly one yh_instance_track call per frame, in batch order, on the tracker of the frame's
stream, so every comparison is array_equal - of frame, instance table and track table of every frame against tests/track_ref.py with
one Tracker per stream fed in batch order, and against the single tracked call. CPU part: the surface. GPU part (-m gpu): the hook
at the smallest shapes at which each part of the schedule can go wrong, the engine on its own detections, the join with the scene
batch, every refusal, the neighbours, the life cycle and a floor on time."""
import ctypes as C
import inspect
import os
import re
import time

import numpy as np
import pytest

import instance_ref as I
import track_ref as T
from test_instance_frame import _dets, _device_u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W0, H0 = 640, 480
BALL = 3 << 24


# ---------------------------------------------------------------- CPU

def test_track_batch_symbols_are_declared_exported_and_bound(built):
    from yolact_amd import capi
    L = capi.load_library()
    bound = {s[0]: s for s in capi.SYMBOLS}
    raw = open(os.path.join(ROOT, "include", "yolact_hip.h")).read()
    strip = lambda f: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", f)).read(), flags=re.S)
    pub, dbg = strip("yolact_hip.h"), strip("yolact_hip_debug.h")
    for name, src, nargs in (("yh_instance_track_batch", pub, 11), ("yh_instance_track_batch_read", pub, 5),
                             ("yh_instance_track_reset_stream", pub, 2), ("yh_op_instance_track_batch", dbg, 17)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name), name
        assert name in bound and len(bound[name][2]) == nargs, name
    assert not re.search(r"\byh_op_instance_track_batch\s*\(", pub)
    assert "#define YH_ABI_VERSION 4" in raw and re.search(r"#define\s+YH_TRACK_STREAMS_MAX\s+64\b", raw)
    hpp = open(os.path.join(ROOT, "tiny-object-detection_amd", "host", "yolact.hpp")).read()
    assert re.search(r"\binstance_track_batch\s*\(", hpp) and re.search(r"\btracks_of\s*\(", hpp)


def test_engine_methods_signatures_and_defaults():
    from yolact_amd import capi
    sig = inspect.signature(capi.Engine.instance_track_batch).parameters
    assert list(sig)[1:] == ["first", "n", "width", "height", "class_map", "min_score", "min_iou", "max_age", "streams", "read"]
    assert sig["class_map"].default is None and sig["min_score"].default == 0.0 and sig["min_iou"].default == 0.3
    assert sig["max_age"].default == 2 and sig["streams"].default is None and sig["read"].default is True
    assert list(inspect.signature(capi.Engine.tracks_of).parameters)[1:] == ["b"]
    sig = inspect.signature(capi.Engine.track_reset).parameters
    assert list(sig)[1:] == ["stream"] and sig["stream"].default == 0
    sig = inspect.signature(capi.Engine.op_instance_track_batch).parameters
    assert list(sig)[1:] == ["masks", "class_ids", "scores", "counts", "width", "height", "class_map", "min_score", "min_iou", "max_age",
                             "streams"]
    assert sig["min_iou"].default == 0.3 and sig["max_age"].default == 2 and sig["streams"].default is None


# ---------------------------------------------------------------- GPU, through yh_op_instance_track_batch

class Bank:
    """The restatement's bank: one Tracker per stream, created empty at first use."""
    def __init__(self):
        self.t = {}

    def __getitem__(self, s):
        return self.t.setdefault(int(s), T.Tracker())


@pytest.fixture(scope="module")
def op_eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=1, max_dets=128, use_graph=False)    # no weights: the hook needs none
    yield e
    e.close()


@pytest.fixture
def pair(op_eng):
    """The engine with every tracker empty and an empty bank of restatements beside it."""
    op_eng.track_reset(None)
    return op_eng, Bank()


def _pad(frames, nd=None):
    """A list of per-frame (masks [c][hp][wp], ids [c], scores [c]) as the hook's arrays [nf][nd]..., and the counts."""
    nd = nd or max(1, max(len(f[0]) for f in frames))
    hp, wp = frames[0][0].shape[1:]
    masks, ids, sc = np.zeros((len(frames), nd, hp, wp), np.uint8), np.zeros((len(frames), nd), np.int32), np.zeros((len(frames), nd), np.float32)
    for b, (m, i, s) in enumerate(frames):
        masks[b, :len(m)], ids[b, :len(m)], sc[b, :len(m)] = m, i, s
    return masks, ids, sc, [len(f[0]) for f in frames]


def _batch(eng, bank, frames, W, H, streams=None, permille=300, max_age=2, nd=None, **kw):
    """One tracked batch on both sides: frame, instance table and track table of every frame equal, the device frames too."""
    masks, ids, sc, counts = _pad(frames, nd)
    got, tables, tracks = eng.op_instance_track_batch(masks, ids, sc, counts, W, H, min_iou=permille / 1000, max_age=max_age,
                                                      streams=streams, **kw)
    assert got.shape == (len(frames), H, W)
    assert np.array_equal(_device_u32(eng.instance_batch_device_frames(), got.size).reshape(got.shape), got)
    for b, (m, i, s) in enumerate(frames):
        ref = bank[streams[b] if streams is not None else 0]
        want, wtable, wtracks = ref.track(m, i, s, W, H, iou_permille=permille, max_age=max_age, **kw)
        assert np.array_equal(got[b], want), b
        assert np.array_equal(tables[b], wtable), (b, tables[b].tolist(), wtable.tolist())
        assert np.array_equal(tracks[b], wtracks), (b, tracks[b].tolist(), wtracks.tolist())
        assert tables[b][:, 3].sum() == np.count_nonzero(got[b]), b
    return got, tables, tracks


def _single(eng, ref, frame, W, H, permille=300, max_age=2, **kw):
    """One single tracked call (stream 0) on both sides."""
    got, table = eng.op_instance_track(*frame, W, H, min_iou=permille / 1000, max_age=max_age, **kw)
    want, wtable, wtracks = ref.track(*frame, W, H, iou_permille=permille, max_age=max_age, **kw)
    assert np.array_equal(got, want) and np.array_equal(table, wtable) and np.array_equal(eng.tracks(), wtracks)
    return got, table, eng.tracks()


def _box(hp, wp, y0, y1, x0, x1):
    m = np.zeros((hp, wp), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def _drift(rng, n, hp, wp, calls, classes=(0, 1, 2, 5), rmax=None):
    """`calls` frames of the same n discs, rolled by one more pixel and rank-permuted per frame."""
    base = I.disc_masks(rng, n, hp, wp, rmax=rmax)
    ids, sc = _dets(rng, n, classes)
    out = []
    for k in range(calls):
        perm = rng.permutation(n) if k else np.arange(n)
        out.append((np.roll(base, k, axis=2)[perm], ids[perm], sc))
    return out


@pytest.mark.gpu
def test_five_by_five_one_stream_six_frames_then_a_single_call_then_a_batch_of_one(pair):
    """5x5 -> 7x3: px = 25 is no multiple of four (frame bases misaligned for the pack's byte path) and less than one wave of the
    sweep. n = 6 on one stream is six rounds and a trailing sweep, which the single call made afterwards reads. The same six frames
    on stream 3 bring a second tracker into the same state: a batch of one frame there equals the single call on stream 0."""
    eng, bank = pair
    rng = np.random.default_rng(55)
    fr = _drift(rng, 12, 5, 5, 7)
    got, tables, tracks = _batch(eng, bank, fr[:6], 7, 3, permille=200)
    want, wtable = I.instance_frame(*fr[0], 7, 3)
    assert np.array_equal(got[0], want) and np.array_equal(tables[0], wtable)     # an empty tracker: yh_instance_frame's ids
    assert np.array_equal(eng.tracks(), tracks[5])                                # stream 0 after the call that advanced it last
    _batch(eng, bank, fr[:6], 7, 3, streams=[3] * 6, permille=200)
    one, otable, otracks = _single(eng, bank[0], fr[6], 7, 3, permille=200)       # the trailing sweep was applied
    got, tables, tracks = _batch(eng, bank, fr[6:], 7, 3, streams=[3], permille=200)
    assert np.array_equal(got[0], one) and np.array_equal(tables[0], otable) and np.array_equal(tracks[0], otracks)
    assert len(otracks) >= len(otable) > 0 and (otracks[:, 5] >= 0).sum() == len(otable)


@pytest.mark.gpu
def test_splitting_a_batch_and_interleaving_single_calls_change_nothing(pair):
    eng, bank = pair
    rng = np.random.default_rng(56)
    fr = _drift(rng, 14, 9, 11, 6)
    whole = _batch(eng, bank, fr, 17, 9, streams=[2] * 6)
    a = _batch(eng, bank, fr[:3], 17, 9, streams=[1] * 3)
    b = _batch(eng, bank, fr[3:], 17, 9, streams=[1] * 3)
    for k in range(3):
        for i, x in enumerate((a, b)):
            assert all(np.array_equal(x[j][k], whole[j][3 * i + k]) for j in range(3)), (i, k)
    # stream 0: batch (0, 1), single 2, batch (3, 4), single 5
    _batch(eng, bank, fr[:2], 17, 9)
    g2 = _single(eng, bank[0], fr[2], 17, 9)
    _, t34, k34 = _batch(eng, bank, fr[3:5], 17, 9)
    g5 = _single(eng, bank[0], fr[5], 17, 9)
    assert all(np.array_equal(g2[j], whole[j][2]) and np.array_equal(g5[j], whole[j][5]) for j in range(3))
    assert np.array_equal(k34[1], whole[2][4]) and np.array_equal(t34[0], whole[1][3])


@pytest.mark.gpu
def test_streams_only_one_round_and_the_bank_grows_under_live_trackers(pair):
    """Three frames on streams 0, 5, 63: one round. Each is a fresh tracker's first call - the instance frame. A second call
    continues all three; a third on stream 40 alone, its first use, leaves 5 and 63 intact: they continue afterwards."""
    eng, bank = pair
    rng = np.random.default_rng(57)
    seqs = [_drift(rng, 10, 6, 7, 3, classes=(0, 1, 2)) for _ in range(4)]
    st = [0, 5, 63]
    got, tables, _ = _batch(eng, bank, [seqs[k][0] for k in range(3)], 17, 9, streams=st)
    for k in range(3):
        want, wtable = I.instance_frame(*seqs[k][0], 17, 9)
        assert np.array_equal(got[k], want) and np.array_equal(tables[k], wtable), k
    _batch(eng, bank, [seqs[k][1] for k in range(3)], 17, 9, streams=st)
    _batch(eng, bank, [seqs[3][0]], 17, 9, streams=[40])
    _, tables, tracks = _batch(eng, bank, [seqs[2][2], seqs[1][2], seqs[3][1], seqs[0][2]], 17, 9, streams=[63, 5, 40, 0])
    assert all(len(t) >= 10 for t in tracks) and all(len(t) == 10 for t in tables)


@pytest.mark.gpu
def test_ragged_mix_of_streams_and_counts_at_thirty_three_by_seventeen(pair):
    """561 prototype pixels: three sweep workgroups, the last one partial. Streams [0, 1, 0, 2, 0, 1] with counts (128, 0, 7, 128,
    0, 30): rounds of three, two and one frames, every round another set of active streams. The second batch, on the same frames
    rolled, meets live trackers: the empty frames age theirs."""
    eng, bank = pair
    assert eng.cfg.max_dets == 128
    rng = np.random.default_rng(58)
    st, counts = [0, 1, 0, 2, 0, 1], (128, 0, 7, 128, 0, 30)
    base = [(I.disc_masks(rng, 128, 17, 33, rmax=3),) + _dets(rng, 128, classes=(0, 1, 2)) for _ in range(6)]
    fr = [(m[:c], i[:c], s[:c]) for (m, i, s), c in zip(base, counts)]
    _, tables, tracks = _batch(eng, bank, fr, 40, 30, streams=st, nd=128)
    assert [len(t) for t in tables] == list(counts) and len(tracks[1]) == 0
    assert len(tracks[4]) > 0 and (tracks[4][:, 3] >= 1).all() and (tracks[4][:, 5] == -1).all()   # frame 4 is empty: stream 0 aged
    fr = [(np.roll(m, 1, axis=2)[:c], i[:c], s[:c]) for (m, i, s), c in zip(base, (30, 0, 128, 7, 0, 128))]
    _, tables, tracks = _batch(eng, bank, fr, 40, 30, streams=st, nd=128)
    assert len(tracks[1]) == 30 and (tracks[1][:, 3] == 1).all()                  # frame 1 is empty: stream 1's thirty tracks aged


@pytest.mark.gpu
@pytest.mark.parametrize("max_age", [0, 2])
def test_a_drop_out_and_a_return_inside_one_batch(pair, max_age):
    """Ball B is in frames 0-1, away in 2-3 while a newcomer N arrives, and back in 4. With max_age = 2 B's slot is lost but alive
    through two sweeps (its keep bit and its pixels of T survive them), N gets id 2 and B its id 1 back; with max_age = 0 B dies
    in frame 2, N takes id 1 and B returns as id 2."""
    eng, bank = pair
    A, B, N = _box(8, 8, 0, 3, 0, 3), _box(8, 8, 4, 8, 4, 8), _box(8, 8, 0, 3, 5, 8)
    mk = lambda *ms: (np.stack(ms), np.full(len(ms), 2, np.int32), np.linspace(0.9, 0.5, len(ms)).astype(np.float32))
    fr = [mk(A, B), mk(A, B), mk(A, N), mk(A, N), mk(A, B, N)]
    got, tables, tracks = _batch(eng, bank, fr, 8, 8, max_age=max_age, nd=3)
    assert tables[1][:, :3].tolist() == [[0, 3, 0], [1, 3, 1]]
    if max_age:
        assert tables[3][:, :3].tolist() == [[0, 3, 0], [1, 3, 2]] and tracks[3][1].tolist() == [1, 3, 1, 2, 16, -1]
        assert tables[4][:, :3].tolist() == [[0, 3, 0], [1, 3, 1], [2, 3, 2]]
        assert (got[4][4:, 4:] == BALL | 1 << 16).all()
    else:
        assert tables[3][:, :3].tolist() == [[0, 3, 0], [1, 3, 1]] and len(tracks[3]) == 2
        assert tables[4][:, :3].tolist() == [[0, 3, 0], [1, 3, 2], [2, 3, 1]]


@pytest.mark.gpu
def test_nothing_but_ties_inside_a_batched_launch(pair):
    """8x8, 128 full masks, 1000 per mille: every I / U is 1, so the match is the whole tie order - 128 rounds of inst_match's loop -
    in frames 1 and 2 of one batch: all 128, ranks 0-63 only (slots 64-127 age), all 128 again."""
    eng, bank = pair
    masks = np.ones((128, 8, 8), np.uint8)
    ids, sc = np.full(128, 2, np.int32), np.linspace(0.9, 0.1, 128).astype(np.float32)
    fr = [(masks, ids, sc), (masks[:64], ids[:64], sc[:64]), (masks, ids, sc)]
    _, _, tracks = _batch(eng, bank, fr, 8, 8, permille=1000)
    assert sorted(tracks[1][:, 3].tolist()) == [0] * 64 + [1] * 64
    assert len(tracks[2]) == 128 and not tracks[2][:, 3].any()


@pytest.mark.gpu
def test_room_inside_one_batch(pair):
    """16x16, 128 one-pixel balls fill the tracker, 64 of them come again, nobody, then 100 new ones: the 64 oldest lost tracks
    die, then the 36 largest slots of the younger ones (tests/test_instance_track.py has the single calls) - as frames 0-3 of one batch."""
    eng, bank = pair

    def px(ks):
        m = np.zeros((len(ks), 256), np.uint8)
        m[np.arange(len(ks)), ks] = 1
        return m.reshape(-1, 16, 16), np.full(len(ks), 2, np.int32), np.linspace(0.9, 0.5, len(ks)).astype(np.float32) if len(ks) else np.zeros(0, np.float32)

    fr = [px(np.arange(128)), px(np.arange(64)), px(np.arange(0)), px(128 + np.arange(100))]
    _, tables, tracks = _batch(eng, bank, fr, 4, 4, max_age=5, nd=128)
    assert tracks[2][:, 3].tolist() == [1] * 64 + [2] * 64
    assert tracks[3][:28].tolist() == [[s, 3, s, 2, 1, -1] for s in range(28)]
    assert tracks[3][28:].tolist() == [[s, 3, s, 0, 1, s - 28] for s in range(28, 128)]
    assert tables[3][:, :3].tolist() == [[c, 3, 28 + c] for c in range(100)]


@pytest.mark.gpu
def test_full_size_two_frames_with_private_squares_at_the_word_boundaries(pair):
    """138x138 -> 64x48, one stream, n = 2: 75 sweep workgroups merge into each frame's matrix. 100 discs, drifted and in another
    rank order in frame 1; the detections at ranks 31, 32, 63, 64 and 99 of each frame own a square no other mask covers."""
    eng, bank = pair
    rng = np.random.default_rng(7)
    n, own = 100, (31, 32, 63, 64, 99)
    base = I.disc_masks(rng, n, 138, 138, rmax=40)
    base[:, 4:10, :] = 0
    ids, sc = _dets(rng, n, classes=(0, 1, 2))
    fr = []
    for order in (np.arange(n), rng.permutation(n)):
        masks = np.roll(base, 2 * len(fr), axis=2)[order]
        for k, d in enumerate(own):
            masks[d, 4:10, 20 * k + 4:20 * k + 10] = 1
        fr.append((masks, ids[order], sc))
    got, tables, tracks = _batch(eng, bank, fr, 64, 48)
    for b in range(2):
        assert len(tables[b]) == n and len(tracks[b]) >= n
        for k, d in enumerate(own):
            assert tables[b][d, 0] == d and tables[b][d, 3] > 0
            assert got[b][2, int((20 * k + 7) * 64 / 138)] == (int(tables[b][d, 1]) << 24) | (int(tables[b][d, 2]) << 16)
    seen = set(tracks[1][tracks[1][:, 5] >= 0][:, 0].tolist())
    assert seen & {31, 32, 63, 64, 96}, "slots on both sides of the word boundaries are in use"
    assert not np.array_equal(tables[1][:, 2], I.instance_frame(*fr[1], 64, 48)[1][:, 2])   # (the ids follow the masks, not the ranks)


@pytest.mark.gpu
def test_every_refusal_leaves_the_batch_and_every_tracker_as_they_were(pair):
    import yolact_amd as ya
    eng, bank = pair
    rng = np.random.default_rng(3)
    fr = _drift(rng, 12, 9, 11, 7, classes=(0, 2, 5, 9))
    cm = np.zeros(80, np.uint8)
    cm[[0, 5, 9]] = (2, 3, 1)
    st = [0, 5, 0]
    _batch(eng, bank, fr[:3], 33, 21, streams=st, class_map=cm)
    got, tables, tracks = _batch(eng, bank, fr[1:4], 33, 21, streams=st, class_map=cm, min_score=float(fr[0][2][9]))
    ptr, t0 = eng.instance_batch_device_frames(), eng.tracks()
    assert np.array_equal(t0, tracks[2])
    masks, ids, sc, counts = _pad(fr[4:7])
    bad = cm.copy()
    bad[0] = 4
    z = np.zeros((65, 1))
    op = eng.op_instance_track_batch
    for fn in (lambda: op(masks[:0], ids[:0], sc[:0], [], 33, 21), lambda: op(np.zeros((65, 1, 2, 2), np.uint8), z, z, [1] * 65, 4, 4),
               lambda: op(masks, ids, sc, counts, 33, 21, streams=[0, -1, 0]), lambda: op(masks, ids, sc, counts, 33, 21, streams=[0, 5, 64]),
               lambda: op(masks, ids, sc, counts, 33, 21, min_iou=0.0004), lambda: op(masks, ids, sc, counts, 33, 21, min_iou=1.001),
               lambda: op(masks, ids, sc, counts, 33, 21, max_age=-1), lambda: op(masks, ids, sc, counts, 33, 21, max_age=256),
               lambda: op(masks, ids, sc, counts, 0, 21), lambda: op(masks, ids, sc, counts, 33, 4097),
               lambda: op(masks, ids, sc, counts, 33, 21, class_map=bad),
               lambda: op(masks, ids, sc, counts, 33, 21, min_score=float("nan"))):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == ya.capi.EINVAL, str(e.value)
        assert eng.instance_batch_device_frames() == ptr and np.array_equal(_device_u32(ptr, got.size).reshape(got.shape), got)
        for b in range(3):
            assert np.array_equal(eng.instances_of(b), tables[b]) and np.array_equal(eng.tracks_of(b), tracks[b]), b
        assert np.array_equal(eng.tracks(), t0)
    with pytest.raises(ya.YhError) as e:
        op(masks, ids, sc, counts, 33, 21, streams=[0, 5, 64])
    assert "frame 2" in str(e.value)                                             # the message names the frame
    n = C.c_int32(-1)
    small = np.zeros((1, 6), np.int32)
    assert eng.L.yh_instance_track_batch_read(eng.h, 1, C.byref(n), small.ctypes.data_as(C.c_void_p), 1) == ya.capi.EOVERFLOW
    assert n.value == len(tracks[1]) > 1 and not small.any()
    with pytest.raises(ya.YhError) as e:
        eng.tracks_of(3)
    assert e.value.code == ya.capi.EINVAL
    _batch(eng, bank, fr[4:7], 33, 21, streams=st, class_map=cm, permille=1, max_age=255)     # every tracker is intact
    _batch(eng, bank, fr[:3], 33, 21, streams=[5, 0, 63], class_map=cm, permille=1000, max_age=0)   # (the bounds are accepted)


@pytest.mark.gpu
def test_neighbours_leave_each_other_alone_and_the_resets(pair):
    import yolact_amd as ya
    eng, bank = pair
    rng = np.random.default_rng(21)
    fr = _drift(rng, 10, 9, 11, 12, classes=(0, 1, 2))
    st = [0, 5]
    got, tables, tracks = _batch(eng, bank, fr[0:2], 17, 9, streams=st)
    one, otable = eng.op_instance_frame(*fr[9], 17, 9)                            # an untracked single frame between two tracked batches
    optr = eng.instance_device_frame()
    assert np.array_equal(_device_u32(eng.instance_batch_device_frames(), got.size).reshape(got.shape), got)
    assert all(np.array_equal(eng.instances_of(b), tables[b]) and np.array_equal(eng.tracks_of(b), tracks[b]) for b in range(2))
    _batch(eng, bank, fr[2:4], 17, 9, streams=st)                                # ... changed no tracker
    assert eng.instance_device_frame() == optr and np.array_equal(eng.instances(), otable)   # and the batch left the single frame alone
    assert np.array_equal(_device_u32(optr, 17 * 9).reshape(9, 17), one)
    before = eng.tracks()
    masks, ids, sc, counts = _pad(fr[4:6])
    plain, ptables = eng.op_instance_batch(masks, ids, sc, counts, 17, 9)         # a plain batch replaces the frames
    for b in range(2):
        want, wtable = I.instance_frame(*fr[4 + b], 17, 9)
        assert np.array_equal(plain[b], want) and np.array_equal(eng.instances_of(b), wtable), b
    with pytest.raises(ya.YhError) as e:
        eng.tracks_of(0)
    assert e.value.code == ya.capi.ESTATE and np.array_equal(eng.tracks(), before)
    _batch(eng, bank, fr[4:6], 17, 9, streams=st)                                # ... and left every tracker alone
    eng.track_reset(stream=5)                                                    # only stream 5
    bank[5].reset()
    _, tables, _ = _batch(eng, bank, fr[6:8], 17, 9, streams=st)
    assert tables[1][:, 2].tolist() == I.instance_frame(*fr[7], 17, 9)[1][:, 2].tolist()
    eng.track_reset(None)                                                        # all
    assert eng.tracks().shape == (0, 6)
    got, tables, _ = _batch(eng, Bank(), fr[8:10], 17, 9, streams=st)
    for b in range(2):
        want, wtable = I.instance_frame(*fr[8 + b], 17, 9)
        assert np.array_equal(got[b], want) and np.array_equal(tables[b], wtable), b
    with pytest.raises(ya.YhError) as e:
        eng.track_reset(stream=64)
    assert e.value.code == ya.capi.EINVAL


@pytest.mark.gpu
def test_another_prototype_size_starts_that_stream_from_an_empty_tracker(pair):
    eng, bank = pair
    rng = np.random.default_rng(9)
    a, b = _drift(rng, 10, 6, 4, 3, classes=(2,)), _drift(rng, 10, 9, 11, 2, classes=(2,))
    _batch(eng, bank, a[:2], 17, 9, streams=[0, 7])
    _, tables, _ = _batch(eng, bank, b, 17, 9, streams=[7, 7])                    # stream 7 at another size: ids from 0 in rank order
    assert tables[0][:, 2].tolist() == list(range(10))
    _, tables, tracks = _batch(eng, bank, a[2:], 17, 9)                          # stream 0 still holds the first size's tracks
    assert len(tracks[0]) >= 10 and bank[0].shape == (6, 4) and bank[7].shape == (9, 11)


# ---------------------------------------------------------------- GPU, through the engine

WS, HS = 64, 48


@pytest.fixture(scope="module")
def evaluated(built):
    """550 R50, seeded weights, a batch of three noise frames evaluated; the frames' detections and a class map over the classes
    they hold except those one of whose detections has an empty mask (tests/test_instance_track.py says why)."""
    import yolact_amd as ya
    eng = ya.Engine(input_size=550, backbone=50, max_batch=3, use_graph=True)
    eng.load_weights(eng.generate_weights(seed=1))
    frames = np.random.default_rng(5).integers(0, 256, (3, 550, 550, 3), dtype=np.uint8)
    eng.set_input(frames)
    eng.evaluate()
    dets = []
    for b in range(3):
        d, masks = eng.detections(b)
        dets.append((masks, np.array([x["class_id"] for x in d], np.int32), np.array([x["score"] for x in d], np.float32)))
    ids = np.concatenate([d[1] for d in dets])
    empty = set(ids[~np.concatenate([d[0] for d in dets]).any((1, 2))].tolist())
    held = [k for k in dict.fromkeys(ids.tolist()) if k not in empty]
    assert min(int(np.isin(d[1], held).sum()) for d in dets) >= 20 and len(held) >= 3
    cm = np.zeros(80, np.uint8)
    for i, k in enumerate(held):
        cm[k] = (3, 1, 2)[i % 3]
    yield dict(eng=eng, frames=frames, dets=dets, cm=cm)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("streams", [None, [0, 1, 0]])
def test_engine_batch_equals_the_single_calls_and_the_restatement(evaluated, streams):
    eng, cm, dets = evaluated["eng"], evaluated["cm"], evaluated["dets"]
    st = streams or [0, 0, 0]
    eng.track_reset(None)
    singles = {}
    for b in (b for b in range(3) if st[b] == 0):                                # stream 0's frames through instance_track, in order
        f = eng.instance_track(b, WS, HS, class_map=cm)
        singles[b] = (f, eng.instances(), eng.tracks())
    sptr, stable = eng.instance_device_frame(), eng.instances()
    eng.track_reset(None)
    got = eng.instance_track_batch(0, 3, WS, HS, class_map=cm, streams=streams)
    dev = _device_u32(eng.instance_batch_device_frames(), 3 * WS * HS).reshape(3, HS, WS)
    assert np.array_equal(dev, got) and got[0].any()
    assert eng.instance_device_frame() == sptr and np.array_equal(eng.instances(), stable)   # the single frame is not touched
    bank = Bank()
    for b in range(3):
        want, wtable, wtracks = bank[st[b]].track(*dets[b], WS, HS, class_map=cm)
        assert np.array_equal(got[b], want) and np.array_equal(eng.instances_of(b), wtable) and np.array_equal(eng.tracks_of(b), wtracks), b
        if b in singles:
            f, table, tracks = singles[b]
            assert np.array_equal(got[b], f) and np.array_equal(eng.instances_of(b), table) and np.array_equal(eng.tracks_of(b), tracks), b
    assert np.array_equal(eng.tracks(), eng.tracks_of(2))
    if streams:                                                                  # stream 1's first frame: the instance frame
        assert np.array_equal(got[1], eng.instance_frame(1, WS, HS, class_map=cm)) and np.array_equal(eng.instances_of(1), eng.instances())
    f = eng.instance_track(1, WS, HS, class_map=cm)                              # a single call continues stream 0 after the batch
    want, wtable, wtracks = bank[0].track(*dets[1], WS, HS, class_map=cm)
    assert np.array_equal(f, want) and np.array_equal(eng.instances(), wtable) and np.array_equal(eng.tracks(), wtracks)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.gpu
def test_device_frames_into_the_scene_batch_equal_the_restatement_fed_from_the_host(evaluated):
    """evaluate -> instance_track_batch(read=False) -> stage_frames from the device pointer -> append(3, SANE) with the frames never
    on the host: every output of read(b) has the bits of a scene batch fed the restatement's frames from the host."""
    import yolact_amd as ya
    from test_scene import _frame
    eng, cm, dets = evaluated["eng"], evaluated["cm"], evaluated["dets"]
    eng.track_reset(None)
    st = [0, 1, 0]
    assert eng.instance_track_batch(0, 3, W0, H0, class_map=cm, streams=st, read=False) is None
    bank = Bank()
    want = np.stack([bank[st[b]].track(*dets[b], W0, H0, class_map=cm)[0] for b in range(3)])
    depths = np.stack([_frame(np.random.default_rng(40 + b), H0, W0)[0] for b in range(3)])
    a, s = ya.SceneBatch(W0, H0, 3), ya.SceneBatch(W0, H0, 3)
    a.stage_frames(0, depths, frames_dev_ptr=eng.instance_batch_device_frames())
    s.stage_frames(0, depths, frames_u32=want)
    a.append(3, ya.COMPAT_SANE); s.append(3, ya.COMPAT_SANE)
    for b in range(3):
        ra, rs = a.read(b), s.read(b)
        assert ra.keys() == rs.keys()
        for k in rs:
            assert ra[k].shape == rs[k].shape and np.array_equal(_bits(ra[k]), _bits(rs[k])), (b, k)
    assert a.read(0)["map"].any()
    a.close(); s.close()


@pytest.mark.gpu
def test_life_cycle_states_frames_outside_the_step_and_destroy_with_several_streams_live(built):
    import yolact_amd as ya
    eng = ya.Engine(input_size=128, max_batch=2, use_graph=False, conf_thresh=0.005)
    eng.track_reset(None)                                                        # valid before anything
    for fn in (lambda: eng.instance_track_batch(0, 1, 8, 8), lambda: eng.tracks_of(0)):
        with pytest.raises(ya.YhError) as e:                                     # no evaluate, no batch
            fn()
        assert e.value.code == ya.capi.ESTATE
    eng.load_weights(eng.generate_weights(seed=1))
    eng.set_input(np.random.default_rng(0).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8))
    eng.invoke()
    with pytest.raises(ya.YhError) as e:                                         # yh_invoke only
        eng.instance_track_batch(0, 2, 8, 8)
    assert e.value.code == ya.capi.ESTATE
    eng.evaluate()
    d = [eng.detections(b) for b in range(2)]
    assert len(d[0][0]) > 0
    cm = np.zeros(80, np.uint8)
    cm[d[0][0][0]["class_id"]] = 3
    for first, n in ((0, 0), (0, 3), (1, 2), (2, 1), (-1, 1)):
        with pytest.raises(ya.YhError) as e:
            eng.instance_track_batch(first, n, 8, 8, class_map=cm)
        assert e.value.code == ya.capi.EINVAL, (first, n)
    assert not eng.instance_batch_device_frames()
    bank = Bank()
    for (w, h), st in (((50, 20), [7, 9]), ((31, 7), [9, 0])):
        got = eng.instance_track_batch(0, 2, w, h, class_map=cm, streams=st)
        for b in range(2):
            masks, ids, sc = d[b][1], [x["class_id"] for x in d[b][0]], [x["score"] for x in d[b][0]]
            want, wtable, wtracks = bank[st[b]].track(masks, ids, sc, w, h, class_map=cm)
            assert np.array_equal(got[b], want) and np.array_equal(eng.instances_of(b), wtable) and np.array_equal(eng.tracks_of(b), wtracks)
    eng.close()                                                                  # streams 0, 7 and 9 are live


@pytest.mark.gpu
def test_one_tracked_batch_beats_the_same_frames_tracked_one_by_one(evaluated):
    """A condition, not a measurement (tools/time_instance_batch.py --track measures): the step's three frames at 640x480 on ONE
    stream - the chain's worst case, three rounds - through one instance_track_batch(read=False) against three
    instance_track(read=False), alternated in this process; median of five, not counting the first of each."""
    eng, cm = evaluated["eng"], evaluated["cm"]
    eng.track_reset(None)

    def batch():
        eng.instance_track_batch(0, 3, W0, H0, class_map=cm, read=False)

    def singles():
        for b in range(3):
            eng.instance_track(b, W0, H0, class_map=cm, read=False)

    def clock(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

    tb, ts = [], []
    for _ in range(6):
        tb.append(clock(batch)); ts.append(clock(singles))
    mb, ms = sorted(tb[1:])[2], sorted(ts[1:])[2]
    print(f"three frames tracked on one stream at 640x480: batch {mb:.3f} ms, three singles {ms:.3f} ms, ratio {mb / ms:.3f}")
    assert mb < ms
