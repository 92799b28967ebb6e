"""The instance batch (yh_instance_batch, yh_instance_batch_read, yh_scene_batch_stage_frames, yh_op_instance_batch; DESIGN.md §11
"Instance batch"): every frame of a step painted in one pair of launches, and n slots of a scene batch staged in one call. There is no
new arithmetic: frame b of a batch is what yh_instance_frame gives for that frame, so every comparison is array_equal - against the
restatement (tests/instance_ref.py) per frame and against the single-frame call. CPU part: the surface and the argument checks of
SceneBatch.stage_frames. GPU part (-m gpu): the hook at tiny and full shapes, the engine on its own detections (frames 1 and 2 of a
batch of 3), the join with the scene batch and its planner, every refusal, the life cycle and a floor on time."""
import ctypes as C
import inspect
import os
import re
import time

import numpy as np
import pytest

import instance_ref as I
from test_instance_frame import _dets, _device_u32
from test_scene import _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W0, H0 = 640, 480


# ---------------------------------------------------------------- CPU

def test_batch_symbols_are_declared_and_bound():
    from yolact_amd import capi
    bound = {s[0]: s for s in capi.SYMBOLS}
    strip = lambda f: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", f)).read(), flags=re.S)
    pub, dbg = strip("yolact_hip.h"), strip("yolact_hip_debug.h")
    for name, src, nargs in (("yh_instance_batch", pub, 8), ("yh_instance_batch_device_frames", pub, 1), ("yh_instance_batch_read", pub, 5),
                             ("yh_scene_batch_stage_frames", pub, 6), ("yh_op_instance_batch", dbg, 14)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in bound and len(bound[name][2]) == nargs, name
    assert not re.search(r"\byh_op_instance_batch\s*\(", pub) and "#define YH_ABI_VERSION 4" in pub
    sig = inspect.signature(capi.Engine.instance_batch).parameters
    assert list(sig)[1:] == ["first", "n", "width", "height", "class_map", "min_score", "read"]
    assert sig["class_map"].default is None and sig["min_score"].default == 0.0 and sig["read"].default is True
    for m in ("instance_batch_device_frames", "instances_of", "op_instance_batch"):
        assert callable(getattr(capi.Engine, m)), m
    sig = inspect.signature(capi.SceneBatch.stage_frames).parameters
    assert list(sig)[1:] == ["first_slot", "depths", "frames_u32", "frames_dev_ptr"]
    hpp = open(os.path.join(ROOT, "tiny-object-detection_amd", "host", "yolact.hpp")).read()
    assert re.search(r"\binstance_batch\s*\(", hpp) and re.search(r"\binstance_batch_device_frames\s*\(", hpp)


def test_library_exports_the_batch_symbols(built):
    from yolact_amd import capi
    L = capi.load_library()
    for name in ("yh_instance_batch", "yh_instance_batch_device_frames", "yh_instance_batch_read", "yh_scene_batch_stage_frames",
                 "yh_op_instance_batch"):
        assert hasattr(L, name), name


def test_stage_frames_refuses_bad_arguments_before_any_call():
    """The checks that need no device: they are made before the library is called (the object here has no handle at all)."""
    from yolact_amd import capi
    sb = capi.SceneBatch.__new__(capi.SceneBatch)
    sb.h, sb.L, sb.W, sb.H, sb.max_frames, sb.n = None, None, 6, 4, 3, 0
    depths, frames = np.zeros((2, 4, 6), np.uint16), np.zeros((2, 4, 6), np.uint32)
    for fn in (lambda: sb.stage_frames(0, depths),                                     # neither source
               lambda: sb.stage_frames(0, depths, frames_u32=frames, frames_dev_ptr=1234),   # both
               lambda: sb.stage_frames(0, depths[0], frames_u32=frames),               # one frame's depth, not [n][h][w]
               lambda: sb.stage_frames(0, np.zeros((2, 6, 4), np.uint16), frames_u32=frames),   # transposed
               lambda: sb.stage_frames(0, depths, frames_u32=frames[:1]),              # fewer frames than depths
               lambda: sb.stage_frames(0, depths, frames_dev_ptr=0)):                  # a null device pointer
        with pytest.raises(ValueError):
            fn()


# ---------------------------------------------------------------- GPU, through yh_op_instance_batch

@pytest.fixture(scope="module")
def op_eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=1, use_graph=False)                  # no weights: the hook needs none
    yield e
    e.close()


def _case(rng, nf, nd, hp, wp, classes=(0, 1, 2, 5), rmax=None):
    """nf frames of nd seeded detections each, different per frame."""
    masks = np.stack([I.disc_masks(rng, nd, hp, wp, rmax=rmax) for _ in range(nf)])
    ds = [_dets(rng, nd, classes) for _ in range(nf)]
    return masks, np.stack([d[0] for d in ds]), np.stack([d[1] for d in ds])


def _check(eng, masks, ids, sc, counts, W, H, single=True, **kw):
    """The batch against the restatement of every frame, against the single-frame hook, and its own counts."""
    got, tables = eng.op_instance_batch(masks, ids, sc, counts, W, H, **kw)
    assert got.shape == (len(counts), H, W)
    dev = _device_u32(eng.instance_batch_device_frames(), got.size).reshape(got.shape)
    assert np.array_equal(dev, got)
    for b, c in enumerate(counts):
        want, wtable = I.instance_frame(masks[b, :c], ids[b, :c], sc[b, :c], W, H, **kw)
        assert np.array_equal(got[b], want), b
        assert np.array_equal(tables[b], wtable), b
        assert tables[b][:, 3].sum() == np.count_nonzero(got[b]), b
        if single:
            one, otable = eng.op_instance_frame(masks[b, :c], ids[b, :c], sc[b, :c], W, H, **kw)
            assert np.array_equal(got[b], one) and np.array_equal(tables[b], otable), b
    if single:                                                                   # the single calls did not disturb the batch
        assert np.array_equal(_device_u32(eng.instance_batch_device_frames(), got.size).reshape(got.shape), got)
        assert all(np.array_equal(eng.instances_of(b), tables[b]) for b in range(len(counts)))
    return got, tables


@pytest.mark.gpu
def test_ties_three_frames_with_different_detections(op_eng):
    """6x4 -> 17x9 has 71 ties (tests/test_instance_frame.py); n = 3, every frame its own 20 detections."""
    rng = np.random.default_rng(617)
    masks, ids, sc = _case(rng, 3, 20, 6, 4)
    got, tables = _check(op_eng, masks, ids, sc, [20, 20, 20], 17, 9)
    assert got[0].any() and not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    assert [len(t) for t in tables] == [int((ids[b] != 5).sum()) for b in range(3)]


@pytest.mark.gpu
def test_the_byte_path_at_a_misaligned_frame_base(op_eng):
    """5x5 -> 7x3 with n_dets = 3: px = 25 and a frame is 75 bytes, so frames 1 and 2 start at odd offsets of the mask buffer."""
    rng = np.random.default_rng(57)
    masks, ids, sc = _case(rng, 3, 3, 5, 5, classes=(0, 1, 2))
    masks[:, 0, 2, :] = 1                                                        # (every frame paints something)
    got, tables = _check(op_eng, masks, ids, sc, [3, 3, 3], 7, 3)
    assert all(g.any() for g in got) and all(len(t) == 3 for t in tables)
    _check(op_eng, masks, ids, sc, [3, 2, 1], 7, 3, single=False)                # the counts differ too


@pytest.mark.gpu
def test_no_state_leaks_between_frames(op_eng):
    """Counts (max_dets, 0, 1, max_dets) at 10x10 -> 5x3: the empty frame is all zeros with an empty table between two full ones,
    and every frame's pixel counts sum to its own non-zero pixels (_check)."""
    md = op_eng.cfg.max_dets
    assert md == 100
    rng = np.random.default_rng(105)
    masks, ids, sc = _case(rng, 4, md, 10, 10, classes=(0, 1, 2))
    got, tables = _check(op_eng, masks, ids, sc, [md, 0, 1, md], 5, 3)
    assert not got[1].any() and tables[1].shape == (0, 4)
    assert len(tables[0]) == md and len(tables[2]) == 1 and len(tables[3]) == md
    assert got[0].any() and got[3].any() and not np.array_equal(got[0], got[3])


@pytest.mark.gpu
def test_full_size_with_private_regions_in_frame_one(op_eng):
    """138x138 -> 640x480, n = 2, 100 discs each. In frame 1 (not 0) ranks 31, 32, 63, 64 and 99 each own a square no other mask
    covers: the last and first bits of the words of the 128-bit set. Frame 0 is another layout."""
    rng = np.random.default_rng(7)
    n, own = 100, (31, 32, 63, 64, 99)
    masks, ids, sc = _case(rng, 2, n, 138, 138, classes=(0, 1, 2), rmax=40)
    for k, d in enumerate(own):
        masks[1, :, 4:10, 20 * k + 4:20 * k + 10] = 0
        masks[1, d, 4:10, 20 * k + 4:20 * k + 10] = 1
    got, tables = _check(op_eng, masks, ids, sc, [n, n], W0, H0, single=False)
    assert not np.array_equal(got[0], got[1])
    vals = {int(r[0]): (int(r[1]) << 24) | (int(r[2]) << 16) for r in tables[1]}
    for k, d in enumerate(own):
        x, y = int((20 * k + 7) * W0 / 138), int(7 * H0 / 138)
        assert got[1][y, x] == vals[d], d
        assert tables[1][tables[1][:, 0] == d][0, 3] > 0
    one, otable = op_eng.op_instance_frame(masks[1], ids[1], sc[1], W0, H0)       # the single call on frame 1
    assert np.array_equal(got[1], one) and np.array_equal(tables[1], otable)


@pytest.mark.gpu
def test_frames_do_not_share_thresholds(op_eng):
    """min_score equals the score of rank 4 of frame 0 only (an eligible detection, kept: >=); frame 1's scores lie elsewhere, so the
    same threshold cuts it at another rank. Then a class map with zeros: the classes mapped to zero neither paint nor occlude, in
    every frame."""
    rng = np.random.default_rng(3)
    masks, ids, sc = _case(rng, 2, 12, 9, 11, classes=(0, 2, 5, 9))
    ms = float(sc[0, 4])
    assert ids[0, 4] == 2 and ms not in sc[1].tolist() and (sc[1] >= np.float32(ms)).sum() != 5
    _, tables = _check(op_eng, masks, ids, sc, [12, 12], 33, 21, min_score=ms)
    assert tables[0][:, 0].max() == 4
    assert set(tables[1][:, 0].tolist()) == {d for d in range(12) if sc[1, d] >= np.float32(ms) and ids[1, d] in (0, 2)}
    cm = np.zeros(80, np.uint8)
    cm[[5, 9]] = (3, 1)
    _, tables = _check(op_eng, masks, ids, sc, [12, 12], 33, 21, class_map=cm)
    for b in range(2):
        assert set(tables[b][:, 0].tolist()) == {d for d in range(12) if ids[b, d] in (5, 9)}


@pytest.mark.gpu
def test_a_smaller_batch_after_a_larger_one_and_the_hooks_refusals(op_eng):
    """Per-call state: n = 3 at 12x16 -> 40x30, then n = 2 at 6x4 -> 17x9 in the same buffers: read(2) is refused, frames 0 and 1
    are the new ones. Every refusal of the hook leaves that batch readable."""
    import yolact_amd as ya
    rng = np.random.default_rng(11)
    masks, ids, sc = _case(rng, 3, 16, 12, 16)
    _check(op_eng, masks, ids, sc, [16, 9, 16], 40, 30)
    ptr = op_eng.instance_batch_device_frames()
    masks, ids, sc = _case(rng, 2, 20, 6, 4)
    got, tables = _check(op_eng, masks, ids, sc, [20, 20], 17, 9)
    assert op_eng.instance_batch_device_frames() == ptr                          # the buffers are reused
    EINVAL = ya.capi.EINVAL
    bad = np.zeros(80, np.uint8)
    bad[0] = 4
    for fn in (lambda: op_eng.instances_of(2), lambda: op_eng.instances_of(-1),
               lambda: op_eng.op_instance_batch(masks, ids, sc, [20, 21], 17, 9), lambda: op_eng.op_instance_batch(masks, ids, sc, [-1, 2], 17, 9),
               lambda: op_eng.op_instance_batch(masks, ids, sc, [20, 20], 0, 9), lambda: op_eng.op_instance_batch(masks, ids, sc, [20, 20], 17, 4097),
               lambda: op_eng.op_instance_batch(masks, ids, sc, [20, 20], 17, 9, class_map=bad),
               lambda: op_eng.op_instance_batch(masks, ids, sc, [20, 20], 17, 9, min_score=float("nan")),
               lambda: op_eng.op_instance_batch(np.zeros((1, 101, 2, 2), np.uint8), np.zeros((1, 101)), np.zeros((1, 101)), [1], 4, 4),
               lambda: op_eng.op_instance_batch(np.zeros((65, 1, 2, 2), np.uint8), np.zeros((65, 1)), np.zeros((65, 1)), [1] * 65, 4, 4)):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == EINVAL
        assert op_eng.instance_batch_device_frames() == ptr
        assert all(np.array_equal(op_eng.instances_of(b), tables[b]) for b in range(2))
        assert np.array_equal(_device_u32(ptr, got.size).reshape(got.shape), got)


# ---------------------------------------------------------------- GPU, through the engine

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


@pytest.fixture(scope="module")
def evaluated(built):
    """550 R50, seeded weights, a batch of three different noise frames evaluated, and the class map the instance frame's engine
    test makes from frame 1's detections: the first class whose most confident detection has a non-empty mask a ball, the next
    distinct class a red robot, the third a blue robot."""
    import yolact_amd as ya
    eng = ya.Engine(input_size=550, backbone=50, max_batch=3, use_graph=True)
    eng.load_weights(eng.generate_weights(seed=1))
    frames = np.random.default_rng(5).integers(0, 256, (3, 550, 550, 3), dtype=np.uint8)
    eng.set_input(frames)
    eng.evaluate()
    dets, masks = eng.detections(1)
    ids = [d["class_id"] for d in dets]
    distinct = list(dict.fromkeys(ids))
    first = {k: ids.index(k) for k in distinct}
    j = next(i for i, k in enumerate(distinct) if masks[first[k]].any())
    assert len(dets) >= 20 and len(distinct) >= j + 2
    cm = np.zeros(80, np.uint8)
    for k, v in zip(distinct[j:], (3, 1, 2)):
        cm[k] = v
    yield dict(eng=eng, frames=frames, cm=cm)
    eng.close()


def _restated(eng, b, W, H, **kw):
    dets, masks = eng.detections(b)
    return I.instance_frame(masks, [d["class_id"] for d in dets], [d["score"] for d in dets], W, H, **kw)


@pytest.mark.gpu
def test_engine_batch_equals_the_single_calls_and_the_restatement(evaluated):
    eng, cm = evaluated["eng"], evaluated["cm"]
    before = eng.instance_frame(0, 64, 48, class_map=cm)                         # a single call made BEFORE the batch ...
    before_table, before_ptr = eng.instances(), eng.instance_device_frame()
    got = eng.instance_batch(1, 2, W0, H0, class_map=cm)
    tables = [eng.instances_of(b) for b in range(2)]
    dev = _device_u32(eng.instance_batch_device_frames(), 2 * W0 * H0).reshape(2, H0, W0)
    assert np.array_equal(dev, got) and got[0].any() and not np.array_equal(got[0], got[1])
    assert eng.instance_device_frame() == before_ptr and np.array_equal(eng.instances(), before_table)   # ... is unchanged after it
    assert np.array_equal(_device_u32(before_ptr, 64 * 48).reshape(48, 64), before)
    for b in range(2):
        want, wtable = _restated(eng, 1 + b, W0, H0, class_map=cm)
        assert np.array_equal(got[b], want) and np.array_equal(tables[b], wtable), b
        one = eng.instance_frame(1 + b, W0, H0, class_map=cm)
        assert np.array_equal(got[b], one) and np.array_equal(tables[b], eng.instances()), b
        assert np.array_equal(_device_u32(eng.instance_device_frame(), W0 * H0).reshape(H0, W0), got[b]), b
    # the single calls, and a tracked one, did not disturb the batch
    eng.instance_track(0, 64, 48, class_map=cm)
    eng.track_reset()
    assert np.array_equal(_device_u32(eng.instance_batch_device_frames(), 2 * W0 * H0).reshape(2, H0, W0), got)
    assert all(np.array_equal(eng.instances_of(b), tables[b]) for b in range(2))
    # read=False, a threshold, the default class map, the whole step
    ms = float(np.median([d["score"] for d in eng.detections(1, want_masks=False)[0]]))
    assert eng.instance_batch(0, 3, 321, 123, min_score=ms, read=False) is None
    dev = _device_u32(eng.instance_batch_device_frames(), 3 * 321 * 123).reshape(3, 123, 321)
    for b in range(3):
        want, wtable = _restated(eng, b, 321, 123, min_score=ms)
        assert np.array_equal(dev[b], want) and np.array_equal(eng.instances_of(b), wtable), b


@pytest.mark.gpu
def test_staged_frames_into_the_scene_batch_and_its_plan(evaluated):
    """evaluate -> instance_batch -> stage_frames -> append -> plan with the class images never on the host, against a SceneBatch
    staged slot by slot from single instance_frame calls: every read(b) output and every plan bit for bit. Slot 2, staged earlier
    and outside the range, is untouched."""
    import yolact_amd as ya
    eng = evaluated["eng"]
    cm = (np.arange(80) % 3 + 1).astype(np.uint8)                                # every class a robot or a ball: frames with balls to plan to
    depths = np.stack([_frame(np.random.default_rng(40 + b), H0, W0)[0] for b in range(3)])
    a, s = ya.SceneBatch(W0, H0, 3), ya.SceneBatch(W0, H0, 3)
    other = np.random.default_rng(9).integers(0, 4, (H0, W0)).astype(np.uint32) << 24
    for sb in (a, s):
        sb.stage(2, depths[2], frame_u32=other)
    for b in range(2):
        eng.instance_frame(1 + b, W0, H0, class_map=cm, read=False)
        s.stage(b, depths[b], frame_dev_ptr=eng.instance_device_frame())
    eng.instance_batch(1, 2, W0, H0, class_map=cm, read=False)
    a.stage_frames(0, depths[:2], frames_dev_ptr=eng.instance_batch_device_frames())
    a.append(2, ya.COMPAT_SANE); s.append(2, ya.COMPAT_SANE)
    for b in range(2):
        assert _same(a.read(b), s.read(b)), b
    assert a.read(0)["map"].any() and not _same(a.read(0), a.read(1))
    starts = [(400, 479), (400, 479)]
    sa, ss = a.plan(starts=starts), s.plan(starts=starts)                        # NULL targets: each frame's own balls
    assert sa == ss
    for b in range(2):
        if sa[b] == ya.capi.OK:
            pa, ps = a.read_plan(b, fields=False), s.read_plan(b, fields=False)
            assert np.array_equal(pa["path"], ps["path"]) and np.array_equal(_bits(pa["directions"]), _bits(ps["directions"])), b
    assert ya.capi.OK in sa
    a.append(3, ya.COMPAT_SANE); s.append(3, ya.COMPAT_SANE)                     # slot 2 as staged before the range was
    assert _same(a.read(2), s.read(2)) and _same(a.read(0), s.read(0))
    # from the host, at another first slot
    host = eng.instance_batch(1, 2, W0, H0, class_map=cm)
    a.stage_frames(1, depths[:2], frames_u32=host)
    for b in range(2):
        s.stage(1 + b, depths[b], frame_u32=host[b])
    a.append(3, ya.COMPAT_SANE); s.append(3, ya.COMPAT_SANE)
    assert all(_same(a.read(b), s.read(b)) for b in range(3))
    # ranges are refused, and a refused range stages nothing
    fresh = ya.SceneBatch(W0, H0, 3)
    for first, n in ((-1, 1), (3, 1), (2, 2), (0, 4)):
        with pytest.raises(ya.YhError) as e:
            fresh.stage_frames(first, np.zeros((n, H0, W0), np.uint16), frames_u32=np.zeros((n, H0, W0), np.uint32))
        assert e.value.code == ya.capi.EINVAL, (first, n)
    assert fresh.L.yh_scene_batch_stage_frames(fresh.h, 0, 0, depths.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p), 0) == ya.capi.EINVAL
    with pytest.raises(ya.YhError) as e:
        fresh.append(1, ya.COMPAT_SANE)
    assert e.value.code == ya.capi.ESTATE
    a.close(); s.close(); fresh.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_previous_batch_readable(evaluated):
    import yolact_amd as ya
    eng, cm = evaluated["eng"], evaluated["cm"]
    want = eng.instance_batch(0, 3, 64, 48, class_map=cm)
    tables, ptr = [eng.instances_of(b) for b in range(3)], eng.instance_batch_device_frames()

    def refused(code, fn):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert eng.instance_batch_device_frames() == ptr
        assert all(np.array_equal(eng.instances_of(b), tables[b]) for b in range(3))
        assert np.array_equal(_device_u32(ptr, 3 * 64 * 48).reshape(3, 48, 64), want)

    bad = cm.copy()
    bad[79] = 4
    EINVAL, ESTATE = ya.capi.EINVAL, ya.capi.ESTATE
    for first, n in ((0, 0), (0, -1), (0, 4), (2, 2), (3, 1), (-1, 2)):
        refused(EINVAL, lambda: eng.instance_batch(first, n, 64, 48, class_map=cm))
    for w, h in ((0, 48), (64, 0), (4097, 48), (64, 4097)):
        refused(EINVAL, lambda: eng.instance_batch(0, 3, w, h, class_map=cm))
    refused(EINVAL, lambda: eng.instance_batch(0, 3, 64, 48, class_map=bad))
    refused(EINVAL, lambda: eng.instance_batch(0, 3, 64, 48, class_map=cm, min_score=float("nan")))
    refused(EINVAL, lambda: eng.instances_of(3))
    n = C.c_int32(-1)
    small = np.zeros((1, 4), np.int32)
    assert eng.L.yh_instance_batch_read(eng.h, 1, C.byref(n), small.ctypes.data_as(C.c_void_p), 1) == ya.capi.EOVERFLOW
    assert n.value == len(tables[1]) > 1 and not small.any()
    eng.invoke()                                                                 # the last step is no longer an evaluate
    refused(ESTATE, lambda: eng.instance_batch(0, 3, 64, 48, class_map=cm))
    eng.evaluate()
    assert np.array_equal(eng.instance_batch(0, 3, 64, 48, class_map=cm), want)
    tables, ptr = [eng.instances_of(b) for b in range(3)], eng.instance_batch_device_frames()
    eng.set_input(evaluated["frames"])                                           # new input since
    refused(ESTATE, lambda: eng.instance_batch(0, 3, 64, 48, class_map=cm))
    eng.evaluate()
    assert np.array_equal(eng.instance_batch(0, 3, 64, 48, class_map=cm), want)


@pytest.mark.gpu
def test_life_cycle_before_any_batch_two_sizes_then_destroy(built):
    import yolact_amd as ya
    eng = ya.Engine(input_size=128, max_batch=2, use_graph=False, conf_thresh=0.005)
    assert not eng.instance_batch_device_frames()
    for fn in (lambda: eng.instance_batch(0, 1, 8, 8), lambda: eng.instances_of(0)):
        with pytest.raises(ya.YhError) as e:                                     # no evaluate, no batch
            fn()
        assert e.value.code == ya.capi.ESTATE
    eng.load_weights(eng.generate_weights(seed=1))
    eng.set_input(np.random.default_rng(0).integers(0, 256, (2, 128, 128, 3), dtype=np.uint8))
    eng.invoke()
    with pytest.raises(ya.YhError) as e:                                         # yh_invoke only
        eng.instance_batch(0, 2, 8, 8)
    assert e.value.code == ya.capi.ESTATE
    eng.evaluate()
    eng.instance_frame(0, 8, 8)                                                  # a single frame is not a batch
    with pytest.raises(ya.YhError) as e:
        eng.instances_of(0)
    assert e.value.code == ya.capi.ESTATE and not eng.instance_batch_device_frames()
    dets, _ = eng.detections(0)
    assert len(dets) > 0
    cm = np.zeros(80, np.uint8)
    cm[dets[0]["class_id"]] = 3
    for w, h, first, n in ((50, 20, 0, 2), (200, 150, 0, 2), (31, 7, 1, 1)):     # grows, then fits
        got = eng.instance_batch(first, n, w, h, class_map=cm)
        for b in range(n):
            want, wtable = _restated(eng, first + b, w, h, class_map=cm)
            assert np.array_equal(got[b], want) and np.array_equal(eng.instances_of(b), wtable), (w, h, b)
    with pytest.raises(ya.YhError) as e:
        eng.instances_of(1)                                                      # the last batch had one frame
    assert e.value.code == ya.capi.EINVAL
    eng.close()


@pytest.mark.gpu
def test_a_batch_of_eight_beats_eight_single_frames(built):
    """A condition, not a measurement (tools/time_instance_batch.py measures): max_batch = 8 at 640x480, instance_batch(0, 8,
    read=False) + stage_frames against eight x (instance_frame(read=False) + stage), in this process; median of five, alternated,
    one warm-up each. The batch makes 2 launches and 2 waits where the singles make 16 and 16."""
    import yolact_amd as ya
    n = 8
    eng = ya.Engine(input_size=550, backbone=50, max_batch=n, use_graph=False)
    eng.load_weights(eng.generate_weights(seed=1))
    eng.set_input(np.random.default_rng(5).integers(0, 256, (n, 550, 550, 3), dtype=np.uint8))
    eng.evaluate()
    cm = (np.arange(80) % 3 + 1).astype(np.uint8)
    depths = np.random.default_rng(1).integers(200, 4000, (n, H0, W0)).astype(np.uint16)
    sb, ss = ya.SceneBatch(W0, H0, n), ya.SceneBatch(W0, H0, n)

    def batch():
        eng.instance_batch(0, n, W0, H0, class_map=cm, read=False)
        sb.stage_frames(0, depths, frames_dev_ptr=eng.instance_batch_device_frames())

    def singles():
        for b in range(n):
            eng.instance_frame(b, W0, H0, class_map=cm, read=False)
            ss.stage(b, depths[b], frame_dev_ptr=eng.instance_device_frame())

    def clock(fn):
        t0 = time.perf_counter(); fn(); return (time.perf_counter() - t0) * 1e3

    batch(); singles()                                                           # warm-up: buffers, code objects
    sb.append(n, ya.COMPAT_SANE); ss.append(n, ya.COMPAT_SANE)
    assert np.array_equal(sb.read(n - 1)["map"], ss.read(n - 1)["map"])
    tb, ts = [], []
    for _ in range(5):
        tb.append(clock(batch)); ts.append(clock(singles))
    mb, ms = sorted(tb)[2], sorted(ts)[2]
    print(f"instance frames of {n} frames into the scene batch: batch {mb:.3f} ms, {n} singles {ms:.3f} ms, ratio {mb / ms:.3f}")
    assert mb < ms
    sb.close(); ss.close(); eng.close()
