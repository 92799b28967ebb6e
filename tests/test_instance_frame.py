"""The instance frame (yh_instance_frame, yh_instance_read, yh_op_instance_frame; DESIGN.md §11 "Instance frame").
CPU part: the restatement (tests/instance_ref.py) on hand cases and against torch's float64 bilinear resize, and the new symbols.
GPU part (-m gpu): the HIP kernels array_equal to the restatement through the single-op hook at tiny and full shapes, and through
the engine on its own detections (frame 1 of a batch of 2), the join with the scene and the planner, every error, the life cycle
and a floor on time."""
import ctypes as C
import inspect
import os
import re
import time

import numpy as np
import pytest

import instance_ref as I
import path_ref as R
from test_scene import _frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (Hp, Wp, W, H): full size, ties (71 of them), a downsample (4 ties), the identity
SHAPES = [(138, 138, 640, 480), (6, 4, 17, 9), (10, 10, 5, 3), (138, 138, 138, 138)]
RED, BLUE, BALL = 1 << 24, 2 << 24, 3 << 24


# ---------------------------------------------------------------- CPU

def test_two_by_two_to_four_by_four_by_hand():
    """Wp = 2 -> W = 4: n = 0, 2, 6, 10 (after the clamp), u0 = 0, 0, 0, 1, fx = 0, 2, 6, 2 of 8 and u1 = 1: the columns weigh the two
    taps 8:0, 6:2, 2:6 and 0:8 (column 3 reads tap 1 twice). The same along y. One corner set: S = (8 - fx)(8 - fy) against 2 W H =
    32, i.e. 64 48 16 0 / 48 36 12 0 / 16 12 4 0 / 0."""
    u0, u1, fx = I.axis_taps(4, 2)
    assert u0.tolist() == [0, 0, 0, 1] and u1.tolist() == [1, 1, 1, 1] and fx.tolist() == [0, 2, 6, 2]
    up = I.upsample(np.array([[1, 0], [0, 0]]), 4, 4)
    assert up.astype(int).tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    # a diagonal pair: the centre pixels see 36 + 4 = 40 > 32 on the diagonal and 12 + 12 = 24 off it
    up = I.upsample(np.array([[1, 0], [0, 1]]), 4, 4)
    assert up.astype(int).tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 1]]
    assert I.upsample(np.ones((2, 2)), 4, 4).all() and not I.upsample(np.zeros((2, 2)), 4, 4).any()


def test_a_tie_stays_off():
    """2 -> 4 has no tie (its weights are odd sixteenths: 9, 3, 3, 1 never sum to 8); 2 -> 3 has: the middle sample lies exactly
    between the taps, n = 3 of 2 W = 6, S = 3 * 2 = 6 = 2 W H with H = 1. The tie is off from either side."""
    u0, u1, fx = I.axis_taps(3, 2)
    assert u0.tolist() == [0, 0, 1] and fx.tolist() == [0, 3, 1] and u1.tolist() == [1, 1, 1]
    assert I.upsample(np.array([[1, 0]]), 3, 1).astype(int).tolist() == [[1, 0, 0]]
    assert I.upsample(np.array([[0, 1]]), 3, 1).astype(int).tolist() == [[0, 0, 1]]
    assert I.upsample(np.array([[1, 0], [0, 1]]), 3, 3).astype(int).tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 1]]


def test_rank_decides_where_two_detections_overlap():
    m = np.zeros((2, 4, 4), np.uint8)
    m[0, :, :3] = 1
    m[1, :, 1:] = 1
    frame, table = I.instance_frame(m, [2, 2], [0.9, 0.8], 4, 4)
    assert (frame[:, :3] == BALL).all() and (frame[:, 3] == BALL | 1 << 16).all()
    assert table.tolist() == [[0, 3, 0, 12], [1, 3, 1, 4]]
    frame, table = I.instance_frame(m[::-1], [2, 2], [0.9, 0.8], 4, 4)
    assert (frame[:, 1:] == BALL).all() and (frame[:, 0] == BALL | 1 << 16).all()
    frame, table = I.instance_frame(m[[0, 0]], [2, 0], [0.9, 0.8], 4, 4)      # fully occluded: in the table with 0 pixels, id kept
    assert table.tolist() == [[0, 3, 0, 12], [1, 1, 0, 0]] and (frame[:, 3] == 0).all()


def test_an_ineligible_detection_neither_paints_nor_occludes():
    m = np.ones((3, 2, 2), np.uint8)
    frame, table = I.instance_frame(m, [5, 2, 2], [0.9, 0.3, 0.8], 2, 2, min_score=0.5)   # an unmapped class, then a low score
    assert (frame == BALL).all() and table.tolist() == [[2, 3, 0, 4]]
    frame, table = I.instance_frame(m, [5, 2, 2], [0.9, 0.5, 0.3], 2, 2, min_score=0.5)   # score == min_score is kept
    assert (frame == BALL).all() and table.tolist() == [[1, 3, 0, 4]]
    cm = np.zeros(80, np.uint8)
    cm[5] = 2
    frame, table = I.instance_frame(m, [5, 2, 2], [0.9, 0.5, 0.3], 2, 2, class_map=cm)
    assert (frame == BLUE).all() and table.tolist() == [[0, 2, 0, 4]]
    frame, table = I.instance_frame(m[:0], [], [], 3, 2)
    assert frame.shape == (2, 3) and not frame.any() and table.shape == (0, 4)


def test_ids_count_per_output_class_in_rank_order():
    ids = [2, 0, 2, 7, 1, 2, 0, 2]
    sc = [.9, .8, .7, .6, .5, .4, .3, .2]
    got = I.ranks(ids, sc, min_score=0.25)
    assert got == [(True, 3, 0), (True, 1, 0), (True, 3, 1), (False, 0, 0), (True, 2, 0), (True, 3, 2), (True, 1, 1), (False, 0, 0)]
    cm = np.zeros(80, np.uint8)
    cm[[2, 7]] = 3                                                               # two foreground classes share an output class
    assert [g[2] for g in I.ranks(ids, sc, class_map=cm) if g[0]] == [0, 1, 2, 3, 4]
    m = np.zeros((8, 1, 8), np.uint8)
    m[np.arange(8), 0, np.arange(8)] = 1
    frame, table = I.instance_frame(m, ids, sc, 8, 1, min_score=0.25)
    assert frame[0].tolist() == [BALL, RED, BALL | 1 << 16, 0, BLUE, BALL | 2 << 16, RED | 1 << 16, 0]
    assert table[:, 0].tolist() == [0, 1, 2, 4, 5, 6] and (table[:, 3] == 1).all()


@pytest.mark.parametrize("Hp,Wp,W,H", SHAPES)
def test_upsample_agrees_with_torch_float64_bilinear(Hp, Wp, W, H):
    import torch
    masks = I.disc_masks(np.random.default_rng(Hp * 1000 + W), 20, Hp, Wp)
    want = torch.nn.functional.interpolate(torch.from_numpy(masks.astype(np.float64))[None], size=(H, W), mode="bilinear",
                                           align_corners=False)[0].numpy() > 0.5
    got = np.stack([I.upsample(m, W, H) for m in masks])
    assert got.any() and np.array_equal(got, want)


def test_instance_symbols_are_declared_and_bound(built):
    from yolact_amd import capi
    L = capi.load_library()
    bound = {s[0]: s for s in capi.SYMBOLS}
    strip = lambda f: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", f)).read(), flags=re.S)
    pub, dbg = strip("yolact_hip.h"), strip("yolact_hip_debug.h")
    for name, src, nargs in (("yh_instance_frame", pub, 7), ("yh_instance_device_frame", pub, 1), ("yh_instance_read", pub, 4),
                             ("yh_op_instance_frame", dbg, 15)):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(L, name), name
        assert len(bound[name][2]) == nargs, name
    assert "yh_op_instance_frame" not in pub and "#define YH_ABI_VERSION 4" in pub
    sig = inspect.signature(capi.Engine.instance_frame).parameters
    assert list(sig)[1:] == ["frame", "width", "height", "class_map", "min_score", "read"]
    assert sig["class_map"].default is None and sig["min_score"].default == 0.0 and sig["read"].default is True
    for m in ("instance_device_frame", "instances", "op_instance_frame"):
        assert callable(getattr(capi.Engine, m))


# ---------------------------------------------------------------- GPU, through yh_op_instance_frame

@pytest.fixture(scope="module")
def op_eng(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=1, use_graph=False)                  # no weights: the hook needs none
    yield e
    e.close()


def _dets(rng, n, classes=(0, 1, 2, 5)):
    """class ids and strictly descending scores for n detections."""
    return rng.choice(classes, n).astype(np.int32), np.sort(rng.random(n).astype(np.float32))[::-1].copy()


def _check(eng, masks, ids, sc, W, H, **kw):
    got, table = eng.op_instance_frame(masks, ids, sc, W, H, **kw)
    want, wtable = I.instance_frame(masks, ids, sc, W, H, **kw)
    assert np.array_equal(got, want)
    assert np.array_equal(table, wtable)
    assert table[:, 3].sum() == np.count_nonzero(got)
    assert np.array_equal(eng.instances(), wtable)
    return got, table


@pytest.mark.gpu
@pytest.mark.parametrize("Hp,Wp,W,H", [(6, 4, 17, 9), (10, 10, 5, 3), (2, 2, 1, 1), (5, 5, 7, 3), (138, 138, 138, 138)])
def test_small_shapes_equal_the_restatement(op_eng, Hp, Wp, W, H):
    """Ties (6x4 -> 17x9), a downsample, a single pixel, masks whose size is no multiple of four (the byte path of inst_pack) and
    the identity."""
    rng = np.random.default_rng(Hp * 100 + W)
    n = 20
    masks = I.disc_masks(rng, n, Hp, Wp)
    ids, sc = _dets(rng, n)
    got, table = _check(op_eng, masks, ids, sc, W, H)
    assert len(table) == int((ids != 5).sum())
    if (Hp, Wp) == (H, W):
        assert np.array_equal(got != 0, masks[ids != 5].any(0))


@pytest.mark.gpu
def test_full_size_with_private_regions_at_the_word_boundaries(op_eng):
    """138x138 -> 640x480, 100 discs. Ranks 31, 32, 63, 64 and 99 each own a square no other mask covers: the last and first bits
    of the words of the 128-bit set."""
    rng = np.random.default_rng(7)
    n, own = 100, (31, 32, 63, 64, 99)
    masks = I.disc_masks(rng, n, 138, 138, rmax=40)
    for k, d in enumerate(own):
        masks[:, 4:10, 20 * k + 4:20 * k + 10] = 0
        masks[d, 4:10, 20 * k + 4:20 * k + 10] = 1
    ids, sc = _dets(rng, n, classes=(0, 1, 2))
    got, table = _check(op_eng, masks, ids, sc, 640, 480)
    vals = {int(r[0]): (int(r[1]) << 24) | (int(r[2]) << 16) for r in table}
    for k, d in enumerate(own):
        x, y = int((20 * k + 7) * 640 / 138), int(7 * 480 / 138)
        assert got[y, x] == vals[d], d
        assert table[table[:, 0] == d][0, 3] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 100])
def test_counts_from_none_to_max_dets(op_eng, n):
    assert op_eng.cfg.max_dets == 100
    rng = np.random.default_rng(n)
    masks = I.disc_masks(rng, n, 12, 16)
    ids, sc = _dets(rng, n, classes=(0, 1, 2))
    got, table = _check(op_eng, masks, ids, sc, 40, 30)
    assert len(table) == n and (n > 0 or not got.any())


@pytest.mark.gpu
def test_threshold_class_map_and_refusals_of_the_hook(op_eng):
    import yolact_amd as ya
    rng = np.random.default_rng(3)
    masks = I.disc_masks(rng, 12, 9, 11)
    ids, sc = _dets(rng, 12, classes=(0, 2, 5, 9))
    _, table = _check(op_eng, masks, ids, sc, 33, 21, min_score=float(sc[6]))   # score == min_score is kept
    assert table[:, 0].max() <= 6 and (6 in table[:, 0] or ids[6] in (5, 9))
    cm = np.zeros(80, np.uint8)
    cm[[5, 9]] = (3, 1)                                                          # classes 0 and 2 map to zero: neither paint nor occlude
    _, table = _check(op_eng, masks, ids, sc, 33, 21, class_map=cm)
    assert set(table[:, 0].tolist()) == {d for d in range(12) if ids[d] in (5, 9)}
    before = op_eng.instances()
    bad = cm.copy()
    bad[0] = 4
    for fn in (lambda: op_eng.op_instance_frame(masks, ids, sc, 0, 21), lambda: op_eng.op_instance_frame(masks, ids, sc, 33, 4097),
               lambda: op_eng.op_instance_frame(masks, ids, sc, 33, 21, class_map=bad),
               lambda: op_eng.op_instance_frame(masks, ids, sc, 33, 21, min_score=float("nan")),
               lambda: op_eng.op_instance_frame(np.zeros((101, 2, 2), np.uint8), np.zeros(101), np.zeros(101), 4, 4)):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == ya.capi.EINVAL
        assert np.array_equal(op_eng.instances(), before)


# ---------------------------------------------------------------- GPU, through the engine

W0, H0 = 640, 480


def _device_u32(ptr, n):
    """n uint32 from device memory (the instance frame's device pointer)."""
    path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), "libamdhip64.so")
    hip = C.CDLL(path)
    out = np.zeros(n, np.uint32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0   # hipMemcpyDeviceToHost
    return out


@pytest.fixture(scope="module")
def evaluated(built):
    """550 R50, seeded weights, a batch of two noise frames evaluated; frame 1's detections and a class map made from them: the
    first class whose most confident detection has a non-empty mask a ball, the next distinct class a red robot, the third a blue
    robot."""
    import yolact_amd as ya
    eng = ya.Engine(input_size=550, backbone=50, max_batch=2, use_graph=True)
    eng.load_weights(eng.generate_weights(seed=1))
    frames = np.random.default_rng(5).integers(0, 256, (2, 550, 550, 3), dtype=np.uint8)
    eng.set_input(frames)
    eng.evaluate()
    dets, masks = eng.detections(1)
    ids = np.array([d["class_id"] for d in dets], np.int32)
    sc = np.array([d["score"] for d in dets], np.float32)
    distinct = list(dict.fromkeys(ids.tolist()))                                 # the classes in the order of their best detection
    first = {k: ids.tolist().index(k) for k in distinct}
    j = next(i for i, k in enumerate(distinct) if masks[first[k]].any())         # (with seeded weights a box crop can leave a mask empty)
    assert len(dets) >= 20 and len(distinct) >= j + 2
    cm = np.zeros(80, np.uint8)
    for k, v in zip(distinct[j:], (3, 1, 2)):                                    # every class ranked before the ball's stays unmapped:
        cm[k] = v                                                                # ball 0 is the first eligible detection, never occluded
    yield dict(eng=eng, frames=frames, masks=masks, ids=ids, sc=sc, cm=cm)
    eng.close()


@pytest.mark.gpu
def test_engine_frame_one_equals_the_restatement(evaluated):
    eng, cm = evaluated["eng"], evaluated["cm"]
    want, wtable = I.instance_frame(evaluated["masks"], evaluated["ids"], evaluated["sc"], W0, H0, class_map=cm)
    got = eng.instance_frame(1, W0, H0, class_map=cm)
    assert np.array_equal(got, want) and np.array_equal(eng.instances(), wtable)
    assert wtable[0, 1:3].tolist() == [3, 0] and wtable[0, 3] > 0 and len(wtable) >= 2                 # ball 0 leads and has pixels
    assert np.array_equal(_device_u32(eng.instance_device_frame(), W0 * H0).reshape(H0, W0), want)
    d0, m0 = eng.detections(0)                                                   # frame 0 is another frame: the batch offset matters
    want0, _ = I.instance_frame(m0, [d["class_id"] for d in d0], [d["score"] for d in d0], W0, H0, class_map=cm)
    assert not np.array_equal(want0, want) and np.array_equal(eng.instance_frame(0, W0, H0, class_map=cm), want0)
    ms = float(np.median(evaluated["sc"]))                                       # a threshold in the middle, the default class map
    want, wtable = I.instance_frame(evaluated["masks"], evaluated["ids"], evaluated["sc"], 321, 123, min_score=ms)
    assert eng.instance_frame(1, 321, 123, min_score=ms, read=False) is None
    assert np.array_equal(eng.instances(), wtable)
    assert np.array_equal(_device_u32(eng.instance_device_frame(), 321 * 123).reshape(123, 321), want)


@pytest.mark.gpu
def test_device_frame_into_the_scene_and_a_plan_to_ball_zero(evaluated):
    """evaluate -> instance frame -> scene -> plan with the class image never on the host: every output of Scene.read() has the
    bits of a scene fed the restatement's class image from the host, and the route to the first ball ends on ball 0's pixel."""
    import yolact_amd as ya
    eng, cm = evaluated["eng"], evaluated["cm"]
    want, wtable = I.instance_frame(evaluated["masks"], evaluated["ids"], evaluated["sc"], W0, H0, class_map=cm)
    depth, _ = _frame(np.random.default_rng(11), H0, W0)
    eng.instance_frame(1, W0, H0, class_map=cm, read=False)
    a, b = ya.Scene(W0, H0), ya.Scene(W0, H0)
    a.append_classified(depth, frame_dev_ptr=eng.instance_device_frame(), mode=ya.COMPAT_SANE)
    b.append(depth, I.class_image(want), ya.COMPAT_SANE)
    fa, fb = a.read(), b.read()
    for k in fb:
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert (wtable[:, 1] == 3).sum() >= 1
    tg = R.ball_targets(fa["balls"], 1, W0, H0)
    assert fa["balls"][0, 2] > 0 and len(tg) == 1                                # ball 0: the most confident ball, never occluded
    a.plan(n_targets=1)
    path = a.read_plan(fields=False)["path"]
    assert tuple(path[0]) == (400, 479) and tuple(path[-1]) == tg[0]
    a.close(); b.close()


@pytest.mark.gpu
def test_every_refusal_leaves_the_previous_frame_readable(evaluated):
    import yolact_amd as ya
    eng, cm = evaluated["eng"], evaluated["cm"]
    want = eng.instance_frame(1, 64, 48, class_map=cm)
    table, ptr = eng.instances(), eng.instance_device_frame()

    def refused(code, fn):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert eng.instance_device_frame() == ptr and np.array_equal(eng.instances(), table)
        assert np.array_equal(_device_u32(ptr, 64 * 48).reshape(48, 64), want)

    bad = cm.copy()
    bad[79] = 4
    EINVAL, ESTATE = ya.capi.EINVAL, ya.capi.ESTATE
    refused(EINVAL, lambda: eng.instance_frame(2, 64, 48, class_map=cm))
    refused(EINVAL, lambda: eng.instance_frame(-1, 64, 48, class_map=cm))
    for w, h in ((0, 48), (64, 0), (4097, 48), (64, 4097)):
        refused(EINVAL, lambda: eng.instance_frame(1, w, h, class_map=cm))
    refused(EINVAL, lambda: eng.instance_frame(1, 64, 48, class_map=bad))
    refused(EINVAL, lambda: eng.instance_frame(1, 64, 48, class_map=cm, min_score=float("nan")))
    n = C.c_int32(-1)
    small = np.zeros((1, 4), np.int32)
    assert eng.L.yh_instance_read(eng.h, C.byref(n), small.ctypes.data_as(C.c_void_p), 1) == ya.capi.EOVERFLOW
    assert n.value == len(table) > 1 and not small.any()
    eng.invoke()                                                                 # the last step is no longer an evaluate
    refused(ESTATE, lambda: eng.instance_frame(1, 64, 48, class_map=cm))
    eng.evaluate()
    assert np.array_equal(eng.instance_frame(1, 64, 48, class_map=cm), want)
    table, ptr = eng.instances(), eng.instance_device_frame()
    eng.set_input(evaluated["frames"])                                           # new input since
    refused(ESTATE, lambda: eng.instance_frame(1, 64, 48, class_map=cm))
    eng.evaluate()
    assert np.array_equal(eng.instance_frame(1, 64, 48, class_map=cm), want)
    assert eng.instance_frame(1, 4096, 1, class_map=cm).shape == (1, 4096)       # the largest side is accepted


@pytest.mark.gpu
def test_life_cycle_before_any_evaluate_two_sizes_then_destroy(built):
    import yolact_amd as ya
    eng = ya.Engine(input_size=128, max_batch=1, use_graph=False, conf_thresh=0.005)
    assert not eng.instance_device_frame()
    for fn in (lambda: eng.instance_frame(0, 8, 8), eng.instances):
        with pytest.raises(ya.YhError) as e:
            fn()
        assert e.value.code == ya.capi.ESTATE
    eng.load_weights(eng.generate_weights(seed=1))
    eng.set_input(np.random.default_rng(0).integers(0, 256, (1, 128, 128, 3), dtype=np.uint8))
    eng.invoke()
    with pytest.raises(ya.YhError) as e:                                         # yh_invoke only
        eng.instance_frame(0, 8, 8)
    assert e.value.code == ya.capi.ESTATE
    eng.evaluate()
    dets, masks = eng.detections(0)
    assert len(dets) > 0
    ids, sc = [d["class_id"] for d in dets], [d["score"] for d in dets]
    cm = np.zeros(80, np.uint8)
    cm[ids[0]] = 3
    for w, h in ((50, 20), (200, 150), (31, 7)):                                 # grows, then fits
        want, wtable = I.instance_frame(masks, ids, sc, w, h, class_map=cm)
        assert np.array_equal(eng.instance_frame(0, w, h, class_map=cm), want) and np.array_equal(eng.instances(), wtable)
    eng.close()


@pytest.mark.gpu
def test_instance_frame_beats_the_numpy_restatement(evaluated):
    """A condition, not a measurement: the device call at 640x480, host copy included, must take less than the numpy restatement of
    the same frame timed here (tools/time_instance.py measures the call)."""
    eng, cm = evaluated["eng"], evaluated["cm"]
    t0 = time.perf_counter()
    want, _ = I.instance_frame(evaluated["masks"], evaluated["ids"], evaluated["sc"], W0, H0, class_map=cm)
    ref = time.perf_counter() - t0
    eng.instance_frame(1, W0, H0, class_map=cm)                                   # (allocations, warm-up)
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = eng.instance_frame(1, W0, H0, class_map=cm)
        runs.append(time.perf_counter() - t0)
    dev = sorted(runs)[2]
    print(f"instance frame 640x480, {len(evaluated['ids'])} detections: {dev * 1e3:.3f} ms with the host copy; numpy restatement {ref * 1e3:.1f} ms")
    assert np.array_equal(got, want) and dev < ref
