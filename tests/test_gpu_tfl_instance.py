"""-m gpu: the TFLite instance frames (csrc/tfl_instance.hip; DESIGN.md §11 "TFLite instance frames") bit for bit: every frame and
every table array_equal. Per camera frame - two tiles, one frame order, a seam - against tests/tfl_instance_ref.py, through
yh_tfl_op_instance_frames on chosen detections and through a model (uint8 and its int8 twin) on its own; per image against
tests/instance_ref.py; the hand-over to the scene batch, every refusal and state, and the ground that must not move."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_ref as IR
import tfl_builder as B
import tfl_builder_q as BQ
import tfl_instance_ref as TR
import tfl_models as M
import tfl_q_cases as Q

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32, 96, 64), (5, 7, 7, 5), (3, 5, 33, 9), (1, 1, 2, 1), (2, 2, 5, 3)]   # (hp, wp, W, H)
CM80 = np.zeros(80, np.uint8)
CM80[:6] = (1, 2, 3, 0, 1, 2)


@pytest.fixture(scope="module")
def eng(built):
    """A handle for yh_tfl_op_instance_frames: it gives the device, the stream and the error text; its model (one RELU) is not involved."""
    import yolact_amd as ya
    e = ya.TfliteEngine(bytes(B.serialize(M.single_op("RELU", np.random.default_rng(0)))))
    yield e
    e.close()


def _random(rng, images, nd, hp, wp, counts, ncls=6, discs=False):
    """masks [images][nd][hp][wp], class ids and scores non-increasing per image [images][nd], counts [images]."""
    if discs:
        masks = np.stack([IR.disc_masks(rng, nd, hp, wp) for _ in range(images)])
    else:
        masks = (rng.random((images, nd, hp, wp)) < 0.45).astype(np.uint8)
    cls = rng.integers(0, ncls, (images, nd)).astype(np.int32)
    sc = -np.sort(-rng.random((images, nd)).astype(np.float32), axis=1)
    return masks, cls, np.ascontiguousarray(sc), np.asarray(counts, np.int32)


def _check(eng, masks, cls, sc, counts, W, H, cm=CM80, min_score=0.0, label=None):
    frames, tables = eng.op_instance_frames(masks, cls, sc, counts, W, H, class_map=cm, min_score=min_score)
    full = np.zeros(80, np.uint8)
    full[:len(cm)] = cm
    for b in range(masks.shape[0] // 2):
        c0, c1 = int(counts[2 * b]), int(counts[2 * b + 1])
        wf, wt = TR.instance_frames(masks[2 * b, :c0], cls[2 * b, :c0], sc[2 * b, :c0], masks[2 * b + 1, :c1], cls[2 * b + 1, :c1],
                                    sc[2 * b + 1, :c1], W, H, full, min_score, 81)
        assert np.array_equal(tables[b], wt), (label, b, tables[b].tolist()[:6], wt.tolist()[:6])
        assert np.array_equal(frames[b], wf), (label, b, int((frames[b] != wf).sum()))
    return frames, tables


@pytest.mark.parametrize("hp,wp,W,H", SHAPES)
@pytest.mark.parametrize("n_frames", (1, 2, 3))
def test_shapes_against_the_restatement(eng, hp, wp, W, H, n_frames):
    rng = np.random.default_rng(1000 * n_frames + 10 * hp + wp)
    nd = 7
    counts = rng.integers(3, nd + 1, 2 * n_frames)
    _, tables = _check(eng, *_random(rng, 2 * n_frames, nd, hp, wp, counts), W, H, label=(hp, wp, W, H, n_frames))
    assert any(len(t) and set(t[:, 0].tolist()) == {0, 1} and t[:, 4].sum() > 0 for t in tables)


def test_px_no_multiple_of_four_and_misaligned_images(eng):
    """(hp, wp) = (3, 3), three frames: px = 9, so the mask bases of images 1 .. 5 are misaligned and inst_pack_body's byte path runs."""
    rng = np.random.default_rng(33)
    _check(eng, *_random(rng, 6, 5, 3, 3, [5, 3, 0, 5, 4, 1]), 10, 7, label="3x3")
    _check(eng, *_random(rng, 6, 5, 3, 3, [1, 5, 5, 5, 2, 0]), 129, 9, label="3x3 wide")    # (more than one workgroup along x)


@pytest.mark.parametrize("counts", [(0, 6), (6, 0), (0, 0)])
def test_an_empty_tile(eng, counts):
    rng = np.random.default_rng(5)
    frames, tables = _check(eng, *_random(rng, 2, 6, 5, 7, counts), 21, 10, label=counts)
    assert (len(tables[0]) == 0) == (counts == (0, 0)) and (frames.any() == (counts != (0, 0)))


def test_both_tiles_full_one_class_ids_run_to_255(eng):
    rng = np.random.default_rng(6)
    masks, cls, sc, counts = _random(rng, 2, 128, 3, 3, (128, 128), ncls=1)
    masks[:] = (rng.random(masks.shape) < 0.1)
    _, tables = _check(eng, masks, cls, sc, counts, 11, 6, label="128+128")
    assert len(tables[0]) == 256 and tables[0][:, 3].tolist() == list(range(256)) and (tables[0][:, 2] == 1).all()
    # with no slot past the counts to hide behind: n_dets = 128 is the kernels' own limit


@pytest.mark.parametrize("hp,wp,W,H", [(5, 7, 7, 5), (3, 5, 33, 9), (2, 2, 5, 3), (32, 32, 96, 64), (4, 4, 131, 6)])
def test_full_masks_in_both_tiles_the_seam_column(eng, hp, wp, W, H):
    masks = np.ones((2, 1, hp, wp), np.uint8)
    frames, tables = _check(eng, masks, np.int32([[0], [1]]), np.float32([[0.9], [0.8]]), [1, 1], W, H, label=("seam", W))
    left, right = frames[0] == 1 << 24, frames[0] == 2 << 24
    assert left[:, :W // 2].all() and right[:, (W + 1) // 2:].all()
    assert (W % 2 == 0) or (frames[0][:, W // 2] == 0).all()                   # odd W: a column that belongs to neither tile
    assert tables[0][:, 4].tolist() == [H * (W // 2)] * 2


def test_a_score_tie_across_tiles(eng):
    rng = np.random.default_rng(8)
    masks, cls, sc, counts = _random(rng, 4, 4, 5, 7, (4, 4, 4, 4), ncls=1)
    sc[:] = np.float32([0.75, 0.5, 0.5, 0.25])                                    # ties within and across tiles, in both frames
    sc[3] = np.float32([0.5, 0.0, -0.0, -0.0])
    _, tables = _check(eng, masks, cls, sc, counts, 21, 10, min_score=-1.0, label="ties")
    assert tables[0][:, :2].tolist() == [[0, 0], [1, 0], [0, 1], [0, 2], [1, 1], [1, 2], [0, 3], [1, 3]]


def test_min_score_on_a_score_and_one_ulp_above(eng):
    rng = np.random.default_rng(9)
    masks, cls, sc, counts = _random(rng, 2, 5, 5, 7, (5, 5), ncls=3)
    s = sc[1, 2]
    sc[0, 3] = s
    sc[0] = -np.sort(-sc[0])
    up = np.nextafter(s, np.float32(2.0))
    _, on = _check(eng, masks, cls, sc, counts, 21, 10, min_score=float(s), label="on the score")
    _, above = _check(eng, masks, cls, sc, counts, 21, 10, min_score=float(up), label="one ulp above")
    n_on, n_above = int((sc >= s).sum()), int((sc >= up).sum())
    assert len(on[0]) == n_on and len(above[0]) == n_above and n_on >= n_above + 2


def test_a_class_map_with_zeros(eng):
    rng = np.random.default_rng(10)
    case = _random(rng, 4, 9, 5, 7, (9, 7, 8, 9))
    cm = np.uint8([0, 3, 0, 1, 0, 2])
    _, tables = _check(eng, *case, 21, 10, cm=cm, label="zeros")
    assert all(len(t) and (t[:, 2] > 0).all() for t in tables) and sum(len(t) for t in tables) < 33
    _, none = _check(eng, *case, 21, 10, cm=np.zeros(6, np.uint8), label="all zero")
    assert all(len(t) == 0 for t in none)


def test_discs_at_32x32_some_on_the_seam(eng):
    rng = np.random.default_rng(11)
    masks, cls, sc, counts = _random(rng, 4, 24, 32, 32, (24, 20, 24, 24), discs=True)
    yy, xx = np.mgrid[0:32, 0:32]
    for img, cx in ((0, 31), (1, 0), (2, 31), (3, 0)):                             # tile 0: centred on column wp - 1; tile 1: on column 0
        for d, (cy, r) in enumerate(((8, 5), (20, 9), (30, 3))):
            masks[img, 2 * d] = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
    frames, tables = _check(eng, masks, cls, sc, counts, 96, 64, label="discs")
    assert all(set(t[:, 0].tolist()) == {0, 1} for t in tables) and (frames[:, :, 44:52] != 0).any()


def test_op_refuses_and_keeps_the_batch(eng):
    import yolact_amd as ya
    rng = np.random.default_rng(12)
    masks, cls, sc, counts = _random(rng, 2, 4, 3, 5, (4, 3))
    frames, tables = eng.op_instance_frames(masks, cls, sc, counts, 9, 4, class_map=CM80)
    ptr = eng.instance_device_frames()
    assert ptr and eng.L.yh_tfl_instance_row_width(eng.h) == 5

    def refused(word, **kw):
        a = dict(masks=masks, class_ids=cls, scores=sc, counts=counts, width=9, height=4, class_map=CM80, min_score=0.0)
        a.update(kw)
        with pytest.raises(ya.YhError) as e:
            eng.op_instance_frames(**a)
        assert e.value.code == ya.capi.EINVAL and word in str(e.value), (word, str(e.value))
    rising = sc.copy()
    rising[0, :2] = np.float32([0.1, 0.2])
    refused("non-increasing", scores=rising)
    nan = sc.copy()
    nan[1, 1] = np.nan
    refused("non-increasing", scores=nan)
    refused("count outside", counts=np.int32([5, 0]))
    refused("class id", class_ids=np.where(np.arange(4) == 1, 80, cls))
    refused("1 .. 4096", width=4097)
    refused("1 .. 4096", height=0)
    refused("above 3", class_map=np.uint8([1, 4]))
    refused("NaN", min_score=float("nan"))
    past = sc.copy()
    past[1, 3] = 9.0                                                              # (rising, but past image 1's count of 3: not looked at)
    eng.op_instance_frames(masks, cls, past, counts, 9, 4, class_map=CM80)
    eng.op_instance_frames(masks, cls, sc, counts, 9, 4, class_map=CM80)
    refused("NaN", min_score=float("nan"))
    # the refused calls left the batch as it was
    assert eng.instance_device_frames() == ptr
    assert all(np.array_equal(eng.instances_of(b), tables[b]) for b in range(1))
    with pytest.raises(ya.YhError) as e:
        eng.instances_of(1)
    assert e.value.code == ya.capi.EINVAL
    with pytest.raises(ya.YhError) as e:                                          # no setup on this handle: the model-side calls refuse
        eng.instance_frames(0, 1, 9, 4)
    assert e.value.code == ya.capi.ESTATE and eng.instance_device_frames() == ptr


# ------------------------------------------------------------------------------------------------------------ through a model
S, C, HP = 128, 6, 32
CFG = dict(top_k=200, max_dets=100, conf_thresh=0.05, nms_thresh=0.5)
CM = np.uint8([1, 2, 3, 1, 2])            # every foreground class painted: noise detections of both tiles are eligible
W0, H0 = 96, 64
_MODELS = {}


def _model(kind):
    if kind not in _MODELS:
        m = M.mobilenetv2_yolact(np.random.default_rng(3), S=S, C=C, fpn=32)
        _MODELS[kind] = BQ.serialize(Q.int8_twin(m, np.random.default_rng(5), dequant_output=None, quant_output=4)) if kind == "i8" else bytes(B.serialize(m))
    return _MODELS[kind]


def _priors():
    import yolact_amd as ya
    return ya.tfl_priors([16, 8, 4, 2, 1], S)


def _frames(n, W=W0, H=H0):
    rgb = np.random.default_rng(6).integers(0, 256, (n, H, W, 3), dtype=np.uint32)
    return ((rgb[..., 0] << 24) | (rgb[..., 1] << 16) | (rgb[..., 2] << 8)).astype(np.uint32)


def _dets(h, i):
    d, k = h.detections(i)
    return k, np.int32([x["class_id"] for x in d]), np.float32([x["score"] for x in d])


def _want_frame(h, b, W, H, cm, min_score):
    return TR.instance_frames(*_dets(h, 2 * b), *_dets(h, 2 * b + 1), W, H, cm, min_score, C)


def _want_image(h, i, W, H, cm, min_score):
    return IR.instance_frame(*_dets(h, i), W, H, cm, min_score, C)


@pytest.mark.parametrize("kind", ("u8", "i8"))
def test_through_a_model(built, kind):
    import yolact_amd as ya
    h = ya.TfliteEngine(_model(kind), max_images=5)
    try:
        h.detect_setup(_priors(), **CFG)
        assert h.proto_dims() == (HP, HP)
        h.classify_batch(frames_u32=_frames(2), width=W0, height=H0, mode=ya.COMPAT_SANE)
        h.detect()
        for i in range(4):                                                        # (the order the stable merge relies on)
            sc = _dets(h, i)[2]
            assert (sc[1:] <= sc[:-1]).all()
        got = h.instance_frames(0, 2, W0, H0, class_map=CM, min_score=0.0)
        assert h.L.yh_tfl_instance_row_width(h.h) == 5
        both = 0
        for b in range(2):
            wf, wt = _want_frame(h, b, W0, H0, CM, 0.0)
            t = h.instances_of(b)
            assert np.array_equal(t, wt) and np.array_equal(got[b], wf), (kind, b)
            both += int(set(t[t[:, 4] > 0, 0].tolist()) == {0, 1})
        assert both >= 1                                                          # (a frame with painted pixels from both tiles)
        one = h.instance_frames(1, 1, 33, 9, class_map=np.uint8([0, 2, 0, 1, 3]), min_score=0.3)   # another frame, size, map, threshold
        wf, wt = _want_frame(h, 1, 33, 9, np.uint8([0, 2, 0, 1, 3]), 0.3)
        assert np.array_equal(one[0], wf) and np.array_equal(h.instances_of(0), wt)
        # per image: each tile as yh_instance_batch paints a frame; the batch replaces the per-frame one, the row width follows
        got = h.instance_batch(0, 4, W0, H0, class_map=CM, min_score=0.0)
        assert h.L.yh_tfl_instance_row_width(h.h) == 4
        painted = 0
        for i in range(4):
            wf, wt = _want_image(h, i, W0, H0, CM, 0.0)
            assert np.array_equal(got[i], wf) and np.array_equal(h.instances_of(i), wt), (kind, i)
            painted += int(wf.any())
        assert painted >= 2
        assert h.instance_batch(0, 1, 7, 5, min_score=0.2, read=False) is None and h.instances_of(0).shape[1] == 4   # (the default map)
        wf, wt = _want_image(h, 0, 7, 5, None, 0.2)
        assert np.array_equal(h.instances_of(0), wt)
        # five images of an evaluate, the middle three
        x = np.random.default_rng(4).integers(0, 256, (5, S, S, 3), dtype=np.uint8)
        h.set_batch(5)
        h.set_input(x)
        h.evaluate()
        got = h.instance_batch(1, 3, 50, 40, class_map=CM, min_score=0.1)
        for i in range(3):
            wf, wt = _want_image(h, 1 + i, 50, 40, CM, 0.1)
            assert np.array_equal(got[i], wf) and np.array_equal(h.instances_of(i), wt), (kind, "evaluate", i)
        got = h.instance_frames(1, 1, 50, 40, class_map=CM)                       # images 2 and 3 read as a frame's two tiles
        wf, wt = _want_frame(h, 1, 50, 40, CM, 0.0)
        assert np.array_equal(got[0], wf) and np.array_equal(h.instances_of(0), wt)
    finally:
        h.close()


def _same(a, b):
    bits = lambda v: np.ascontiguousarray(v).view(np.uint32) if v.dtype == np.float32 else v
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])) for k in a)


def test_hand_over_to_the_scene_batch(built):
    import yolact_amd as ya
    h = ya.TfliteEngine(_model("u8"), max_images=4)
    a, s = ya.SceneBatch(W0, H0, 2), ya.SceneBatch(W0, H0, 2)
    try:
        h.detect_setup(_priors(), **CFG)
        h.classify_batch(frames_u32=_frames(2), width=W0, height=H0, mode=ya.COMPAT_SANE)
        h.detect()
        depths = np.random.default_rng(2).integers(200, 4000, (2, H0, W0)).astype(np.uint16)
        host = h.instance_frames(0, 2, W0, H0, class_map=CM)
        assert host.any() and h.instance_device_frames()
        a.stage_frames(0, depths, frames_dev_ptr=h.instance_device_frames())
        s.stage_frames(0, depths, frames_u32=host)
        a.append(2, ya.COMPAT_SANE); s.append(2, ya.COMPAT_SANE)
        for b in range(2):
            assert _same(a.read(b), s.read(b)), b
        assert a.read(0)["map"].any()
    finally:
        a.close(); s.close(); h.close()


def _ground(h):
    """What the instance calls must leave alone: the detections, the classify batch's pointer (its frames: _scene_of), the plan's
    launch counts."""
    dets = [(tuple((d["class_id"], d["prior"], np.float32(d["score"]).tobytes(), np.float32(d["box"]).tobytes()) for d in h.detections(i)[0]),
             h.detections(i)[1].tobytes()) for i in range(4)]
    return dets, h.classify_batch_device_frames(), h.plan_summary()


def _scene_of(depths, ptr=None, host=None):
    """What the scene batch makes of two frames staged from a device pointer or from the host: the package's reader of device frames."""
    import yolact_amd as ya
    sb = ya.SceneBatch(W0, H0, 2)
    try:
        sb.stage_frames(0, depths, frames_dev_ptr=ptr, frames_u32=host)
        sb.append(2, ya.COMPAT_SANE)
        return [sb.read(b) for b in range(2)]
    finally:
        sb.close()


def test_refusals_states_and_unchanged_ground(built):
    import yolact_amd as ya
    h = ya.TfliteEngine(_model("u8"), max_images=5)
    try:
        def refused(code, word, fn, *a, **kw):
            with pytest.raises(ya.YhError) as e:
                fn(*a, **kw)
            assert e.value.code == code and word in str(e.value), (word, str(e.value))
        n = ya.capi.C.c_int32()
        # no setup, then a setup with no tail yet
        assert h.L.yh_tfl_instance_frames(h.h, 0, 1, W0, H0, None, ya.capi.C.c_float(0.0), None) == ya.capi.ESTATE
        assert h.L.yh_tfl_instance_batch(h.h, 0, 1, W0, H0, None, ya.capi.C.c_float(0.0), None) == ya.capi.ESTATE
        assert h.L.yh_tfl_instance_read(h.h, 0, ya.capi.C.byref(n), None, 0) == ya.capi.ESTATE
        assert h.instance_device_frames() is None
        h.detect_setup(_priors(), **CFG)
        refused(ya.capi.ESTATE, "no detections", h.instance_frames, 0, 1, W0, H0)
        classified, _ = h.classify_batch(frames_u32=_frames(2), width=W0, height=H0, mode=ya.COMPAT_SANE)
        refused(ya.capi.ESTATE, "no detections", h.instance_batch, 0, 1, W0, H0)          # an invoke, no tail since
        h.detect()
        before = _ground(h)
        depths = np.random.default_rng(2).integers(200, 4000, (2, H0, W0)).astype(np.uint16)
        cls_scene = _scene_of(depths, host=classified)
        assert all(_same(x, y) for x, y in zip(_scene_of(depths, ptr=before[1]), cls_scene))
        first = h.instance_frames(0, 2, W0, H0, class_map=CM)
        ptr, tables = h.instance_device_frames(), [h.instances_of(b) for b in range(2)]
        assert ptr and first.any()
        for fn, what in ((h.instance_frames, "frames"), (h.instance_batch, "images")):
            two = what == "frames"
            refused(ya.capi.EINVAL, "at least 1", fn, 0, 0, W0, H0)
            refused(ya.capi.EINVAL, "at least 1", fn, 0, -1, W0, H0)
            refused(ya.capi.EINVAL, "outside the last tail", fn, -1, 1, W0, H0)
            refused(ya.capi.EINVAL, "outside the last tail", fn, 2 if two else 4, 1, W0, H0)
            refused(ya.capi.EINVAL, "outside the last tail", fn, 1, 2 if two else 4, W0, H0)
            refused(ya.capi.EINVAL, "1 .. 4096", fn, 0, 1, 0, H0)
            refused(ya.capi.EINVAL, "1 .. 4096", fn, 0, 1, W0, 4097)
            refused(ya.capi.EINVAL, "above 3", fn, 0, 1, W0, H0, class_map=np.uint8([1, 2, 3, 4, 0]))
            refused(ya.capi.EINVAL, "NaN", fn, 0, 1, W0, H0, min_score=float("nan"))
            # every refused call left the batch, its pointer and its tables as they were
            assert h.instance_device_frames() == ptr and h.L.yh_tfl_instance_row_width(h.h) == 5
            assert all(np.array_equal(h.instances_of(b), tables[b]) for b in range(2))
        assert all(_same(x, y) for x, y in zip(_scene_of(depths, ptr=ptr), _scene_of(depths, host=first)))
        refused(ya.capi.EINVAL, "outside the last batch", h.instances_of, 2)
        assert h.L.yh_tfl_instance_read(h.h, 0, ya.capi.C.byref(n), np.zeros(5, np.int32).ctypes.data_as(ya.capi.C.c_void_p), 0) == \
            (ya.capi.EOVERFLOW if len(tables[0]) else ya.capi.OK)
        # a per-image batch replaces it and the row width follows; then the per-frame one again
        h.instance_batch(0, 4, W0, H0, class_map=CM, read=False)
        assert h.L.yh_tfl_instance_row_width(h.h) == 4 and h.instances_of(3).shape[1] == 4
        again = h.instance_frames(0, 2, W0, H0, class_map=CM)
        assert np.array_equal(again, first) and all(np.array_equal(h.instances_of(b), tables[b]) for b in range(2))
        # the ground has not moved: detections, the classify batch's frames and pointer, the plan
        after = _ground(h)
        assert after == before and all(_same(x, y) for x, y in zip(_scene_of(depths, ptr=after[1]), cls_scene))
        # a newer input or invoke: the detections are no longer current, and the refused call keeps the batch
        ptr = h.instance_device_frames()
        h.set_batch(2)
        h.set_input(np.zeros((2, S, S, 3), np.uint8))
        refused(ya.capi.ESTATE, "no detections", h.instance_frames, 0, 1, W0, H0)
        assert h.instance_device_frames() == ptr and np.array_equal(h.instances_of(1), tables[1])
        h.evaluate()
        h.invoke()
        refused(ya.capi.ESTATE, "no detections", h.instance_batch, 0, 1, W0, H0)
        h.detect()
        refused(ya.capi.EINVAL, "outside the last tail", h.instance_frames, 1, 1, W0, H0)   # two images: one frame
        h.instance_frames(0, 1, W0, H0, class_map=CM)
        assert h.instances_of(0).shape[1] == 5
    finally:
        h.close()
