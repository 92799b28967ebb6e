"""-m gpu: the TFLite detections (csrc/tfl_detect.hip; DESIGN.md §11 "TFLite detections") against tests/tfl_detect_ref.py, bit for
bit: (class, prior, score bits, box bits) tuples equal and masks array_equal. Through yh_tfl_op_detect - geometry, kind
combinations and zero points, the cases of tests/tfl_detect_cases.py - through a model (uint8, its int8 twin, float32 heads behind
DEQUANTIZE) at 1, 2 and 5 images, and the refusals, the states and the ground that must not move."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfl_builder as B
import tfl_builder_q as BQ
import tfl_cases as TC
import tfl_detect_cases as K
import tfl_detect_ref as R
import tfl_models as M
import tfl_q_cases as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(built):
    """A handle for yh_tfl_op_detect: it gives the device, the stream and the error text; its model (one RELU) is not involved."""
    import yolact_amd as ya
    e = ya.TfliteEngine(bytes(B.serialize(M.single_op("RELU", np.random.default_rng(0)))))
    yield e
    e.close()


def _op(eng, case, cfg=None):
    eng.op_detect(case["loc"], case["conf"], case["mask"], case["proto"], case["priors"], quant=case["quant"], **(cfg or case["cfg"]))


def _check(oracle, eng, case, label, cfg=None, min_dets=0):
    _op(eng, case, cfg)
    total = 0
    for b in range(case["n"]):
        dets, masks = eng.detections(b)
        wd, wm = R.detect(oracle, R.image(case, b), case["quant"], case["priors"], cfg or case["cfg"])
        assert R.tuples(dets) == R.tuples(wd), (label, b, len(dets), len(wd))
        assert masks.shape == wm.shape and np.array_equal(masks, wm), (label, b, int((masks != wm).sum()))
        total += len(wd)
    assert total >= min_dets, (label, total)
    return total


GEOMETRY = [(C, hw, n) for C in (2, 6, 81) for hw, n in (((16, 16), 1), ((7, 9), 2), ((2, 2), 3))] + [(6, (16, 16), n) for n in (2, 3, 9)] + \
           [(81, (7, 9), 9)]


@pytest.mark.parametrize("C,hw,n", GEOMETRY)
def test_geometry(oracle, eng, C, hw, n):
    """P = 250 (K1q's last workgroup and wave are ragged), every class count, a map of 256 pixels, one whose pixel count is no
    multiple of 4 (the byte-store path) and one smaller than a dword row, and every grouping of the mask grid's detections."""
    case = K.random_case(K.COMBOS["all_u8"], (128, 120, 131, 100), n, C, hw[0], hw[1], 1000 + C + n)
    _check(oracle, eng, case, (C, hw, n), min_dets=10 * n)


@pytest.mark.parametrize("combo", list(K.COMBOS))
@pytest.mark.parametrize("zi", (0, 1, 2))
def test_kinds_and_zero_points(oracle, eng, combo, zi):
    kinds = K.COMBOS[combo]
    zps = tuple(0 if k == "f32" else K.ZPS[k][zi] for k in kinds)
    for scales in (K.POW2, K.ODD):
        case = K.random_case(kinds, zps, 2, 6, 16, 16, 200 + zi, scales=scales)
        _check(oracle, eng, case, (combo, zi, scales["mask"]), min_dets=20)
        case = K.random_case(kinds, zps, 1, 6, 7, 9, 300 + zi, scales=scales)
        _check(oracle, eng, case, (combo, zi, "7x9"), min_dets=20)


@pytest.mark.parametrize("combo,zps", [("all_f32", (0, 0, 0, 0)), ("all_i8", (3, -7, 5, -100)), ("f32proto_u8mask", (128, 1, 200, 0))])
def test_81_classes_in_every_kind(oracle, eng, combo, zps):
    """K1q's three forms at C = 81: float32 rows are its largest LDS image (128 x 81 dwords) and the dword re-pitch loop; byte rows
    of 81 start on every byte of a dword (P = 250: image 1 begins at byte 20 250 of the tensor)."""
    case = K.random_case(K.COMBOS[combo], zps, 2, 81, 7, 9, 77)
    _check(oracle, eng, case, (combo, 81), min_dets=40)


def test_ties(oracle, eng):
    _check(oracle, eng, K.ties(), "ties", min_dets=7)
    _check(oracle, eng, K.ties(K.COMBOS["all_i8"], (0, 0, 0, 0)), "ties i8", min_dets=7)


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_topk_and_dets_cut(oracle, eng, delta):
    assert _check(oracle, eng, K.topk_cut(8 + delta), ("topk", delta)) == min(8 + delta, 8)
    assert _check(oracle, eng, K.dets_cut(6 + delta), ("dets", delta)) == min(6 + delta, 6)


def test_suppress_pair_and_none(oracle, eng):
    assert _check(oracle, eng, K.suppress_pair(True), "pair") == 1
    assert _check(oracle, eng, K.suppress_pair(False), "no pair") == 2


def test_threshold_on_and_one_ulp_either_side(oracle, eng):
    case = K.threshold_group()
    _op(eng, case)
    dets, _ = eng.detections(0)
    shared = [d for d in dets if d["prior"] in case["shared_priors"]]
    assert len(shared) == 5
    for t, n in zip(K.thresholds(shared[0]["score"]), (6, 1, 1)):
        assert _check(oracle, eng, case, ("thresh", t), cfg=dict(case["cfg"], conf_thresh=t)) == n


def test_no_candidate_then_a_full_call(oracle, eng):
    """The second call runs on the first call's workspaces as they were left (same geometry: yh_tfl_op_detect keeps them), and the
    full call before them has left masks and survivor slots behind."""
    empty, full = K.empty_then_full()
    assert _check(oracle, eng, full, "full") > 40
    assert _check(oracle, eng, empty, "empty") == 0
    assert _check(oracle, eng, full, "full again") > 40
    assert _check(oracle, eng, empty, "empty again") == 0


def test_windows_band_and_saturation(oracle, eng):
    for kinds, zps in ((K.COMBOS["all_u8"], (128, 128, 128, 128)), (K.COMBOS["all_i8"], (0, 0, -5, 3)), (K.COMBOS["f32proto_u8mask"], (128, 128, 128, 0))):
        assert _check(oracle, eng, K.windows(kinds, zps), ("windows", kinds)) == len(K.WINDOWS)
    for kinds, zps in ((K.COMBOS["all_u8"], (128, 128, 128, 128)), (K.COMBOS["u8proto_i8mask"], (128, 0, 0, 128)), (K.COMBOS["i8proto_u8mask"], (0, 128, 128, 0))):
        assert _check(oracle, eng, K.band(kinds, zps), ("band", kinds)) == 1
    for sign in (1, -1):
        for combo in ("all_u8", "all_i8", "u8proto_i8mask", "i8proto_u8mask"):
            _check(oracle, eng, K.saturated(sign, K.COMBOS[combo]), ("saturated", sign, combo), min_dets=5)


def test_op_detect_refuses(eng):
    import yolact_amd as ya
    case = K.random_case(K.COMBOS["all_u8"], (128,) * 4, 1, 6, 4, 4, 1, P=10)
    for cfg, quant, word in ((dict(top_k=257), None, "top_k"), (dict(max_dets=129), None, "max_dets"), (dict(conf_thresh=float("nan")), None, "conf_thresh"),
                             ({}, dict(case["quant"], mask=(0.0, 128)), "finite and positive"), ({}, dict(case["quant"], proto=(0.05, 256)), "zero point")):
        with pytest.raises(ya.YhError) as e:
            eng.op_detect(case["loc"], case["conf"], case["mask"], case["proto"], case["priors"], quant=quant or case["quant"], **dict(case["cfg"], **cfg))
        assert e.value.code == ya.capi.EINVAL and word in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------------------ through a model
S, C, P, HP = 128, 6, 1023, 32
CFG = dict(top_k=200, max_dets=100, conf_thresh=0.05, nms_thresh=0.5)
_MODELS = {}


def _model(kind):
    """(model, blob, its reference outputs for 5 images, the images): computed once per kind and left unchanged."""
    if kind not in _MODELS:
        m = M.mobilenetv2_yolact(np.random.default_rng(3), S=S, C=C, fpn=32)
        x = np.random.default_rng(4).integers(0, 256, (5, S, S, 3), dtype=np.uint8)
        if kind == "i8":
            m = Q.int8_twin(m, np.random.default_rng(5), dequant_output=None, quant_output=4)
            blob, want = BQ.serialize(m), Q.reference_images(m, x)
        else:
            if kind == "f32":
                m = K.dequantized_heads(m)
            blob, want = bytes(B.serialize(m)), TC.oracle_images(m, x)
        _MODELS[kind] = (m, blob, want, x)
    return _MODELS[kind]


def _quant(m):
    return {r: (float(m.tensors[m.outputs[i]].scale), int(np.atleast_1d(m.tensors[m.outputs[i]].zp)[0])) for i, r in enumerate(R.ROLES)
            if m.tensors[m.outputs[i]].dtype != "f32"}


def _priors():
    import yolact_amd as ya
    return ya.tfl_priors([16, 8, 4, 2, 1], S)


@pytest.mark.parametrize("kind", ("u8", "i8", "f32"))
def test_evaluate_through_a_model(oracle, eng, kind):
    import yolact_amd as ya
    m, blob, want, x = _model(kind)
    quant, pri = _quant(m), _priors()
    assert pri.shape == (P, 4) and [m.tensors[o].dtype for o in m.outputs[:4]] == [kind] * 4
    ref = []
    for b in range(5):
        img = {r: np.asarray(want[b][m.outputs[i]])[0] for i, r in enumerate(R.ROLES)}
        ref.append(R.detect(oracle, img, quant, pri, CFG))
    assert any(len(d) > 0 and k.any() for d, k in ref)            # (equality below is not vacuous)
    h = ya.TfliteEngine(blob, max_images=5)
    try:
        h.detect_setup(pri, **CFG)
        assert h.proto_dims() == (HP, HP)
        for nb in (1, 2, 5):
            h.set_batch(nb)
            h.set_input(np.ascontiguousarray(x[:nb]))
            h.evaluate()
            got = [h.detections(b) for b in range(nb)]
            for b in range(nb):
                assert R.tuples(got[b][0]) == R.tuples(ref[b][0]), (kind, nb, b)
                assert np.array_equal(got[b][1], ref[b][1]), (kind, nb, b)
            # ... and op_detect on the bytes yh_tfl_output_read returns
            outs = [h.output(i).reshape((nb,) + tuple(m.tensors[m.outputs[i]].shape[1:])) for i in range(4)]
            eng.op_detect(*outs, pri, quant=quant, **CFG)
            for b in range(nb):
                d2, k2 = eng.detections(b)
                assert R.tuples(d2) == R.tuples(got[b][0]) and np.array_equal(k2, got[b][1]), (kind, nb, b)
            # the tail alone gives the same again
            h.detect()
            d3, k3 = h.detections(nb - 1)
            assert R.tuples(d3) == R.tuples(got[nb - 1][0]) and np.array_equal(k3, got[nb - 1][1])
    finally:
        h.close()


def test_stage_times_run_the_tail_and_keep_its_results(oracle):
    """yh_tfl_detect_stage_times (the measurement entry tools/time_tflite.py --detect uses): the states of yh_tfl_detect, four finite
    non-negative times, and afterwards the detections an evaluate gives."""
    import yolact_amd as ya
    m, blob, _, x = _model("u8")
    h = ya.TfliteEngine(blob, max_images=5)
    try:
        def refused(code, word, fn, *a, **kw):
            with pytest.raises(ya.YhError) as e:
                fn(*a, **kw)
            assert e.value.code == code and word in str(e.value), (word, str(e.value))
        refused(ya.capi.ESTATE, "no detections", h.detections, 0)                    # (no setup: the library's own state error)
        refused(ya.capi.ESTATE, "before yh_tfl_detect_setup", h.detect_stage_times, 2)
        h.detect_setup(_priors(), max_images=2, **CFG)
        refused(ya.capi.ESTATE, "before any invoke", h.detect_stage_times, 2)
        h.set_batch(3)
        h.set_input(np.ascontiguousarray(x[:3]))
        h.invoke()
        refused(ya.capi.EINVAL, "max_images", h.detect_stage_times, 2)
        assert h.L.yh_tfl_detect_stage_times(h.h, 0, None) == ya.capi.EINVAL
        h.set_batch(2)
        h.set_input(np.ascontiguousarray(x[:2]))
        h.evaluate()
        want = [h.detections(b) for b in range(2)]
        assert all(len(d) > 0 for d, _ in want)
        h.invoke()                                                                   # (detections no longer current ...)
        ms = h.detect_stage_times(2)
        assert len(ms) == 4 and all(np.isfinite(v) and v >= 0.0 for v in ms) and sum(ms) > 0.0
        for b in range(2):                                                           # (... and current again: the tail has run)
            d, k = h.detections(b)
            assert R.tuples(d) == R.tuples(want[b][0]) and np.array_equal(k, want[b][1])
        refused(ya.capi.EINVAL, "image out of range", h.detections, 2)
    finally:
        h.close()


def _frames(n, W=96, H=64):
    rgb = np.random.default_rng(6).integers(0, 256, (n, H, W, 3), dtype=np.uint32)
    return ((rgb[..., 0] << 24) | (rgb[..., 1] << 16) | (rgb[..., 2] << 8)).astype(np.uint32)


def test_detect_after_a_classify_batch_runs_on_its_2n_tiles(oracle):
    import yolact_amd as ya
    m, blob, _, _ = _model("u8")
    frames = _frames(2)
    h = ya.TfliteEngine(blob, max_images=5)
    try:
        h.detect_setup(_priors(), **CFG)
        h.classify_batch(frames_u32=frames.copy(), width=96, height=64, mode=ya.COMPAT_SANE)
        h.detect()
        h.set_batch(4)                  # (the outputs hold the four tiles of that invoke; this only says how many to read)
        outs = [h.output(i).reshape((4,) + tuple(m.tensors[m.outputs[i]].shape[1:])) for i in range(4)]
        assert len({outs[1][b].tobytes() for b in range(4)}) == 4
        for b in range(4):
            img = {r: outs[i][b] for i, r in enumerate(R.ROLES)}
            wd, wm = R.detect(oracle, img, _quant(m), _priors(), CFG)
            dets, masks = h.detections(b)
            assert R.tuples(dets) == R.tuples(wd) and np.array_equal(masks, wm), b
        with pytest.raises(ya.YhError) as e:
            h.detections(4)
        assert e.value.code == ya.capi.EINVAL
    finally:
        h.close()


def _ground(h, x, frame):
    """What everybody already uses: the five outputs of an invoke of two images, a classified frame and the plan's launch counts."""
    import yolact_amd as ya
    h.set_batch(2)
    h.set_input(np.ascontiguousarray(x[:2]))
    h.invoke()
    outs = [h.output(i).tobytes() for i in range(5)]
    f = frame.copy()
    h.classify_frame(f, 96, 64, ya.COMPAT_SANE)
    return outs, f.tobytes(), h.plan_summary()


def test_refusals_states_and_unchanged_ground(oracle):
    import yolact_amd as ya
    m, blob, _, x = _model("u8")
    frame = _frames(1)[0].reshape(-1)
    fresh = ya.TfliteEngine(blob, max_images=5)
    want = _ground(fresh, x, frame)
    fresh.close()
    h = ya.TfliteEngine(blob, max_images=5)
    pri = _priors()
    try:
        def refused(code, word, fn, *a, **kw):
            with pytest.raises(ya.YhError) as e:
                fn(*a, **kw)
            assert e.value.code == code and word in str(e.value), (word, str(e.value))
        # states before a setup / before an invoke
        refused(ya.capi.ESTATE, "before yh_tfl_detect_setup", h.evaluate)
        refused(ya.capi.ESTATE, "before yh_tfl_detect_setup", h.detect)
        assert h.L.yh_tfl_detections_device(h.h) is None
        # setup rules on this model: shapes by pointing a role at another output, the prior count, the limits, max_images
        refused(ya.capi.EINVAL, "loc must be [1,P,4]", h.detect_setup, pri, outputs=(1, 0, 2, 3))
        refused(ya.capi.EINVAL, "mask must be [1,P,32]", h.detect_setup, pri, outputs=(0, 1, 1, 3))
        refused(ya.capi.EINVAL, "proto must be [1,hp,wp,32]", h.detect_setup, pri, outputs=(0, 1, 2, 4))
        refused(ya.capi.EINVAL, "disagree on the number of priors", h.detect_setup, pri, outputs=(0, 4, 2, 3))
        refused(ya.capi.EINVAL, "not an index", h.detect_setup, pri, outputs=(0, 1, 2, 5))
        refused(ya.capi.EINVAL, "n_priors is 1022", h.detect_setup, pri[:-1])
        refused(ya.capi.EINVAL, "top_k", h.detect_setup, pri, top_k=300)
        refused(ya.capi.EINVAL, "max_images", h.detect_setup, pri, max_images=6)
        refused(ya.capi.EINVAL, "reserved", h.detect_setup, pri, reserved=(0, 0, 1, 0))
        refused(ya.capi.ESTATE, "before yh_tfl_detect_setup", h.evaluate)           # (a refused setup is no setup)
        assert _ground(h, x, frame) == want
        # a setup for 2 images; detect before this handle's... the ground above has invoked: detect runs; a batch of 5 is refused
        h.detect_setup(pri, max_images=2, **CFG)
        refused(ya.capi.ESTATE, "no detections", h.detections, 0)
        h.set_batch(5)
        refused(ya.capi.EINVAL, "max_images", h.evaluate)
        h.set_input(np.ascontiguousarray(x))
        h.invoke()
        refused(ya.capi.EINVAL, "max_images", h.detect)
        h.set_batch(2)
        h.set_input(np.ascontiguousarray(x[:2]))
        h.evaluate()
        first = h.detections(1)
        h.set_input(np.ascontiguousarray(x[:2]))
        refused(ya.capi.ESTATE, "no detections", h.detections, 1)                   # a newer input
        h.evaluate()
        h.invoke()
        refused(ya.capi.ESTATE, "no detections", h.detections, 1)                   # a newer invoke without a tail
        h.detect()
        again = h.detections(1)
        assert R.tuples(again[0]) == R.tuples(first[0]) and np.array_equal(again[1], first[1]) and len(first[0]) > 0
        refused(ya.capi.EINVAL, "image out of range", h.detections, 2)
        # a second setup replaces the first: other thresholds, room for 5
        h.detect_setup(pri, **dict(CFG, max_dets=7))
        h.set_batch(5)
        h.set_input(np.ascontiguousarray(x))
        h.evaluate()
        assert [len(h.detections(b)[0]) for b in range(5)] == [7] * 5
        assert h.L.yh_tfl_detections_device(h.h) and h.L.yh_tfl_masks_device(h.h) and h.L.yh_tfl_detection_counts_device(h.h)
        # the ground has not moved under a setup
        assert _ground(h, x, frame) == want
    finally:
        h.close()


def test_detect_before_any_invoke(built):
    import yolact_amd as ya
    _, blob, _, _ = _model("u8")
    h = ya.TfliteEngine(blob, max_images=2)
    try:
        with pytest.raises(ya.YhError) as e:           # (no setup at all: the library's state error, not a Python one)
            h.detections(0)
        assert e.value.code == ya.capi.ESTATE and "no detections" in str(e.value)
        h.detect_setup(_priors(), **CFG)
        with pytest.raises(ya.YhError) as e:
            h.detect()
        assert e.value.code == ya.capi.ESTATE and "before any invoke" in str(e.value)
    finally:
        h.close()


@pytest.mark.parametrize("dtype", ("u8", "i8"))
def test_setup_rules_one_small_model_each(oracle, dtype):
    """tfl_detect_cases.heads_model bends one output per rule; the refused handle's invoke still gives a fresh handle's bytes. The
    unbent model is accepted and detects what the restatement says. (classify is not run here: these models have a [1,P,4] input
    and four outputs, which classify refuses by itself; invoke, a classified frame and the plan's launch counts are compared
    together, against a fresh handle, for the rules bent on the full model in test_refusals_states_and_unchanged_ground.)"""
    import yolact_amd as ya
    x = np.random.default_rng(9).integers(K.LIM[dtype][0], K.LIM[dtype][1] + 1, (1, 20, 4)).astype(K.DT[dtype])
    pri = K.grid_priors(20)
    for rule in [None] + list(K.RULES):
        m = K.heads_model(dtype, break_rule=rule)
        want = Q.reference_images(m, x)[0]
        h = ya.TfliteEngine(BQ.serialize(m))
        try:
            if rule is None:
                h.detect_setup(pri, conf_thresh=0.01)
            else:
                with pytest.raises(ya.YhError) as e:
                    h.detect_setup(pri, conf_thresh=0.01)
                assert e.value.code == ya.capi.EINVAL and K.RULES[rule] in str(e.value), (rule, str(e.value))
                if rule == "axis0":
                    h.detect_setup(pri, conf_thresh=0.01, max_images=1)     # one image per invoke: allowed
            h.set_input(x)
            h.invoke()
            for i, o in enumerate(m.outputs):
                if m.tensors[o].data is None:            # (a constant among the outputs is not an invoke's result)
                    assert np.array_equal(h.output(i).reshape(-1), np.asarray(want[o]).reshape(-1)), (rule, i)
            if rule in (None, "axis0"):
                h.evaluate()
                img = {r: np.asarray(want[m.outputs[i]])[0] for i, r in enumerate(R.ROLES)}
                wd, wm = R.detect(oracle, img, _quant(m), pri, dict(CFG, conf_thresh=0.01))
                dets, masks = h.detections(0)
                assert R.tuples(dets) == R.tuples(wd) and np.array_equal(masks, wm) and len(wd) > 0
        finally:
            h.close()
    # a head quantised per channel never reaches a handle: the reader refuses the file
    ok, _, _, msg = ya.tfl_validate(BQ.serialize(K.heads_model(dtype, break_rule="per_channel")))
    assert not ok and "per-channel" in msg


def test_tfl_priors_equal_the_engines(built):
    import yolact_amd as ya
    e = ya.Engine(input_size=128, max_batch=1, use_graph=False)
    try:
        want = e.priors()
    finally:
        e.close()
    assert want.shape == (P, 4)
    assert np.array_equal(ya.tfl_priors([16, 8, 4, 2, 1], 128), want)
