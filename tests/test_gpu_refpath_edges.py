"""Deterministic edge cases of the reference-compat path (csrc/refpath.hip: resize_v / resize_h, cells_postprocess, upsample_codes;
cells_f32 of elementwise.hip) on the device, bit for bit against the CPU oracle. The cases come from
tests/refpath_cases.py; tests/test_refpath_cases.py proves on the CPU that each of them does what it claims and that the oracle
agrees with a second restatement (tests/refpath_ref.py) on every one, so equality here is not vacuous. There are no tolerances:
the path is integer logic and f32 arithmetic with one rounding per operation. YH_EDIVERGE is expected exactly where the oracle
reports that the reference's flood fill does not terminate, and nowhere else. One test per case id:

  a  all 9^4 4-tuples over {NaN, -inf, -1, -0, +0, 2^-149, 1, 1 + ulp, +inf} as the first four logits (grid 28 with 81 and 5 logits
     per cell, grid 64), logits 4 .. C-1 = +inf / NaN / 3e38: classes and ids in SANE mode, the verdict per tile in STRICT mode
  b  SANE components on grids 8, 9, 28, 64: spirals, a serpentine, a U and a comb whose labels travel against raster order, one
     component over the whole tile, checkerboards (ids 0 .. 126, then 127), 127 / 128 / 129 balls, balls across the row wrap
  c  the STRICT predicate: one offending pair per linear neighbour (row wrap, last two rows, cells 0 1, cells nc-2 nc-1) and the
     nearest tiles without one; the checkerboard, which diverges through the row wrap on even grids only
  d  call sequences over one handle: a diverging two-tile call, one tile, two tiles with fewer balls, both modes
  e  yh_resize_triangle_rgb8 on one-pixel sources, one-pixel targets, exact 2:1 and 1:2, primes; constants, checkers that give
     exact halves, ramps
  f  yh_classify_frame_u32 at S = 224 on frames of 448x224 (both passes must be the identity), 1x1, 3x2, 447x225, 200x600 and
     1280x720: the oracle's post half on the engine's own output 4, the oracle's pre half through set_input + invoke
  g  yh_tfl_classify_frame_u32 through a painter model (one 8x8 stride-8 convolution: a frame painted in 8x8 blocks gives chosen
     classes), on 128x64 frames (identity) and, for one pattern, 160x120 and 37x91. The plain painter is eligible for the batch
     plan (both tiles in one invoke); the variant with a CONCATENATION along the image axis runs one invoke per tile. Both run.

Engine(input_size=512, max_batch=2, use_graph=False) is created in 0.01 s on an MI355X, like the other sizes, so grid 64 keeps
every family. The file's 157 tests take 7 s together."""
import numpy as np
import pytest

import refpath_cases as R
import tfl_builder as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(built):
    """One engine per (input_size, num_classes), made on first use and closed at the end. Only the S = 224, C = 81 engine needs
    the network (family f): it gets weights and the graph; the others are used for their compat scratch alone."""
    import yolact_amd as ya
    made = {}

    def get(S, C):
        if (S, C) not in made:
            net = (S, C) == (224, 81)
            e = ya.Engine(input_size=S, max_batch=2, use_graph=net, num_classes=C)
            if net:
                e.load_weights(e.generate_weights(seed=1))
            made[(S, C)] = e
        return made[(S, C)]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def painters(built):
    import yolact_amd as ya
    made = {}

    def get(image_axis):
        if image_axis not in made:
            model = R.painter(image_axis)
            made[image_axis] = (model, ya.TfliteEngine(B.serialize(model)))
        return made[image_axis]
    yield get
    for _, e in made.values():
        e.close()


def _expect_diverge(ya, call):
    with pytest.raises(ya.YhError) as e:
        call()
    assert e.value.code == ya.EDIVERGE


@pytest.mark.parametrize("cid", R.POST_IDS)
def test_postprocess_edge_case(engines, oracle, cid):
    import yolact_amd as ya
    case = R.build_post(cid)
    eng = engines(case["grid"] * 8, case["C"])
    n_div = 0
    for idx, mode in case["calls"]:
        div, want = R.post_reference(oracle, case, idx, mode)
        cells = case["tiles"][idx]
        if div:
            n_div += 1
            _expect_diverge(ya, lambda: eng.postprocess_cells(cells, mode))
        else:
            assert np.array_equal(eng.postprocess_cells(cells, mode), want), (cid, idx, mode)
    if cid.startswith("c_") and case["pairs"]:
        assert n_div == 1                                  # the STRICT call of an offending tile
    if cid.startswith("d_"):
        assert n_div == 1


@pytest.mark.parametrize("rid", R.RESIZE_IDS)
def test_resize_edge_case(engines, oracle, rid):
    (sw, sh), (dw, dh) = R.RESIZE_SHAPES[R.RESIZE_IDS.index(rid)]
    eng = engines(64, 5)
    for content in R.RESIZE_CONTENTS:
        src = R.resize_content(content, sw, sh)
        assert np.array_equal(eng.resize_triangle(src, dw, dh), oracle.resize_triangle_rgb8(src, dw, dh)), (rid, content)


@pytest.mark.parametrize("fid", R.FRAME_IDS)
def test_classify_frame_edge_case(engines, oracle, golden_dir, fid):
    """Yolact::classify in place, the network in the middle: SANE first (it never diverges), then STRICT with the verdict the
    oracle gives on the same cells - equal to the oracle, or YH_EDIVERGE with the frame untouched."""
    import yolact_amd as ya
    k = R.FRAME_IDS.index(fid)
    (w, h), content = R.FRAME_SIZES[k // len(R.FRAME_CONTENTS)], R.FRAME_CONTENTS[k % len(R.FRAME_CONTENTS)]
    eng = engines(224, 81)
    frame0 = oracle.pack_rgb(R.frame_rgb(content, w, h, golden_dir))
    frame = frame0.copy()
    eng.classify_frame(frame, w, h, ya.COMPAT_SANE)
    cells = eng.output(4)
    assert cells.shape == (2, 28, 28, 81)
    rc, want = oracle.classify_post(cells, 224, 81, ya.COMPAT_SANE, w, h)
    assert rc == 0 and np.array_equal(frame, want)
    rc, want = oracle.classify_post(cells, 224, 81, ya.COMPAT_STRICT, w, h)
    frame = frame0.copy()
    if rc:
        _expect_diverge(ya, lambda: eng.classify_frame(frame, w, h, ya.COMPAT_STRICT))
        assert np.array_equal(frame, frame0)
    else:
        eng.classify_frame(frame, w, h, ya.COMPAT_STRICT)
        assert np.array_equal(frame, want)
        assert (oracle.consumer_low16(frame) == 0).all()
    assert np.array_equal(eng.output(4), cells)            # the same tiles, the same network: STRICT saw the same cells
    # the pre-processing half: the oracle's tiles through invoke give the same output 4
    tiles = oracle.classify_pre(frame0, w, h, 224)
    if (w, h) == (448, 224):
        rgb = oracle.unpack_rgb(frame0).reshape(224, 448, 3)
        assert np.array_equal(tiles[0], rgb[:, :224]) and np.array_equal(tiles[1], rgb[:, 224:])   # the oracle copies here
    eng.set_input(tiles)
    eng.invoke()
    assert np.array_equal(eng.output(4), cells)


def _painter_frame(ya, oracle, model, eng, frame0, w, h, mode):
    """One yh_tfl_classify_frame_u32 against the oracle on the painter's own cells; returns whether it diverged."""
    tiles = oracle.classify_pre(frame0, w, h, R.PAINT_S)
    cells, _ = R.painter_cells(oracle, model, tiles)
    rc, want = oracle.classify_post(cells, R.PAINT_S, R.PAINT_C, mode, w, h)
    frame = frame0.copy()
    if rc:
        _expect_diverge(ya, lambda: eng.classify_frame(frame, w, h, mode))
        assert np.array_equal(frame, frame0)
    else:
        eng.classify_frame(frame, w, h, mode)
        assert np.array_equal(frame, want)
    return bool(rc), cells


@pytest.mark.parametrize("image_axis", [False, True])
def test_painter_model_matches_the_tflite_oracle(painters, oracle, image_axis):
    import tfl_oracle as TO
    import yolact_amd as ya
    model, eng = painters(image_axis)
    if image_axis:                                         # which branch classify takes: the batch plan needs set_batch(2) to hold
        with pytest.raises(ya.YhError) as e:
            eng.set_batch(2)
        assert e.value.code == ya.capi.EINVAL
    else:
        eng.set_batch(2)
        eng.set_batch(1)
    tiles = oracle.classify_pre(R.painted_frame(R.paint_tiles("separated")), 128, 64, R.PAINT_S)
    for t in range(2):
        val = TO.run_model(model, {model.inputs[0]: tiles[t:t + 1]})
        eng.set_input(tiles[t:t + 1])
        eng.invoke()
        for i in range(5):
            assert np.array_equal(eng.output(i), val[model.outputs[i]]), (image_axis, t, i)


@pytest.mark.parametrize("image_axis", [False, True])
@pytest.mark.parametrize("gid", R.PAINT_IDS)
def test_painted_classify_edge_case(painters, oracle, gid, image_axis):
    """image_axis False: the batch plan (both tiles in one invoke); True: one invoke per tile."""
    import yolact_amd as ya
    name = gid[len("g_painter_"):]
    model, eng = painters(image_axis)
    cl2 = R.paint_tiles(name)
    frame0 = R.painted_frame(cl2)
    pairs = R.linear_pairs(cl2[0], 8)
    for mode in (ya.COMPAT_SANE, ya.COMPAT_STRICT, ya.COMPAT_SANE):           # the last: a clean call after a diverging one
        div, cells = _painter_frame(ya, oracle, model, eng, frame0, 128, 64, mode)
        assert div == (mode == ya.COMPAT_STRICT and bool(pairs))
        for t in range(2):
            assert np.array_equal(oracle.gated_argmax(cells[t], R.PAINT_C), cl2[t])   # chosen classes, end to end
    if name == R.PAINT_RESIZED[0]:
        for w, h in R.PAINT_RESIZED[1]:
            _painter_frame(ya, oracle, model, eng, R.painted_frame(cl2, w, h), w, h, ya.COMPAT_SANE)
