"""The cases of tests/refpath_cases.py, proven on the CPU alone: every builder's inputs do what the case claims, so that the bit-exact
comparison of tests/test_gpu_refpath_edges.py cannot pass vacuously (a wrong compare really changes a class, a spiral really is one
long component, an exact half really occurs, the painter really paints the class it is told), and the oracle (oracle/orc_ref.c) is
pinned against a second restatement of the same source lines (tests/refpath_ref.py) on every one of them."""
import numpy as np
import pytest

import refpath_cases as R
import refpath_ref as P

POP_CAP = 20000            # > 4096 cells: see refpath_ref.terrible_id


def _classes_ids(img, grid):
    """Class and id byte of every cell from a code image."""
    cells = np.asarray(img).reshape(grid * 8, grid * 8)[::8, ::8].reshape(-1)
    return (cells >> 24).astype(np.uint8), ((cells >> 16) & 0xFF).astype(np.uint8)


@pytest.mark.parametrize("cid", R.POST_IDS)
def test_oracle_and_restatement_agree_on_every_postprocess_case(oracle, cid):
    case = R.build_post(cid)
    g, C = case["grid"], case["C"]
    assert case["tiles"].dtype == np.float32 and case["tiles"].shape[1:] == (g * g, C)
    used = set()
    for idx, mode in case["calls"]:
        used.update(idx)
        assert 1 <= len(idx) <= 2 and mode in (R.STRICT, R.SANE)
    assert used == set(range(len(case["tiles"])))
    for t, tile in enumerate(case["tiles"]):
        for mode in (R.STRICT, R.SANE):
            rc, want = oracle.postprocess_tile(tile, g, C, mode)
            div, img = P.postprocess_tile(tile, g, mode, POP_CAP)
            assert bool(rc) == div, (cid, t, mode)
            if not div:
                assert np.array_equal(img.reshape(-1), want), (cid, t, mode)
            assert mode == R.STRICT or not div


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("cid", [c for c in R.POST_IDS if c.startswith("a_")])
def test_a_lattice_is_complete_and_sensitive(oracle, cid):
    case = R.build_post(cid)
    C = case["C"]
    cells = case["tiles"].reshape(-1, C)
    index = case["index"].reshape(-1)
    live = index >= 0
    assert sorted(index[live].tolist()) == list(range(6561))                       # every pattern once
    pats = cells[live, :4]
    assert len({p.tobytes() for p in pats}) == 6561                                # ... and they are 6561 different bit patterns
    for v in R.LATTICE:                                                            # each value in each of the four places
        same = (pats.view(np.uint32) == np.float32(v).view(np.uint32))
        assert (same.sum(0) == 729).all()
    assert float(R.LATTICE[5]) == 2.0 ** -149 and np.signbit(R.LATTICE[3]) and R.LATTICE[3] == 0
    if C > 4:
        junk = cells[:, 4:]
        assert np.isnan(junk).any() and np.isposinf(junk).any() and (junk == np.float32(3e38)).any()
    right = P.gated_argmax(cells)
    assert np.array_equal(right, oracle.gated_argmax(cells, C))
    assert set(right[live].tolist()) == {0, 1, 2, 3}
    for variant in ("flush", "ge", "nanmax"):                                      # each wrong compare is visible
        wrong = P.gated_argmax(cells, variant)
        assert (wrong[live] != right[live]).any(), variant
    # the lattice's STRICT verdict per tile is the oracle's; most tiles hold adjacent balls
    assert any(oracle.postprocess_tile(t, case["grid"], C, R.STRICT)[0] for t in case["tiles"])


# ---------------------------------------------------------------------------------------------- (b)
def _sane(oracle, case):
    rc, img = oracle.postprocess_tile(case["tiles"][0], case["grid"], case["C"], R.SANE)
    assert rc == 0
    cls, ids = _classes_ids(img, case["grid"])
    assert np.array_equal(cls, case["classes"])
    assert (ids[cls != 3] == 0xFF).all()
    return cls, ids


@pytest.mark.parametrize("g", R.GRIDS)
def test_b_long_paths_are_one_component_of_the_claimed_length(oracle, g):
    nc = g * g
    for name in ("spiral_in", "spiral_out"):
        case = R.build_post(f"b_{name}_g{g}")
        cls, ids = _sane(oracle, case)
        path = case["path"]
        assert len(path) == len(set(path)) == int((cls == 3).sum()) >= nc // 2 - g
        on = set(path)
        for a, b in zip(path, path[1:]):                                           # a path of 4-connected steps ...
            assert abs(a - b) == g or (abs(a - b) == 1 and a // g == b // g)
        for k, c in enumerate(path):                                               # ... one cell wide: only path neighbours touch
            y, x = divmod(c, g)
            nb = {q for ok, q in ((x > 0, c - 1), (x < g - 1, c + 1), (y > 0, c - g), (y < g - 1, c + g)) if ok and q in on}
            assert nb == set(path[max(k - 1, 0):k] + path[k + 1:k + 2])
        assert (ids[cls == 3] == 0).all()
        root = min(path)
        assert root == 0
        assert path.index(root) == (0 if name == "spiral_in" else 2 * (g - 1))     # where the root sits along the path
    for name in ("serpentine", "u", "comb", "all3"):
        case = R.build_post(f"b_{name}_g{g}")
        cls, ids = _sane(oracle, case)
        assert (ids[cls == 3] == 0).all() and (cls == 3).sum() >= (nc // 2 if name in ("serpentine", "all3") else 3 * g - 3)
    assert (R.build_post(f"b_all3_g{g}")["classes"] == 3).all()
    assert int(np.nonzero(R.build_post(f"b_u_g{g}")["classes"])[0][0]) == g - 1    # the U's root: top of the right arm
    comb = R.build_post(f"b_comb_g{g}")["classes"]
    assert (np.nonzero(comb[:g])[0] == [(g - 1) // 2 * 2]).all()                   # the comb's root: top of the last tooth


@pytest.mark.parametrize("g", R.GRIDS)
def test_b_id_ranks_and_the_clamp(oracle, g):
    nc = g * g
    cls, ids = _sane(oracle, R.build_post(f"b_checker_g{g}"))
    n = (nc + 1) // 2
    assert int((cls == 3).sum()) == n == {8: 32, 9: 41, 28: 392, 64: 2048}[g]
    hist = np.bincount(ids[cls == 3], minlength=128)
    if n > 128:
        assert (hist[:127] == 1).all() and hist[127] == n - 127
    else:
        assert (hist[:n] == 1).all() and hist[n:].sum() == 0
    if g >= 28:
        for n, top in ((127, 126), (128, 127), (129, 127)):
            case = R.build_post(f"b_balls{n}_g{g}")
            cls, ids = _sane(oracle, case)
            assert int((cls == 3).sum()) == n and int(ids[cls == 3].max()) == top
            assert np.array_equal(np.sort(ids[cls == 3])[:127], np.arange(127))
    cls, ids = _sane(oracle, R.build_post(f"b_wrap_balls_g{g}"))
    assert ids[cls == 3].tolist() == [0, 1]
    case = R.build_post(f"b_wrap_balls_g{g}")
    assert [(a % g, b % g, b - a) for a, b in R.linear_pairs(case["classes"], g)] == [(g - 1, 0, 1)]
    cls, ids = _sane(oracle, R.build_post(f"b_separated_g{g}"))
    assert set(cls.tolist()) == {1, 2, 3} and sorted(set(ids[cls == 3].tolist())) == list(range((g + 1) // 2))
    cls, ids = _sane(oracle, R.build_post(f"b_corners_g{g}"))
    assert np.nonzero(cls == 3)[0].tolist() == [0, g - 1, nc - g, nc - 1] and ids[cls == 3].tolist() == [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("g", R.GRIDS)
def test_c_each_strict_tile_has_the_pairs_it_claims(oracle, g):
    nc = g * g
    want_pair = dict(wrap_pair=lambda a, b: b == a + 1 and a % g == g - 1, vertical_pair=lambda a, b: b == a + g and b >= nc - g,
                     pair_first=lambda a, b: (a, b) == (0, 1), pair_last=lambda a, b: (a, b) == (nc - 2, nc - 1))
    for name in R.C_SHAPES:
        case = R.build_post(f"c_{name}_g{g}")
        pairs = R.linear_pairs(case["classes"], g)
        assert len(pairs) == case["pairs"], name
        if name in want_pair:
            assert len(pairs) == 1 and want_pair[name](*pairs[0])
        elif name == "checker":
            assert all(b == a + 1 and a % g == g - 1 for a, b in pairs) and (len(pairs) > 0) == (g % 2 == 0)
        else:
            assert not pairs and int((case["classes"] == 3).sum()) >= 2
        rc, img = oracle.postprocess_tile(case["tiles"][0], g, case["C"], R.STRICT)
        assert bool(rc) == bool(pairs)
        if not pairs:
            assert np.array_equal(img.reshape(g * 8, g * 8)[::8, ::8].reshape(-1), case["classes"].astype(np.uint32) << 24)


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("cid", [c for c in R.POST_IDS if c.startswith("d_")])
def test_d_sequence_diverges_in_tile_one_of_the_first_call_only(oracle, cid):
    case = R.build_post(cid)
    g = case["grid"]
    npairs = [len(R.linear_pairs(c, g)) for c in case["classes"]]
    assert npairs[1] >= 1 and npairs[0] == npairs[2] == npairs[3] == npairs[4] == 0
    balls = [int((c == 3).sum()) for c in case["classes"]]
    assert balls[0] > balls[2] > balls[3] > balls[4] >= 1
    verdicts = [R.post_reference(oracle, case, idx, mode)[0] for idx, mode in case["calls"]]
    assert verdicts == [True] + [False] * 6
    assert [m for _, m in case["calls"]] == [0, 0, 0, 1, 1, 1, 0] and case["calls"][0][0] == [0, 1]


# ---------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("rid", R.RESIZE_IDS)
def test_e_resize_restatement_equals_the_oracle(oracle, rid):
    (sw, sh), (dw, dh) = R.RESIZE_SHAPES[R.RESIZE_IDS.index(rid)]
    for content in R.RESIZE_CONTENTS:
        src = R.resize_content(content, sw, sh)
        assert src.shape == (sh, sw, 3) and src.dtype == np.uint8
        want = oracle.resize_triangle_rgb8(src, dw, dh)
        assert np.array_equal(P.resize(src, dw, dh), want), (rid, content)
        if content == "full":
            assert (want == 255).all()
        if content == "zero":
            assert (want == 0).all()
        if content == "channels":
            assert (want == [0, 128, 255]).all()
        if (sw, sh, dw, dh) == (448, 224, 224, 112) and content in ("checker_0_1", "checker_254_255"):
            even = P.resize(src, dw, dh, round="even")                           # exact halves: the rounding rule decides
            assert not np.array_equal(even, want)
            lo = int(content.split("_")[1])
            assert (want[1:-1, 1:-1] == lo + 1).all() and (even[1:-1, 1:-1] == lo + (lo % 2)).all()


def test_e_shapes_are_the_ones_named():
    assert R.RESIZE_SHAPES == [((1, 1), (5, 3)), ((1, 7), (9, 1)), ((2, 3), (640, 1)), ((1280, 1), (1, 1)), ((640, 480), (1, 1)),
                               ((3, 3), (4, 3)), ((448, 224), (224, 112)), ((224, 112), (448, 224)), ((97, 89), (101, 83))]
    assert len(R.RESIZE_CONTENTS) == 8 and len(set(R.CASE_IDS)) == len(R.CASE_IDS)
    assert R.FRAME_SIZES == [(448, 224), (1, 1), (3, 2), (447, 225), (200, 600), (1280, 720)]


# ---------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("image_axis", [False, True])
def test_g_painter_paints_the_chosen_classes_with_margin(oracle, image_axis):
    model = R.painter(image_axis)
    assert len(model.outputs) == 5
    for name in R.PAINT_PATTERNS:
        cl2 = R.paint_tiles(name)
        frame = R.painted_frame(cl2)
        tiles = oracle.classify_pre(frame, 2 * R.PAINT_S, R.PAINT_S, R.PAINT_S)       # 128 x 64: the identity
        assert np.array_equal(tiles[0][::8, ::8].reshape(-1, 3), R.PAINT_RGB[cl2[0]])
        cells, q = R.painter_cells(oracle, model, tiles)
        for t in range(2):
            assert np.array_equal(oracle.gated_argmax(cells[t], R.PAINT_C), cl2[t]), name
            assert np.array_equal(P.gated_argmax(cells[t]), cl2[t])
        steps = q.astype(np.int64)[..., :4] - R.PAINT_ZP
        assert (np.abs(steps) >= 2).all()                                             # every logit two steps from 0 ...
        srt = np.sort(steps, axis=-1)
        won = np.concatenate(cl2) > 0
        assert ((srt[..., -1] - srt[..., -2]).reshape(-1)[won] >= 2).all()            # ... and the winner two from its rival
        assert (cells[..., 4] > np.maximum(cells[..., :4].max(-1), 0)).all()              # channel 4 is the largest, and ignored
    assert set(np.concatenate([R.paint_tiles(n)[0] for n in R.PAINT_PATTERNS] + [R.paint_other()]).tolist()) == {0, 1, 2, 3}
