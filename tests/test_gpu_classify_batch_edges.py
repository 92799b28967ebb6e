"""The classify batch's two kernels alone (csrc/classify_batch.hip: resize_tables, classify_pre_batch, classify_post_batch; DESIGN.md
§11 "Classify batch") through yh_op_classify_pre_batch / yh_op_classify_post_batch, bit for bit against the CPU oracle's classify_pre
and classify_post. The shapes are the smallest at which the kernels can go wrong. Two engines without weights, max_batch 8:
input 64 (grid 8) and input 72 (grid 9: S is no multiple of the pre kernel's 32-column block, so a block straddles the seam between
the two tiles, and the last block row and column are partial). The frame sizes cover the identity, one pixel more and less than it,
magnification and minification in each direction separately, a single pixel, and minification strong enough that the pre kernel's
block window exceeds its LDS budget (2000 columns into 128 or 144: the fallback form). There are no tolerances."""
import numpy as np
import pytest

import refpath_cases as R

pytestmark = pytest.mark.gpu

SIZES = (64, 72)


def shapes(S):
    return [(640, 480), (2 * S, S), (2 * S + 1, S - 1), (33, 17), (1, 1), (300, 20), (50, 200), (7, 3), (2000, 9), (9, 1500)]


PARAMS = [(S, k) for S in SIZES for k in range(len(shapes(64)))]
IDS = [f"S{S}-{shapes(S)[k][0]}x{shapes(S)[k][1]}" for S, k in PARAMS]


@pytest.fixture(scope="module")
def engines(built):
    import yolact_amd as ya
    made = {S: ya.Engine(input_size=S, max_batch=8, use_graph=False) for S in SIZES}
    yield made
    for e in made.values():
        e.close()


def _frames(n, w, h, seed):
    """n distinct frames uint32 [n][h][w]: every channel uniform over 0 .. 255, the low byte never zero."""
    f = np.random.default_rng(seed).integers(0, 2 ** 32, (n, h, w), dtype=np.uint64).astype(np.uint32)
    return f | np.uint32(0x5A)


def _check_pre(eng, oracle, S, w, h, seed=None):
    f = _frames(3, w, h, w * 7919 + h if seed is None else seed)
    if w * h >= 640 * 480:
        for sh in (24, 16, 8):
            assert np.unique((f >> np.uint32(sh)) & 0xFF).size == 256                # all values in every channel
    tiles, form = eng.op_classify_pre_batch(f, w, h)
    assert tiles.shape == (6, S, S, 3) and form in (0, 1)
    for b in range(3):
        want = oracle.classify_pre(f[b], w, h, S)
        assert np.array_equal(tiles[2 * b:2 * b + 2], want), (S, w, h, b, np.argwhere(tiles[2 * b:2 * b + 2] != want)[:4].tolist())
        alone, form1 = eng.op_classify_pre_batch(f[b:b + 1], w, h)                   # frames do not leak into each other
        assert form1 == form and np.array_equal(alone, want), (S, w, h, b)
    return form


@pytest.mark.parametrize("S,k", PARAMS, ids=IDS)
def test_pre_kernel(engines, oracle, S, k):
    w, h = shapes(S)[k]
    _check_pre(engines[S], oracle, S, w, h)


@pytest.mark.parametrize("S", SIZES)
def test_pre_kernel_takes_both_forms_over_the_list(engines, S):
    """Which form a geometry takes is decided when its tables are made: both sides of the threshold are in the list."""
    forms = {(w, h): engines[S].op_classify_pre_batch(_frames(1, w, h, 1), w, h)[1] for w, h in shapes(S)}
    assert set(forms.values()) == {0, 1}, forms
    assert forms[(2000, 9)] == 1 and forms[(640, 480)] == 0 and forms[(9, 1500)] == 0, forms


@pytest.mark.parametrize("S", SIZES)
def test_tables_are_rebuilt_per_geometry(engines, oracle, S):
    """The same geometry twice with others in between - among them the transposed one and one that shares the width only."""
    for w, h in ((300, 20), (20, 300), (300, 21), (300, 20), (2000, 9), (300, 20)):
        _check_pre(engines[S], oracle, S, w, h, seed=5)


def _post_patterns(g, n):
    """name -> classes uint8 [2n][g*g], every one terminating in STRICT. 'checker': single cells of all four classes, every cell
    different from its four neighbours, shifted per tile; 'one_class': a whole frame one class (robots or background: a tile of
    balls does not terminate); 'per_tile': one class per tile - the stitch seam shows."""
    y, x = np.divmod(np.arange(g * g), g)
    out = {
        "checker": np.stack([((x + 2 * y + t) % 4).astype(np.uint8) for t in range(2 * n)]),
        "one_class": np.stack([np.full(g * g, (0, 1, 2, 1)[(t // 2) % 4], np.uint8) for t in range(2 * n)]),
        "per_tile": np.stack([np.full(g * g, ((1, 2), (2, 0), (0, 1), (2, 1))[(t // 2) % 4][t % 2], np.uint8) for t in range(2 * n)]),
    }
    for name, cl in out.items():
        assert not any(R.linear_pairs(c, g) for c in cl), name
    assert set(np.unique(out["checker"]).tolist()) == {0, 1, 2, 3}
    return out


@pytest.mark.parametrize("S,k", PARAMS, ids=IDS)
def test_post_kernel(engines, oracle, S, k):
    import yolact_amd as ya
    w, h = shapes(S)[k]
    eng, g, nch = engines[S], S // 8, 81
    for n in (1, 4):
        for name, cl in _post_patterns(g, n).items():
            cells = np.stack([R.paint(c, nch) for c in cl])
            for mode in (ya.COMPAT_SANE, ya.COMPAT_STRICT):
                got, div = eng.op_classify_post_batch(cells, w, h, mode)
                assert got.shape == (n, h, w) and not div.any()
                for b in range(n):
                    rc, want = oracle.classify_post(cells[2 * b:2 * b + 2], S, nch, mode, w, h)
                    assert rc == 0 and np.array_equal(got[b].reshape(-1), want), (S, w, h, n, name, mode, b)
                if name == "checker" and mode == ya.COMPAT_SANE and w >= 2 * S and h >= S:
                    assert {0, 1, 2, 3} <= set(np.unique(got >> 24).tolist())
                    assert {0, 1, 0xFF} <= set(np.unique((got >> 16) & 0xFF).tolist())   # ball ids beside the no-id byte
