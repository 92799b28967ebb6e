"""CPU: the restatement of the TFLite instance frame (tests/tfl_instance_ref.py; DESIGN.md §11 "TFLite instance frames") checked
against tests/instance_ref.py where the two must agree, the seam facts the definition implies, and two wrong readings of the
definition that the cases here tell apart from the right one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instance_ref as IR
import tfl_instance_ref as TR

SHAPES = [(32, 32, 96, 64), (5, 7, 7, 5), (3, 5, 33, 9), (1, 1, 2, 1), (2, 2, 5, 3)]   # (hp, wp, W, H)
CM = np.array([1, 2, 3, 0, 1, 2], np.uint8)


def _empty(hp, wp):
    return np.zeros((0, hp, wp), np.uint8), np.zeros(0, np.int64), np.zeros(0, np.float32)


@pytest.mark.parametrize("hp,wp,W,H", SHAPES)
def test_tile_1_empty_is_the_engines_frame_on_padded_masks(hp, wp, W, H):
    rng = np.random.default_rng(hp * 100 + wp)
    n = 9
    masks = IR.disc_masks(rng, n, hp, wp) if min(hp, wp) > 2 else rng.integers(0, 2, (n, hp, wp)).astype(np.uint8)
    cls = rng.integers(0, 6, n)
    sc = np.sort(rng.random(n).astype(np.float32))[::-1].copy()
    frame, table = TR.instance_frames(masks, cls, sc, *_empty(hp, wp), W, H, CM, 0.2, 7)
    padded = np.concatenate([masks, np.zeros_like(masks)], axis=2)
    wf, wt = IR.instance_frame(padded, cls, sc, W, H, CM, 0.2, 7)
    assert np.array_equal(frame, wf)
    assert np.array_equal(table[:, 0], np.zeros(len(table), np.int32)) and np.array_equal(table[:, 1:], wt)
    # ... and with tile 0 empty, the same detections in tile 1 live in the right half
    frame1, table1 = TR.instance_frames(*_empty(hp, wp), masks, cls, sc, W, H, CM, 0.2, 7)
    padded1 = np.concatenate([np.zeros_like(masks), masks], axis=2)
    wf1, wt1 = IR.instance_frame(padded1, cls, sc, W, H, CM, 0.2, 7)
    assert np.array_equal(frame1, wf1) and np.array_equal(table1[:, 1:], wt1) and (table1[:, 0] == 1).all()


def _seam(hp, wp, W, H):
    """Columns owned by tile 0, by tile 1 and by neither under two full masks of different classes."""
    full = np.ones((1, hp, wp), np.uint8)
    frame, table = TR.instance_frames(full, [0], [0.9], full, [1], [0.8], W, H, CM, 0.0, 7)
    assert len(table) == 2 and table[:, 4].sum() == int((frame != 0).sum())
    cols0, cols1 = (frame == 1 << 24).all(axis=0), (frame == 2 << 24).all(axis=0)
    none = (frame == 0).all(axis=0)
    assert (cols0 | cols1 | none).all()                     # every column is one thing from top to bottom
    return np.flatnonzero(cols0), np.flatnonzero(cols1), np.flatnonzero(none)


def test_seam_facts():
    c0, c1, none = _seam(32, 32, 96, 64)
    assert c0.tolist() == list(range(48)) and c1.tolist() == list(range(48, 96)) and none.size == 0
    c0, c1, none = _seam(5, 7, 7, 5)
    assert c0.tolist() == [0, 1, 2] and c1.tolist() == [4, 5, 6] and none.tolist() == [3]
    c0, c1, none = _seam(3, 5, 33, 9)
    assert c0.tolist() == list(range(16)) and c1.tolist() == list(range(17, 33)) and none.tolist() == [16]
    c0, c1, none = _seam(1, 1, 2, 1)
    assert c0.tolist() == [0] and c1.tolist() == [1] and none.size == 0
    c0, c1, none = _seam(2, 2, 5, 3)
    assert c0.tolist() == [0, 1] and c1.tolist() == [3, 4] and none.tolist() == [2]


@pytest.mark.parametrize("hp,wp,W,H", SHAPES + [(32, 32, 640, 480)])
def test_no_pixel_is_on_for_both_tiles(hp, wp, W, H):
    """The seam weights: tile 0's two taps sum to (2W - fx) 2H and tile 1's to fx 2H, so at most one side passes 2WH; where fx = W
    neither does. Checked on the stitched full masks themselves, and the seam columns are counted at 640 x 480."""
    left, right = np.zeros((hp, 2 * wp), np.uint8), np.zeros((hp, 2 * wp), np.uint8)
    left[:, :wp], right[:, wp:] = 1, 1
    a, b = IR.upsample(left, W, H), IR.upsample(right, W, H)
    assert not (a & b).any()
    gap = ~(a | b)
    assert gap.any() == (W % 2 == 1) and (not gap.any() or (gap.all(axis=0).sum() == 1 and gap[:, W // 2].all()))
    if (W, H) == (640, 480):
        _, _, fx = IR.axis_taps(W, 2 * wp)
        u0, u1, _ = IR.axis_taps(W, 2 * wp)
        assert int(((u0 == wp - 1) & (u1 == wp)).sum()) == 10 and not gap.any()


def test_ids_count_across_tiles():
    hp = wp = 4
    m = np.zeros((2, hp, wp), np.uint8)
    m[0, :2], m[1, 2:] = 1, 1                                 # two disjoint bands per tile
    # one output class everywhere; frame order by score: t0r0 (.9), t1r0 (.8), t0r1 (.7), t1r1 (.6)
    frame, table = TR.instance_frames(m, [0, 4], [0.9, 0.7], m, [4, 0], [0.8, 0.6], 16, 8, CM, 0.0, 7)
    assert table[:, :4].tolist() == [[0, 0, 1, 0], [1, 0, 1, 1], [0, 1, 1, 2], [1, 1, 1, 3]]
    assert sorted(np.unique(frame).tolist()) == [(1 << 24) | (i << 16) for i in range(4)]
    # the wrong reading "ids counted per tile" would give 0, 0, 1, 1: two pairs of instances with one id
    per_tile = [IR.ranks(c, s, CM, 0.0, 7) for c, s in (([0, 4], [0.9, 0.7]), ([4, 0], [0.8, 0.6]))]
    assert [i for _, _, i in per_tile[0]] + [i for _, _, i in per_tile[1]] == [0, 1, 0, 1]
    assert table[:, 3].tolist() != [0, 0, 1, 1]


def test_a_score_tie_across_tiles_goes_to_tile_0():
    hp, wp, W, H = 1, 1, 2, 1
    full = np.ones((1, hp, wp), np.uint8)
    _, table = TR.instance_frames(full, [0], [0.5], full, [0], [0.5], W, H, CM, 0.0, 7)
    assert table[:, :4].tolist() == [[0, 0, 1, 0], [1, 0, 1, 1]]
    # ... and within the tie the smaller rank first; -0.0 ties with 0.0
    two = np.ones((2, hp, wp), np.uint8)
    _, table = TR.instance_frames(two, [0, 1], [0.0, -0.0], two, [0, 1], [0.0, 0.0], W, H, CM, -1.0, 7)
    assert table[:, :2].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]


def test_concatenation_without_the_merge_is_rejected():
    """Tile 1's best detection outscores tile 0's second: concatenated lists would paint tile 0's second first and give it the
    smaller id. Both own pixels of one class, so the frames differ."""
    hp = wp = 2
    m = np.ones((2, hp, wp), np.uint8)
    m[1] = 0
    m[1, 1] = 1
    args = (m, [0, 0], [0.9, 0.3], m, [0, 0], [0.6, 0.5])
    frame, table = TR.instance_frames(*args, 8, 4, CM, 0.0, 7)
    assert table[:, :2].tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    stitched = []
    for t in (0, 1):
        for r in (0, 1):
            s = np.zeros((hp, 2 * wp), np.uint8)
            s[:, t * wp:(t + 1) * wp] = m[r]
            stitched.append(s)
    wrong, _ = IR.instance_frame(np.stack(stitched), [0] * 4, [0.9, 0.3, 0.6, 0.5], 8, 4, CM, 0.0, 7)
    assert not np.array_equal(frame, wrong)
    merged, mt = IR.instance_frame(np.stack([stitched[i] for i in (0, 2, 3, 1)]), [0] * 4, [0.9, 0.6, 0.5, 0.3], 8, 4, CM, 0.0, 7)
    assert np.array_equal(frame, merged) and np.array_equal(table[:, 2:], mt[:, 1:])


def test_min_score_and_class_map_decide_eligibility():
    hp, wp = 2, 3
    m = np.ones((2, hp, wp), np.uint8)
    s = np.float32(0.25)
    up = np.nextafter(s, np.float32(1.0))
    _, on = TR.instance_frames(m, [0, 3], [0.5, s], m, [1, 1], [s, 0.1], 6, 2, CM, float(s), 7)
    assert on[:, :3].tolist() == [[0, 0, 1], [1, 0, 2]]             # class 3 maps to 0; 0.1 is below
    _, above = TR.instance_frames(m, [0, 3], [0.5, s], m, [1, 1], [s, 0.1], 6, 2, CM, float(up), 7)
    assert above[:, :3].tolist() == [[0, 0, 1]]
