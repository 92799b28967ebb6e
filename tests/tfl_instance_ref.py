"""The TFLite instance frame of a camera frame restated (DESIGN.md §11 "TFLite instance frames"): numpy, integers but for the two
float32 comparisons of the definition (score >= min_score, score against score). classify cuts a camera frame into two tiles, so a
frame is painted from two detection lists: tile 0 is the left half, tile 1 the right.

The definition is followed literally: every eligible detection gets its stitched mask [hp][2 wp] - its own mask in its tile's
half, zeros in the other - the detections are sorted by (score descending, tile, rank within the tile), and they are painted in that
order with instance_ref.upsample, the first to claim a pixel keeping it. Nothing here knows where the seam is."""
import numpy as np

import instance_ref as IR


def instance_frames(masks0, cls0, sc0, masks1, cls1, sc1, W, H, class_map=None, min_score=0.0, num_classes=81):
    """frame uint32 [H][W] of class << 24 | id << 16 and the table int32 [m][5] = (tile, rank within the tile, output class, id,
    pixels won) in frame order. masks_t uint8 [n_t][hp][wp], cls_t, sc_t [n_t]: tile t's detections as the tail returns them."""
    cm = IR.default_class_map(num_classes) if class_map is None else np.asarray(class_map, np.uint8)
    tiles = ((np.asarray(masks0), cls0, sc0), (np.asarray(masks1), cls1, sc1))
    hp, wp = next((m.shape[1:] for m, _, _ in tiles if m.ndim == 3 and m.shape[0] > 0), (1, 1))
    entries = []
    for t, (m, cls, sc) in enumerate(tiles):
        for r, (k, s) in enumerate(zip(np.asarray(cls, np.int64).reshape(-1).tolist(), np.asarray(sc, np.float32).reshape(-1))):
            c = int(cm[k])
            if c == 0 or not bool(s >= np.float32(min_score)):
                continue                                  # not eligible: no rank, no id, paints nothing, occludes nothing
            stitched = np.zeros((hp, 2 * wp), np.uint8)
            stitched[:, t * wp:(t + 1) * wp] = m[r]
            entries.append((s, t, r, c, stitched))
    # score descending; a tie goes to tile 0 before tile 1, then to the smaller rank (float32 compares: -0.0 ties with 0.0)
    order = sorted(range(len(entries)), key=lambda i: (-float(entries[i][0]), entries[i][1], entries[i][2]))
    frame = np.zeros((H, W), np.uint32)
    free = np.ones((H, W), bool)
    seen, table = {}, []
    for i in order:
        _, t, r, c, stitched = entries[i]
        ident = seen.get(c, 0)
        seen[c] = ident + 1
        won = IR.upsample(stitched, W, H) & free
        frame[won] = (c << 24) | (ident << 16)
        free &= ~won
        table.append((t, r, c, ident, int(won.sum())))
    return frame, np.array(table, np.int32).reshape(-1, 5)
