"""Deterministic edge cases for the reference-compat path (csrc/refpath.hip, cells_f32 in elementwise.hip). Not a
test: builders of inputs for tests/test_refpath_cases.py (which proves on the CPU, with the oracle and tests/refpath_ref.py, that
every case does what it claims) and for tests/test_gpu_refpath_edges.py (which runs them on the device, bit for bit against the
oracle). numpy only.

A postprocess case (families a - d) is a dict with
    grid, C              cells per side (input size = 8 grid) and logits per cell
    tiles                float32 [n][grid^2][C]: the cell tensors
    calls                [(tile indices, mode)]: the yh_postprocess_cells calls to make, in order
plus what the case claims about itself (classes, index, pairs, ...). paint() gives a cell the class it is told: logit k = 1 for
class k in 1 .. 3, every other of the first four -1; logits 4 .. C-1 rotate +inf, NaN, 3e38 (yolact.rs:110 takes four and ignores them).

Families e (triangle resize), f (classify frames through the engine) and g (classify through a painted TFLite model) are tables
of shapes and contents with their builders; see the comments there."""
import numpy as np

import tfl_builder as B

F32 = np.float32
STRICT, SANE = 0, 1
GRIDS = (8, 9, 28, 64)                 # input sizes 64, 72 (odd grid), 224, 512 (= YH_GRID_MAX cells)
CLASSES_OF = {8: 5, 9: 81, 28: 81, 64: 81}
JUNK = (np.inf, np.nan, 3e38)


def paint(classes, C, junk=True):
    """Cells [nc][C] whose gated argmax is `classes`."""
    cl = np.asarray(classes).reshape(-1)
    cells = np.full((cl.size, C), -1.0, np.float32)
    for k in (1, 2, 3):
        cells[cl == k, k] = 1.0
    fill_junk(cells, junk)
    return cells


def fill_junk(cells, junk=True):
    n, C = cells.shape
    for j in range(4, C):
        cells[:, j] = np.array(JUNK, np.float32)[(np.arange(n) + j) % 3] if junk else 50.0


def pair_calls(n, mode):
    """Two tiles per call (one in the last if n is odd)."""
    return [(list(range(i, min(i + 2, n))), mode) for i in range(0, n, 2)]


def both_modes(n):
    """SANE two tiles at a time, so ids are compared; STRICT a tile at a time, so each tile's divergence is pinned by itself."""
    return pair_calls(n, SANE) + [([i], STRICT) for i in range(n)]


# ---------------------------------------------------------------------------------------------- (a) argmax lattice
LATTICE = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, np.float32(1e-45), 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), np.inf],
                   np.float32)


def lattice_patterns():
    """All 9^4 4-tuples over LATTICE, float32 [6561][4], in an order that spreads each value over the whole range (a stride
    coprime to 6561 - so neighbouring cells differ in every logit and no tile holds only one leading value)."""
    idx = (np.arange(6561) * 2755) % 6561              # gcd(2755, 3) = 1
    digits = np.stack([(idx // 9 ** k) % 9 for k in (3, 2, 1, 0)], 1)
    return LATTICE[digits], idx


def a_lattice(grid, C):
    nc = grid * grid
    n_tiles = {28: 10, 64: 2}[grid]                   # five two-tile calls at grid 28, one at grid 64
    pats, idx = lattice_patterns()
    cells = np.full((n_tiles * nc, C), -1.0, np.float32)   # cells past the 6561st: padding, class 0
    cells[:6561, :4] = pats
    fill_junk(cells)
    index = np.full(n_tiles * nc, -1, np.int64)
    index[:6561] = idx
    return dict(grid=grid, C=C, tiles=cells.reshape(n_tiles, nc, C), index=index.reshape(n_tiles, nc), calls=both_modes(n_tiles))


# ---------------------------------------------------------------------------------------------- (b) SANE shapes
def spiral(g):
    """A one-cell-wide clockwise spiral from cell 0 inwards with one free cell between its arms; returns the path (cells in order)."""
    on = np.zeros((g, g), bool)
    y, x, d = 0, 0, 0
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))
    on[0, 0] = True
    path = [0]

    def free(yy, xx):
        return 0 <= yy < g and 0 <= xx < g and not on[yy, xx]

    def can(yy, xx, dd):
        dy, dx = steps[dd]
        ny, nx = yy + dy, xx + dx
        if not free(ny, nx):
            return False
        # the cell after the next one, and the next one's side neighbours, must not touch an earlier arm
        for qy, qx in ((ny + dy, nx + dx), (ny + dx, nx - dy), (ny - dx, nx + dy)):
            if 0 <= qy < g and 0 <= qx < g and on[qy, qx] and (qy, qx) != (yy, xx):
                return False
        return True

    while True:
        if not can(y, x, d):
            d = (d + 1) % 4
            if not can(y, x, d):
                break
        y, x = y + steps[d][0], x + steps[d][1]
        on[y, x] = True
        path.append(y * g + x)
    return path


def _cls(g, cells3):
    cl = np.zeros(g * g, np.uint8)
    cl[np.asarray(list(cells3), np.int64)] = 3
    return cl


def b_spiral_in(g):
    """Root (cell 0) at the outer end: the label travels the whole path to the centre."""
    p = spiral(g)
    return dict(classes=_cls(g, p), path=p)


def b_spiral_out(g):
    """The same spiral turned by 180 degrees: its outer end is the LAST cell of the tile, the path runs left along the bottom row,
    up the first column and right along the top row. (The root of a spiral cannot lie at its centre: the smallest index of a
    component is in its top row, which belongs to the outermost ring.) The root, cell 0, is 2 (grid - 1) cells from the outer end:
    the label travels that stretch downwards and rightwards back to the end, against every arm's direction, and the rest inwards."""
    p = [g * g - 1 - c for c in spiral(g)]
    return dict(classes=_cls(g, p), path=p)


def b_serpentine(g):
    """Every even row, joined at alternating ends: one component over the whole tile, its path about nc / 2 + grid / 2 long."""
    cl = np.zeros((g, g), np.uint8)
    cl[0::2] = 3
    for k, y in enumerate(range(1, g - 1, 2)):
        cl[y, g - 1 if k % 2 == 0 else 0] = 3
    return dict(classes=cl.reshape(-1))


def b_u(g):
    """Right arm from row 0, left arm from row 1, joined along the bottom row: the root is the top of the RIGHT arm, and the left
    arm is reached only leftwards along the bottom and then upwards - against raster order."""
    cl = np.zeros((g, g), np.uint8)
    cl[:, g - 1] = 3
    cl[1:, 0] = 3
    cl[g - 1, :] = 3
    return dict(classes=cl.reshape(-1))


def b_comb(g):
    """A spine along the bottom row with a tooth on every even column; only the last tooth reaches row 0, the others stop at row 1:
    the root is the top of the last tooth, every other tooth is reached leftwards along the spine and upwards."""
    cl = np.zeros((g, g), np.uint8)
    cl[g - 1, :] = 3
    last = (g - 1) // 2 * 2
    for x in range(0, g, 2):
        cl[(0 if x == last else 1):, x] = 3
    return dict(classes=cl.reshape(-1))


def b_all3(g):
    return dict(classes=np.full(g * g, 3, np.uint8))


def checker(g):
    y, x = np.divmod(np.arange(g * g), g)
    return np.where((x + y) % 2 == 0, 3, 0).astype(np.uint8)


def b_checker(g):
    """(grid^2 + 1) // 2 one-cell components: ids 0 .. 126, then 127 for all the rest (392 at grid 28, 2048 at grid 64)."""
    return dict(classes=checker(g))


def _balls(g, n):
    cl = np.zeros(g * g, np.uint8)
    cl[np.nonzero(checker(g))[0][:n]] = 3
    return dict(classes=cl, n=n)


def b_balls127(g):
    return _balls(g, 127)


def b_balls128(g):
    return _balls(g, 128)


def b_balls129(g):
    return _balls(g, 129)


def b_wrap_balls(g):
    """Balls at (x, y) = (grid - 1, y) and (0, y + 1): linear neighbours, not 4-connected - two components in SANE."""
    y = g // 2
    return dict(classes=_cls(g, [y * g + g - 1, (y + 1) * g]))


def b_separated(g):
    """Class-3 columns on the even x, class 1 and 2 alternating down the odd columns: components separated by robots only."""
    cl = np.zeros((g, g), np.uint8)
    cl[:, 0::2] = 3
    cl[0::2, 1::2] = 1
    cl[1::2, 1::2] = 2
    return dict(classes=cl.reshape(-1))


def b_corners(g):
    return dict(classes=_cls(g, [0, g - 1, g * g - g, g * g - 1]))


# ---------------------------------------------------------------------------------------------- (c) STRICT predicate
def c_wrap_pair(g):
    y = g // 2 - 1
    return dict(classes=_cls(g, [y * g + g - 1, (y + 1) * g]), pairs=1)


def c_vertical_pair(g):
    """In the last two rows: `c + grid < nc` holds for the upper cell only just."""
    x = g - 2
    return dict(classes=_cls(g, [(g - 2) * g + x, (g - 1) * g + x]), pairs=1)


def c_pair_first(g):
    return dict(classes=_cls(g, [0, 1]), pairs=1)


def c_pair_last(g):
    return dict(classes=_cls(g, [g * g - 2, g * g - 1]), pairs=1)


def c_two_apart(g):
    """Two apart in a row, two apart in a column, and two apart across the row wrap."""
    y = g // 2
    return dict(classes=_cls(g, [y * g + 1, y * g + 3, (y + 2) * g + 1, 2 * g - 1, 2 * g + 1]), pairs=0)


def c_diagonal(g):
    c = (g // 2) * g + g // 2
    return dict(classes=_cls(g, [c, c + g + 1, c + 2 * g]), pairs=0)         # down-right, then down-left of that


def c_wrap_miss(g):
    y = g // 2 - 1
    return dict(classes=_cls(g, [y * g + g - 1, (y + 1) * g + 1]), pairs=0)


def c_first_last(g):
    return dict(classes=_cls(g, [0, g * g - 1]), pairs=0)


def c_checker(g):
    """On an even grid the checkerboard's only linear neighbours are (grid - 1, y), (0, y + 1) for the odd y: it diverges through
    the row wrap alone. On the odd grid 9 it has none."""
    return dict(classes=checker(g), pairs=g // 2 - 1 if g % 2 == 0 else 0)


def linear_pairs(classes, g):
    """Unordered pairs of class-3 cells that are neighbours in linear index space (c, c + 1) and (c, c + grid): the scan of
    yolact.rs:61-76 seen from the lower cell; (c, c + 1) includes the row wrap."""
    cl = np.asarray(classes).reshape(-1)
    nc = cl.size
    return [(c, q) for c in range(nc) if cl[c] == 3 for q in (c + 1, c + g) if q < nc and cl[q] == 3]


# ---------------------------------------------------------------------------------------------- (d) call sequences
def d_sequence(g, C):
    """Stale state across calls (diverged and codes persist in the handle): two tiles of which only tile 1 diverges; one clean
    tile; two clean tiles with fewer balls than the first call; then the same three calls in the other mode, and call 3 again in
    STRICT after the SANE ones have left ids in the code buffer."""
    many = np.nonzero(checker(g))[0][1::2][: g]                       # isolated balls, no row-wrap neighbours (every other one)
    t0 = _cls(g, many)
    t1 = _cls(g, list(many) + [int(many[-1]) + 1])                    # ... and one adjacent pair
    t2 = _cls(g, many[: g // 2])
    t3 = _cls(g, many[:2])
    t4 = _cls(g, many[:1])
    tiles = np.stack([paint(t, C) for t in (t0, t1, t2, t3, t4)])
    calls = []
    for mode in (STRICT, SANE):
        calls += [([0, 1], mode), ([2], mode), ([3, 4], mode)]
    calls.append(([3, 4], STRICT))
    return dict(grid=g, C=C, tiles=tiles, classes=[t0, t1, t2, t3, t4], calls=calls)


# ---------------------------------------------------------------------------------------------- the postprocess case table
B_SHAPES = dict(spiral_in=b_spiral_in, spiral_out=b_spiral_out, serpentine=b_serpentine, u=b_u, comb=b_comb, all3=b_all3,
                checker=b_checker, balls127=b_balls127, balls128=b_balls128, balls129=b_balls129, wrap_balls=b_wrap_balls,
                separated=b_separated, corners=b_corners)
C_SHAPES = dict(wrap_pair=c_wrap_pair, vertical_pair=c_vertical_pair, pair_first=c_pair_first, pair_last=c_pair_last,
                two_apart=c_two_apart, diagonal=c_diagonal, wrap_miss=c_wrap_miss, first_last=c_first_last, checker=c_checker)
BIG = ("balls127", "balls128", "balls129")     # need 129 isolated cells: at most 32 fit grid 8 and 41 grid 9

POST_CASES = {}                                # id -> (builder, grid, C)


def _shape_case(fn, g, C):
    def build():
        case = fn(g)
        case.update(grid=g, C=C, tiles=paint(case["classes"], C)[None], calls=both_modes(1))
        return case
    return build


for _C in (81, 5):
    POST_CASES[f"a_lattice_g28_c{_C}"] = (lambda C=_C: a_lattice(28, C), 28, _C)
POST_CASES["a_lattice_g64_c81"] = (lambda: a_lattice(64, 81), 64, 81)
for _g in GRIDS:
    for _name, _fn in B_SHAPES.items():
        if not (_name in BIG and _g < 28):
            POST_CASES[f"b_{_name}_g{_g}"] = (_shape_case(_fn, _g, CLASSES_OF[_g]), _g, CLASSES_OF[_g])
    for _name, _fn in C_SHAPES.items():
        POST_CASES[f"c_{_name}_g{_g}"] = (_shape_case(_fn, _g, CLASSES_OF[_g]), _g, CLASSES_OF[_g])
for _g, _C in ((8, 5), (9, 81), (28, 5), (28, 81), (64, 81)):
    POST_CASES[f"d_sequence_g{_g}_c{_C}"] = (lambda g=_g, C=_C: d_sequence(g, C), _g, _C)
POST_IDS = list(POST_CASES)


def build_post(cid):
    case = POST_CASES[cid][0]()
    case["id"] = cid
    return case


# ---------------------------------------------------------------------------------------------- (e) triangle resize
RESIZE_SHAPES = [((1, 1), (5, 3)), ((1, 7), (9, 1)), ((2, 3), (640, 1)), ((1280, 1), (1, 1)), ((640, 480), (1, 1)), ((3, 3), (4, 3)),
                 ((448, 224), (224, 112)), ((224, 112), (448, 224)), ((97, 89), (101, 83))]        # (w, h) -> (w, h)
RESIZE_CONTENTS = ("zero", "full", "channels", "checker_0_255", "checker_0_1", "checker_254_255", "ramp_h", "ramp_v")
RESIZE_IDS = [f"e_resize_{sw}x{sh}_to_{dw}x{dh}" for (sw, sh), (dw, dh) in RESIZE_SHAPES]


def resize_content(name, w, h):
    """uint8 [h][w][3]."""
    y, x = np.mgrid[0:h, 0:w]
    if name == "zero":
        v = np.zeros((h, w), np.int64)
    elif name == "full":
        v = np.full((h, w), 255, np.int64)
    elif name == "channels":
        return np.broadcast_to(np.array([0, 128, 255], np.uint8), (h, w, 3)).copy()
    elif name.startswith("checker_"):
        lo, hi = (int(s) for s in name.split("_")[1:])
        v = np.where((x + y) % 2 == 0, lo, hi)
    elif name == "ramp_h":
        v = (x * 255) // max(w - 1, 1)
    elif name == "ramp_v":
        v = (y * 255) // max(h - 1, 1)
    else:
        raise KeyError(name)
    return np.repeat(v.astype(np.uint8)[:, :, None], 3, axis=2)


# ---------------------------------------------------------------------------------------------- (f) classify frames, engine path
FRAME_SIZES = [(448, 224), (1, 1), (3, 2), (447, 225), (200, 600), (1280, 720)]     # 2S x S is the identity at S = 224
FRAME_CONTENTS = ("frc_balls", "red_robot", "checker")
FRAME_IDS = [f"f_classify_{w}x{h}_{c}" for w, h in FRAME_SIZES for c in FRAME_CONTENTS]


def frame_rgb(content, w, h, golden_dir):
    """uint8 [h][w][3]: a golden photograph resized on the CPU, or a 0 / 255 checker."""
    if content == "checker":
        return resize_content("checker_0_255", w, h)
    import os
    from PIL import Image
    return np.asarray(Image.open(os.path.join(golden_dir, content + ".png")).convert("RGB").resize((w, h), Image.BILINEAR))


# ---------------------------------------------------------------------------------------------- (g) the painter
PAINT_S, PAINT_C = 64, 5
PAINT_RGB = np.array([[0, 0, 0], [255, 0, 0], [0, 0, 255], [0, 255, 0]], np.uint8)     # class 0 black, 1 red, 2 blue, 3 green
PAINT_SCALE, PAINT_ZP = 204.0 / 8192.0, 128


def painter(image_axis=False):
    """A TFLite model whose output 4 a painted frame decides: one uint8 CONV_2D, 8x8, stride 8, 3 -> 5 channels over a [1,64,64,3]
    input (scale 1/128, zero point 0). Weights (scale 1/64, zero point 128) are +1 on a class's own colour channel and -1 on the
    other two (class 0: -1 on all three); bias -4080. A cell of pure colour accumulates 64 * 255 = 16320 on its own class: +12240
    there, -20400 on the others, -4080 on black; the output scale 204/8192 makes those +60, -100 and -20 steps. Channel 4 is +1
    on all three channels with bias +4080: +100 steps on a colour, +20 on black - the largest logit of every cell, to be ignored. Outputs 0 .. 3 are four 3 -> 1 convolutions of the same extent.
    image_axis=True makes output 0 a CONCATENATION of two of them along axis 0: the executor then runs one image per invoke."""
    m = B.Model()
    x = m.add(B.T("input", (1, PAINT_S, PAINT_S, 3), "u8", scale=1 / 128, zp=0))
    w = np.full((PAINT_C, 8, 8, 3), 127, np.uint8)                     # -1
    for k, ch in ((1, 0), (2, 2), (3, 1)):
        w[k, :, :, ch] = 129                                           # +1
    w[4] = 129
    g = PAINT_S // 8

    def conv(name, wdata, bias, co, so, zo):
        wt = m.add(B.T(name + "_w", (co, 8, 8, 3), "u8", data=wdata, scale=1 / 64, zp=128))
        bt = m.add(B.T(name + "_b", (co,), "i32", data=np.broadcast_to(np.asarray(bias, np.int32), (co,)), scale=1 / 8192, zp=0))
        y = m.add(B.T(name, (1, g, g, co), "u8", scale=so, zp=zo))
        m.ops.append(B.Op("CONV_2D", [x, wt, bt], [y], padding=1, stride_w=8, stride_h=8, act=0))
        return y
    small = [conv(f"small{i}", np.full((1, 8, 8, 3), 128 + i, np.uint8), 100 * i, 1, 1.0, 10 * i) for i in range(4)]
    if image_axis:
        cat = m.add(B.T("joined", (2, g, g, 1), "u8", scale=1.0, zp=0))
        m.ops.append(B.Op("CONCATENATION", [small[0], small[0]], [cat], axis=0))
        small[0] = cat
    cells = conv("cells", w, [-4080, -4080, -4080, -4080, 4080], PAINT_C, PAINT_SCALE, PAINT_ZP)
    m.inputs = [x]
    m.outputs = small + [cells]
    return m


def painted_frame(classes2, w=2 * PAINT_S, h=PAINT_S):
    """Packed uint32 frame [h * w] showing two tiles' classes (each [64]) as 8x8 blocks of PAINT_RGB, tile 0 on the left; for a
    size other than 128x64 the painted image is enlarged / reduced by nearest sampling (the cells are then no longer pure)."""
    g = PAINT_S // 8
    img = np.concatenate([np.asarray(c).reshape(g, g) for c in classes2], axis=1)
    img = np.repeat(np.repeat(img, 8, axis=0), 8, axis=1)
    yy = (np.arange(h) * PAINT_S) // h
    xx = (np.arange(w) * 2 * PAINT_S) // w
    rgb = PAINT_RGB[img[yy][:, xx]].astype(np.uint32)
    return ((rgb[..., 0] << 24) | (rgb[..., 1] << 16) | (rgb[..., 2] << 8)).reshape(-1)


# patterns for the painter: the grid-8 members of (b) and (c), two tiles per frame; robots share the second tile's free cells
PAINT_PATTERNS = {}
for _name, _fn in list(B_SHAPES.items()) + [("c_" + n, f) for n, f in C_SHAPES.items()]:
    if _name not in BIG:
        PAINT_PATTERNS[_name] = _fn
PAINT_IDS = [f"g_painter_{n}" for n in PAINT_PATTERNS]
PAINT_RESIZED = ("comb", [(160, 120), (37, 91)])          # one SANE pattern through a real resize back


def paint_other():
    """The second tile of every painted frame: robots of both colours and two balls that no scan joins - clean in both modes."""
    cl = np.zeros((8, 8), np.uint8)
    cl[0::2, 1::2] = 1
    cl[1::2, 0::2] = 2
    cl[3, 3] = cl[5, 6] = 3
    return cl.reshape(-1)


def paint_tiles(name):
    """Two tiles' classes for pattern `name`: the shape itself on the left, paint_other() on the right."""
    return [PAINT_PATTERNS[name](8)["classes"], paint_other()]


def painter_cells(oracle, model, tiles):
    """What yolact.rs:169-177 makes of the painter's output 4 on two uint8 tiles [2][64][64][3], by the numpy TFLite oracle:
    (float32 cells [2][64][C], the raw uint8 codes [2][64][C])."""
    import tfl_oracle as TO
    q = np.stack([TO.run_model(model, {model.inputs[0]: tiles[t:t + 1]})[model.outputs[4]].reshape(-1, PAINT_C) for t in range(2)])
    return oracle.dequant_u8(q.reshape(-1), PAINT_SCALE, PAINT_ZP).reshape(q.shape), q


def post_reference(oracle, case, idx, mode):
    """The oracle's answer for one yh_postprocess_cells call on tiles `idx`: (diverges, code images [len(idx)][S][S])."""
    S = case["grid"] * 8
    res = [oracle.postprocess_tile(case["tiles"][t], case["grid"], case["C"], mode) for t in idx]
    return any(rc for rc, _ in res), np.stack([img.reshape(S, S) for _, img in res])


CASE_IDS = POST_IDS + RESIZE_IDS + FRAME_IDS + PAINT_IDS
