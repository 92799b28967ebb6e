"""The reference's own pre- and post-processing (src/yolact.rs:52-131, :192-234, and the `sample` passes of image 0.24's
imageops::resize), restated a second time in plain Python / numpy for tests/test_refpath_cases.py: an opinion independent of
oracle/orc_ref.c, so that the oracle's own edge behaviour (NaN, the i8 id, the pop budget, exact halves) is pinned by something
other than itself. Nothing here is fast and nothing here is shared with the oracle or the kernels.

  gated_argmax   yolact.rs:108-118 as a literal loop over np.float32 scalars (and three deliberately wrong variants)
  terrible_id    yolact.rs:52-88 literally, usize wrap included, with a pop cap that answers "diverges"
  sane_ids       4-connected components of the class-3 cells by union-find; ids in raster order of each component's first cell,
                 saturating at 127 (the oracle does a depth-first fill, the kernel a min-label propagation)
  pack / upsample / stitch / postprocess_tile     yolact.rs:127-128, :219-220
  resize         vertical then horizontal Triangle pass in np.float32, one rounding per operation, in the order
                 weight / sum, sample * weight, accumulator + product; round= picks f32::round (half away) or the wrong half-even"""
import numpy as np

F32 = np.float32
U64 = 1 << 64


# ---------------------------------------------------------------------------------------------- gated argmax
def _flush(v):
    """A subnormal as a flush-to-zero compare sees it."""
    return F32(0.0) if (v != 0 and abs(float(v)) < float(np.finfo(np.float32).tiny)) else v


def gated_argmax(cells, variant=None):
    """cells [n][C] -> classes uint8 [n]. variant None is yolact.rs:108-118; "flush" compares with subnormals flushed to zero,
    "ge" uses >= in place of >, "nanmax" keeps the running maximum with a NaN-propagating max: the three ways to be wrong."""
    cells = np.asarray(cells, np.float32)
    out = np.zeros(len(cells), np.uint8)
    for n, row in enumerate(cells):
        mx = F32(0.0)
        hit = []
        for i in range(4):
            v = F32(row[i])
            if variant == "flush":
                h = bool(_flush(v) > _flush(mx))
            elif variant == "ge":
                h = bool(v >= mx)
            else:
                h = bool(v > mx)
            if variant == "nanmax":
                with np.errstate(invalid="ignore"):
                    mx = np.maximum(mx, v)       # NaN in, NaN kept: every later compare is false
            elif h:
                mx = v
            hit.append(h)
        if hit == [False, True, False, False]:
            out[n] = 1
        elif not hit[0] and hit[2] and not hit[3]:
            out[n] = 2
        elif not hit[0] and hit[3]:
            out[n] = 3
    return out


# ---------------------------------------------------------------------------------------------- ids
def terrible_id(classes, grid, pop_cap=100000):
    """yolact.rs:52-88. Returns (diverges, ids int8). A fill that terminates pops each start once and pushes nothing (a push needs
    two class-3 cells that are linear neighbours, and those push each other for ever), so pop_cap > number of cells decides."""
    img = [int(c) for c in np.asarray(classes).reshape(-1)]
    N = len(img)
    out = [-1] * N
    ident, pops = -1, 0
    for start in range(N):
        if not (img[start] == 3 and out[start] == -1):
            continue
        ident = (ident + 1 + 128) % 256 - 128          # i8 += 1, wrapping as a release build does
        stack = [start]
        while stack:
            px = stack.pop()
            pops += 1
            if pops > pop_cap:
                return True, np.array(out, np.int8)
            for q in ((px - 1) % U64, px + 1, (px - grid) % U64, px + grid):   # usize arithmetic; img.get(q)
                if q < N and img[q] == 3:
                    out[q] = ident
                    stack.append(q)
    return False, np.array(out, np.int8)


def sane_ids(classes, grid):
    cl = np.asarray(classes).reshape(grid, grid)
    parent = list(range(grid * grid))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for y in range(grid):
        for x in range(grid):
            if cl[y, x] != 3:
                continue
            c = y * grid + x
            for ok, q in ((x > 0, c - 1), (y > 0, c - grid)):
                if ok and cl.reshape(-1)[q] == 3:
                    a, b = find(c), find(q)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    ids = np.full(grid * grid, -1, np.int8)
    seen = {}
    for c in range(grid * grid):
        if cl.reshape(-1)[c] == 3:
            r = find(c)
            if r not in seen:
                seen[r] = min(len(seen), 127)
            ids[c] = seen[r]
    return ids


# ---------------------------------------------------------------------------------------------- codes
def pack(classes, ids, mode):
    """yolact.rs:127: `cls << 24 & id << 16` with `id as u32` sign-extending (STRICT); SANE means `|` and the id's low byte."""
    cls = np.asarray(classes).astype(np.uint64).reshape(-1) << np.uint64(24)
    idu = np.asarray(ids, np.int8).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    if mode == 0:
        return (cls & ((idu << 16) & 0xFFFFFFFF).astype(np.uint64)).astype(np.uint32)
    return (cls | (((idu & 0xFF) << 16).astype(np.uint64))).astype(np.uint32)


def upsample8(codes, grid):
    return np.repeat(np.repeat(np.asarray(codes).reshape(grid, grid), 8, axis=0), 8, axis=1)


def stitch(t1, t2):
    return np.concatenate([t1, t2], axis=1)


def postprocess_tile(cells, grid, mode, pop_cap=100000):
    """(diverges, code image uint32 [8 grid][8 grid] or None)."""
    classes = gated_argmax(np.asarray(cells, np.float32).reshape(grid * grid, -1))
    if mode == 0:
        div, ids = terrible_id(classes, grid, pop_cap)
        if div:
            return True, None
    else:
        ids = sane_ids(classes, grid)
    return False, upsample8(pack(classes, ids, mode), grid)


# ---------------------------------------------------------------------------------------------- triangle resize
def _weights(out_i, in_size, out_size):
    ratio = F32(in_size) / F32(out_size)
    sratio = F32(1.0) if ratio < F32(1.0) else ratio
    support = F32(1.0) * sratio
    centre = (F32(out_i) + F32(0.5)) * ratio
    left = min(max(int(np.floor(centre - support)), 0), in_size - 1)
    right = min(max(int(np.ceil(centre + support)), left + 1), in_size)
    centre = centre - F32(0.5)
    ws, total = [], F32(0.0)
    for i in range(left, right):
        a = abs((F32(i) - centre) / sratio)
        w = F32(1.0) - a if a < F32(1.0) else F32(0.0)
        ws.append(F32(w))
        total = F32(total + w)
    return left, [F32(w / total) for w in ws]


def _to_u8(t, round):
    t = np.clip(t, F32(0.0), F32(255.0)).astype(np.float64)
    if round == "away":
        return np.floor(t + 0.5).astype(np.uint8)          # t >= 0 and exact in float64: half away from zero
    assert round == "even"
    return np.rint(t).astype(np.uint8)


def resize(src, dw, dh, round="away"):
    """src uint8 [sh][sw][3] -> uint8 [dh][dw][3]."""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape[:2]
    if (sw, sh) == (dw, dh):
        return src.copy()
    s = src.astype(np.float32)
    tmp = np.zeros((dh, sw, 3), np.float32)
    for oy in range(dh):
        left, ws = _weights(oy, sh, dh)
        for i, w in enumerate(ws):
            tmp[oy] = tmp[oy] + s[left + i] * w
    out = np.zeros((dh, dw, 3), np.float32)
    for ox in range(dw):
        left, ws = _weights(ox, sw, dw)
        for i, w in enumerate(ws):
            out[:, ox] = out[:, ox] + tmp[:, left + i] * w
    return _to_u8(out, round)
