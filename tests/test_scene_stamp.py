"""The stamping kernel (cloud_strips_body in csrc/scene_dev.h, launched as scene_cloud_strips and batch_cloud_strips) on frames in which
every pixel's bump is visible (tests/scene_stamp_ref.py; DESIGN.md §11 "A max is tested with visible contributors"). The height map is a
MAX over bumps: on the dense frames of tests/test_scene.py about 2-6 % of the stamping pixels decide any map cell, so most of the
kernel's per-pixel bookkeeping (strips of 16 columns with a 20-column halo, bands of 64 rows, four pixel rows per wave, row groups 32 apart,
ballot / readlane hand-offs, per-lane tap tables) could be wrong without a test noticing. Here every pixel of a shape stamps alone.
CPU part: the frame sets do what they claim (every pixel visible, windows disjoint), the oracle's bumps against float64, depth_for's
round trip. GPU part (-m gpu): HIP == oracle/orc_scene.c, np.array_equal on every comparison."""
import ctypes as C

import numpy as np
import pytest

import scene_stamp_ref as R

KEYS = ("map", "balls", "world", "conn1", "conn0")
ISOLATED = [(70, 37, 0, R.TERRAIN_L), (70, 37, 1, R.ROBOT_L), (133, 19, 0, R.TERRAIN_L)]


# ------------------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("H,W,cls,L", ISOLATED)
def test_every_pixel_is_a_visible_isolated_stamp(oracle, H, W, cls, L):
    """A condition on the inputs of the GPU tests, not a measurement: each pixel of the shape stamps in exactly one frame, alone in its
    window, and the oracle's map shows it - every pixel as a robot, every pixel of rows >= 2 as terrain (a terrain bump's tallest tap is
    trunc(y - 0.1): 0 for rows 0 and 1). The target rows sweep 0 .. H, and the stamps that meet a band seam (map rows 64, 128) or the
    frame's first / last rows come from all four lane rows and all sixteen lane columns of a wave and from all eight waves."""
    frames, maps = R.isolated_frames(H, W, cls, L), R.isolated_maps(H, W, cls, L)
    seen, hidden = R.audit(frames, maps)                              # asserts disjoint windows and nothing outside them
    stamps = [s for fr in frames for s in fr.stamps]
    assert len(stamps) == H * W and {(x, y) for (x, y, _, _) in stamps} == {(x, y) for x in range(W) for y in range(H)}
    lowest = 2 if cls == 0 else 0
    assert {(x, y) for (_, x, y) in seen} == {(x, y) for x in range(W) for y in range(lowest, H)}
    assert {y for (_, _, y) in hidden} == set(range(lowest))
    print(f"{H} x {W} class {cls}: {len(frames)} frames, {len(seen)} of {W * (H - lowest)} pixels visible")
    assert {ny for (_, _, ny, _) in stamps} == set(range(H + 1))
    meets = {"top": lambda ny: ny - L <= 1, "bottom": lambda ny: ny + L - 1 >= H - 2}
    for seam in range(64, H, 64):
        meets[f"seam {seam}"] = lambda ny, seam=seam: ny - L < seam <= ny + L - 1
    for name, meet in meets.items():
        at = [(x, y) for (x, y, ny, _) in stamps if meet(ny)]
        assert {y % 4 for _, y in at} == set(range(4)) and {x % 16 for x, _ in at} == set(range(min(16, W))), name
        assert {(y // 4) % 8 for _, y in at} == set(range(8)), name


def test_bump_heights_against_float64(oracle):
    """The oracle's bump - float32, pow() as exp(e log a) on the spec functions - against the shader's formula in float64: every terrain
    row 1 .. 479 (val = the row) as one isolated stamp in the middle of a 480 x 41 frame, and the robot bump (val = 100). Truncation
    allows a distance just under 1 from the real value and nothing else; no tap sits within float32 rounding of an integer."""
    H, W, ny, x = 480, 41, 240, 20
    worst = 0.0
    for y in range(1, H):
        L = R.TERRAIN_L
        fr = R.with_stamps(H, W, [(x, y, ny, L)], 0)
        m = oracle.scene(fr.depth, fr.ci, 1)["map"]
        want, real = R.bump_f64(float(y), L)
        got = m[ny - L:ny + L, x - L:x + L]
        assert np.array_equal(got, want), (y, np.argwhere(got != want).tolist())
        m = m.copy()
        m[ny - L:ny + L, x - L:x + L] = 0
        assert not m.any(), y
        worst = max(worst, float(np.abs(got - real)[real >= 1].max(initial=0.0)))
    assert worst < 1.0
    print(f"terrain rows 1 .. {H - 1}: {(H - 1) * 4 * R.TERRAIN_L ** 2} taps equal, worst distance from the real value {worst:.6f}")
    for cls in R.ROBOT_CLASSES:
        L, H, W, ny, x = R.ROBOT_L, 96, 96, 50, 41
        fr = R.with_stamps(H, W, [(x, 30, ny, L)], cls)
        m = oracle.scene(fr.depth, fr.ci, 1)["map"]
        want, real = R.bump_f64(100.0, L)
        assert np.array_equal(m[ny - L:ny + L, x - L:x + L], want), (cls, np.argwhere(m[ny - L:ny + L, x - L:x + L] != want).tolist())
        assert int(m.sum()) == int(want.sum()) and want[L, L] == 99 and want[0, L] == 0


def test_depth_for_round_trip(oracle):
    """The oracle puts an isolated pixel where depth_for was asked to put it: a ball pixel's y "mean" IS its target row (any row, above
    the map included), and a robot's mound is symmetric about it."""
    for (H, W) in ((70, 37), (133, 19), (480, 41), (16, 16)):
        xs, ys = sorted({0, 1, W // 2, W - 2, W - 1}), sorted({0, 1, H // 2, H - 2, H - 1})
        for x in xs:
            for y in ys:
                for ny in (H, H - 1, H // 2, 1, 0, -1, -25, -H):
                    d = R.depth_for(H, W, x, y, ny)
                    assert d.dtype == np.uint16 and int(R.target_row(H, W, x, y, d)) == ny
                    depth, ci = R.quiet(H, W)
                    depth[y, x], ci[y, x] = d, (3, 42)
                    balls = oracle.scene(depth, ci, 1)["balls"]
                    assert balls[42].tolist() == [x, ny, 1, 0] and not balls[np.arange(100) != 42].any(), (H, W, x, y, ny)
        with pytest.raises(ValueError):
            R.depth_for(H, W, 0, 0, H + 1)
    H, W = 70, 70
    for (x, y, ny) in ((0, 0, 30), (W - 1, H - 1, 40), (35, 0, 21), (30, H - 1, 48), (0, 35, 35)):
        fr = R.with_stamps(H, W, [(x, y, ny, R.ROBOT_L)], 1)
        rows = np.flatnonzero(oracle.scene(fr.depth, fr.ci, 1)["map"].any(1))
        assert rows.min() + rows.max() == 2 * ny and rows.max() - rows.min() < 2 * R.ROBOT_L, (x, y, ny)


# ------------------------------------------------------------------------------------------------------------------------------ GPU
def _differ(got, want, keys=KEYS):
    return [k for k in keys if not np.array_equal(got[k], want[k])]


def _batch(sb, frames, mode, full_every=16, light=("map", "balls")):
    """Stages `frames` into slots 0 .., appends them in `mode` and returns [(slot, outputs)]: all five outputs of every full_every-th
    slot, the `light` ones of the others."""
    import yolact_amd as ya
    sb.stage_frames(0, np.stack([f.depth for f in frames]), frames_u32=np.stack([ya.SceneBatch.pack(f.ci) for f in frames]))
    sb.append(len(frames), mode)
    return [(b, sb.read(b) if b % full_every == 0 else sb.read(b, which=light)) for b in range(len(frames))]


class _DeviceFrame:
    """A packed frame in device memory of its own (the HIP runtime the library has loaded, through ctypes)."""

    def __init__(self, frame):
        path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), "libamdhip64.so")
        self.hip, self.ptr = C.CDLL(path), C.c_void_p()
        frame = np.ascontiguousarray(frame, np.uint32)
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(frame.nbytes)) == 0
        assert self.hip.hipMemcpy(self.ptr, frame.ctypes.data_as(C.c_void_p), C.c_size_t(frame.nbytes), 1) == 0   # hipMemcpyHostToDevice

    def free(self):
        assert self.hip.hipFree(self.ptr) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,cls,L", ISOLATED)
def test_every_pixel_isolated_matches_the_oracle(built, oracle, H, W, cls, L):
    """3a. The whole isolated set through the batch handle, up to 256 slots per append (blockIdx.z up to 255), in both modes: every
    frame's map equals the oracle's, every 16th frame's five outputs do; then at least 64 frames spread over the set through the single
    handle. 70 x 37: two bands (the second of 6 rows), three strips (the last of 5 columns), three row-group iterations (the last
    partial), H % 4 = 2. 133 x 19: three bands (64, 64, 5), two strips (16 + 3)."""
    import yolact_amd as ya
    frames, maps = R.isolated_frames(H, W, cls, L), R.isolated_maps(H, W, cls, L)
    n, bad = len(frames), []
    sb = ya.SceneBatch(W, H, 256)
    for mode in (1, 0):
        for lo in range(0, n, 256):
            for b, got in _batch(sb, frames[lo:lo + 256], mode, light=("map",)):
                i = lo + b
                if not np.array_equal(got["map"], maps[i]):
                    bad.append((mode, i, int((got["map"] != maps[i]).sum()), frames[i].stamps))
                elif len(got) > 1:
                    d = _differ(got, oracle.scene(frames[i].depth, frames[i].ci, mode))
                    if d:
                        bad.append((mode, i, d))
    sb.close()
    assert not bad, f"batch handle: {len(bad)} of 2 x {n} frames differ from the oracle; (mode, frame, cells | outputs, stamps): {bad[:4]}"
    sc = ya.Scene(W, H)
    for k, i in enumerate(sorted(set(np.linspace(0, n - 1, 80).astype(int).tolist()))):
        sc.append(frames[i].depth, frames[i].ci, k % 2)
        d = _differ(sc.read(), oracle.scene(frames[i].depth, frames[i].ci, k % 2))
        if d:
            bad.append((k % 2, i, d, frames[i].stamps))
    sc.close()
    assert not bad, f"single handle: {len(bad)} frames differ from the oracle; (mode, frame, outputs, stamps): {bad[:4]}"


@pytest.mark.gpu
def test_targets_beyond_the_map(built, oracle):
    """3b. Isolated terrain and robot stamps whose target rows lie above the map (the window wholly outside, one row inside, across
    row 0), on its last rows and at row H, in the columns at the strips' edges; whole frames at depth 65535 and depth 0. All five
    outputs, both modes, batch handle; the whole frames and every eighth stamp through the single handle too."""
    import yolact_amd as ya
    H, W = 70, 37
    frames = R.edge_frames(H, W)
    assert len(frames) == 2 * 9 * 8 + 4 and all(R.windows_disjoint(f.stamps) for f in frames)
    want = {mode: [oracle.scene(f.depth, f.ci, mode) for f in frames] for mode in (0, 1)}
    assert not any(w["map"].any() for w in want[1][-4:-2])                       # depth 65535: every bump misses the map
    assert all(w["map"][H - 8:H - 1, 1:W - 1].all() and not w["map"][:H - 20].any() for w in want[1][-2:])   # depth 0: every target is row H
    sb, sc, bad = ya.SceneBatch(W, H, 256), ya.Scene(W, H), []
    for mode in (1, 0):
        bad += [("batch", mode, b, _differ(got, want[mode][b]), frames[b].stamps) for b, got in _batch(sb, frames, mode, full_every=1)]
        for b in list(range(0, len(frames) - 4, 8)) + list(range(len(frames) - 4, len(frames))):
            sc.append(frames[b].depth, frames[b].ci, mode)
            bad.append(("single", mode, b, _differ(sc.read(), want[mode][b]), frames[b].stamps))
    sb.close(); sc.close()
    bad = [b for b in bad if b[3]]
    assert not bad, f"{len(bad)} frames differ from the oracle; (handle, mode, frame, outputs, stamps): {bad[:4]}"


@pytest.mark.gpu
def test_balls_every_id_one_id_and_negative_sums(built, oracle):
    """3c. Ball sums: all 100 ids at once (99, 100 and 255 side by side; each id in every strip and on both sides of pixel row 64), one
    id on every pixel (count W * H), and depth 65535 - every target row far below zero, the y sums large negative numbers that pass
    through unsigned 64-bit LDS and global atomics - with an all-zero map."""
    import yolact_amd as ya
    H, W = 70, 37
    frames = R.ball_frames(H, W)
    ids = frames[0].ci[..., 1]
    for k in range(100):
        ys, xs = np.nonzero(ids == k)
        assert {x // 16 for x in xs} == {0, 1, 2} and (ys < 64).any() and (ys >= 64).any(), k
    assert ids[5, 10:13].tolist() == [99, 100, 255] and (ids >= 100).sum() > 3
    want = {mode: [oracle.scene(f.depth, f.ci, mode) for f in frames] for mode in (0, 1)}
    assert (want[1][0]["balls"][:, 2] > 0).all() and want[1][0]["balls"][:, 2].sum() == (ids < 100).sum()
    assert want[1][1]["balls"][7, 2] == W * H and not want[1][1]["balls"][np.arange(100) != 7].any()
    assert (want[1][2]["balls"][:, 1] < -250).all() and not any(w["map"].any() for m in (0, 1) for w in want[m])
    sb, sc = ya.SceneBatch(W, H, 4), ya.Scene(W, H)
    for mode in (1, 0):
        for b, got in _batch(sb, frames, mode, full_every=1):
            assert not _differ(got, want[mode][b]), ("batch", mode, b)
            sc.append(frames[b].depth, frames[b].ci, mode)
            assert not _differ(sc.read(), want[mode][b]), ("single", mode, b)
    sb.close(); sc.close()


@pytest.mark.gpu
def test_class_decode_of_all_three_input_forms(built, oracle):
    """3d. Every class value 0 .. 255 with ids 0, 99, 100, 255 as (1) the class / id image, (2) a packed frame in SANE layout (class
    bits 31-24, id bits 23-16) with garbage in bits 15-0, (3) a packed frame read in STRICT mode (class bits 7-0, id bits 15-8: `as u16`
    then R8G8, src/scene.rs:93, :198) with garbage in bits 31-16. One map and one ball table for all three; conn0 / conn1 are the
    oracle's for the mode the form was appended in. The SANE-layout frame read in STRICT mode is the oracle on ITS low 16 bits. Single
    and batch handle, frame on the host and on the device."""
    import yolact_amd as ya
    H, W = 70, 37
    fr = R.decode_frame(H, W)
    assert {(c, i) for c, i in fr.ci.reshape(-1, 2).tolist()} == {(c, i) for c in range(256) for i in (0, 99, 100, 255)}
    rng = np.random.default_rng(11)
    cls, ident = fr.ci[..., 0].astype(np.uint32), fr.ci[..., 1].astype(np.uint32)
    sane = cls << 24 | ident << 16 | rng.integers(0, 1 << 16, (H, W)).astype(np.uint32)
    strict = rng.integers(0, 1 << 16, (H, W)).astype(np.uint32) << 16 | ident << 8 | cls
    low = np.stack([sane & 0xFF, (sane >> 8) & 0xFF], -1).astype(np.uint8)       # what STRICT reads in the SANE-layout frame
    assert len(np.unique(low[..., 0])) == 256 and not np.array_equal(low, fr.ci)
    want = {mode: oracle.scene(fr.depth, fr.ci, mode) for mode in (0, 1)}
    want_low = oracle.scene(fr.depth, low, 0)
    assert all(np.array_equal(want[0][k], want[1][k]) for k in ("map", "balls", "world")) and want[1]["map"].any()
    forms = [("sane frame", sane, ya.COMPAT_SANE, want[1]), ("strict frame", strict, ya.COMPAT_STRICT, want[0]),
             ("sane frame read strictly", sane, ya.COMPAT_STRICT, want_low)]
    sc, sb = ya.Scene(W, H), ya.SceneBatch(W, H, 4)
    for mode in (0, 1):
        sc.append(fr.depth, fr.ci, mode)
        assert not _differ(sc.read(), want[mode]), ("class / id image", mode)
    for name, frame, mode, w in forms:
        dev = _DeviceFrame(frame)
        sc.append_classified(fr.depth, frame_u32=frame, mode=mode)
        assert not _differ(sc.read(), w), ("single, host", name)
        sc.append_classified(fr.depth, frame_dev_ptr=dev.ptr.value, mode=mode)
        assert not _differ(sc.read(), w), ("single, device", name)
        quiet = ya.SceneBatch.pack(R.quiet(H, W)[1])
        sb.stage(0, fr.depth, frame_u32=frame)
        sb.stage(1, fr.depth, frame_u32=quiet)
        sb.stage(2, fr.depth, frame_dev_ptr=dev.ptr.value)
        sb.append(3, mode)
        assert not _differ(sb.read(0), w), ("batch, host", name)
        assert not _differ(sb.read(2), w), ("batch, device", name)
        assert not sb.read(1, which=("map", "balls"))["map"].any()
        dev.free()
    for mode in (0, 1):                                                          # SceneBatch.pack: the frame both modes read the same
        sb.stage(0, fr.depth, cls_id=fr.ci)
        sb.append(1, mode)
        assert not _differ(sb.read(0), want[mode]), ("batch, packed class / id image", mode)
    sc.close(); sb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(3, 3), (3, 40), (40, 3), (4, 16), (5, 17), (63, 37), (64, 16), (65, 15), (129, 36)])
def test_small_and_seam_sizes(built, oracle, H, W):
    """3e. The smallest legal sizes and sizes around the strip width (16), the halo's reach (36), the band height (64) and two bands
    (128): a dense frame and a sparse one (about one pixel in forty stamps: class and depth random, targets above the map included),
    both modes, all five outputs; each frame is followed on the same handle by a different one, whose results show no trace of it."""
    import yolact_amd as ya
    rng = np.random.default_rng(1000 * H + W)
    dense, sparse, other = R.dense_frame(rng, H, W), R.sparse_frame(rng, H, W), R.sparse_frame(rng, H, W)
    assert not np.array_equal(sparse.depth, other.depth)
    order = (dense, sparse, other, dense)
    sc, sb = ya.Scene(W, H), ya.SceneBatch(W, H, 2)
    for mode in (0, 1):
        want = [oracle.scene(f.depth, f.ci, mode) for f in order]
        for k, f in enumerate(order):
            sc.append(f.depth, f.ci, mode)
            assert not _differ(sc.read(), want[k]), ("single", mode, k)
        for k in (0, 1, 2):                                                      # slots (dense, sparse), (sparse, other), (other, dense)
            for b, got in _batch(sb, order[k:k + 2], mode, full_every=1):
                assert not _differ(got, want[k + b]), ("batch", mode, k, b)
    sc.close(); sb.close()


@pytest.mark.gpu
def test_a_batch_of_256_different_frames(built, oracle):
    """3f. All 256 slots of a batch handle, every slot a different 70 x 37 frame from the sets above, appended with n = 256 and then -
    the first slots restaged - with n = 3 on the same handle: slots 0 .. n - 1 equal the oracle (map and balls of every slot, all
    five outputs of every 16th and of the three)."""
    import yolact_amd as ya
    H, W = 70, 37
    terrain, robot = R.isolated_frames(H, W, 0, R.TERRAIN_L), R.isolated_frames(H, W, 1, R.ROBOT_L)
    pool = list(R.ball_frames(H, W)) + [R.decode_frame(H, W)] + list(R.edge_frames(H, W)[-4:]) + list(R.edge_frames(H, W)[:-4:3])
    pool += list(terrain[::4]) + list(robot[::14])
    frames, rest = pool[:256], pool[256:259]
    assert len(frames) == 256 and len(rest) == 3 and len({f.depth.tobytes() + f.ci.tobytes() for f in pool[:259]}) == 259
    sb = ya.SceneBatch(W, H, 256)
    for b, got in _batch(sb, frames, 1):
        assert not _differ(got, oracle.scene(frames[b].depth, frames[b].ci, 1), tuple(got)), (256, b)
    for b, got in _batch(sb, rest, 0, full_every=1):
        assert not _differ(got, oracle.scene(rest[b].depth, rest[b].ci, 0)), (3, b)
    with pytest.raises(ya.YhError):
        sb.read(3, which=("map",))                                               # the last append had three frames
    sb.close()
