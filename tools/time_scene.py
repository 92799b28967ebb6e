"""The scene back-end (yh_scene_*: shaders/pt_cloud.comp + pt_cloud_weights.comp as HIP kernels) on one 640x480 frame:
device milliseconds per frame (five launches), for a terrain-only frame and one with robots and balls.
--memory: the memory append (yh_scene_append_memory: stamps, ball memory and ONE fuse launch) against the plain append on the same
frames, in one process: the two alternated, one warm-up each, the median of five runs of 30 frames, and the spread of each.
--memory-search: the search append (yh_scene_append_memory_search: the same with the registration between the stamps and the fuse)
against the memory append, likewise, over (n_rot, radius) = (1, 0), (1, 4), (5, 4), (9, 8): ms per frame of both, ms of the
registration launches alone, and its rate in pixel-candidates per second.
--memory-pyramid: the pyramid append (yh_scene_append_memory_pyramid: the registration made coarse to fine) against the search
append at the same n_rot with radius 8, likewise, over (n_rot, levels, radius, refine) = (1, 3, 8, 1), (5, 3, 8, 1), (9, 3, 8, 2):
ms per frame of both and ms of the registration launches alone of both, their ratio and the spread of each.
--memory-search-norm: the normalised search append (yh_scene_append_memory_search_norm: three sums per shift, no empty-tile exit)
against the plain search append with the same candidates, likewise, over the grids of --memory-search: ms per frame of both, ms of
the registration launches alone of both, their ratio and the spread of each.
--memory-pyramid-norm: the normalised pyramid append (yh_scene_append_memory_pyramid_norm: every level decided by S / U) against the
plain pyramid append with the same candidates, on a second handle, likewise, over the grids of --memory-pyramid: ms per frame of
both, ms of the registration launches alone of both, their ratio and the spread of each."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-object-detection_amd"))
import yolact_amd as ya
H, W = 480, 640
rng = np.random.default_rng(0)
depth = rng.integers(200, 4000, (H, W)).astype(np.uint16)


def frames():
    for name, robots in (("terrain only", False), ("robots + balls", True)):
        ci = np.zeros((H, W, 2), np.uint8)
        if robots:
            ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
        yield name, ci


def memory_table(runs=5, reps=30):
    """rows of (frame, median ms plain, median ms memory, ratio of the medians, (max - min) / median of plain, of memory)"""
    plain, mem = ya.Scene(W, H), ya.Scene(W, H)
    motion = ya.scene_motion(3.0, -2.0, 0.05)           # a small turn and a step: gathers that cross rows, most sources inside the frame
    rows = []
    for name, ci in frames():
        plain.append(depth, ci, ya.COMPAT_SANE)
        mem.append_memory(depth, cls_id=ci, motion=motion)   # the memory is filled: the replayed append fuses this frame into it
        mem.append_memory(depth, cls_id=ci, motion=motion)
        plain.time(reps); mem.memory_time(reps)              # one warm-up each
        tp, tm = [], []
        for _ in range(runs):
            tp.append(plain.time(reps)); tm.append(mem.memory_time(reps))
        mp, mm = float(np.median(tp)), float(np.median(tm))
        rows.append((name, mp, mm, mm / mp, (max(tp) - min(tp)) / mp, (max(tm) - min(tm)) / mm))
    plain.close(); mem.close()
    return rows


SEARCH_GRIDS = ((1, 0), (1, 4), (5, 4), (9, 8))


def memory_search_table(grids=SEARCH_GRIDS, runs=5, reps=30):
    """rows of (frame, n_rot, radius, median ms memory, median ms search append, ratio, median ms of the registration alone,
    pixel-candidates per second, (max - min) / median of memory, of the search append)"""
    mem, srch = ya.Scene(W, H), ya.Scene(W, H)
    prior = (3.0, -2.0, 0.05)                            # memory_table's motion: the prior is right, the search confirms it
    motion = ya.scene_motion(*prior)
    rows = []
    for name, ci in frames():
        for n_rot, radius in grids:
            cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=(n_rot - 1) // 2)
            for sc in (mem, srch):
                sc.memory_reset()
                sc.append_memory(depth, cls_id=ci, motion=motion)
            mem.append_memory(depth, cls_id=ci, motion=motion)
            srch.append_memory_search(depth, cls_id=ci, candidates=cands, radius=radius)
            mem.memory_time(reps); srch.memory_search_time(reps)
            tm, ts, tr = [], [], []
            for _ in range(runs):
                tm.append(mem.memory_time(reps))
                a, b = srch.memory_search_time(reps)
                ts.append(a); tr.append(b)
            mm, ms, mr = float(np.median(tm)), float(np.median(ts)), float(np.median(tr))
            rate = W * H * n_rot * (2 * radius + 1) ** 2 / (mr * 1e-3)
            rows.append((name, n_rot, radius, mm, ms, ms / mm, mr, rate, (max(tm) - min(tm)) / mm, (max(ts) - min(ts)) / ms))
    mem.close(); srch.close()
    return rows


def memory_search_norm_table(grids=SEARCH_GRIDS, runs=5, reps=30):
    """rows of (frame, n_rot, radius, median ms search append, median ms normalised append, median ms of the plain registration
    alone, of the normalised registration alone, their ratio, (max - min) / median of the plain registration, of the normalised)"""
    srch, norm = ya.Scene(W, H), ya.Scene(W, H)
    prior = (3.0, -2.0, 0.05)                            # memory_search_table's prior: it is right, both searches confirm it
    motion = ya.scene_motion(*prior)
    rows = []
    for name, ci in frames():
        for n_rot, radius in grids:
            cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=(n_rot - 1) // 2)
            for sc in (srch, norm):
                sc.memory_reset()
                sc.append_memory(depth, cls_id=ci, motion=motion)
            srch.append_memory_search(depth, cls_id=ci, candidates=cands, radius=radius)
            norm.append_memory_search_norm(depth, cls_id=ci, candidates=cands, radius=radius)
            srch.memory_search_time(reps); norm.memory_search_norm_time(reps)
            ts, tr, tn, tq = [], [], [], []
            for _ in range(runs):
                a, b = srch.memory_search_time(reps)
                ts.append(a); tr.append(b)
                a, b = norm.memory_search_norm_time(reps)
                tn.append(a); tq.append(b)
            ms, mr, mn, mq = (float(np.median(t)) for t in (ts, tr, tn, tq))
            rows.append((name, n_rot, radius, ms, mn, mr, mq, mq / mr, (max(tr) - min(tr)) / mr, (max(tq) - min(tq)) / mq))
    srch.close(); norm.close()
    return rows


PYRAMID_GRIDS = ((1, 3, 8, 1), (5, 3, 8, 1), (9, 3, 8, 2))


def memory_pyramid_table(grids=PYRAMID_GRIDS, runs=5, reps=30):
    """rows of (frame, n_rot, levels, radius, refine, median ms search append, median ms pyramid append, median ms of the plain
    registration alone, of the pyramid registration alone, their ratio, (max - min) / median of the plain registration, of the
    pyramid registration)"""
    srch, pyr = ya.Scene(W, H), ya.Scene(W, H)
    prior = (3.0, -2.0, 0.05)                            # memory_search_table's prior: it is right, both searches confirm it
    motion = ya.scene_motion(*prior)
    rows = []
    for name, ci in frames():
        for n_rot, levels, radius, refine in grids:
            cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=(n_rot - 1) // 2)
            for sc in (srch, pyr):
                sc.memory_reset()
                sc.append_memory(depth, cls_id=ci, motion=motion)
            srch.append_memory_search(depth, cls_id=ci, candidates=cands, radius=8)
            pyr.append_memory_pyramid(depth, cls_id=ci, candidates=cands, levels=levels, radius=radius, refine=refine)
            srch.memory_search_time(reps); pyr.memory_pyramid_time(reps)
            ts, tr, tp, tq = [], [], [], []
            for _ in range(runs):
                a, b = srch.memory_search_time(reps)
                ts.append(a); tr.append(b)
                a, b = pyr.memory_pyramid_time(reps)
                tp.append(a); tq.append(b)
            ms, mr, mp, mq = (float(np.median(t)) for t in (ts, tr, tp, tq))
            rows.append((name, n_rot, levels, radius, refine, ms, mp, mr, mq, mq / mr, (max(tr) - min(tr)) / mr, (max(tq) - min(tq)) / mq))
    srch.close(); pyr.close()
    return rows


def memory_pyramid_norm_table(grids=PYRAMID_GRIDS, runs=5, reps=30):
    """rows of (frame, n_rot, levels, radius, refine, median ms pyramid append, median ms normalised pyramid append, median ms of
    the plain pyramid registration alone, of the normalised one alone, their ratio, (max - min) / median of the plain pyramid
    registration, of the normalised)"""
    pyr, norm = ya.Scene(W, H), ya.Scene(W, H)
    prior = (3.0, -2.0, 0.05)                            # memory_pyramid_table's prior: it is right, both descents confirm it
    motion = ya.scene_motion(*prior)
    rows = []
    for name, ci in frames():
        for n_rot, levels, radius, refine in grids:
            cands = ya.scene_motion_candidates(prior=prior, dtheta_step=0.01, n_side=(n_rot - 1) // 2)
            for sc in (pyr, norm):
                sc.memory_reset()
                sc.append_memory(depth, cls_id=ci, motion=motion)
            pyr.append_memory_pyramid(depth, cls_id=ci, candidates=cands, levels=levels, radius=radius, refine=refine)
            norm.append_memory_pyramid_norm(depth, cls_id=ci, candidates=cands, levels=levels, radius=radius, refine=refine)
            pyr.memory_pyramid_time(reps); norm.memory_pyramid_norm_time(reps)
            tp, tr, tn, tq = [], [], [], []
            for _ in range(runs):
                a, b = pyr.memory_pyramid_time(reps)
                tp.append(a); tr.append(b)
                a, b = norm.memory_pyramid_norm_time(reps)
                tn.append(a); tq.append(b)
            mp, mr, mn, mq = (float(np.median(t)) for t in (tp, tr, tn, tq))
            rows.append((name, n_rot, levels, radius, refine, mp, mn, mr, mq, mq / mr, (max(tr) - min(tr)) / mr, (max(tq) - min(tq)) / mq))
    pyr.close(); norm.close()
    return rows


if __name__ == "__main__":
    if "--memory-pyramid-norm" in sys.argv[1:]:
        print(f"scene {W}x{H}: pyramid append (yh_scene_memory_pyramid_time) against normalised pyramid append (yh_scene_memory_pyramid_norm_time), ms, median of 5 x 30 replays")
        print(f"{'frame':<16} {'n_rot':>5} {'L':>1} {'R':>1} {'r':>1} {'pyramid':>8} {'norm':>8} {'reg pyr':>8} {'reg norm':>8} {'ratio':>7} {'spread pyr':>11} {'spread norm':>12}")
        for name, n_rot, levels, radius, refine, mp, mn, mr, mq, ratio, sr, sq in memory_pyramid_norm_table():
            print(f"{name:<16} {n_rot:5d} {levels:1d} {radius:1d} {refine:1d} {mp:8.4f} {mn:8.4f} {mr:8.4f} {mq:8.4f} {ratio:7.3f} {100 * sr:10.1f}% {100 * sq:11.1f}%")
    elif "--memory-pyramid" in sys.argv[1:]:
        print(f"scene {W}x{H}: search append at radius 8 (yh_scene_memory_search_time) against pyramid append (yh_scene_memory_pyramid_time), ms, median of 5 x 30 replays")
        print(f"{'frame':<16} {'n_rot':>5} {'L':>1} {'R':>1} {'r':>1} {'search':>8} {'pyramid':>8} {'reg plain':>9} {'reg pyr':>8} {'ratio':>7} {'spread plain':>13} {'spread pyr':>11}")
        for name, n_rot, levels, radius, refine, ms, mp, mr, mq, ratio, sr, sq in memory_pyramid_table():
            print(f"{name:<16} {n_rot:5d} {levels:1d} {radius:1d} {refine:1d} {ms:8.4f} {mp:8.4f} {mr:9.4f} {mq:8.4f} {ratio:7.3f} {100 * sr:12.1f}% {100 * sq:10.1f}%")
    elif "--memory-search-norm" in sys.argv[1:]:
        print(f"scene {W}x{H}: search append (yh_scene_memory_search_time) against normalised search append (yh_scene_memory_search_norm_time), ms, median of 5 x 30 replays")
        print(f"{'frame':<16} {'n_rot':>5} {'R':>2} {'search':>8} {'norm':>8} {'reg plain':>9} {'reg norm':>8} {'ratio':>7} {'spread plain':>13} {'spread norm':>12}")
        for name, n_rot, radius, ms, mn, mr, mq, ratio, sr, sq in memory_search_norm_table():
            print(f"{name:<16} {n_rot:5d} {radius:2d} {ms:8.4f} {mn:8.4f} {mr:9.4f} {mq:8.4f} {ratio:7.3f} {100 * sr:12.1f}% {100 * sq:11.1f}%")
    elif "--memory-search" in sys.argv[1:]:
        print(f"scene {W}x{H}: memory append (yh_scene_memory_time) against search append (yh_scene_memory_search_time), ms per frame, median of 5 x 30 frames")
        print(f"{'frame':<16} {'n_rot':>5} {'R':>2} {'memory':>8} {'search':>8} {'ratio':>7} {'alone':>8} {'Gpx-cand/s':>11} {'spread memory':>14} {'spread search':>14}")
        for name, n_rot, radius, mm, ms, ratio, mr, rate, sm, ss in memory_search_table():
            print(f"{name:<16} {n_rot:5d} {radius:2d} {mm:8.4f} {ms:8.4f} {ratio:7.3f} {mr:8.4f} {rate / 1e9:11.2f} {100 * sm:13.1f}% {100 * ss:13.1f}%")
    elif "--memory" in sys.argv[1:]:
        print(f"scene {W}x{H}: plain append (yh_scene_time) against memory append (yh_scene_memory_time), ms per frame, median of 5 x 30 frames")
        print(f"{'frame':<16} {'plain':>8} {'memory':>8} {'ratio':>7} {'spread plain':>13} {'spread memory':>14}")
        for name, mp, mm, ratio, sp, sm in memory_table():
            print(f"{name:<16} {mp:8.4f} {mm:8.4f} {ratio:7.3f} {100 * sp:12.1f}% {100 * sm:13.1f}%")
    else:
        sc = ya.Scene(W, H)
        for name, ci in frames():
            sc.append(depth, ci, ya.COMPAT_SANE)
            out = sc.read()
            print(f"scene 640x480, {name}: {sc.time(30):.3f} ms per frame (map max {out['map'].max()}, {int((out['balls'][:, 2] > 0).sum())} balls)")
