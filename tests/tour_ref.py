"""The tour planner's frozen definition (DESIGN.md §11 "Tour"), restated on the CPU for tests/test_scene_tour.py on top of
path_ref: K <= TOUR_MAX distinct targets, one single-target cost field d_b and successor field next_b per target (path_ref's,
unchanged, for the connectivity conn = 4 or 8), the label of the nearest target per pixel, the leg matrix, the best visiting order and the joined route.

legs f32 [K + 1][K]: legs[0][b] = d_b[start], legs[1 + a][b] = d_b[t_a] - the cost to travel FROM t_a TO t_b (costs accumulate
from the target outward, so d_b[t_a] and d_a[t_b] differ in their last bits: the direction is part of the definition).
order: the permutation o minimising fl(...fl(fl(legs[0][o_0] + legs[1 + o_0][o_1]) + legs[1 + o_1][o_2])...), summed left to
right and compared in f32; ties go to the lexicographically smallest permutation."""
import itertools

import numpy as np

import path_ref as R

TOUR_MAX = 6


def distinct(targets):
    """Targets in their order without repeats (a ball whose pixel equals an earlier ball's is dropped)."""
    out = []
    for t in targets:
        if tuple(t) not in out:
            out.append(tuple(t))
    return out


def fields(hmap, conn0, conn1, targets, conn=4):
    """(cost f32 [K][H][W], next i32 [K][H][W]): field b has the single target t_b; other targets are ordinary pixels of it."""
    cost = np.stack([R.dijkstra(hmap, conn0, conn1, [t], conn) for t in targets])
    nxt = np.stack([R.successors(cost[b], hmap, conn0, conn1, [t], conn) for b, t in enumerate(targets)])
    return cost, nxt


def labels(cost):
    """label[v] = the smallest b with d_b[v] == min_b d_b[v] (the reference's ball[node], path.rs:35,66), u8."""
    return np.argmin(cost, axis=0).astype(np.uint8)


def leg_matrix(cost, targets, start):
    K = len(targets)
    legs = np.zeros((K + 1, K), np.float32)
    for b in range(K):
        legs[0, b] = cost[b, start[1], start[0]]
        for a, (x, y) in enumerate(targets):
            legs[1 + a, b] = cost[b, y, x]
    return legs


def tour_total(legs, order):
    total = legs[0, order[0]]
    for a, b in zip(order[:-1], order[1:]):
        total = np.float32(total + legs[1 + a, b])
    return np.float32(total)


def best_order(legs):
    """(order tuple, total f32): all K! permutations in lexicographic order, the first strictly smallest total wins."""
    K = legs.shape[1]
    best, best_total = None, None
    for o in itertools.permutations(range(K)):
        t = tour_total(legs, o)
        if best is None or t < best_total:
            best, best_total = o, t
    return best, best_total


def nearest_first(legs):
    """The greedy order (always the cheapest next leg, lowest index on ties): what the tour is compared against."""
    K = legs.shape[1]
    left, row, order = list(range(K)), 0, []
    while left:
        b = min(left, key=lambda k: (legs[row, k], k))
        order.append(b); left.remove(b); row = 1 + b
    return tuple(order)


def route(cost, nxt, targets, order, start, conn=4):
    """(path i32 [L][2], directions f32 [L - 1][2], leg_ends i32 [K]): the legs' walks joined, a junction node once; a leg whose
    start is its own target adds no node. Step i inside leg j has magnitude d_{o_j}[n_i] - d_{o_j}[n_{i+1}]; rot_0 = 0, else
    path_ref.rotation: on the 4-connected grid float32(pi) when straight, float32(pi / 2) for a turn; 0.0 when n_{i-1} == n_{i+1} (a
    reversal, at a junction only)."""
    nodes, field_of_step, leg_ends = [tuple(start)], [], []
    at = tuple(start)
    for b in order:
        seg, _ = R.walk(cost[b], nxt[b], at, conn)
        assert tuple(seg[-1]) == tuple(targets[b])
        for n in seg[1:]:
            nodes.append(tuple(int(v) for v in n)); field_of_step.append(b)
        leg_ends.append(len(nodes) - 1)
        at = tuple(targets[b])
    path = np.array(nodes, np.int32).reshape(-1, 2)
    dirs = np.zeros((len(nodes) - 1, 2), np.float32)
    for i, b in enumerate(field_of_step):
        (x0, y0), (x1, y1) = nodes[i], nodes[i + 1]
        dirs[i, 0] = cost[b, y0, x0] - cost[b, y1, x1]
        if i > 0:
            dirs[i, 1] = R.rotation(nodes[i - 1], nodes[i], nodes[i + 1])
    return path, dirs, np.array(leg_ends, np.int32)


def tour(hmap, conn0, conn1, targets, start, conn=4):
    """Everything yh_scene_tour_read returns, as a dict."""
    targets = [tuple(t) for t in targets]
    assert 1 <= len(targets) <= TOUR_MAX and len(set(targets)) == len(targets)
    cost, nxt = fields(hmap, conn0, conn1, targets, conn)
    legs = leg_matrix(cost, targets, start)
    order, total = best_order(legs)
    path, dirs, leg_ends = route(cost, nxt, targets, order, start, conn)
    return dict(targets=np.array(targets, np.int32).reshape(-1, 2), order=np.array(order, np.int32), legs=legs, total=total, cost=cost,
                next=nxt, label=labels(cost), path=path, directions=dirs, leg_ends=leg_ends)


def flat_fields(H, W):
    """A flat map with unit lengths: costs are Manhattan distances."""
    hmap = np.zeros((H, W), np.uint32)
    return (hmap,) + R.sane_connections(hmap)


def camera_like_frame(H=480, W=640):
    """(depth u16 [H][W], class image u8 [H][W][2]): the robots-and-balls frame the planner is timed on (tools/time_path.py's)."""
    depth = np.random.default_rng(0).integers(200, 4000, (H, W)).astype(np.uint16)
    ci = np.zeros((H, W, 2), np.uint8)
    ci[100:220, 150:330, 0] = 1; ci[260:330, 380:520, 0] = 2; ci[60:75, 60:80] = (3, 4); ci[400:420, 500:530] = (3, 9)
    return depth, ci
