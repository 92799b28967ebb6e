"""The turn-aware tour's frozen definition (DESIGN.md §11 "Turn tour"), restated on the CPU for tests/test_scene_turn_tour.py on top
of turn_ref (states (pixel, heading), the price tau per 45 degrees, the action rule, the walk) and tour_ref (K <= TOUR_MAX distinct
targets, a field per target, all K! orders in lexicographic order).

Per target t_b: d_b f32 [8][H][W] and act_b u8 [8][H][W], turn_ref's fields with the single target {t_b}; the other targets are
ordinary pixels of field b. label u8 [8][H][W]: the smallest b with d_b[h][v] == min_b d_b[h][v].
The leg table has rows r = 0 .. 8K: row 0 is the state (start, h0), row 1 + 8a + h the state (t_a, h). legs f32 [1 + 8K][K]:
legs[r][b] = d_b at row r's state. arrive u8 [1 + 8K][K]: the heading with which turn_ref.walk along act_b from row r's state reaches
t_b (the row's own heading where its pixel is t_b: act_b is 255 there in every layer).
Total of an order o: pos = start, g = h0, tot = 0; for each j: tot = fl(tot + d_{o_j}[g][pos]), g = arrive(pos, g -> o_j),
pos = t_{o_j}. A leg is the turn plan's route from the state in which the leg before ended: the arrival heading is taken as it
comes, not optimised over. The order of least total, compared in f32; ties go to the lexicographically smallest permutation."""
import itertools

import numpy as np

import tour_ref as T
import turn_ref as U

TOUR_MAX = T.TOUR_MAX


def fields(hmap, conn0, conn1, targets, tau):
    """(cost f32 [K][8][H][W], act u8 [K][8][H][W]): field b has the single target t_b."""
    cost = np.stack([U.dijkstra(hmap, conn0, conn1, [t], tau) for t in targets])
    act = np.stack([U.actions(cost[b], hmap, conn0, conn1, [t], tau) for b, t in enumerate(targets)])
    return cost, act


def labels(cost):
    """label[h][v] = the smallest b with d_b[h][v] == min_b d_b[h][v], u8 [8][H][W]."""
    return np.argmin(cost, axis=0).astype(np.uint8)


def leg(cost_b, act_b, pos, heading):
    """(path, directions, turns, arrival heading) of turn_ref.walk along one field from the state (pos, heading)."""
    path, dirs, turns = U.walk(cost_b, act_b, pos, heading)
    return path, dirs, turns, (int(heading) + int(turns.sum())) % 8            # (no turn is made on the target: act is 255 there)


def row_of(a, h):
    """The leg table's row of the state (t_a, h); the start state is row 0."""
    return 1 + 8 * a + h


def leg_tables(cost, act, targets, start, heading):
    """(legs f32 [1 + 8K][K], arrive u8 [1 + 8K][K])."""
    K = len(targets)
    states = [(tuple(start), int(heading))] + [(tuple(t), h) for t in targets for h in range(8)]
    legs = np.zeros((1 + 8 * K, K), np.float32)
    arrive = np.zeros((1 + 8 * K, K), np.uint8)
    for r, ((x, y), h) in enumerate(states):
        for b in range(K):
            legs[r, b] = cost[b, h, y, x]
            arrive[r, b] = leg(cost[b], act[b], (x, y), h)[3]
    return legs, arrive


def tour_total(legs, arrive, order):
    """(total f32, the rows the legs start from, the headings they arrive with) of the order, from row 0."""
    tot, r, rows, heads = np.float32(0), 0, [], []
    for b in order:
        rows.append(r)
        tot = np.float32(tot + legs[r, b])
        heads.append(int(arrive[r, b]))
        r = row_of(b, heads[-1])
    return tot, rows, heads


def best_order(legs, arrive):
    """(order tuple, total f32): all K! permutations in lexicographic order, the first strictly smallest total wins."""
    best, best_total = None, None
    for o in itertools.permutations(range(legs.shape[1])):
        t = tour_total(legs, arrive, o)[0]
        if best is None or t < best_total:
            best, best_total = o, t
    return best, best_total


def route(cost, act, targets, order, start, heading):
    """(path i32 [L][2], directions f32 [L - 1][2], turns i32 [L - 1], leg_ends i32 [K], leg_headings i32 [K]): the legs' walks
    joined, a junction node once; a leg that starts on its own target adds no node and passes the heading on. The first turns and
    directions entry of a leg is counted from the heading the leg before arrived with, in this leg's action field."""
    path, dirs, turns, leg_ends, leg_headings = [np.array([start], np.int32).reshape(1, 2)], [], [], [], []
    at, g, n = tuple(start), int(heading), 1
    for b in order:
        p, d, t, g = leg(cost[b], act[b], at, g)
        assert tuple(p[-1]) == tuple(targets[b]) and (np.abs(t) <= 4).all()
        path.append(p[1:]); dirs.append(d); turns.append(t)
        n += len(p) - 1
        leg_ends.append(n - 1); leg_headings.append(g)
        at = tuple(targets[b])
    return (np.concatenate(path).astype(np.int32), np.concatenate(dirs).astype(np.float32).reshape(-1, 2), np.concatenate(turns).astype(np.int32),
            np.array(leg_ends, np.int32), np.array(leg_headings, np.int32))


def turn_tour(hmap, conn0, conn1, targets, start, heading, tau, solved=None):
    """Everything yh_scene_turn_tour_read returns, as a dict. solved: (cost, act) if the caller has them already."""
    targets = [tuple(t) for t in targets]
    assert 1 <= len(targets) <= TOUR_MAX and len(set(targets)) == len(targets)
    cost, act = solved if solved is not None else fields(hmap, conn0, conn1, targets, tau)
    legs, arrive = leg_tables(cost, act, targets, start, heading)
    order, total = best_order(legs, arrive)
    path, dirs, turns, leg_ends, leg_headings = route(cost, act, targets, order, start, heading)
    return dict(targets=np.array(targets, np.int32).reshape(-1, 2), order=np.array(order, np.int32), legs=legs, arrive=arrive, total=total,
                leg_headings=leg_headings, cost=cost, act=act, label=labels(cost), path=path, directions=dirs, turns=turns, leg_ends=leg_ends)
