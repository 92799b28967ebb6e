"""Instance tracks restated (DESIGN.md §11 "Instance tracks"): numpy int64, no float anywhere. Everything not defined here is the
instance frame's (instance_ref): eligibility, the class map, min_score, the integer resize, "smallest rank wins a pixel".

A Tracker holds 128 slots; a live slot has an output class (1..3), an id (0..127), an age (calls since it was last matched), the
area and the binary mask at prototype resolution it was last seen with. One tracked call (`track`) associates the frame's eligible
detections with the live slots by mask overlap, ages, frees and creates slots, and paints the frame with the slots' ids.
Outputs: the frame uint32 [H][W], the instance table int32 [m][4] = (rank, class, track id, pixels won) and the track table
int32 [m][6] = (slot, class, id, age, area, rank or -1), one row per live slot in slot order."""
import functools

import numpy as np

import instance_ref as I

SLOTS = 128


_POP = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def overlap(T, C):
    """I[s][c] = |T_s AND C_c| for boolean mask stacks T [S][hp][wp], C [n][hp][wp]: int64 [S][n] (bytes of eight pixels ANDed,
    their set bits counted from a table)."""
    S, n = len(T), len(C)
    Tb, Cb = np.packbits(T.reshape(S, -1), axis=1), np.packbits(C.reshape(n, -1), axis=1)
    out = np.zeros((S, n), np.int64)
    cs = np.flatnonzero(Cb.any(1))
    for s in np.flatnonzero(Tb.any(1)).tolist():
        out[s, cs] = _POP[Tb[s][None, :] & Cb[cs]].sum(1, dtype=np.int64)
    return out


def candidates(Iov, cls_s, area_s, cls_c, area_c, live, elig, iou_permille):
    """The pairs (s, c) with equal class, I > 0 and 1000 I >= iou_permille U, U = area_s + A_c - I: a list of (s, c, I, U)."""
    out = []
    for s in np.flatnonzero(live).tolist():
        for c in np.flatnonzero(elig).tolist():
            i = int(Iov[s, c])
            u = int(area_s[s]) + int(area_c[c]) - i
            if cls_s[s] == cls_c[c] and i > 0 and 1000 * i >= iou_permille * u:
                out.append((s, c, i, u))
    return out


def better(a, b, age):
    """Candidate a = (s, c, I, U) precedes b: larger I / U by cross-multiplication, then smaller age, smaller c, smaller s."""
    (s1, c1, i1, u1), (s2, c2, i2, u2) = a, b
    if i1 * u2 != i2 * u1:
        return i1 * u2 > i2 * u1
    return (int(age[s1]), c1, s1) < (int(age[s2]), c2, s2)


def greedy(cand, age):
    """Repeatedly the best candidate; it removes every candidate that shares its slot or its rank. Returns {c: s} in the order
    taken. (The order is total, so this is one pass over the candidates sorted by it.)"""
    order = functools.cmp_to_key(lambda a, b: -1 if better(a, b, age) else 1)
    match, slots = {}, set()
    for s, c, _, _ in sorted(cand, key=order):
        if s not in slots and c not in match:
            match[c] = s
            slots.add(s)
    return match


class Tracker:
    def __init__(self):
        self.reset()

    def reset(self):
        self.shape = None
        self.cls = np.zeros(SLOTS, np.int64)                                       # 0: the slot is free
        self.id = np.zeros(SLOTS, np.int64)
        self.age = np.zeros(SLOTS, np.int64)
        self.area = np.zeros(SLOTS, np.int64)
        self.T = None                                                            # bool [SLOTS][hp][wp]

    def table(self, rank_of=None):
        rank_of = rank_of or {}
        rows = [(s, self.cls[s], self.id[s], self.age[s], self.area[s], rank_of.get(s, -1)) for s in range(SLOTS) if self.cls[s]]
        return np.array(rows, np.int32).reshape(-1, 6)

    def track(self, masks, class_ids, scores, W, H, class_map=None, min_score=0.0, iou_permille=300, max_age=2, num_classes=81):
        assert 1 <= iou_permille <= 1000 and 0 <= max_age <= 255
        masks = np.asarray(masks) != 0                                           # [n][hp][wp], n = 0 included
        n = len(masks)
        assert masks.ndim == 3 and n <= SLOTS
        if self.shape != masks.shape[1:]:
            self.reset()                                                         # another prototype size: an empty tracker
            self.shape = masks.shape[1:]
            self.T = np.zeros((SLOTS,) + self.shape, bool)
        rk = I.ranks(class_ids, scores, class_map, min_score, num_classes)
        elig = np.array([r[0] for r in rk] + [False] * (SLOTS - n), bool)
        cls_c = np.array([r[1] for r in rk] + [0] * (SLOTS - n), np.int64)
        C = np.zeros((SLOTS,) + self.shape, bool)
        for c in range(n):
            if elig[c]:
                C[c] = masks[c]
        area_c = C.reshape(SLOTS, -1).sum(1).astype(np.int64)
        live = self.cls != 0
        # 1-3: overlap, candidates, greedy match
        match = greedy(candidates(overlap(self.T, C), self.cls, self.area, cls_c, area_c, live, elig, iou_permille), self.age)
        matched = set(match.values())
        # 4: ageing
        for s in np.flatnonzero(live).tolist():
            if s not in matched:
                self.age[s] += 1
                if self.age[s] > max_age:
                    self._free(s)
        # 5: room
        born = [c for c in np.flatnonzero(elig).tolist() if c not in match]
        while int((self.cls == 0).sum()) < len(born):
            lost = [s for s in range(SLOTS) if self.cls[s] and s not in matched]
            self._free(max(lost, key=lambda s: (int(self.age[s]), s)))
        # 6: births
        for c in born:
            s = int(np.flatnonzero(self.cls == 0)[0])
            held = set(self.id[self.cls == cls_c[c]].tolist())
            self.cls[s], self.id[s] = cls_c[c], next(i for i in range(SLOTS) if i not in held)
            match[c] = s
        # 7: update
        for c, s in match.items():
            self.age[s], self.area[s], self.T[s] = 0, area_c[c], C[c]
        # 8: paint
        frame = np.zeros((H, W), np.uint32)
        free = np.ones((H, W), bool)
        table = []
        for c in sorted(match):
            s = match[c]
            won = I.upsample(C[c], W, H) & free
            frame[won] = (int(self.cls[s]) << 24) | (int(self.id[s]) << 16)
            free &= ~won
            table.append((c, self.cls[s], self.id[s], int(won.sum())))
        return frame, np.array(table, np.int32).reshape(-1, 4), self.table({s: c for c, s in match.items()})

    def _free(self, s):
        self.cls[s] = self.id[s] = self.age[s] = self.area[s] = 0
        self.T[s] = False
