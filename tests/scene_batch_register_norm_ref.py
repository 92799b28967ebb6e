"""The scene batch's normalised registration (DESIGN.md §11 "Scene batch: normalised registration") restated: a bank of
scene_register_norm_ref.Memory objects, one per camera stream, and a batched normalised search append that is nothing but the single
normalised search step applied in batch order, frame b on the memory of streams[b] as the frames before it left it. Imports nothing
from the library: the tests compare the library against this, and this against answers worked out by hand."""
import scene_memory_ref as R
import scene_register_norm_ref as NR

STREAMS_MAX = 64


class Bank:
    def __init__(self, W, H):
        self.W, self.H = W, H
        self.mem = [NR.Memory(W, H) for _ in range(STREAMS_MAX)]

    def reset(self, stream=-1):
        for s in (range(STREAMS_MAX) if stream < 0 else (stream,)):
            self.mem[s].reset()

    def append_search_norm(self, stamps, frame_balls, streams=None, candidates=None, radius=4, min_inside=None, keep=224, max_age=30):
        """stamps[n]: every frame's own height map N, frame_balls[n]: its own ball rows; streams[n] or None (all 0); candidates[n] =
        (gathers, carries) pairs of n_rot rows each or None (the identity alone); min_inside: one value for the call, None: W H // 4.
        Returns (the per-frame outputs, the per-frame ball tables - the table of frame b's stream right after frame b -, the per-frame
        motions as scene_register_norm_ref.search returns them)."""
        n = len(stamps)
        streams = [0] * n if streams is None else list(streams)
        candidates = [([R.IDENTITY], [R.IDENTITY])] * n if candidates is None else list(candidates)
        min_inside = (self.W * self.H) // 4 if min_inside is None else min_inside
        assert len(frame_balls) == len(streams) == len(candidates) == n and all(0 <= s < STREAMS_MAX for s in streams)
        assert len(set(len(g) for g, _ in candidates)) == 1 and all(len(g) == len(c) for g, c in candidates)
        out, tables, motions = [], [], []
        for b in range(n):
            m = self.mem[streams[b]]
            out.append(m.append_search_norm(stamps[b], frame_balls[b], candidates[b][0], candidates[b][1], radius, min_inside, keep, max_age))
            tables.append(m.B.copy())
            motions.append(m.motion)
        return out, tables, motions
