"""The scene batch's registration (DESIGN.md §11 "Scene batch: registration") restated: a bank of scene_register_ref.Memory objects, one
per camera stream, and a batched search append that is nothing but the single search step applied in batch order, frame b on the
memory of streams[b] as the frames before it left it. Imports nothing from the library: the tests compare the library against this,
and this against answers worked out by hand."""
import scene_memory_ref as R
import scene_register_ref as G

STREAMS_MAX = 64


class Bank:
    def __init__(self, W, H):
        self.W, self.H = W, H
        self.mem = [G.Memory(W, H) for _ in range(STREAMS_MAX)]

    def reset(self, stream=-1):
        for s in (range(STREAMS_MAX) if stream < 0 else (stream,)):
            self.mem[s].reset()

    def append(self, stamps, frame_balls, streams=None, motions=None, keep=224, max_age=30):
        """scene_batch_memory_ref.Bank.append on this bank: the motions given"""
        n = len(stamps)
        motions = [(R.IDENTITY, R.IDENTITY)] * n if motions is None else list(motions)
        out, tables, _ = self.append_search(stamps, frame_balls, streams, [([m[0]], [m[1]]) for m in motions], 0, keep, max_age)
        return out, tables

    def append_search(self, stamps, frame_balls, streams=None, candidates=None, radius=4, keep=224, max_age=30):
        """stamps[n]: every frame's own height map N, frame_balls[n]: its own ball rows; streams[n] or None (all 0); candidates[n] =
        (gathers, carries) pairs of n_rot rows each or None (the identity alone). Returns (the per-frame outputs, the per-frame ball
        tables - the table of frame b's stream right after frame b -, the per-frame motions as scene_register_ref.search returns them)."""
        n = len(stamps)
        streams = [0] * n if streams is None else list(streams)
        candidates = [([R.IDENTITY], [R.IDENTITY])] * n if candidates is None else list(candidates)
        assert len(frame_balls) == len(streams) == len(candidates) == n and all(0 <= s < STREAMS_MAX for s in streams)
        assert len(set(len(g) for g, _ in candidates)) == 1 and all(len(g) == len(c) for g, c in candidates)
        out, tables, motions = [], [], []
        for b in range(n):
            m = self.mem[streams[b]]
            out.append(m.append_search(stamps[b], frame_balls[b], candidates[b][0], candidates[b][1], radius, keep, max_age))
            tables.append(m.B.copy())
            motions.append(m.motion)
        return out, tables, motions
