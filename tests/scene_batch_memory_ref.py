"""The scene batch's memory (DESIGN.md §11 "Scene batch: memory") restated: a bank of scene_memory_ref.Memory objects, one per camera
stream, and a batched append that is nothing but the single step applied in batch order, frame b on the memory of streams[b]. Imports
nothing from the library: the tests compare the library against this, and this against answers worked out by hand."""
import numpy as np

import scene_memory_ref as R

STREAMS_MAX = 64


class Bank:
    def __init__(self, W, H):
        self.W, self.H = W, H
        self.mem = [R.Memory(W, H) for _ in range(STREAMS_MAX)]

    def reset(self, stream=-1):
        for s in (range(STREAMS_MAX) if stream < 0 else (stream,)):
            self.mem[s].reset()

    def append(self, stamps, frame_balls, streams=None, motions=None, keep=224, max_age=30):
        """stamps[n]: every frame's own height map N, frame_balls[n]: its own ball rows; streams[n] or None (all 0); motions[n] =
        (gather_q16, carry_q16) pairs or None (identity). Returns (the per-frame outputs, the per-frame ball tables: the table of
        frame b's stream right after frame b)."""
        n = len(stamps)
        streams = [0] * n if streams is None else list(streams)
        motions = [(R.IDENTITY, R.IDENTITY)] * n if motions is None else list(motions)
        assert len(frame_balls) == len(streams) == len(motions) == n and all(0 <= s < STREAMS_MAX for s in streams)
        out, tables = [], []
        for b in range(n):
            m = self.mem[streams[b]]
            out.append(m.append(stamps[b], frame_balls[b], motions[b][0], motions[b][1], keep, max_age))
            tables.append(m.B.copy())
        return out, tables
