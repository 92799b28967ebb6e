"""bench.py --dump-outputs without a GPU: what bench.dump_outputs writes from an engine-shaped stand-in - names, dtypes,
shapes, the padding past each frame's detections, whole small outputs, the seeded sample of large ones."""
import types

import numpy as np

import bench

NAMES = ("loc", "conf", "mask", "proto", "cells")


class StandInEngine:
    """The part of yolact_amd.Engine that dump_outputs reads, with seeded contents."""

    def __init__(self, n=3, P=50, C=5, hp=6, wp=7, max_dets=4):
        rng = np.random.default_rng(7)
        self.n, self.hp, self.wp = n, hp, wp
        self.cfg = types.SimpleNamespace(max_dets=max_dets)
        self.outs = [rng.standard_normal(s).astype(np.float32) for s in
                     ((n, P, 4), (n, P, C), (n, P, 32), (n, hp, wp, 32), (n, 3, 3, C))]
        self.outs[1] = rng.standard_normal((n, 9000, 256)).astype(np.float32)     # larger than DUMP_SAMPLE: sampled
        self.dets = []
        for f in range(n):
            nd = f % (max_dets + 1)
            self.dets.append(([dict(class_id=f + j, prior=10 * f + j, score=0.5 + 0.1 * j, box=(0.1 * j, 0.2, 0.3, 0.4)) for j in range(nd)],
                              rng.integers(0, 2, (nd, hp, wp), dtype=np.uint8)))

    def sync(self):
        pass

    def output_count(self):
        return len(NAMES)

    def output_info(self, i):
        return dict(name=NAMES[i], dims=self.outs[i].shape)

    def output(self, i):
        return self.outs[i].copy()

    def detections(self, frame, want_masks=True):
        return self.dets[frame]


def test_dump_outputs_writes_the_last_step_as_float_arrays(tmp_path):
    eng = StandInEngine()
    bench.dump_outputs(eng, str(tmp_path / "a"))
    bench.dump_outputs(eng, str(tmp_path / "b"))
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(f"{n}.npy" for n in NAMES + ("det_count", "det_class", "det_prior", "det_score", "det_box", "det_mask_area", "det_masks"))
    out = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert out[f[:-4]].dtype in (np.float32, np.float64), f
        assert np.array_equal(out[f[:-4]], np.load(tmp_path / "b" / f)), f          # the same sample in every run
    for i, name in enumerate(NAMES):
        if name != "conf":
            assert np.array_equal(out[name], eng.outs[i]), name                     # small outputs whole
    conf = eng.outs[1].reshape(-1)
    assert out["conf"].ndim == 1 and bench.DUMP_SAMPLE // 2 < out["conf"].size <= bench.DUMP_SAMPLE   # (seeded draws, repeats dropped)
    assert np.isin(out["conf"], conf).all()
    assert list(out["det_count"]) == [len(d) for d, _ in eng.dets]
    for f, (dets, masks) in enumerate(eng.dets):
        nd = len(dets)
        assert list(out["det_class"][f, :nd]) == [d["class_id"] for d in dets] and (out["det_class"][f, nd:] == -1).all()
        assert list(out["det_prior"][f, :nd]) == [d["prior"] for d in dets] and (out["det_prior"][f, nd:] == -1).all()
        assert np.allclose(out["det_score"][f, :nd], [d["score"] for d in dets]) and (out["det_score"][f, nd:] == 0).all()
        assert np.allclose(out["det_box"][f, :nd], np.reshape([d["box"] for d in dets], (nd, 4))) and (out["det_box"][f, nd:] == 0).all()
        assert list(out["det_mask_area"][f, :nd]) == [int(m.sum()) for m in masks] and (out["det_mask_area"][f, nd:] == 0).all()
        assert np.array_equal(out["det_masks"][f, :nd], masks) and (out["det_masks"][f, nd:] == 0).all()


def test_dump_sample_keeps_small_arrays_and_samples_large_ones_at_fixed_positions():
    small = np.arange(10, dtype=np.float32)
    assert bench.dump_sample(small, k=10) is small
    big = np.arange(1000, dtype=np.float64).reshape(10, 100)
    s = bench.dump_sample(big, k=100)
    assert s.ndim == 1 and 90 <= s.size <= 100 and (np.diff(s) > 0).all()          # distinct positions, in order
    assert np.array_equal(s, bench.dump_sample(big.copy(), k=100))
