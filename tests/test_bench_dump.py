"""bench.py --dump-outputs: what the last timed step returned, stored as float32 / float64 .npy
within the size limit; an output over the limit as a fixed seeded sample, the same from run to
run.  (Host logic only: the tensors here are CPU tensors of the step's output forms.)"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _step_output(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    wav = torch.rand(shape, generator=g) * 2 - 1
    return wav, torch.full((shape[0],), shape[1], dtype=torch.int64)


@pytest.mark.parametrize("shape", [(3, 517), (2, 301, 2)])
def test_dump_whole_output(tmp_path, shape):
    import bench
    wav, lens = _step_output(shape)
    bench.dump_outputs(str(tmp_path / "o"), wav, lens)
    got = _load(tmp_path / "o")
    assert sorted(got) == ["lens", "wav"]
    assert got["wav"].dtype == np.float32 and got["lens"].dtype == np.float32
    assert np.array_equal(got["wav"], wav.numpy())
    assert np.array_equal(got["lens"], lens.numpy().astype(np.float32))


def test_dump_over_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 2 ** 20)
    wav, lens = _step_output((4, 250001, 2))            # 8 MB of float32: over the 3 MB limit
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), wav, lens)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["lens", "wav_sample", "wav_sample_index"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= 3 * 2 ** 20
    assert a["wav_sample"].dtype == np.float32 and a["wav_sample_index"].dtype == np.float64
    idx = a["wav_sample_index"].astype(np.int64)
    assert idx.min() >= 0 and idx.max() < wav.numel() and np.all(np.diff(idx) >= 0)
    assert np.array_equal(a["wav_sample"], wav.numpy().reshape(-1)[idx])
    # another output of the same shape is sampled at the same positions
    bench.dump_outputs(str(tmp_path / "c"), *_step_output((4, 250001, 2), seed=1))
    assert np.array_equal(_load(tmp_path / "c")["wav_sample_index"], a["wav_sample_index"])
