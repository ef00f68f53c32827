"""bench.py --dump-outputs: the files two builds are compared by.  An output is written whole as
float32 channel values, one row per pixel; one larger than DUMP_MAX_PIXELS as the same fixed sample
of its pixels on every run."""
import os
import sys

import numpy as np
import torch

from tests.conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _frame(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, generator=g)


def test_dump_small_output_whole(tmp_path):
    f = _frame(37, 53, 1)
    bench.dump_outputs(str(tmp_path / "d"), {"frame": f})
    a = np.load(tmp_path / "d" / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (37 * 53, 4)
    assert np.array_equal(a, f.reshape(-1, 4).numpy().astype(np.float32))


def test_dump_large_output_fixed_sample(tmp_path):
    n = bench.DUMP_MAX_PIXELS
    f = _frame(1100, 2000, 2)                     # 2.2 M pixels > DUMP_MAX_PIXELS
    assert f.shape[0] * f.shape[1] > n
    bench.dump_outputs(str(tmp_path / "a"), {"frames": f})
    bench.dump_outputs(str(tmp_path / "b"), {"frames": f.clone()})
    a, b = np.load(tmp_path / "a" / "frames.npy"), np.load(tmp_path / "b" / "frames.npy")
    assert a.dtype == np.float32 and a.shape == (n, 4) and np.array_equal(a, b)
    assert os.path.getsize(tmp_path / "a" / "frames.npy") <= 64 * 1000 * 1000
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(f.shape[0] * f.shape[1], n, replace=False))
    assert np.array_equal(a, f.reshape(-1, 4).numpy()[idx].astype(np.float32))
    # a changed pixel inside the sample shows
    g = f.clone().reshape(-1, 4)
    g[idx[12345], 1] ^= 1
    bench.dump_outputs(str(tmp_path / "c"), {"frames": g.reshape(f.shape)})
    assert not np.array_equal(a, np.load(tmp_path / "c" / "frames.npy"))
