"""bench.py's --dump-outputs writer and --steps check, on CPU tensors: the packed output whole
when it fits, else the same seeded sample on every call with its positions, within the size
budget; rank-suffixed names with N ranks."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_whole_and_sampled(tmp_path, monkeypatch):
    import torch
    out = torch.arange(1000, dtype=torch.float32)
    logz = torch.tensor([1.5, -2.0, 3.25])
    bench.dump_outputs(str(tmp_path / "whole"), out, logz, 1, 0)
    assert sorted(os.listdir(tmp_path / "whole")) == ["bpp_packed.npy", "log_z.npy"]
    assert np.array_equal(np.load(tmp_path / "whole" / "bpp_packed.npy"), out.numpy())
    assert np.array_equal(np.load(tmp_path / "whole" / "log_z.npy"), logz.numpy())

    monkeypatch.setattr(bench, "DUMP_BPP_BYTES", 12 * 500)
    big = torch.arange(1 << 20, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, logz, 1, 0)
    vals = np.load(tmp_path / "a" / "bpp_packed_sample.npy")
    pos = np.load(tmp_path / "a" / "bpp_packed_sample_positions.npy")
    assert vals.dtype == np.float32 and pos.dtype == np.float64 and len(vals) == len(pos) == 500
    assert np.all(np.diff(pos) >= 0) and pos.min() >= 0 and pos.max() < big.numel()
    assert np.array_equal(vals, big.numpy()[pos.astype(np.int64)])
    assert np.array_equal(vals, np.load(tmp_path / "b" / "bpp_packed_sample.npy"))
    assert np.array_equal(pos, np.load(tmp_path / "b" / "bpp_packed_sample_positions.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) <= 64 << 20

    bench.dump_outputs(str(tmp_path / "r"), big, logz, 2, 1)
    assert sorted(os.listdir(tmp_path / "r")) == ["bpp_packed_sample_positions_rank1.npy",
                                                  "bpp_packed_sample_rank1.npy", "log_z_rank1.npy"]
    assert len(np.load(tmp_path / "r" / "bpp_packed_sample_rank1.npy")) == 250


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr
