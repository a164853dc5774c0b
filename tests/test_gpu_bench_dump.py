"""bench.py --dump-outputs end to end on a small batch: the files hold the reference-order result
of the timed steps, in the order the timed path ran the sequences, and not the tree-order pass
the same run makes afterwards into the same device buffers (the tree-order batch leg)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def canonical(a):
    """the libm-exp branch (p >= 0.9999) canonicalised, as bench.golden_digest compares it"""
    a = np.array(a, dtype=np.float32, copy=True)
    a[a >= 0.9999] = 1.0
    return a


@pytest.mark.gpu
def test_dump_holds_the_last_timed_step(params, tmp_path):
    count = 8  # ~18 MB of packed output: dumped whole
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--batch-count", str(count), "--no-n4096", "--no-cpu-baseline",
                        "--no-transfers", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert "tree_batch" in line, "the tree-order leg did not run after the timed steps"
    assert sorted(os.listdir(out)) == ["bpp_packed.npy", "log_z.npy"]

    import bench
    from rna_algos_amd import workloads as W
    from rna_algos_amd.mccaskill_algo import Context
    seqs, _ = bench.build_workload("batch10k", count)
    order = bench.shard_banded(W.sweep_cost(np.array([len(s) for s in seqs])), 1)[0]
    ctx = Context(params, device=0)
    try:
        mats, logz = ctx.bpp_batch([seqs[i] for i in order], False, False)
    finally:
        ctx.close()
    assert np.array_equal(np.load(out / "log_z.npy"), logz)
    want = np.concatenate([m.packed for m in mats])
    assert np.array_equal(canonical(np.load(out / "bpp_packed.npy")), canonical(want))
