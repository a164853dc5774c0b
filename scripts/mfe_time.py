"""Time the maximum-score structure (rnamc_mfe_batch) against the call that shares its grouping and
traceback machinery: rnamc_sample_batch with ONE sample per sequence (the reference-order inside
sweep plus a trivial traceback).  Cases: the bench's 10 000-sequence batch (workloads.batch_lengths
/ batch_seq, 256-2048 nt), lone n = 1024 and n = 4096; both models.  Prints one JSON line per case.
argv: [--quick] (the first 1 000 sequences of the batch)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402,F401

from rna_algos_amd.mccaskill_algo import Context  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402
from rna_algos_amd.workloads import batch_lengths, batch_seq, synthetic_seq  # noqa: E402


def best_of(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def case(ctx, name, seqs, contra, reps):
    warm = seqs[:200]
    ctx.mfe_batch(warm, contra, False)  # warm-up: code objects, staging buffers
    ctx.sample_batch(warm, 1, contra, False)
    t_mfe = best_of(lambda: ctx.mfe_batch(seqs, contra, False), reps)
    t_s1 = best_of(lambda: ctx.sample_batch(seqs, 1, contra, False), reps)
    nt = int(sum(len(s) for s in seqs))
    print(json.dumps({"case": name, "model": "contra" if contra else "turner", "n_seqs": len(seqs),
                      "nt": nt, "s_mfe": round(t_mfe, 5), "mfe_nt_per_s": round(nt / t_mfe, 1),
                      "s_sample_1": round(t_s1, 5), "sample_1_nt_per_s": round(nt / t_s1, 1),
                      "speedup": round(t_s1 / t_mfe, 3)}), flush=True)


def main():
    quick = "--quick" in sys.argv
    ctx = Context(FoldScoreSets.synthetic(1), device=0)
    lens = batch_lengths()[:1000 if quick else 10000]
    batch = [batch_seq(s, lengths=lens) for s in range(len(lens))]
    for contra in (False, True):
        case(ctx, "n1024", [synthetic_seq(1024, 1024)], contra, 3)
        case(ctx, "n4096", [synthetic_seq(4096, 4096)], contra, 1)
        case(ctx, f"batch{len(batch)}_256_2048", batch, contra, 1)
    ctx.close()


if __name__ == "__main__":
    main()
