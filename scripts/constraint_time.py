"""Time the hard-constraint entries against the unconstrained ones (include/rnamc.h, DESIGN.md
section 11).  Each case alternates the two calls in one process, best of `reps`:
  - bpp: the first 1 000 sequences of the bench batch (workloads.batch_lengths / batch_seq) in both
    summation modes and both models, against rnamc_bpp_batch, with two kinds of constraint:
      "active_neutral": '<' on the first base and '>' on the last, no span limit -- installed and
      tested at every pair, yet it forbids nothing (the results are checked to equal the
      unconstrained ones bit for bit): the cost of the predicate itself;
      "mixed": an 'x' window, a bracket pair, '<' '>' marks and a span limit of 400 (2 000 at
      n = 4096): fewer pairs, so fewer cells with work;
  - lone n = 1024 and n = 4096 sequences, the same two kinds;
  - accessibility: all 20-nt windows of one 2 000-nt sequence as one rnamc_log_partition_batch
    call (1 981 records plus the unconstrained one) against rnamc_bpp_batch on 200 of those records
    (1 982 triangles of 2 000 nt would take 16 GB of host memory), scaled to 1 982.
Prints one JSON line per case.  argv: [--quick] (200 sequences, n = 4096 skipped) [--neutral-only]
(the "active_neutral" cases alone)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from rna_algos_amd.mccaskill_algo import Context  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402
from rna_algos_amd.workloads import batch_lengths, batch_seq, synthetic_seq  # noqa: E402


def constraint_for(n, k):
    """an 'x' window, one bracket pair and a '<' '>' couple, placed by k"""
    c = ["."] * n
    a = (37 * k) % max(1, n - 40)
    for p in range(a, a + min(12, n)):
        c[p] = "x"
    if n >= 60:
        c[n // 4], c[n - n // 4] = "(", ")"
        c[n // 8], c[n - n // 8] = "<", ">"
    return "".join(c)


def neutral_for(n):
    return "<" + "." * (n - 2) + ">"


def alternate(f_plain, f_cons, reps):
    tp, tc = [], []
    for _ in range(reps):
        for f, ts in ((f_plain, tp), (f_cons, tc)):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
    return min(tp), min(tc), tp, tc


def case(ctx, name, seqs, contra, summation, reps, span=400, kind="mixed"):
    ctx.set("summation_mode", summation)
    if kind == "mixed":
        cons = [constraint_for(len(s), k) for k, s in enumerate(seqs)]
    else:
        cons, span = [neutral_for(len(s)) for s in seqs], 0
        a, za = ctx.bpp_batch(seqs, contra, False)
        b, zb = ctx.bpp_batch(seqs, contra, False, cons, span)
        assert all(x.packed.tobytes() == y.packed.tobytes() for x, y in zip(a, b)) and za.tobytes() == zb.tobytes()
    warm = seqs[:50]
    ctx.bpp_batch(warm, contra, False)
    ctx.bpp_batch(warm, contra, False, cons[:50], span)
    tp, tc, all_p, all_c = alternate(lambda: ctx.bpp_batch(seqs, contra, False),
                                     lambda: ctx.bpp_batch(seqs, contra, False, cons, span), reps)
    ctx.set("summation_mode", 0)
    print(json.dumps({"case": name, "constraint": kind, "model": "contra" if contra else "turner",
                      "summation": "tree" if summation else "reference", "n_seqs": len(seqs),
                      "s_plain": round(tp, 4), "s_constrained": round(tc, 4),
                      "ratio": round(tc / tp, 4), "runs_plain": [round(x, 4) for x in all_p],
                      "runs_constrained": [round(x, 4) for x in all_c]}), flush=True)


def accessibility(ctx, contra, reps):
    n, w = 2000, 20
    seq = synthetic_seq(n, 2000)
    cons = [None] + ["." * a + "x" * w + "." * (n - a - w) for a in range(n - w + 1)]
    seqs = [seq] * len(cons)
    ctx.log_partition_batch(seqs[:8], contra, False, cons[:8])
    tb, tl, all_b, all_l = alternate(lambda: ctx.bpp_batch(seqs[:200], contra, False, cons[:200]),
                                     lambda: ctx.log_partition_batch(seqs, contra, False, cons), reps)
    print(json.dumps({"case": "accessibility_2000nt_w20", "model": "contra" if contra else "turner",
                      "windows": n - w + 1, "s_log_partition_batch": round(tl, 4),
                      "windows_per_s": round((n - w + 1) / tl, 1), "s_bpp_batch_200_records": round(tb, 4),
                      "s_bpp_batch_scaled_to_same_records": round(tb * len(seqs) / 200, 3),
                      "runs_log_partition": [round(x, 4) for x in all_l],
                      "runs_bpp": [round(x, 4) for x in all_b]}), flush=True)


def main():
    quick = "--quick" in sys.argv
    ctx = Context(FoldScoreSets.synthetic(1), device=0)
    lens = batch_lengths()[:200 if quick else 1000]
    batch = [batch_seq(s, lengths=lens) for s in range(len(lens))]
    kinds = ["active_neutral"] if "--neutral-only" in sys.argv else ["active_neutral", "mixed"]
    for kind in kinds:
        for contra in (False, True):
            for summation in (0, 1):
                case(ctx, f"batch{len(batch)}_256_2048", batch, contra, summation, 3, kind=kind)
            case(ctx, "n1024", [synthetic_seq(1024, 1024)], contra, 0, 5, kind=kind)
            case(ctx, "n1024", [synthetic_seq(1024, 1024)], contra, 1, 5, kind=kind)
            if not quick:
                case(ctx, "n4096", [synthetic_seq(4096, 4096)], contra, 0, 2, span=2000, kind=kind)
                case(ctx, "n4096", [synthetic_seq(4096, 4096)], contra, 1, 2, span=2000, kind=kind)
    if "--neutral-only" not in sys.argv:
        for contra in (False, True):
            accessibility(ctx, contra, 2)
    ctx.close()


if __name__ == "__main__":
    main()
