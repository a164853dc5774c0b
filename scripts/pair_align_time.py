"""Time pairwise alignment on the device: route (a) pair_align_batch (lists,
marginals and alignments made off the device-resident matrices) against route (b), what a caller has
without it: durbin_algo_batch for the same pairs (every dense matrix to the host), numpy
thresholding, and match_align per pair and gamma on the host.  One process, one context (device 0),
the two routes alternating after a warm-up; bytes returned by each route beside the times.

    python scripts/pair_align_time.py [--records 200] [--long 1500] [--reps 3] [--routes a,b]
        [--min-prob 0.01] [--out FILE]

Workloads: all pairs of the first --records records of tests/golden/sampled_trnas.fa, made up to that
number with synthetic records of 60-120 nt (fixed seed), and one pair of two --long nt sequences
(0 skips either).  Every line is printed as soon as it is measured and appended to --out."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rna_algos_amd.durbin_algo import AlignScores, durbin_algo_batch, with_pseudo_bases  # noqa: E402
from rna_algos_amd.mccaskill_algo import Context  # noqa: E402
from rna_algos_amd.pair_align import match_align, pair_align_batch  # noqa: E402
from rna_algos_amd.utils import EXAMPLE_FASTA_FILE_PATH, FoldScoreSets, read_fasta  # noqa: E402

GAMMAS = (1.5, 2.0, 8.0)


def records(count):
    seqs = [s for _, s in read_fasta(EXAMPLE_FASTA_FILE_PATH)][:count]
    rng = np.random.default_rng(200)
    while len(seqs) < count:
        seqs.append(rng.integers(0, 4, int(rng.integers(60, 121))).astype(np.uint8))
    return [with_pseudo_bases(s) for s in seqs]


def route_a(ctx, seqs, pairs, scores, min_prob):
    t0 = time.perf_counter()
    res = pair_align_batch(seqs, pairs, scores, gammas=GAMMAS, min_prob=min_prob, ctx=ctx)
    dt = time.perf_counter() - t0
    nbytes = sum(12 * len(r.p) + 4 * (r.n1 + r.n2) + len(GAMMAS) * (4 * r.n1 + 8) + 16 for r in res)
    return dt, nbytes, res


def route_b(ctx, seqs, pairs, scores, min_prob):
    t0 = time.perf_counter()
    mats = durbin_algo_batch(seqs, pairs, scores, ctx)
    t1 = time.perf_counter()
    out = []
    thr = np.float32(min_prob)
    for m in mats:
        ii, jj = np.nonzero((m > 0) & (m >= thr))
        # (the sums of numpy are pairwise: the marginals of this route are not the stage's bits)
        out.append((ii, jj, m[ii, jj], m.sum(axis=1), m.sum(axis=0), [match_align(m, g) for g in GAMMAS]))
    dt = time.perf_counter() - t0
    return dt, sum(4 * m.size for m in mats), out, t1 - t0


def agree(res_a, res_b):
    for r, (ii, jj, pp, _, _, al) in zip(res_a, res_b):
        if not (np.array_equal(r.i, ii) and np.array_equal(r.j, jj) and np.array_equal(r.p, pp)):
            return False
        for g, (mate, count, acc) in enumerate(al):
            if not (np.array_equal(r.mate[g], mate) and r.n_matched[g] == count and r.expect_accuracy[g] == acc):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200)
    ap.add_argument("--long", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--routes", default="a,b")
    ap.add_argument("--min-prob", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    ctx = Context(FoldScoreSets.new(0.0), device=0)
    scores = AlignScores.new(0.0)
    scores.transfer()
    sets = []
    if args.records > 1:
        seqs = records(args.records)
        sets.append((f"all pairs of {len(seqs)} records",
                     seqs, [(a, b) for a in range(len(seqs)) for b in range(a + 1, len(seqs))]))
    if args.long > 0:
        rng = np.random.default_rng(1500)
        sets.append((f"one pair of {args.long} x {args.long}",
                     [with_pseudo_bases(rng.integers(0, 4, args.long)) for _ in range(2)], [(0, 1)]))
    routes = args.routes.split(",")
    warm = records(8)
    # (context warm-up: module load, streams, both routes once)
    pair_align_batch(warm, [(0, 1), (2, 3)], scores, gammas=GAMMAS, min_prob=args.min_prob, ctx=ctx)
    durbin_algo_batch(warm, [(0, 1), (2, 3)], scores, ctx)
    for name, seqs, pairs in sets:
        cells = sum(len(seqs[a]) * len(seqs[b]) for a, b in pairs)
        head = f"{name} ({len(pairs)} pairs, {cells} cells), {len(GAMMAS)} gammas, min_prob {args.min_prob}"
        best, last = {}, {}
        for rep in range(args.reps):
            if "a" in routes:
                dt, nbytes, last["a"] = route_a(ctx, seqs, pairs, scores, args.min_prob)
                best["a"] = min(best.get("a", dt), dt)
                say(f"{head} | (a) pair_align_batch: {dt:9.3f} s, {nbytes} bytes returned")
            if "b" in routes:
                dt, nbytes, last["b"], t_hmm = route_b(ctx, seqs, pairs, scores, args.min_prob)
                best["b"] = min(best.get("b", dt), dt)
                say(f"{head} | (b) durbin_algo_batch + numpy + match_align per pair: {dt:9.3f} s "
                    f"(durbin_algo_batch {t_hmm:.3f} s), {nbytes} bytes returned")
        if len(last) == 2:
            say(f"{head} | best of {args.reps}: (a) {best['a']:.3f} s, (b) {best['b']:.3f} s, "
                f"(b) / (a) = {best['b'] / best['a']:.2f}; lists and alignments identical: "
                f"{agree(last['a'], last['b'])}")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
