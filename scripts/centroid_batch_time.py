"""Time batched centroid folding: route (a) rnamc_centroid_fold_batch against
route (b) rnamc_bpp_batch followed by rnamc_centroid_fold_multi per record, alternately in one
process on one context (device 0), with the launch counts of rnamc_ctx_stats.

    python scripts/centroid_batch_time.py [--count 1000] [--long 4096] [--models turner,contra]
        [--modes 0,1] [--thresholds 18,1] [--reps 1] [--routes a,b] [--out FILE]

Workloads: the first --count records of workloads.batch() (0 skips it) and one record of --long nt
(0 skips it).  Every line is printed as soon as it is measured and appended to --out."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rna_algos_amd import workloads  # noqa: E402
from rna_algos_amd.centroid_fold import MAX_POW_2, MIN_POW_2, centroid_fold_multi  # noqa: E402
from rna_algos_amd.mccaskill_algo import Context  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402

GRID = [2.0 ** k for k in range(MIN_POW_2, MAX_POW_2 + 1)]


def launches(st):
    return int(st["launches_inside"] + st["launches_outside"] + st["launches_other"])


def route_a(ctx, seqs, gammas, contra):
    t0 = time.perf_counter()
    folds, _ = ctx.centroid_fold_batch(seqs, gammas, contra, False)
    dt = time.perf_counter() - t0
    st = ctx.stats()
    return dt, launches(st), int(st["n_groups"]), [[f[0] for f in row] for row in folds]


def route_b(ctx, seqs, gammas, contra):
    from rna_algos_amd.centroid_fold import get_fold_str
    t0 = time.perf_counter()
    mats, _ = ctx.bpp_batch(seqs, contra, False)
    t1 = time.perf_counter()
    st = ctx.stats()
    folds = [centroid_fold_multi(ctx, m, len(s), gammas) for s, m in zip(seqs, mats)]
    dt = time.perf_counter() - t0
    # (rnamc_centroid_fold_multi makes n - 1 launches per record by construction; it keeps no statistics)
    n_launch = launches(st) + sum(len(s) - 1 for s in seqs)
    strs = [[get_fold_str(f, len(s)) for f in row] for s, row in zip(seqs, folds)]
    return dt, n_launch, int(st["n_groups"]), strs, t1 - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--long", type=int, default=4096)
    ap.add_argument("--models", default="turner,contra")
    ap.add_argument("--modes", default="0,1")
    ap.add_argument("--thresholds", default="18,1")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--routes", default="a,b")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    ctx = Context(FoldScoreSets.synthetic(1), device=0)
    sets = []
    if args.count > 0:
        sets.append((f"batch[:{args.count}]", workloads.batch(args.count)))
    if args.long > 0:
        sets.append((f"n={args.long}", [workloads.synthetic_seq(args.long, args.long)]))
    routes = args.routes.split(",")
    ctx.bpp_batch([workloads.synthetic_seq(64, 1)], False, False)  # (context warm-up: module load, streams)
    for name, seqs in sets:
        nt = sum(len(s) for s in seqs)
        for model in args.models.split(","):
            contra = model == "contra"
            for mode in (int(x) for x in args.modes.split(",")):
                ctx.set("summation_mode", mode)
                for ng in (int(x) for x in args.thresholds.split(",")):
                    gammas = GRID if ng == 18 else [4.0] if ng == 1 else GRID[:ng]
                    head = f"{name} ({len(seqs)} records, {nt} nt) {model} mode {mode} {len(gammas)} thresholds"
                    last = {}
                    for rep in range(args.reps):
                        if "a" in routes:
                            dt, nl, groups, strs = route_a(ctx, seqs, gammas, contra)
                            last["a"] = strs
                            say(f"{head} | (a) centroid_fold_batch: {dt:9.3f} s, {nl} launches, {groups} groups")
                        if "b" in routes:
                            dt, nl, groups, strs, t_bpp = route_b(ctx, seqs, gammas, contra)
                            last["b"] = strs
                            say(f"{head} | (b) bpp_batch + centroid_fold_multi per record: {dt:9.3f} s "
                                f"(bpp_batch {t_bpp:.3f} s), {nl} launches, {groups} groups")
                    if mode == 0 and len(last) == 2:  # (mode 0 is deterministic across calls)
                        say(f"{head} | strings identical: {last['a'] == last['b']}")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
