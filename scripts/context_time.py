"""Time structural context profiles on one context (device 0): the profile
entry (rnamc_context_profile_batch) against the sweep alone -- rnamc_bpp_batch_sparse with min_prob
above 1 and no lists, which runs the same reference-order sweep and returns nothing but the log
partitions -- on the same batch, in the same process, alternating.

    python scripts/context_time.py [--count 1000] [--longest] [--reps 3] [--out FILE]

The batch is the first --count records of the 10 000-record benchmark batch (workloads.batch_seq),
or with --longest its --count longest records.  Both entries run under Turner and CONTRAfold in
summation mode 0 (the profile entry always does).  Per model: one warm-up of each entry, --reps
alternating repetitions, the median wall times; then one profiled call (profile = 1) of the profile
entry for ms_context over ms_inside + ms_outside.  Every line is printed as soon as it is measured
and appended to --out."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rna_algos_amd import _lib, workloads  # noqa: E402
from rna_algos_amd.mccaskill_algo import Context, _pack  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--longest", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    lengths = workloads.batch_lengths()
    pick = np.argsort(-lengths, kind="stable")[:args.count] if args.longest else np.arange(args.count)
    seqs = [workloads.batch_seq(int(s), lengths=lengths) for s in pick]
    nt = sum(len(s) for s in seqs)
    say(f"{'the ' + str(args.count) + ' longest records' if args.longest else 'batch[:%d]' % args.count}: "
        f"{len(seqs)} records, {nt} nt, lengths {min(map(len, seqs))} .. {max(map(len, seqs))}; summation mode 0")
    ctx = Context(FoldScoreSets.synthetic(1), device=0)
    ctx.bpp_batch([workloads.synthetic_seq(64, seed=64)], False, False)  # (context warm-up: module load, streams)

    def profile_call(contra):
        t0 = time.perf_counter()
        ctx.context_profile_batch(seqs, contra, False)
        return time.perf_counter() - t0

    def sweep_call(contra):
        t0 = time.perf_counter()
        lens, offsets, bases = _pack(seqs)
        total = C.c_uint64(0)
        logz = np.empty(len(seqs), np.float32)
        _lib.check(_lib.lib().rnamc_bpp_batch_sparse(ctx._h, len(seqs), bases.ctypes.data, offsets.ctypes.data, None, 0,
                                                     int(contra), 0, 2.0, None, None, None, None, None, 0,
                                                     C.byref(total), None, logz.ctypes.data))
        assert total.value == 0
        return time.perf_counter() - t0

    for contra in (False, True):
        model = "contra" if contra else "turner"
        profile_call(contra)
        sweep_call(contra)
        tp, ts = [], []
        for _ in range(args.reps):
            tp.append(profile_call(contra))
            ts.append(sweep_call(contra))
        mp, ms = statistics.median(tp), statistics.median(ts)
        say(f"{model} | profile entry {mp:8.3f} s {['%.3f' % t for t in tp]} | sweep alone (sparse entry, min_prob 2, "
            f"no lists) {ms:8.3f} s {['%.3f' % t for t in ts]} | profile / sweep = {mp / ms:.3f}")
        ctx.set("profile", 1)
        profile_call(contra)
        st = ctx.stats()
        ctx.set("profile", 0)
        sweep_ms = st["ms_inside"] + st["ms_outside"]
        say(f"{model} | profile = 1: groups {st['n_groups']} | ms_inside {st['ms_inside']:.1f} ms_outside "
            f"{st['ms_outside']:.1f} ms_other {st['ms_other']:.1f} | ms_context {st['ms_context']:.1f} over "
            f"{st['launches_context']} launches | ms_context / (ms_inside + ms_outside) = "
            f"{st['ms_context'] / sweep_ms:.4f}")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
