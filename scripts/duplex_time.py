"""Time RNA-RNA duplex folding on one context (device 0): one 22-nt query
against the first --count records of the 10 000-record benchmark batch (workloads.batch_seq), as
rnamc_duplex_batch runs it.

    python scripts/duplex_time.py [--count 1000] [--reps 3] [--ref 20] [--out FILE] [--trace N]

Under Turner and CONTRAfold, with and without match_probs (the scan form keeps every nA x nB matrix
on the device): one warm-up, then --reps repetitions, the median wall time of the whole call (packing,
upload, sweeps, copies back).  Then the sweeps' share of it: the C entry alone on packed arguments,
with outputs that need one sweep more each time (ln Z alone: the inside sweep; with the bound
probabilities: inside and outside; with the best scores: all three); the differences are the sweeps'
wall times.  For orientation only, the f64 numpy evaluation of the test helper
(tests/duplex_ref.py) on the first --ref targets, scaled to the count.  Every line is printed as soon
as it is measured and appended to --out.

--trace N runs nothing but N + 1 calls of the scan form under Turner (the first is the warm-up) and
prints their wall times: the run to put under a kernel trace, whose kernel durations over N + 1 calls
against these wall times give the kernels' share of a call."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from rna_algos_amd import _lib, workloads  # noqa: E402
from rna_algos_amd.duplex import _duplex_batch  # noqa: E402
from rna_algos_amd.mccaskill_algo import Context, _pack  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref", type=int, default=20, help="targets the f64 numpy reference is timed on (0: skip)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0, metavar="N")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    lengths = workloads.batch_lengths()
    targets = [workloads.batch_seq(s, lengths=lengths) for s in range(args.count)]
    query = workloads.synthetic_seq(22, seed=22)
    seqs = [query] + targets
    pairs = [(0, t + 1) for t in range(len(targets))]
    cells = sum(22 * len(t) for t in targets)
    say(f"query 22 nt x batch[:{args.count}]: {len(targets)} targets, {sum(map(len, targets))} nt, lengths "
        f"{min(map(len, targets))} .. {max(map(len, targets))}; {cells} cells")
    params = FoldScoreSets.synthetic(1)
    ctx = Context(params, device=0)
    ctx.bpp_batch([workloads.synthetic_seq(64, seed=64)], False, False)  # (context warm-up: module load, streams)
    entry = _lib.lib().rnamc_duplex_batch

    def full(contra, want_probs):
        t0 = time.perf_counter()
        _duplex_batch(entry, ctx._h, seqs, pairs, contra, want_probs=want_probs)
        return time.perf_counter() - t0

    if args.trace:
        ts = [full(False, False) for _ in range(args.trace + 1)]
        say(f"turner | without match_probs | {args.trace + 1} calls, wall ms {['%.2f' % (t * 1e3) for t in ts]}")
        ctx.close()
        return 0

    lens, offsets, bases = _pack([np.ascontiguousarray(s, dtype=np.uint8) for s in seqs])
    pa = np.zeros(len(pairs), np.uint32)
    pb = np.arange(1, len(pairs) + 1, dtype=np.uint32)
    boff = np.zeros(len(pairs) + 1, np.uint64)
    np.cumsum(22 + lens[1:], out=boff[1:])
    logz = np.empty(len(pairs), np.float32)
    bound = np.empty(int(boff[-1]), np.float32)
    best = np.empty(len(pairs), np.float32)

    def raw(contra, with_bound, with_best):
        """the C entry alone on packed arguments: ln Z (inside sweep), + bound probabilities (outside
        sweep), + best scores (max-plus sweep, no traceback)"""
        t0 = time.perf_counter()
        _lib.check(entry(ctx._h, len(seqs), bases.ctypes.data, offsets.ctypes.data, len(pairs), pa.ctypes.data,
                         pb.ctypes.data, int(contra), None, None,
                         bound.ctypes.data if with_bound else None, bound.ctypes.data if with_bound else None,
                         boff.ctypes.data, logz.ctypes.data, None, None, best.ctypes.data if with_best else None))
        return time.perf_counter() - t0

    def med(fn, *a):
        fn(*a)
        ts = [fn(*a) for _ in range(args.reps)]
        return statistics.median(ts), ts

    for contra in (False, True):
        model = "contra" if contra else "turner"
        for want_probs in (False, True):
            m, ts = med(full, contra, want_probs)
            say(f"{model} | {'with' if want_probs else 'without'} match_probs | wall {m * 1e3:8.2f} ms "
                f"{['%.2f' % (t * 1e3) for t in ts]} | {cells / m / 1e6:.1f} Mcells/s")
        t1, _ = med(raw, contra, False, False)
        t2, _ = med(raw, contra, True, False)
        t3, _ = med(raw, contra, True, True)
        say(f"{model} | C entry alone: ln Z {t1 * 1e3:.2f} ms | + bound probabilities {t2 * 1e3:.2f} ms | + best "
            f"scores {t3 * 1e3:.2f} ms -> inside {t1 * 1e3:.2f}, outside {(t2 - t1) * 1e3:.2f}, max-plus "
            f"{(t3 - t2) * 1e3:.2f} ms (each 22 launches and its reduction)")
    ctx.close()
    if args.ref:
        import duplex_ref as R
        t0 = time.perf_counter()
        for t in targets[:args.ref]:
            R.Recurrences(R.Scores(params, query, t, False))
        dt = time.perf_counter() - t0
        say(f"for orientation: tests/duplex_ref.py (oracle scores + f64 numpy recurrences, one CPU core) on {args.ref} "
            f"targets {dt:.2f} s -> {dt / args.ref * len(targets):.1f} s for {len(targets)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
