"""Time the thresholded sparse pair-probability entry: route (a)
rnamc_bpp_batch_sparse against route (b) rnamc_bpp_batch (dense triangles to host buffers),
alternately in one process on one context (device 0).

    python scripts/sparse_bpp_time.py [--count 1000] [--models turner,contra] [--modes 0,1]
        [--min-probs 0,1e-3,1e-2] [--reps 3] [--out FILE]

Workload: the first --count records of workloads.batch().  Per configuration one warm-up of each
route, then --reps alternating repetitions; the median wall time of each route, the listed pairs
per nucleotide and the bytes each route returns.  Route (a) is called the way a caller does: one
call with arrays of a few entries per nucleotide, a second one only if they were too small (the
line says so).  Every line is printed as soon as it is measured and appended to --out."""
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
from rna_algos_amd.mccaskill_algo import SPARSE_PAIRS_PER_NT, Context, _pack  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1000)
    ap.add_argument("--models", default="turner,contra")
    ap.add_argument("--modes", default="0,1")
    ap.add_argument("--min-probs", default="0,1e-3,1e-2")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    L = _lib.lib()
    ctx = Context(FoldScoreSets.synthetic(1), device=0)
    seqs = workloads.batch(args.count)
    lens, offsets, bases = _pack(seqs)
    ns, nt = len(seqs), int(offsets[-1])
    out_offsets = np.zeros(ns + 1, dtype=np.uint64)
    np.cumsum(lens * (lens + 1) // 2, out=out_offsets[1:])
    # every buffer is allocated and touched once, outside the timed region, for both routes
    dense = np.zeros(int(out_offsets[-1]), dtype=np.float32)
    logz = np.zeros(ns, dtype=np.float32)
    start, count = np.zeros(ns, dtype=np.uint64), np.zeros(ns, dtype=np.uint64)
    paired = np.zeros(nt, dtype=np.float32)
    most = int(np.sum(lens * (lens + 1) // 2 - lens))
    cap = [min(SPARSE_PAIRS_PER_NT * nt, most)]
    lists = [[np.zeros(cap[0], dtype=t) for t in (np.uint32, np.uint32, np.float32)]]
    total = C.c_uint64(0)

    def route_a(contra, min_prob):
        t0 = time.perf_counter()
        calls = 0
        while True:
            pi, pj, pp = lists[0]
            st = L.rnamc_bpp_batch_sparse(ctx._h, ns, bases.ctypes.data, offsets.ctypes.data, None, 0, int(contra), 0,
                                          min_prob, start.ctypes.data, count.ctypes.data, pi.ctypes.data,
                                          pj.ctypes.data, pp.ctypes.data, cap[0], C.byref(total),
                                          paired.ctypes.data, logz.ctypes.data)
            calls += 1
            if st == _lib.ERR_INVALID_ARG and calls == 1 and total.value > cap[0]:
                cap[0] = int(total.value)
                lists[0] = [np.zeros(cap[0], dtype=t) for t in (np.uint32, np.uint32, np.float32)]
                continue
            _lib.check(st)
            return time.perf_counter() - t0, calls

    def route_b(contra):
        t0 = time.perf_counter()
        _lib.check(L.rnamc_bpp_batch(ctx._h, ns, bases.ctypes.data, offsets.ctypes.data, int(contra), 0,
                                     dense.ctypes.data, out_offsets.ctypes.data, logz.ctypes.data))
        return time.perf_counter() - t0

    say(f"batch[:{ns}]: {ns} records, {nt} nt, {int(out_offsets[-1])} triangle cells "
        f"({4 * int(out_offsets[-1])} bytes dense); first-call capacity {cap[0]} entries")
    ctx.bpp_batch([workloads.synthetic_seq(64, 1)], False, False)  # (context warm-up: module load, streams)
    for model in args.models.split(","):
        contra = model == "contra"
        for mode in (int(x) for x in args.modes.split(",")):
            ctx.set("summation_mode", mode)
            for min_prob in (float(x) for x in args.min_probs.split(",")):
                head = f"{model} mode {mode} min_prob {min_prob:g}"
                _, calls = route_a(contra, min_prob)  # warm-up (and, once, the retry that sizes the arrays)
                route_b(contra)
                ta, tb = [], []
                for _ in range(args.reps):
                    dt, c2 = route_a(contra, min_prob)
                    calls = max(calls, c2)
                    ta.append(dt)
                    tb.append(route_b(contra))
                listed = int(total.value)
                bytes_a = 12 * listed + 16 * ns + 4 * nt + 4 * ns
                bytes_b = 4 * int(out_offsets[-1]) + 4 * ns
                present = int(np.count_nonzero(dense > -0.5))
                say(f"{head} | (a) sparse {statistics.median(ta):8.3f} s {['%.3f' % t for t in ta]} "
                    f"| (b) dense {statistics.median(tb):8.3f} s {['%.3f' % t for t in tb]} "
                    f"| listed {listed} = {listed / nt:.3f} per nt (present cells {present} = {present / nt:.1f} per nt) "
                    f"| bytes (a) {bytes_a} (b) {bytes_b} | calls of (a) at most {calls}")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
