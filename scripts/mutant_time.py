"""Time the point-mutation scan on one context (device 0): route (a)
rnamc_mutant_scan against route (b), what a caller had to do before it: the dense entry
(rnamc_bpp_batch_constrained) over the same mutants, 256 at a time into one host buffer, and the
reduction of the contract in numpy (fixed-point squared distance, largest move, paired
probabilities).

    python scripts/mutant_time.py [--n 1000] [--modes 1,0] [--reps 3] [--chunk 256] [--out FILE]

Per summation mode: one warm-up of route (a), --reps repetitions, the median wall time (the entry
returns after its stream is drained: the host clock is fenced by the call itself), once with all
mutants in one staged call of the sweep (the default) and once with "mutant_chunk_nt" set to route
(b)'s --chunk mutants a call; route (b) once (its sweeps are warmed by route (a)'s: same kernels,
same shapes).  Then one more call of (a) with the "profile" knob on: the device time of the
compare and paired kernels (ms_mutant) beside the sweeps'.  The routes' outputs are compared bit
for bit: in summation mode 0 every run of (a) must equal (b); in mode 1 the sweep picks its form per
staged call and group, so there the run of (a) with (b)'s call structure must.  Every line is
printed as soon as it is measured and appended to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rna_algos_amd import _lib, workloads  # noqa: E402
from rna_algos_amd.mccaskill_algo import Context, mutant_plan  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402

Q = float(2 ** 44)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--modes", default="1,0")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=256)
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
    n, chunk = args.n, args.chunk
    seq = workloads.synthetic_seq(n, seed=n)
    pos, base = mutant_plan(seq)
    M = len(pos)
    ctx.bpp_batch([seq[:64]], False, False)  # (context warm-up: module load, streams)
    tri_len = n * (n + 1) // 2
    tri = np.zeros(chunk * tri_len, dtype=np.float32)  # allocated and touched once, outside the timed region
    logz = np.zeros(chunk, dtype=np.float32)
    starts = np.array([d * n - d * (d - 1) // 2 for d in range(n)], np.int64)
    say(f"n {n}  mutants {M}  Turner  | triangles kept on the device {4 * (M + 1) * tri_len} bytes, route (b) moves them "
        f"to the host {chunk} at a time")

    def route_a():
        t0 = time.perf_counter()
        res = ctx.mutant_scan(seq, False, False)
        return time.perf_counter() - t0, res

    def dense(recs, m):
        bases = np.concatenate(recs)
        offs = np.arange(m + 1, dtype=np.uint64) * np.uint64(n)
        out_offs = np.arange(m + 1, dtype=np.uint64) * np.uint64(tri_len)
        _lib.check(L.rnamc_bpp_batch_constrained(ctx._h, m, bases.ctypes.data, offs.ctypes.data, None, 0, 0, 0,
                                                 tri.ctypes.data, out_offs.ctypes.data, logz.ctypes.data))
        return tri[:m * tri_len].reshape(m, tri_len)

    def paired_of(t):
        """rows of triangles -> rows of paired probabilities, in rnamc_bpp_batch_sparse's order"""
        paired = np.zeros((t.shape[0], n), np.float32)
        off = n
        for d in range(1, n):
            add = t[:, off:off + n - d]
            off += n - d
            add = np.where(add > -0.5, add, np.float32(0))
            paired[:, :n - d] += add
            paired[:, d:] += add
        return paired

    def route_b():
        """-> (seconds, log_z, dist2_q, max_dp, max_pair, paired, wt_log_z, wt_paired)"""
        t0 = time.perf_counter()
        wt = dense([seq], 1)[0].copy()
        wt_z = logz[0].copy()
        wt_paired = paired_of(wt[None, :])[0]
        fa = np.where(wt > -0.5, wt, np.float32(0))[n:]
        fa64 = fa.astype(np.float64)
        zs, q, dp, pair, paired = [], [], [], [], []
        for c0 in range(0, M, chunk):
            m = min(chunk, M - c0)
            recs = []
            for x in range(c0, c0 + m):
                r = seq.copy()
                r[pos[x]] = base[x]
                recs.append(r)
            t = dense(recs, m)
            zs.append(logz[:m].copy())
            paired.append(paired_of(t))
            fb = np.where(t > -0.5, t, np.float32(0))[:, n:]
            e = fa64[None, :] - fb.astype(np.float64)
            q.append(np.minimum(np.rint((e * e) * Q), 2.0 * Q).astype(np.int64).sum(axis=1))
            d32 = np.abs(fa[None, :] - fb)
            c = np.argmax(d32, axis=1)  # (the first of equal maxima: the smallest packed index)
            best = d32[np.arange(m), c]
            c = c + n
            d = np.searchsorted(starts, c, side="right") - 1
            i = c - starts[d]
            pr = np.stack([i, i + d], axis=1)
            pr[best <= 0] = -1
            dp.append(best)
            pair.append(pr)
        res = (np.concatenate(zs), np.concatenate(q), np.concatenate(dp), np.concatenate(pair), np.concatenate(paired),
               wt_z, wt_paired)
        return (time.perf_counter() - t0,) + res

    def bits(a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()

    def same_as(res, b):
        """True, or the names of the outputs that differ"""
        zs, q, dp, pair, paired, wt_z, wt_paired = b
        pairs = (("log_z", res.log_z, zs), ("dist2_q", res.dist2_q, q), ("max_dp", res.max_dp, dp),
                 ("max_pair", res.max_pair, pair), ("paired_prob", res.paired_prob, paired),
                 ("wt_paired_prob", res.wt_paired_prob, wt_paired),
                 ("wt_log_z", np.float32(res.wt_log_z), np.float32(wt_z)))
        differ = [name for name, x, y in pairs if not bits(x, y)]
        return True if not differ else "False: " + ", ".join(differ)

    def timed_a(label):
        route_a()  # warm-up: buffers, workspace
        ta = []
        for _ in range(args.reps):
            dt, res = route_a()
            ta.append(dt)
        med = statistics.median(ta)
        say(f"{label} {med:8.3f} s {['%.3f' % t for t in ta]} | result {res.paired_prob.nbytes + 28 * M} bytes")
        return med, res

    failed = False
    for mode in (int(x) for x in args.modes.split(",")):
        ctx.set("summation_mode", mode)
        ctx.set("mutant_chunk_nt", 64 << 20)
        med_a, res = timed_a(f"mode {mode}: (a) rnamc_mutant_scan, all {M} mutants in one staged call")
        # the call structure of route (b): in summation mode 1 the sweep picks its form per staged call and
        # group, so only this run of (a) can share (b)'s bits there
        ctx.set("mutant_chunk_nt", chunk * n)
        med_c, res_c = timed_a(f"mode {mode}: (a) rnamc_mutant_scan, mutant_chunk_nt = {chunk} mutants a staged call")
        ctx.set("mutant_chunk_nt", 64 << 20)
        tb, *b = route_b()
        same, same_c = same_as(res, b), same_as(res_c, b)
        say(f"mode {mode}: (b) dense entry, {chunk} mutants a call, + numpy {tb:8.3f} s | (b) / (a) = {tb / med_a:.2f} "
            f"(one staged call), {tb / med_c:.2f} ({chunk} a staged call) | outputs bit-identical: {same} (one staged call), "
            f"{same_c} ({chunk} a staged call)")
        ctx.set("profile", 1)
        dt, _ = route_a()
        st = ctx.stats()
        ctx.set("profile", 0)
        sweeps = st["ms_inside"] + st["ms_outside"] + st["ms_other"]
        say(f"mode {mode}: profiled call {dt:8.3f} s | sweeps {sweeps:9.1f} ms (inside {st['ms_inside']:.1f}, outside "
            f"{st['ms_outside']:.1f}, finalize {st['ms_other']:.1f}) | compare + paired kernels {st['ms_mutant']:8.2f} ms in "
            f"{st['launches_mutant']} launches = {100 * st['ms_mutant'] / (sweeps + st['ms_mutant']):.2f} % of the device "
            f"time, {100 * st['ms_mutant'] / (1e3 * dt):.2f} % of the call | groups {st['n_groups']}")
        failed = failed or same_c is not True or (mode == 0 and same is not True)
    ctx.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
