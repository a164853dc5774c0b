"""Time alignment folding on one context (device 0): route (a)
rnamc_bpp_alignment with three gammas against route (b), what a caller had to do before it: the dense
entry (rnamc_bpp_batch_constrained) over the ungapped rows in ONE call into one host buffer (in
summation mode 1 the sweep picks its form per staged call, so only the same list of records gives
the same bits), the accumulation of the contract in numpy, and rnamc_centroid_fold_multi on the host
triangle.

    python scripts/align_time.py [--rows 200,1000] [--bases 1500] [--mode 1] [--reps 3] [--skip-b]
        [--out FILE]

The alignment is synthetic and reproducible: every row is workloads.synthetic_seq(bases, bases) with
about 10 % of its bases substituted, laid into bases + 5 % columns of which the row leaves a random
5 % as gaps; every draw comes from workloads.splitmix_u64.  Per size: one warm-up of route (a), --reps
repetitions, the median wall time; route (b) once (its sweeps are warmed by route (a)'s: same kernels,
same shapes; its host buffer is allocated and touched outside the timed region).  The two triangles
and the folds are compared bit for bit.  The gammas are 2, 8 and 32: the averaged probabilities of
this diffuse synthetic family stay below 0.1, so smaller gammas give empty folds that never reach the
(max,+) fill.  --skip-b leaves route (b)
out (kernel-trace runs: scripts/prof_align.sh).  Every line is printed as soon as it is measured and
appended to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rna_algos_amd import _lib, workloads  # noqa: E402
from rna_algos_amd.centroid_fold import centroid_fold_multi, get_fold_str  # noqa: E402
from rna_algos_amd.mccaskill_algo import BppMatrix, Context, bpp_len  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402

Q = float(2 ** 44)
GAP = 4
GAMMAS = (2.0, 8.0, 32.0)


def synthetic_alignment(n_rows, n_bases):
    """-> u8 (n_rows, n_cols): the seed sequence with ~10 % substitutions per row, ~5 % gap columns per row"""
    seed_seq = workloads.synthetic_seq(n_bases, seed=n_bases)
    n_gaps = n_bases // 20
    n_cols = n_bases + n_gaps
    rows = np.full((n_rows, n_cols), GAP, np.uint8)
    for s in range(n_rows):
        u = workloads.splitmix_u64((n_bases << 20) + s, 2 * n_bases + n_cols)
        seq = seed_seq.copy()
        hit = (u[:n_bases] % np.uint64(10)) == 0
        # a substitution is one of the three OTHER bases
        seq[hit] = (seq[hit] + 1 + (u[n_bases:2 * n_bases][hit] % np.uint64(3)).astype(np.uint8)) % 4
        gaps = np.argsort(u[2 * n_bases:], kind="stable")[:n_gaps]  # the columns with the smallest draws
        keep = np.ones(n_cols, bool)
        keep[gaps] = False
        rows[s, keep] = seq
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="200,1000")
    ap.add_argument("--bases", type=int, default=1500)
    ap.add_argument("--mode", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-b", action="store_true")
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
    ctx.set("summation_mode", args.mode)
    nb = args.bases
    ctx.bpp_batch([workloads.synthetic_seq(64, seed=64)], False, False)  # (context warm-up: module load, streams)
    say(f"rows of {nb} bases  Turner  summation mode {args.mode}  gammas {list(GAMMAS)}")
    tri_len = bpp_len(nb)
    # packed cell -> (i, j) of a record of nb bases, once
    d_of = np.repeat(np.arange(nb, dtype=np.int64), np.arange(nb, 0, -1))
    i_of = np.arange(tri_len, dtype=np.int64) - (d_of * nb - d_of * (d_of - 1) // 2)
    pair = d_of >= 1
    i_of, j_of = i_of[pair], (i_of + d_of)[pair]

    def route_a(rows):
        t0 = time.perf_counter()
        res = ctx.bpp_alignment(rows, False, False, GAMMAS)
        return time.perf_counter() - t0, res

    def route_b(rows, tri, logz):
        """-> (seconds, avg f32 triangle, folds); tri, logz: the host buffers of the dense entry"""
        t0 = time.perf_counter()
        n_rows, n_cols = rows.shape
        S = np.zeros(bpp_len(n_cols), dtype=np.int64)
        present = np.zeros(bpp_len(n_cols), dtype=np.uint32)
        offs = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(nb)
        out_offs = np.arange(n_rows + 1, dtype=np.uint64) * np.uint64(tri_len)
        bases = rows[rows != GAP]
        _lib.check(L.rnamc_bpp_batch_constrained(ctx._h, n_rows, bases.ctypes.data, offs.ctypes.data, None, 0, 0, 0,
                                                 tri.ctypes.data, out_offs.ctypes.data, logz.ctypes.data))
        t_dense = time.perf_counter() - t0
        for s in range(n_rows):
            cells = tri[s * tri_len:(s + 1) * tri_len][pair]
            cmap = np.nonzero(rows[s] != GAP)[0].astype(np.int64)
            have = cells > -0.5
            q = np.minimum(np.rint(cells[have].astype(np.float64) * Q), 2.0 * Q).astype(np.int64)
            ci, cj = cmap[i_of[have]], cmap[j_of[have]]
            dd = cj - ci
            at = dd * n_cols - dd * (dd - 1) // 2 + ci  # (distinct inside one row)
            S[at] += q
            present[at] += 1
        val = (S.astype(np.float64) / (np.float64(n_rows) * Q)).astype(np.float32)
        avg = np.where(present > 0, val, np.float32(-1)).astype(np.float32)
        avg[:n_cols] = -1
        folds = centroid_fold_multi(ctx, BppMatrix(n_cols, avg), n_cols, GAMMAS)
        folds = [(get_fold_str(f, n_cols), np.float32(f.expect_accuracy)) for f in folds]
        return time.perf_counter() - t0, t_dense, avg, folds

    for n_rows in (int(x) for x in args.rows.split(",")):
        rows = synthetic_alignment(n_rows, nb)
        n_cols = rows.shape[1]
        assert np.all((rows != GAP).sum(axis=1) == nb)
        route_a(rows)  # warm-up: buffers, workspace
        ta = []
        for _ in range(args.reps):
            dt, res = route_a(rows)
            ta.append(dt)
        med_a = statistics.median(ta)
        st = ctx.stats()
        say(f"{n_rows} x {n_cols}: (a) rnamc_bpp_alignment {med_a:8.3f} s {['%.3f' % t for t in ta]} | groups "
            f"{st['n_groups']} | result {4 * bpp_len(n_cols)} bytes to the host, row triangles kept on the device "
            f"{4 * n_rows * tri_len} bytes, accumulators and result on the device {16 * bpp_len(n_cols)} bytes | pairs "
            f"in the folds {[db.count('(') for db, _ in res.folds]}")
        if args.skip_b:
            continue
        tri = np.zeros(n_rows * tri_len, dtype=np.float32)  # allocated and touched once, outside the timed region
        tb, t_dense, avg, folds = route_b(rows, tri, np.zeros(n_rows, dtype=np.float32))
        tri_bytes = tri.nbytes
        del tri
        same = np.asarray(res.bpp.packed).tobytes() == avg.tobytes()
        same_folds = [(db, np.float32(a).tobytes()) for db, a in res.folds] == [(db, a.tobytes()) for db, a in folds]
        say(f"{n_rows} x {n_cols}: (b) dense entry + numpy + centroid_fold_multi {tb:8.3f} s (the dense entry alone "
            f"{t_dense:.3f} s, {tri_bytes} bytes to the host) | (b) / (a) = "
            f"{tb / med_a:.2f} | triangles bit-identical: {same} | folds identical: {same_folds}")
        assert same and same_folds
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
