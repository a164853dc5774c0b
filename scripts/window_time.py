"""Time windowed local folding on one context (device 0): route (a)
rnamc_bpp_windowed against route (b), what a caller had to do before it: the dense entry
(rnamc_bpp_batch_constrained, max_bp_span = B) over the same windows, 4096 at a time into one host
buffer, and the accumulation of the contract in numpy.

    python scripts/window_time.py [--n 65535] [--window 200] [--strides 10,1] [--span 150] [--mode 1]
        [--reps 3] [--reps-b 1] [--b-max-windows 0] [--out FILE]

Per stride: one warm-up of route (a), --reps repetitions, the median wall time; route (b) --reps-b
times (its first chunk is warmed by route (a)'s sweeps: same kernels, same shapes).  With
--b-max-windows K > 0 route (b) runs on the first K windows only and its time is scaled to the whole
list; the line says so (its cost is linear in the windows: equal groups, equal triangles).  Then
one more call of (a) with the "profile" knob on: the device time of the accumulate, finalise and
paired kernels (ms_window) beside the sweeps'.  The two bands are compared bit for bit.  Route (b)'s
sums go through numpy.bincount in f64, exact while at most 256 windows contain a cell.  Every line
is printed as soon as it is measured and appended to --out."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rna_algos_amd import _lib, workloads  # noqa: E402
from rna_algos_amd.mccaskill_algo import Context, window_plan  # noqa: E402
from rna_algos_amd.utils import FoldScoreSets  # noqa: E402

Q = float(2 ** 44)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65535)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--strides", default="10,1")
    ap.add_argument("--span", type=int, default=150)
    ap.add_argument("--mode", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reps-b", type=int, default=1)
    ap.add_argument("--b-max-windows", type=int, default=0)
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
    n, w = args.n, args.window
    seq = workloads.synthetic_seq(n, seed=n)
    ctx.bpp_batch([seq[:64]], False, False)  # (context warm-up: module load, streams)
    chunk = 4096
    tri_len = w * (w + 1) // 2
    tri = np.zeros(chunk * tri_len, dtype=np.float32)  # allocated and touched once, outside the timed region
    logz = np.zeros(chunk, dtype=np.float32)
    say(f"N {n}  W {w}  L {args.span}  Turner  summation mode {args.mode}")

    def route_a(stride):
        t0 = time.perf_counter()
        res = ctx.bpp_windowed(seq, w, False, False, stride=stride, max_bp_span=args.span)
        return time.perf_counter() - t0, res

    def route_b(starts, band, stride):
        """-> (seconds, band f32[n, B]); starts may be a prefix of the window list (then only timed)"""
        t0 = time.perf_counter()
        wl = min(w, n)
        S = np.zeros((band, n), dtype=np.int64)
        present = np.zeros((band, n), dtype=np.int64)
        offs = np.arange(chunk + 1, dtype=np.uint64) * np.uint64(wl)
        out_offs = np.arange(chunk + 1, dtype=np.uint64) * np.uint64(tri_len)
        for c0 in range(0, len(starts), chunk):
            st = starts[c0:c0 + chunk].astype(np.int64)
            m = len(st)
            bases = np.concatenate([seq[a:a + wl] for a in st])
            _lib.check(L.rnamc_bpp_batch_constrained(ctx._h, m, bases.ctypes.data, offs.ctypes.data, None, band, 0, 0,
                                                     tri.ctypes.data, out_offs.ctypes.data, logz.ctypes.data))
            t = tri[:m * tri_len].reshape(m, tri_len)
            off = wl
            for d in range(1, wl):
                rows = t[:, off:off + wl - d]
                off += wl - d
                if d >= band:
                    continue
                have = rows > -0.5
                q = np.minimum(np.rint(np.where(have, rows, 0).astype(np.float64) * Q), 2.0 * Q)
                idx = (st[:, None] + np.arange(wl - d)[None, :]).ravel()
                S[d] += np.bincount(idx, weights=q.ravel(), minlength=n).astype(np.int64)
                present[d] += np.bincount(idx, weights=have.ravel(), minlength=n).astype(np.int64)
        # denom(i, d) in closed form: grid windows x with x * stride <= i and i + d < x * stride + w, and the last one
        n_grid = (n - wl) // stride + 1
        has_last = (n_grid - 1) * stride + wl < n
        i = np.arange(n, dtype=np.int64)[None, :]
        d = np.arange(band, dtype=np.int64)[:, None]
        j = i + d
        lo = np.where(j >= wl, (j - wl + stride) // stride, 0)
        hi = np.minimum(i // stride, n_grid - 1)
        denom = np.maximum(hi - lo + 1, 0) + (has_last & (i >= n - wl))
        ok = (present > 0) & (denom > 0) & (j < n) & (d >= 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = (S.astype(np.float64) / (denom.astype(np.float64) * Q)).astype(np.float32)
        res = np.ascontiguousarray(np.where(ok, val, np.float32(-1)).astype(np.float32).T)
        return time.perf_counter() - t0, res

    for stride in (int(x) for x in args.strides.split(",")):
        starts, band = window_plan(n, w, stride, args.span)
        assert (w + stride - 1) // stride + 1 <= 256, "route (b) sums in f64: at most 256 windows a cell"
        nw = len(starts)
        route_a(stride)  # warm-up: buffers, workspace
        ta = []
        for _ in range(args.reps):
            dt, res = route_a(stride)
            ta.append(dt)
        med_a = statistics.median(ta)
        say(f"stride {stride}: {nw} windows, band {band} | (a) rnamc_bpp_windowed {med_a:8.3f} s {['%.3f' % t for t in ta]} "
            f"| result {res.band.nbytes} bytes, triangles kept on the device {4 * nw * tri_len} bytes")
        part = starts if args.b_max_windows <= 0 or args.b_max_windows >= nw else starts[:args.b_max_windows]
        tb = []
        for _ in range(args.reps_b):
            dt, ref = route_b(part, band, stride)
            tb.append(dt)
        med_b = statistics.median(tb)
        if len(part) == nw:
            same = bool(np.array_equal(ref.view(np.uint32), res.band.view(np.uint32)))
            say(f"stride {stride}: (b) dense entry + numpy {med_b:8.3f} s {['%.3f' % t for t in tb]} "
                f"| (b) / (a) = {med_b / med_a:.2f} | bands bit-identical: {same}")
        else:
            scaled = med_b * nw / len(part)
            say(f"stride {stride}: (b) dense entry + numpy on the first {len(part)} of {nw} windows {med_b:8.3f} s "
                f"{['%.3f' % t for t in tb]}, scaled to the list (x {nw / len(part):.2f}): {scaled:8.3f} s (NOT measured whole) "
                f"| (b) / (a) = {scaled / med_a:.2f}")
        ctx.set("profile", 1)
        dt, _ = route_a(stride)
        st = ctx.stats()
        ctx.set("profile", 0)
        sweeps = st["ms_inside"] + st["ms_outside"] + st["ms_other"]
        say(f"stride {stride}: profiled call {dt:8.3f} s | sweeps {sweeps:9.1f} ms (inside {st['ms_inside']:.1f}, outside "
            f"{st['ms_outside']:.1f}, finalize {st['ms_other']:.1f}) | window kernels {st['ms_window']:8.2f} ms in "
            f"{st['launches_window']} launches = {100 * st['ms_window'] / (sweeps + st['ms_window']):.2f} % of the device time, "
            f"{100 * st['ms_window'] / (1e3 * dt):.2f} % of the call | groups {st['n_groups']}")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
