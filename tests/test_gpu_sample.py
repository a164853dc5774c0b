"""Boltzmann sampling on the GPU (rnamc_sample_batch): the sampled distribution against the exact
one (oracle/bruteforce.c, oracle/mccaskill_exact.c), every sample's log-weight against the host
scorer (rnamc_structure_score), determinism and independence of the counter-based RNG, edge cases
and the public layers."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN, CLOSE, DOT = ord("("), ord(")"), ord(".")


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def pairs_of(row):
    st, out = [], []
    for q, ch in enumerate(bytes(row)):
        if ch == OPEN:
            st.append(q)
        elif ch == CLOSE:
            assert st, "unbalanced"
            out.append((st.pop(), q))
        else:
            assert ch == DOT
    assert not st, "unbalanced"
    return out


def unique_rows(rows):
    u, cnt = np.unique(rows, axis=0, return_counts=True)
    return u, cnt


def pair_freq(rows):
    n = rows.shape[1]
    f = np.zeros((n, n))
    u, cnt = unique_rows(rows)
    for r, c in zip(u, cnt):
        for i, j in pairs_of(r):
            f[i, j] += c
    return f / rows.shape[0]


def score(params, seq, row, contra, short):
    from rna_algos_amd.mccaskill_algo import structure_score
    return structure_score(seq, bytes(row).decode(), contra, short, params)


def sigma(p, n):
    return np.sqrt(np.clip(p * (1 - p), 0, None) / n)


DIST_SEQS = [O.splitmix_seq(16 + k % 7, 9100 + k) for k in range(8)]


@pytest.mark.parametrize("contra", [False, True])
def test_exact_distribution_small(ctx, params, contra):
    N = 200_000
    rows, weights, logz = ctx.sample_batch(DIST_SEQS, N, contra, False, seed=11)
    for seq, r in zip(DIST_SEQS, rows):
        lz, bp, _ = O.bruteforce(params.ptr, seq, contra, False)
        f = pair_freq(r)
        bound = 5 * sigma(bp, N) + 1e-3
        assert np.all(np.abs(f - bp) <= bound), f"max excess {np.max(np.abs(f - bp) - bound)}"
        u, cnt = unique_rows(r)
        for x in np.argsort(-cnt)[:5]:
            fs = cnt[x] / N
            ps = math.exp(score(params, seq, u[x], contra, False) - lz)
            assert abs(fs - ps) <= 5 * math.sqrt(ps * (1 - ps) / N) + 1e-3, (bytes(u[x]), fs, ps)


@pytest.mark.parametrize("contra", [False, True])
def test_weights_and_validity_trnas(ctx, params, trnas, contra):
    seqs = [s for _, s in trnas]
    N = 2000
    rows, weights, logz = ctx.sample_batch(seqs, N, contra, False, seed=3)
    mats, logz_bpp = ctx.bpp_batch(seqs, contra, False)
    assert logz.tobytes() == logz_bpp.tobytes()
    worst = 0.0
    for seq, r, w, m in zip(seqs, rows, weights, mats):
        u, inv = np.unique(r, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for x, row in enumerate(u):
            prs = pairs_of(row)
            for i, j in prs:
                assert m[i, j] >= 0.0, f"sampled pair ({i},{j}) is not in the bpp key set"
            ref = score(params, seq, row, contra, False)
            assert math.isfinite(ref)
            # The kernel adds the sample's loop scores in f32, one rounding per local score (at most
            # three per pair: its loop, its branch term, its closing term; plus the exterior's), the
            # scorer the same f32 scores in f64.  Each rounding is <= ulp/2 of a partial sum, which
            # stays within max(1, |w|) times a small factor: 4 (n_pairs + 1) ulps.
            tol = 4 * (len(prs) + 1) * float(np.spacing(np.float32(max(1.0, abs(ref)))))
            got = w[inv == x]
            assert np.all(got == got[0]), "one structure, several log-weights"
            worst = max(worst, abs(float(got[0]) - ref) / tol)
            assert abs(float(got[0]) - ref) <= tol, (bytes(row), float(got[0]), ref, tol)
    print(f"log-weight error: at most {worst:.3f} of the bound")


@pytest.mark.parametrize("contra", [False, True])
def test_marginals_at_size(ctx, params, trnas, contra):
    from rna_algos_amd.mccaskill_algo import bpp_index
    seqs = [s for _, s in trnas]
    N = 20_000
    rows, _, _ = ctx.sample_batch(seqs, N, contra, False, seed=5)
    for seq, r in zip(seqs, rows):
        n = len(seq)
        ex, _ = O.exact_bpp(params.ptr, seq, contra, False)
        p = np.zeros((n, n))
        iu = np.triu_indices(n)
        p[iu] = np.array([max(0.0, ex[bpp_index(n, i, j)]) for i, j in zip(*iu)])
        f = pair_freq(r)
        assert np.all(np.abs(f - p) <= 5 * sigma(p, N) + 3e-3), float(np.max(np.abs(f - p)))
        counts = (r == OPEN).sum(axis=1)
        sd = float(counts.std())
        assert abs(counts.mean() - p.sum()) <= 5 * sd / math.sqrt(N) + 0.01 * p.sum()


def test_determinism_and_independence(ctx, params, trnas):
    seqs = [s for _, s in trnas]
    extra = [O.splitmix_seq(40 + 13 * k, 77 + k) for k in range(5)]
    for contra in (False, True):
        a = ctx.sample_batch(seqs, 300, contra, False, seed=42)
        b = ctx.sample_batch(seqs, 300, contra, False, seed=42)
        for x, y in zip(a[0], b[0]):
            assert x.tobytes() == y.tobytes()
        assert a[1].tobytes() == b[1].tobytes()
        ctx.set("group_max_seqs", 1)
        try:
            g = ctx.sample_batch(seqs, 300, contra, False, seed=42)
        finally:
            ctx.set("group_max_seqs", 8192)
        for x, y in zip(a[0], g[0]):
            assert x.tobytes() == y.tobytes()
        assert a[1].tobytes() == g[1].tobytes()
        # sequence 2 with other neighbours (longer and shorter ones) at the same batch index
        other = [extra[0], extra[3], seqs[2], extra[4], extra[1]]
        o = ctx.sample_batch(other, 300, contra, False, seed=42)
        assert o[0][2].tobytes() == a[0][2].tobytes() and o[1][2].tobytes() == a[1][2].tobytes()
        ctx.set("summation_mode", 1)
        try:
            t = ctx.sample_batch(seqs, 300, contra, False, seed=42)
        finally:
            ctx.set("summation_mode", 0)
        for x, y in zip(a[0], t[0]):
            assert x.tobytes() == y.tobytes()
        assert a[1].tobytes() == t[1].tobytes()
        d = ctx.sample_batch(seqs, 300, contra, False, seed=43)
        assert any(x.tobytes() != y.tobytes() for x, y in zip(a[0], d[0]))


def raw_sample(ctx, seqs, n_samples, structs=True):
    from rna_algos_amd import _lib
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    bases = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs])
    rows = np.zeros(max(1, int(offsets[-1]) * n_samples), dtype=np.uint8)
    w = np.zeros(max(1, len(seqs) * n_samples), dtype=np.float32)
    st = _lib.lib().rnamc_sample_batch(ctx._h, len(seqs), bases.ctypes.data, offsets.ctypes.data,
                                       0, 0, n_samples, 1, rows.ctypes.data if structs else None,
                                       w.ctypes.data, None)
    return st, rows, w


def test_edges(ctx, params):
    from rna_algos_amd import _lib
    short = np.array([2, 0, 0, 1], dtype=np.uint8)  # n < 5
    homo = np.zeros(30, dtype=np.uint8)
    ext_unpair = np.float32(params.field("contra.external_score_unpair")[0])
    for contra in (False, True):
        rows, w, _ = ctx.sample_batch([short, homo], 50, contra, False, seed=1)
        for r, ws, seq in zip(rows, w, [short, homo]):
            assert np.all(r == DOT)
            want = np.float32(ext_unpair * np.float32(len(seq))) if contra else np.float32(0.0)
            assert np.all(ws == want)
    st, rows, w = raw_sample(ctx, [homo], 0)
    assert st == _lib.OK and not rows.any() and not w.any()
    st, _, _ = raw_sample(ctx, [np.array([0, 1, 4, 2], dtype=np.uint8)], 4)
    assert st == _lib.ERR_INVALID_BASE
    st, _, _ = raw_sample(ctx, [np.zeros(65536, dtype=np.uint8)], 1)
    assert st == _lib.ERR_SEQ_TOO_LONG
    st, _, _ = raw_sample(ctx, [homo], 4, structs=False)
    assert st == _lib.ERR_INVALID_ARG
    big = O.splitmix_seq(4096, 4096)
    for contra in (False, True):
        rows, w, logz = ctx.sample_batch([big], 64, contra, False, seed=9)
        assert np.all(np.isfinite(w))
        for r in rows[0]:
            prs = pairs_of(r)
            assert all((int(big[i]) + int(big[j])) in (3, 5) and j - i >= 4 for i, j in prs)


def test_interfaces(ctx, params, trnas, tmp_path):
    from rna_algos_amd.mccaskill_algo import sample_structures, structure_score
    seq = trnas[0][1]
    for contra in (False, True):
        rows, w, logz = ctx.sample_batch([seq], 40, contra, False, seed=8)
        got, lz = sample_structures(seq, 40, contra, False, params, seed=8)
        assert lz == float(logz[0])
        assert [db for db, _ in got] == [bytes(r).decode() for r in rows[0]]
        assert [x for _, x in got] == [float(x) for x in w[0]]
        db = got[0][0]
        ref = C.c_double()
        from rna_algos_amd import _lib
        s = np.ascontiguousarray(seq, dtype=np.uint8)
        _lib.check(_lib.lib().rnamc_structure_score(params.ptr, s.ctypes.data, len(s), db.encode(),
                                                    int(contra), 0, C.byref(ref)))
        assert structure_score(seq, db, contra, False, params) == ref.value
    fa = os.path.join(ROOT, "tests", "golden", "sampled_trnas.fa")
    out = tmp_path / "samples.txt"
    subprocess.run([sys.executable, "-m", "rna_algos_amd.bin.sample_fold", "-i", fa, "-o", str(out),
                    "-n", "7", "-s", "3", "--synthetic-tables", "1"], cwd=ROOT, check=True, timeout=300)
    lines = out.read_text().splitlines()
    assert len(lines) == len(trnas) * 8
    for k, (_, s) in enumerate(trnas):
        assert lines[8 * k] == f">{k}"
        for ln in lines[8 * k + 1:8 * k + 8]:
            db, lp = ln.split("\t")
            assert len(db) == len(s)
            pairs_of(db.encode())
            assert float(lp) <= 1e-3
