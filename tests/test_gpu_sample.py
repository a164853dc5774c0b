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
import short_pairs as SP

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


def short_mass(f):
    """sampled pairs of span 1, 2, 3 per structure, from a pair-frequency matrix.  The callers assert from the
    oracle that the exact ensemble expects at least 1 and from the samples that they hold more than 0.5: half
    of that, far outside the sampling error of 20 000 draws and more, and 0 for a build that ignores the flag"""
    return float(sum(np.trace(f, offset=d) for d in (1, 2, 3)))


def sigma(p, n):
    return np.sqrt(np.clip(p * (1 - p), 0, None) / n)


DIST_SEQS = [O.splitmix_seq(16 + k % 7, 9100 + k) for k in range(8)]


def check_exact_distribution_small(ctx, params, contra, short=False):
    N = 200_000
    rows, weights, logz = ctx.sample_batch(DIST_SEQS, N, contra, short, seed=11)
    for seq, r in zip(DIST_SEQS, rows):
        lz, bp, _ = O.bruteforce(params.ptr, seq, contra, short)
        f = pair_freq(r)
        if short:  # the pairs that exist under the flag alone are sampled
            assert short_mass(f) > 0.5, short_mass(f)
        bound = 5 * sigma(bp, N) + 1e-3
        assert np.all(np.abs(f - bp) <= bound), f"max excess {np.max(np.abs(f - bp) - bound)}"
        u, cnt = unique_rows(r)
        for x in np.argsort(-cnt)[:5]:
            fs = cnt[x] / N
            ps = math.exp(score(params, seq, u[x], contra, short) - lz)
            assert abs(fs - ps) <= 5 * math.sqrt(ps * (1 - ps) / N) + 1e-3, (bytes(u[x]), fs, ps)


@pytest.mark.parametrize("contra", [False, True])
def test_exact_distribution_small(ctx, params, contra):
    check_exact_distribution_small(ctx, params, contra)


def test_exact_distribution_small_short_hairpins(ctx, params):
    """allows_short_hairpins = 1 (CONTRAfold): the brute-force ensemble then holds 1.07 .. 3.77 pairs of
    span < 4 per structure on these sequences (asserted from the oracle: at least 1)"""
    SP.assert_input_has_short_pairs(params, DIST_SEQS)
    check_exact_distribution_small(ctx, params, *SP.MODEL)


def check_weights_and_validity_trnas(ctx, params, trnas, contra, short=False):
    seqs = [s for _, s in trnas]
    N = 2000
    rows, weights, logz = ctx.sample_batch(seqs, N, contra, short, seed=3)
    mats, logz_bpp = ctx.bpp_batch(seqs, contra, short)
    assert logz.tobytes() == logz_bpp.tobytes()
    worst = 0.0
    for seq, r, w, m in zip(seqs, rows, weights, mats):
        u, inv = np.unique(r, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for x, row in enumerate(u):
            prs = pairs_of(row)
            for i, j in prs:
                assert m[i, j] >= 0.0, f"sampled pair ({i},{j}) is not in the bpp key set"
            ref = score(params, seq, row, contra, short)
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
        if short:  # the exact probability of the likeliest pair of span < 4 is 0.47 .. 0.96 on every tRNA
            f = pair_freq(r)
            assert max(f[i, j] for i in range(len(seq)) for j in range(i + 1, min(i + 4, len(seq)))) > 0.1
    print(f"log-weight error: at most {worst:.3f} of the bound")


@pytest.mark.parametrize("contra", [False, True])
def test_weights_and_validity_trnas(ctx, params, trnas, contra):
    check_weights_and_validity_trnas(ctx, params, trnas, contra)


def test_weights_and_validity_trnas_short_hairpins(ctx, params, trnas):
    """allows_short_hairpins = 1 (CONTRAfold): the same ulp bound on every log-weight, every sampled pair in
    the key set of the bpp with the flag, and on every tRNA some pair with j - i < 4 sampled with a frequency
    above 0.1 (the oracle's exact ensemble expects 4.07 .. 6.57 such pairs per structure: asserted >= 1)"""
    SP.assert_input_has_short_pairs(params, [s for _, s in trnas])
    for _, s in trnas:
        ex, _ = O.exact_bpp(params.ptr, s, True, True)
        assert ex[SP.short_cells(len(s))].max() > 0.4  # (the largest single one: 0.47 .. 0.96)
    check_weights_and_validity_trnas(ctx, params, trnas, *SP.MODEL)


def check_marginals_at_size(ctx, params, trnas, contra, short=False):
    from rna_algos_amd.mccaskill_algo import bpp_index
    seqs = [s for _, s in trnas]
    N = 20_000
    rows, _, _ = ctx.sample_batch(seqs, N, contra, short, seed=5)
    for seq, r in zip(seqs, rows):
        n = len(seq)
        ex, _ = O.exact_bpp(params.ptr, seq, contra, short)
        p = np.zeros((n, n))
        iu = np.triu_indices(n)
        p[iu] = np.array([max(0.0, ex[bpp_index(n, i, j)]) for i, j in zip(*iu)])
        f = pair_freq(r)
        assert np.all(np.abs(f - p) <= 5 * sigma(p, N) + 3e-3), float(np.max(np.abs(f - p)))
        counts = (r == OPEN).sum(axis=1)
        sd = float(counts.std())
        assert abs(counts.mean() - p.sum()) <= 5 * sd / math.sqrt(N) + 0.01 * p.sum()
        if short:  # the pairs that exist under the flag alone are sampled
            assert short_mass(f) > 0.5, short_mass(f)


@pytest.mark.parametrize("contra", [False, True])
def test_marginals_at_size(ctx, params, trnas, contra):
    check_marginals_at_size(ctx, params, trnas, contra)


def test_marginals_at_size_short_hairpins(ctx, params, trnas):
    """allows_short_hairpins = 1 (CONTRAfold) against the exact f64 ensemble with the flag"""
    SP.assert_input_has_short_pairs(params, [s for _, s in trnas])
    check_marginals_at_size(ctx, params, trnas, *SP.MODEL)


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


def test_edges_short_hairpins(ctx, params):
    """the n = 4 record and the homopolymer of test_edges under allows_short_hairpins = 1 (CONTRAfold): not
    assumed all dots -- every row's pairs lie in the oracle's key set (O.bpp(..., True, True) >= 0) and its
    log-weight equals structure_score within the ulp bound of test_weights_and_validity_trnas.  G A A C has
    one key, (0, 3), a pair of span 3 with the exact probability 0.0106: among 2 000 samples it is missing
    with probability 5e-10, and its frequency meets the bound of test_exact_distribution_small; poly-A has
    no key and all its rows are dots."""
    from rna_algos_amd.mccaskill_algo import bpp_index
    N = 2000
    short = np.array([2, 0, 0, 1], dtype=np.uint8)
    homo = np.zeros(30, dtype=np.uint8)
    rows, w, logz = ctx.sample_batch([short, homo], N, True, True, seed=1)
    for r, ws, seq in zip(rows, w, [short, homo]):
        n = len(seq)
        ref, _ = O.bpp(params.ptr, seq, True, True)
        keys = {(i, j) for i in range(n) for j in range(i + 1, n) if ref[bpp_index(n, i, j)] >= 0}
        u, inv = np.unique(r, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for x, row in enumerate(u):
            prs = pairs_of(row)
            assert set(prs) <= keys, (bytes(row), sorted(keys))
            want = score(params, seq, row, True, True)
            tol = 4 * (len(prs) + 1) * float(np.spacing(np.float32(max(1.0, abs(want)))))
            got = ws[inv == x]
            assert np.all(got == got[0]) and abs(float(got[0]) - want) <= tol, (bytes(row), float(got[0]), want, tol)
        lz, bp, _ = O.bruteforce(params.ptr, seq, True, True) if n <= 22 else (None, np.zeros((n, n)), None)
        assert {(i, j) for i, j in zip(*np.nonzero(bp))} == keys
        f = pair_freq(r)
        assert np.all(np.abs(f - bp) <= 5 * sigma(bp, N) + 1e-3), (f[f > 0], bp[bp > 0])
        if keys:
            assert keys == {(0, 3)} and np.count_nonzero(f) == 1
        else:
            assert np.all(r == DOT)
    assert logz.tobytes() == ctx.bpp_batch([short, homo], True, True)[1].tobytes()


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
