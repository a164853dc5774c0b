"""The seven pool entries over THREE contexts on device 0 against their Context counterparts, bit for
bit: fewer records than shards, as many, and more (rna_algos_amd/csrc/rnamc_shards.h, rnamc_pool.cpp).
The files of the single entries hold the same comparison for two shards and pin the context entries
themselves; nothing here has a tolerance."""
import os

import numpy as np
import pytest

from test_gpu_sparse_bpp import sparse_raw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# distinct lengths in 5 .. 48 and one tie; 1, 3 and 7 records for three shards
LENS = {1: [31], 3: [23, 48, 23], 7: [48, 5, 31, 17, 31, 9, 40]}
SPAN = 30
GAMMAS = [0.5, 4.0]


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool(params):
    from rna_algos_amd.mccaskill_algo import Pool
    p = Pool(params, devices=[0, 0, 0])
    assert len(p) == 3
    yield p
    p.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def records(count):
    """the records of a case and their constraints: every second record constrained (an unpaired run, a
    base that pairs downstream only), the others free"""
    from rna_algos_amd.workloads import synthetic_seq
    seqs = [synthetic_seq(n, seed=4100 + 17 * x + n) for x, n in enumerate(LENS[count])]
    cons = []
    for x, s in enumerate(seqs):
        c = ["."] * len(s)
        if x % 2 == 0:
            c[1] = "<"
            c[len(s) // 2:len(s) // 2 + 2] = "xx"
        cons.append("".join(c) if x % 2 == 0 else None)
    return seqs, cons


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("count", [1, 3, 7])
def test_bpp_batch(ctx, pool, count, contra):
    seqs, cons = records(count)
    want, want_z = ctx.bpp_batch(seqs, contra, False, constraints=cons, max_bp_span=SPAN)
    got, got_z = pool.bpp_batch(seqs, contra, False, constraints=cons, max_bp_span=SPAN)
    assert same_bits(got_z, want_z)
    for a, b in zip(got, want):
        assert a.n == b.n and same_bits(a.packed, b.packed)
    # without strings: the unconstrained entry's route through the same shards
    want, want_z = ctx.bpp_batch(seqs, contra, False)
    got, got_z = pool.bpp_batch(seqs, contra, False)
    assert same_bits(got_z, want_z) and all(same_bits(a.packed, b.packed) for a, b in zip(got, want))


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("count", [1, 3, 7])
def test_centroid_fold_batch(ctx, pool, count, contra):
    seqs, cons = records(count)
    kw = dict(constraints=cons, max_bp_span=SPAN, return_bpp=True)
    want, want_z, want_m = ctx.centroid_fold_batch(seqs, GAMMAS, contra, False, **kw)
    got, got_z, got_m = pool.centroid_fold_batch(seqs, GAMMAS, contra, False, **kw)
    assert same_bits(got_z, want_z)
    assert [[(db, np.float32(a).tobytes()) for db, a in f] for f in got] == \
        [[(db, np.float32(a).tobytes()) for db, a in f] for f in want]
    for a, b in zip(got_m, want_m):
        assert same_bits(a.packed, b.packed)
    got, got_z = pool.centroid_fold_batch(seqs, GAMMAS, contra, False, constraints=cons, max_bp_span=SPAN)
    assert same_bits(got_z, want_z) and [[db for db, _ in f] for f in got] == [[db for db, _ in f] for f in want]


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("count", [1, 3, 7])
def test_bpp_batch_sparse(ctx, pool, count, contra):
    from rna_algos_amd import _lib
    L = _lib.lib()
    seqs, cons = records(count)
    kw = dict(cons=cons, span=SPAN)
    st, want = sparse_raw(L.rnamc_bpp_batch_sparse, ctx._h, seqs, contra, 1e-3, **kw)
    assert st == _lib.OK and want["total"] > 1
    st, got = sparse_raw(L.rnamc_bpp_batch_sparse_multi, pool._h, seqs, contra, 1e-3, **kw)
    assert st == _lib.OK
    assert got["total"] == want["total"] and np.array_equal(got["count"], want["count"])
    spans = sorted((int(a), int(a + c)) for a, c in zip(got["start"], got["count"]) if c)
    assert all(hi <= lo for (_, hi), (lo, _) in zip(spans, spans[1:])) and spans[-1][1] <= got["total"]
    for a, b in zip(got["lists"], want["lists"]):
        assert all(same_bits(u, v) for u, v in zip(a, b))
    assert all(same_bits(a, b) for a, b in zip(got["paired"], want["paired"]))
    assert same_bits(got["logz"], want["logz"])
    # arrays one entry short: an argument error of the host, with the total and the counts of the context's
    cap = want["total"] - 1
    st_c, short_c = sparse_raw(L.rnamc_bpp_batch_sparse, ctx._h, seqs, contra, 1e-3, cap=cap, **kw)
    st_p, short_p = sparse_raw(L.rnamc_bpp_batch_sparse_multi, pool._h, seqs, contra, 1e-3, cap=cap, **kw)
    assert st_c == st_p == _lib.ERR_INVALID_ARG
    assert short_p["total"] == short_c["total"] == want["total"]
    assert np.array_equal(short_p["count"], short_c["count"]) and np.array_equal(short_p["count"], want["count"])


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("count", [1, 3, 7])
def test_context_profile_batch(ctx, pool, count, contra):
    seqs, cons = records(count)
    want, want_z = ctx.context_profile_batch(seqs, contra, False, constraints=cons, max_bp_span=SPAN)
    got, got_z = pool.context_profile_batch(seqs, contra, False, constraints=cons, max_bp_span=SPAN)
    assert same_bits(got_z, want_z)
    assert len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("stride,n_windows", [(1, 37), (7, 7)])
def test_bpp_windowed(ctx, pool, stride, n_windows, contra):
    """n = 60, window 24: 37 windows at stride 1; at stride 7 six on the grid and the tail window"""
    from rna_algos_amd.workloads import synthetic_seq
    seq = synthetic_seq(60, seed=4260)
    want = ctx.bpp_windowed(seq, 24, contra, False, stride=stride)
    got = pool.bpp_windowed(seq, 24, contra, False, stride=stride)
    assert len(want.starts) == n_windows and got.starts.tolist() == want.starts.tolist()
    assert same_bits(got.band, want.band) and same_bits(got.paired_prob, want.paired_prob)
    assert same_bits(got.window_log_z, want.window_log_z)


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("positions", [[], [11], [0, 3, 8, 13, 19]])
def test_mutant_scan(ctx, pool, positions, contra):
    from rna_algos_amd.workloads import synthetic_seq
    seq = synthetic_seq(20, seed=4220)
    want = ctx.mutant_scan(seq, contra, False, positions=positions)
    got = pool.mutant_scan(seq, contra, False, positions=positions)
    assert len(got) == len(want) == 3 * len(positions)
    assert got.wt_log_z == want.wt_log_z and same_bits(got.wt_paired_prob, want.wt_paired_prob)
    for f in ("pos", "base", "log_z", "dist2_q", "max_dp", "max_pair", "paired_prob"):
        assert same_bits(getattr(got, f), getattr(want, f)), f


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("n_rows", [2, 5])
def test_bpp_alignment(ctx, pool, n_rows, contra):
    """rows of tests/golden/align_small.sto; the file has four, so the fifth row is the first once more
    (more rows than shards, and two of equal length)"""
    from rna_algos_amd import utils
    rows, _ = utils.read_align(os.path.join(ROOT, "tests", "golden", "align_small.sto"))
    rows = np.vstack([rows, rows[:1]])[:n_rows]
    assert rows.shape == (n_rows, 37)
    want = ctx.bpp_alignment(rows, contra, False, GAMMAS)
    got = pool.bpp_alignment(rows, contra, False, GAMMAS)
    assert same_bits(np.asarray(got.bpp.packed), np.asarray(want.bpp.packed))
    assert same_bits(got.col_paired, want.col_paired) and same_bits(got.log_z, want.log_z)
    assert got.row_len.tolist() == want.row_len.tolist()
    assert [(db, np.float32(a).tobytes()) for db, a in got.folds] == \
        [(db, np.float32(a).tobytes()) for db, a in want.folds]
