"""rnamc_bpp_windowed / rnamc_bpp_windowed_multi on the GPU: the pair probabilities of the windows of
one sequence, averaged per pair over the windows that contain it.

The yardstick is a numpy restatement of the contract in include/rnamc.h — int64 sums of
min(rint(p * 2^44), 2^45), window counters, a brute-force denominator, the division formula, the
paired-probability loop — fed with the triangles of the dense entry (rnamc_bpp_batch_constrained)
on the same context for the same window list with max_bp_span = B.  Every comparison is bit for
bit, no tolerances (but for the one the contract itself states for a single window)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = float(2 ** 44)


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def reset(ctx):
    for k, v in (("summation_mode", 0), ("group_max_seqs", 8192), ("window_chunk_nt", 64 << 20)):
        ctx.set(k, v)


def seq_of(n):
    from rna_algos_amd.workloads import synthetic_seq
    return synthetic_seq(n, seed=1400 + n)


def windows(n, w, s):
    """the window list, by brute force -> (starts, window length)"""
    if n <= w:
        return [0], n
    starts = []
    x = 0
    while x + w <= n:
        starts.append(x)
        x += s
    if starts[-1] + w < n:
        starts.append(n - w)
    return starts, w


def band_of(n, w, span):
    return min(x for x in (w, n, span) if x)


def yardstick(n, starts, wl, B, tris):
    """include/rnamc.h restated: packed triangles of the windows -> (band f32[n, B], paired f32[n])"""
    S = np.zeros((n, B), np.int64)
    present = np.zeros((n, B), np.uint32)
    denom = np.zeros((n, B), np.int64)
    for st, tri in zip(starts, tris):
        assert tri.shape == (wl * (wl + 1) // 2,)
        off = wl
        for d in range(1, wl):
            row = tri[off:off + wl - d]
            off += wl - d
            if d >= B:
                assert np.all(row < -0.5)  # the span limit: no such pair in any window
                continue
            have = row > -0.5
            q = np.minimum(np.rint(np.where(have, row, 0).astype(np.float64) * Q), 2.0 * Q)  # (ties to even)
            S[st:st + wl - d, d] += q.astype(np.int64)
            present[st:st + wl - d, d] += have
            denom[st:st + wl - d, d] += 1  # windows with start <= i and i + d < start + w
    ok = (present > 0) & (denom > 0)
    ok[:, 0] = False
    with np.errstate(divide="ignore", invalid="ignore"):
        val = (S.astype(np.float64) / (denom.astype(np.float64) * Q)).astype(np.float32)
    band = np.where(ok, val, np.float32(-1)).astype(np.float32)
    paired = np.zeros(n, np.float32)
    for d in range(1, B):
        col = band[:n - d, d] if d < n else band[:0, d]
        add = np.where(col > -0.5, col, np.float32(0)).astype(np.float32)  # (x + 0 == x: an absent pair adds nothing)
        paired[:n - d] = paired[:n - d] + add
        paired[d:] = paired[d:] + add
    return band, paired


def dense_windows(ctx, seq, starts, wl, B, contra, cons=None, short=False):
    """the dense entry on the window list with max_bp_span = B -> (packed triangles, ln Z)"""
    seqs = [seq[a:a + wl] for a in starts]
    cs = None if cons is None else [cons[a:a + wl] for a in starts]
    mats, logz = ctx.bpp_batch(seqs, contra, short, constraints=cs, max_bp_span=B)
    return [np.asarray(m.packed) for m in mats], logz


def run_case(ctx, n, w, s, span=0, contra=False, cons=None, seq=None, short=False):
    seq = seq_of(n) if seq is None else seq
    starts, wl = windows(n, w, s)
    B = band_of(n, w, span)
    tris, logz = dense_windows(ctx, seq, starts, wl, B, contra, cons, short)
    want_band, want_paired = yardstick(n, starts, wl, B, tris)
    res = ctx.bpp_windowed(seq, w, contra, short, stride=s, max_bp_span=span, constraint=cons)
    assert res.band.shape == (n, B) and res.starts.tolist() == starts
    assert np.array_equal(res.band.view(np.uint32), want_band.view(np.uint32)), (n, w, s, span, contra)
    assert np.array_equal(res.paired_prob.view(np.uint32), want_paired.view(np.uint32)), (n, w, s, span, contra)
    assert np.array_equal(res.window_log_z.view(np.uint32), logz.view(np.uint32)), (n, w, s, span, contra)
    return res, seq, starts, wl, B


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("shape", [(1, 5, 1), (4, 5, 1), (5, 5, 1), (6, 5, 1), (37, 16, 3), (38, 16, 3)])
def test_edge_shapes(ctx, shape, contra):
    """nothing can pair (1, 4), the first admissible span alone and in two windows (5, 6), a last grid window
    that ends at N (37: 21 = 7 * 3) and a final window off the stride grid (38: 22 after 21)"""
    reset(ctx)
    res, _, starts, wl, _ = run_case(ctx, *shape, contra=contra)
    n = shape[0]
    if n <= 4:
        assert np.all(res.band == -1) and np.all(res.paired_prob == 0)
    if n == 37:
        assert starts[-1] == 21 and starts[-2] == 18
    if n == 38:
        assert starts[-1] == 22 and starts[-2] == 21
    assert np.all(res.band[:, 0] == -1)


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("shape", [(64, 64, 1), (65, 64, 1), (130, 65, 7), (300, 23, 5)])
def test_block_and_wave_edges(ctx, shape, contra):
    """a window of one wave of bases, one more, a 65-wide band (two tiles of the finalize kernel), and a
    276-cell triangle: one cell past a 256-cell block"""
    reset(ctx)
    res, *_ = run_case(ctx, *shape, contra=contra)
    assert np.any(res.band > 0)


def test_gaps(ctx):
    """stride above the window: uncovered bases have no pairs at all"""
    reset(ctx)
    n, w, s = 120, 16, 23
    res, _, starts, wl, _ = run_case(ctx, n, w, s)
    covered = np.zeros(n, bool)
    for a in starts:
        covered[a:a + wl] = True
    assert not covered.all() and covered.any()
    assert np.all(res.band[~covered] == -1)
    assert np.all(res.paired_prob[~covered].view(np.uint32) == 0)
    assert np.any(res.band[covered] > 0)


@pytest.mark.parametrize("span", [7, 33])
def test_band_narrower_than_window(ctx, span):
    reset(ctx)
    res, *_ = run_case(ctx, 200, 64, 4, span=span)
    assert res.band.shape == (200, span)  # no cell with d >= B exists
    assert np.any(res.band > 0)


def test_single_window_equals_plain_bpp(ctx):
    """N <= W: one window; the band is the plain dense bpp, exactly where p >= 2^-20 and within 2^-45 below
    (the quantum of the integer sums); the key sets are identical"""
    reset(ctx)
    n = 50
    res, seq, starts, wl, B = run_case(ctx, n, 64, 1)
    assert starts == [0] and wl == n and B == n
    mats, logz = ctx.bpp_batch([seq], False, False)
    dense = mats[0].dense()  # [i, j]
    i, d = np.nonzero(np.ones((n, n), bool))
    ok = (i + d < n) & (d >= 1)
    plain = np.full((n, n), -1.0, np.float32)
    plain[i[ok], d[ok]] = dense[i[ok], i[ok] + d[ok]]
    assert np.array_equal(res.band > -0.5, plain > -0.5)
    assert np.count_nonzero(plain > -0.5) > 0
    big = plain >= np.float32(2.0 ** -20)
    assert np.array_equal(res.band[big].view(np.uint32), plain[big].view(np.uint32))
    small = (plain > -0.5) & ~big
    assert np.all(np.abs(res.band[small].astype(np.float64) - plain[small].astype(np.float64)) <= 2.0 ** -45)
    assert res.window_log_z.view(np.uint32)[0] == logz.view(np.uint32)[0]


def test_constraint(ctx):
    """x over bases 40 .. 55, a '<' and a '>': each window gets its slice of the string"""
    reset(ctx)
    n = 150
    c = ["."] * n
    c[40:56] = "x" * 16
    c[70], c[100] = "<", ">"
    cons = "".join(c)
    res, *_ = run_case(ctx, n, 32, 5, cons=cons)
    assert np.all(res.paired_prob[40:56].view(np.uint32) == 0)
    assert np.all(res.band[40:56] == -1)
    i, j, p = res.pairs()
    assert len(p) > 0
    assert not np.any((j >= 40) & (j < 56)) and not np.any(j == 70) and not np.any(i == 100)
    free, *_ = run_case(ctx, n, 32, 5)
    assert not np.array_equal(free.band.view(np.uint32), res.band.view(np.uint32))


def test_invariance(ctx, params):
    """the same bytes whatever the grouping, the chunking and the number of contexts"""
    from rna_algos_amd.mccaskill_algo import Pool
    reset(ctx)
    n, w, s = 300, 64, 1
    base, seq, starts, *_ = run_case(ctx, n, w, s)

    def same(res):
        assert np.array_equal(res.band.view(np.uint32), base.band.view(np.uint32))
        assert np.array_equal(res.paired_prob.view(np.uint32), base.paired_prob.view(np.uint32))
        assert np.array_equal(res.window_log_z.view(np.uint32), base.window_log_z.view(np.uint32))
        assert np.array_equal(res.starts, base.starts)
    try:
        for knobs in (dict(group_max_seqs=3), dict(window_chunk_nt=64 * 5), dict(group_max_seqs=3, window_chunk_nt=64 * 5)):
            reset(ctx)
            for k, v in knobs.items():
                ctx.set(k, v)
            same(ctx.bpp_windowed(seq, w, False, False, stride=s))
            if "window_chunk_nt" in knobs:  # several chunks: the statistics are the call's, not the last chunk's
                st = ctx.stats()
                assert st["n_groups"] >= len(starts) // 5 and st["launches_window"] >= len(starts) // 5 + 2
        reset(ctx)
        small = ctx.bpp_windowed(seq[:37], 16, False, False, stride=3)
        ctx.set("window_chunk_nt", 1)  # below one window: a window a chunk
        one = ctx.bpp_windowed(seq[:37], 16, False, False, stride=3)
        assert np.array_equal(one.band.view(np.uint32), small.band.view(np.uint32))
        assert ctx.stats()["n_groups"] == len(small.starts) == 8
    finally:
        reset(ctx)
    pool = Pool(params, devices=[0, 0])
    try:
        same(pool.bpp_windowed(seq, w, False, False, stride=s))
        pool.set("window_chunk_nt", 64 * 7)
        same(pool.bpp_windowed(seq, w, False, False, stride=s))
        one = pool.bpp_windowed(seq[:40], 64, False, False)  # one window: one shard
        alone = ctx.bpp_windowed(seq[:40], 64, False, False)
        assert np.array_equal(one.band.view(np.uint32), alone.band.view(np.uint32))
        assert np.array_equal(one.paired_prob.view(np.uint32), alone.paired_prob.view(np.uint32))
    finally:
        pool.close()


def test_chunks_groups_and_profile_together(ctx):
    """several chunks, several groups a chunk and a profiled call at once: (2000, 200, 100) is 19 windows; 1000
    nucleotides a chunk are 5 + 5 + 5 + 4 windows, three windows a group are two groups a chunk.  The same bytes
    as the call of one chunk and one group, and the statistics of the whole call: a window launch per group, then
    the finalize and the paired launch"""
    reset(ctx)
    n, w, s = 2000, 200, 100
    seq = seq_of(n)
    base = ctx.bpp_windowed(seq, w, False, False, stride=s)
    plain = ctx.stats()
    assert len(base.starts) == 19 and plain["n_groups"] == 1 and plain["launches_window"] == 3
    assert plain["ms_window"] == 0
    try:
        ctx.set("window_chunk_nt", 1000)
        ctx.set("group_max_seqs", 3)
        counts = []
        for profile in (0, 1):
            ctx.set("profile", profile)
            res = ctx.bpp_windowed(seq, w, False, False, stride=s)
            st = ctx.stats()
            assert np.array_equal(res.band.view(np.uint32), base.band.view(np.uint32))
            assert np.array_equal(res.paired_prob.view(np.uint32), base.paired_prob.view(np.uint32))
            assert np.array_equal(res.window_log_z.view(np.uint32), base.window_log_z.view(np.uint32))
            assert st["n_groups"] == 8 and st["launches_window"] == 8 + 2
            assert st["launches_other"] >= st["launches_window"] + st["n_groups"]
            assert st["launches_inside"] >= 8 and st["launches_outside"] >= 8
            assert st["workspace_bytes"] == plain["workspace_bytes"]  # (the context's workspace never shrinks)
            assert (0 < st["ms_window"] < 1e3 and st["ms_inside"] > 0 and st["ms_outside"] > 0) if profile else \
                (st["ms_window"] == 0 and st["ms_inside"] == 0 and st["ms_outside"] == 0)
            counts.append({k: v for k, v in st.items() if not k.startswith("ms_")})
        assert counts[0] == counts[1]  # (timing a call changes none of its counts)
    finally:
        ctx.set("profile", 0)
        reset(ctx)


def test_tree_order_mode(ctx):
    """summation mode 1: against the dense entry in mode 1 on the identical window batch"""
    reset(ctx)
    ctx.set("summation_mode", 1)
    try:
        res, *_ = run_case(ctx, 300, 64, 1)
        assert np.any(res.band > 0)
    finally:
        reset(ctx)


def check_against_the_cpu_oracle(ctx, params, contra=False, short=False):
    import oracle_lib as O
    reset(ctx)
    n, w, s = 40, 12, 2
    seq = seq_of(n)
    starts, wl = windows(n, w, s)
    tris, zs = [], []
    for a in starts:
        ref, z = O.bpp(params.ptr, seq[a:a + wl], contra, short)
        tris.append(np.where(ref < 0, np.float32(-1), ref).astype(np.float32))
        zs.append(z)
    want_band, want_paired = yardstick(n, starts, wl, w, tris)
    res = ctx.bpp_windowed(seq, w, contra, short, stride=s)
    assert np.count_nonzero(want_band > 0) > 0
    assert np.array_equal(res.band.view(np.uint32), want_band.view(np.uint32))
    assert np.array_equal(res.paired_prob.view(np.uint32), want_paired.view(np.uint32))
    assert np.array_equal(res.window_log_z.view(np.uint32), np.asarray(zs, np.float32).view(np.uint32))
    return res, seq


def test_against_the_cpu_oracle(ctx, params):
    """(40, 12, 2), Turner, reference order: the yardstick fed with the CPU oracle's bpp of every window (B = W:
    the span limit admits every pair of a window)"""
    check_against_the_cpu_oracle(ctx, params)


# ---- allows_short_hairpins = 1 (CONTRAfold): the windows' triangles carry pairs of span 1, 2 and 3

SHORT_SHAPES = [(6, 5, 1), (38, 16, 3), (130, 65, 7)]


@pytest.mark.parametrize("shape", SHORT_SHAPES)
def test_short_hairpins(ctx, params, shape):
    """two windows of the first admissible length, a final window off the stride grid, and a 65-wide band,
    against the dense entry with the same flag; the columns d = 1, 2, 3 of the band hold present cells.
    The input condition from the oracle alone: the exact ensemble of the sequence expects at least one pair
    with j - i < 4 (3.34 at n = 38, 8.07 at n = 130).  The 6-nt sequence is too short for that -- its
    ensemble expects 0.43 -- so for it the condition is that such pairs exist at all (expectation > 0)."""
    import short_pairs as SP
    reset(ctx)
    n = shape[0]
    e = SP.expected_short_pairs(params, seq_of(n))
    assert e >= 1.0 if n > 6 else e > 0.0, e
    res, *_ = run_case(ctx, *shape, contra=True, short=True)
    assert np.any(res.band[:, 1:4] > -0.5)
    assert np.all(res.band[:, 0] == -1)


def test_against_the_cpu_oracle_short_hairpins(ctx, params):
    """(40, 12, 2) with O.bpp(..., True, True) of every window"""
    import short_pairs as SP
    SP.assert_input_has_short_pairs(params, [seq_of(40)])
    res, _ = check_against_the_cpu_oracle(ctx, params, True, True)
    assert np.any(res.band[:, 1:4] > -0.5)


@pytest.mark.parametrize("span", [2, 3, 4])
def test_narrow_span_limits(ctx, params, span):
    """max_bp_span = 2, 3, 4 admits the spans j - i < 2, 3, 4 alone, which only exist with the flag: (60, 16,
    2) has a band of that width whose d = 1 column holds present cells; without the flag every cell of the
    band is -1 and paired_prob is all zero"""
    import short_pairs as SP
    reset(ctx)
    SP.assert_input_has_short_pairs(params, [seq_of(60)])
    res, *_ = run_case(ctx, 60, 16, 2, span=span, contra=True, short=True)
    assert res.band.shape == (60, span)
    assert np.any(res.band[:, 1] > -0.5)
    assert np.any(res.paired_prob > 0)
    plain, *_ = run_case(ctx, 60, 16, 2, span=span, contra=True, short=False)
    assert plain.band.shape == (60, span)
    assert np.all(plain.band == -1) and np.all(plain.paired_prob.view(np.uint32) == 0)


def test_window_log_partition(ctx):
    """ln Z of every window, in window order = rnamc_log_partition_batch of the windows"""
    reset(ctx)
    n, w, s, span = 130, 40, 9, 25
    seq = seq_of(n)
    starts, wl = windows(n, w, s)
    res = ctx.bpp_windowed(seq, w, True, False, stride=s, max_bp_span=span)
    want = ctx.log_partition_batch([seq[a:a + wl] for a in starts], True, False, max_bp_span=span)
    assert len(want) == len(starts) > 1
    assert np.array_equal(res.window_log_z.view(np.uint32), want.view(np.uint32))


def test_errors_leave_the_context_usable(ctx):
    from rna_algos_amd import _lib
    reset(ctx)
    seq = seq_of(37)
    with pytest.raises(_lib.RnamcError) as e:
        ctx.bpp_windowed(seq, 16, False, False, stride=3, constraint="." * 20 + "(" + "." * 16)
    assert e.value.status == _lib.ERR_INVALID_ARG and "position 20" in str(e.value)
    bad = seq.copy()
    bad[5] = 4
    with pytest.raises(_lib.RnamcError) as e:
        ctx.bpp_windowed(bad, 16, False, False)
    assert e.value.status == _lib.ERR_INVALID_BASE
    run_case(ctx, 37, 16, 3)


def test_cli_round_trip(params, tmp_path):
    """local_fold on a two-record FASTA: the triples of every record are `.pairs(0.01)` of the API"""
    import subprocess
    import sys
    from rna_algos_amd import utils
    from rna_algos_amd.bin.mccaskill_algo import HEADER, fmt_f32
    from rna_algos_amd.mccaskill_algo import mccaskill_algo_windowed
    utils.set_default_tables(params)
    seqs = [seq_of(90), seq_of(141)]
    fa = os.path.join(tmp_path, "in.fa")
    with open(fa, "w") as fh:
        for k, s in enumerate(seqs):
            fh.write(f">r{k}\n" + "".join("ACGU"[x] for x in s) + "\n")
    out = os.path.join(tmp_path, "out.dat")
    subprocess.check_call([sys.executable, "-m", "rna_algos_amd.bin.local_fold", "--synthetic-tables", "1", "-i", fa,
                           "-o", out, "-w", "40", "-l", "30", "--stride", "7"], cwd=ROOT, stderr=subprocess.DEVNULL,
                          timeout=300)
    fss = utils.FoldScoreSets.new(0.0)
    fss.transfer()
    want = [HEADER]
    total = 0
    for k, s in enumerate(seqs):
        res = mccaskill_algo_windowed(s, 40, False, False, fss, stride=7, max_bp_span=30)
        i, j, p = res.pairs(0.01)
        total += len(p)
        assert np.all(p >= np.float32(0.01)) and np.all(j - i < 30)
        want.append(f"\n\n>{k}\n" + "".join(f"{a},{b},{fmt_f32(q)} " for a, b, q in zip(i, j, p)))
    assert total > 0
    assert open(out).read() == "".join(want)
