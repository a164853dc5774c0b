"""rnamc_mutant_scan / rnamc_mutant_scan_multi on the GPU: every single-base mutant of one sequence folded
and its pair-probability triangle compared with the wild type's on the device.

The yardstick is a numpy restatement of the contract in include/rnamc.h -- per cell of span >= 1 the f64
difference of the two probabilities (absent pairs as 0), np.rint of its square times 2^44 capped at 2^45,
int64 sums, the f32 |difference| with ties to the smallest packed index, the paired-probability loop --
fed with the triangles of the dense entry (rnamc_bpp_batch_constrained) on the same context: the wild type
as a call of one record, then the mutants with the same constraint and span.  Every comparison is bit
for bit, no tolerances.

The compare kernel walks a triangle in strips of 4096 cells, one workgroup each, while at most 64 strips
cover it; longer triangles get 64 strips of a 64th of their cells rounded up to a multiple of 256
(mutant_strip_of, rnamc_device.h).  The shapes below are derived from that: see test_strip_edges."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = float(2 ** 44)
MIN_STRIP, MAX_STRIPS = 4096, 64
CANONICAL = {(0, 3), (3, 0), (1, 2), (2, 1), (2, 3), (3, 2)}


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def reset(ctx):
    for k, v in (("summation_mode", 0), ("group_max_seqs", 8192), ("mutant_chunk_nt", 64 << 20)):
        ctx.set(k, v)


def seq_of(n):
    from rna_algos_amd.workloads import synthetic_seq
    return synthetic_seq(n, seed=1500 + n)


def mutants_of(seq, positions=None):
    """the mutant list, by brute force -> (positions, base codes, records)"""
    pos, base, recs = [], [], []
    for x in (range(len(seq)) if positions is None else positions):
        for b in range(4):
            if b != seq[x]:
                r = seq.copy()
                r[x] = b
                pos.append(x)
                base.append(b)
                recs.append(r)
    return pos, base, recs


def paired_of(n, tri):
    """rnamc_bpp_batch_sparse's paired_prob restated: d ascending, p(x, x+d) then p(x-d, x), rounded f32 adds"""
    paired = np.zeros(n, np.float32)
    off = n
    for d in range(1, n):
        row = tri[off:off + n - d]
        off += n - d
        add = np.where(row > -0.5, row, np.float32(0)).astype(np.float32)  # (x + 0 == x: an absent pair adds nothing)
        paired[:n - d] = paired[:n - d] + add
        paired[d:] = paired[d:] + add
    return paired


def yardstick(n, wt, muts):
    """include/rnamc.h restated: packed triangles -> (dist2_q i64[M], max_dp f32[M], max_pair i64[M, 2])"""
    length = n * (n + 1) // 2
    starts = np.array([d * n - d * (d - 1) // 2 for d in range(n)], np.int64)
    assert wt.shape == (length,) and wt.dtype == np.float32
    fa = np.where(wt > -0.5, wt, np.float32(0)).astype(np.float32)[n:]  # (span 0, c < n, is skipped)
    q, dp, pair = [], [], []
    for mut in muts:
        assert mut.shape == (length,) and mut.dtype == np.float32
        fb = np.where(mut > -0.5, mut, np.float32(0)).astype(np.float32)[n:]
        e = fa.astype(np.float64) - fb.astype(np.float64)
        q.append(int(np.minimum(np.rint((e * e) * Q), 2.0 * Q).astype(np.int64).sum()))  # (rint: ties to even)
        t = np.abs(fa - fb)  # one f32 subtraction
        assert t.dtype == np.float32
        if t.size and t.max() > 0:
            c = n + int(np.argmax(t))  # (the first of equal maxima: the smallest packed index)
            d = int(np.searchsorted(starts, c, side="right")) - 1
            dp.append(t.max())
            pair.append((c - int(starts[d]), c - int(starts[d]) + d))
        else:
            dp.append(np.float32(0))
            pair.append((-1, -1))
    return np.array(q, np.int64), np.array(dp, np.float32), np.array(pair, np.int64).reshape(len(muts), 2)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_scan(a, b):
    assert same_bits(a.pos, b.pos) and same_bits(a.base, b.base)
    assert same_bits(a.log_z, b.log_z) and np.float32(a.wt_log_z).tobytes() == np.float32(b.wt_log_z).tobytes()
    assert same_bits(a.dist2_q, b.dist2_q) and same_bits(a.max_dp, b.max_dp) and same_bits(a.max_pair, b.max_pair)
    assert same_bits(a.paired_prob, b.paired_prob) and same_bits(a.wt_paired_prob, b.wt_paired_prob)


def check_against(res, n, seq, positions, wt, wt_z, tris, zs):
    """a MutantScan against the yardstick fed with the given triangles and log partitions"""
    pos, base, _ = mutants_of(seq, positions)
    M = len(pos)
    assert len(res) == M and res.pos.tolist() == pos and res.base.tolist() == base
    want_q, want_dp, want_pair = yardstick(n, wt, tris)
    print("dist2_q", res.dist2_q[:6].tolist(), "want", want_q[:6].tolist(), "max_dp", res.max_dp[:6].tolist())
    assert res.dist2_q.dtype == np.int64 and same_bits(res.dist2_q, want_q)
    assert same_bits(res.max_dp, want_dp)
    assert same_bits(res.max_pair, want_pair)
    assert same_bits(res.log_z, np.asarray(zs, np.float32))
    assert np.float32(res.wt_log_z).tobytes() == np.float32(wt_z).tobytes()
    assert res.paired_prob.shape == (M, n)
    for m in range(M):
        assert same_bits(res.paired_prob[m], paired_of(n, tris[m])), m
    assert same_bits(res.wt_paired_prob, paired_of(n, wt))
    assert np.all(res.dist2 == want_q.astype(np.float64) / Q)


def run_case(ctx, n, contra=False, positions=None, cons=None, span=0, seq=None, short=False):
    seq = seq_of(n) if seq is None else seq
    _, _, recs = mutants_of(seq, positions)
    wt_mats, wt_z = ctx.bpp_batch([seq], contra, short, constraints=None if cons is None else [cons], max_bp_span=span)
    mats, zs = ctx.bpp_batch(recs, contra, short, constraints=None if cons is None else [cons] * len(recs),
                             max_bp_span=span)
    res = ctx.mutant_scan(seq, contra, short, positions=positions, constraint=cons, max_bp_span=span)
    check_against(res, n, seq, positions, np.asarray(wt_mats[0].packed), wt_z[0], [np.asarray(m.packed) for m in mats],
                  zs)
    return res, seq, recs


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("n", [1, 4, 5, 6])
def test_edge_shapes(ctx, n, contra):
    """nothing can pair at n <= 4: distance 0 and no pair named; n = 5 has the first admissible span"""
    reset(ctx)
    res, *_ = run_case(ctx, n, contra=contra)
    assert len(res) == 3 * n
    if n <= 4:
        assert np.all(res.dist2_q == 0) and np.all(res.max_dp.view(np.uint32) == 0)
        assert np.all(res.max_pair == -1)
        assert np.all(res.paired_prob.view(np.uint32) == 0) and np.all(res.wt_paired_prob.view(np.uint32) == 0)


def test_the_raw_entry_names_no_pair_with_all_ones(ctx):
    """max_i = max_j = 0xffffffff at the C boundary, and every output pointer but log_partition may be NULL"""
    from rna_algos_amd import _lib
    reset(ctx)
    n = 4
    seq = seq_of(n)
    logz = np.zeros(3 * n, np.float32)
    mi = np.zeros(3 * n, np.uint32)
    mj = np.zeros(3 * n, np.uint32)
    L = _lib.lib()
    _lib.check(L.rnamc_mutant_scan(ctx._h, seq.ctypes.data, n, None, 0, 0, 0, None, 0, logz.ctypes.data, None, None,
                                   mi.ctypes.data, mj.ctypes.data, None, None, None))
    assert np.all(mi == 0xffffffff) and np.all(mj == 0xffffffff)
    want = ctx.log_partition_batch(mutants_of(seq)[2], False, False)
    assert same_bits(logz, want)
    _lib.check(L.rnamc_mutant_scan(ctx._h, seq.ctypes.data, n, None, 0, 0, 0, None, 0, logz.ctypes.data, None, None,
                                   None, None, None, None, None))
    # an empty list: the wild type's outputs alone
    none = np.zeros(1, np.uint32)
    wt_z = np.zeros(1, np.float32)
    wt_p = np.full(n, 7, np.float32)
    logz[:] = 7
    _lib.check(L.rnamc_mutant_scan(ctx._h, seq.ctypes.data, n, None, 0, 0, 0, none.ctypes.data, 0, logz.ctypes.data,
                                   None, None, None, None, None, wt_z.ctypes.data, wt_p.ctypes.data))
    assert np.all(logz == 7) and np.all(wt_p.view(np.uint32) == 0)
    assert same_bits(wt_z, ctx.log_partition_batch([seq], False, False))


def strips_of(n):
    length = n * (n + 1) // 2
    per = -(-length // MAX_STRIPS)
    strip = max(MIN_STRIP, -(-per // 256) * 256)
    return length, strip, -(-length // strip)


@pytest.mark.parametrize("n,positions", [(22, None), (23, None), (90, [0, 44, 89]), (91, [0, 45, 90]),
                                         (128, [3, 64, 127]), (723, [10, 361, 722]), (724, [10, 362, 723])])
def test_strip_edges(ctx, n, positions):
    """22, 23: triangles of 253 and 276 cells, one short of and past a workgroup's 256 lanes.  Strips of
    4096 cells: n = 90 has 4095 cells, one short of a strip (no triangular number is 4096, nor 4097: a
    triangle exactly at or one past a strip does not exist); n = 91 has 4186, a second strip of 90 cells;
    n = 128 has 8256 = 2 strips and 64 cells.  n = 723 (261 726 cells) is the last length with strips of
    4096 cells, 64 of them; at n = 724 (262 450 cells) the strip grows to 4352 cells and 61 strips."""
    reset(ctx)
    want = {22: (253, 4096, 1), 23: (276, 4096, 1), 90: (4095, 4096, 1), 91: (4186, 4096, 2), 128: (8256, 4096, 3),
            723: (261726, 4096, 64), 724: (262450, 4352, 61)}
    assert strips_of(n) == want[n]
    res, *_ = run_case(ctx, n, positions=positions)
    assert np.any(res.dist2_q > 0) and np.any(res.max_dp > 0)


@pytest.mark.parametrize("contra", [False, True])
def test_trna_size_all_positions(ctx, contra):
    reset(ctx)
    res, *_ = run_case(ctx, 76, contra=contra)
    assert len(res) == 228 and np.all(res.dist2_q >= 0)
    assert np.count_nonzero(res.dist2_q) > 100
    moved = res.max_dp > 0
    assert np.all(res.max_pair[moved, 0] < res.max_pair[moved, 1]) and np.all(res.max_pair[moved, 1] < 76)
    r = res.profile_correlation()
    assert np.all((r[~np.isnan(r)] <= 1 + 1e-12) & (r[~np.isnan(r)] >= -1 - 1e-12))
    assert res.top(5).tolist() == np.argsort(-res.dist2, kind="stable")[:5].tolist()


def test_position_lists(ctx):
    """a subset, unsorted, with a duplicate whose two copies give identical rows"""
    reset(ctx)
    positions = [150, 7, 99, 7, 0, 199]
    res, *_ = run_case(ctx, 200, positions=positions)
    assert res.pos.tolist() == [p for p in positions for _ in range(3)]
    a, b = slice(3, 6), slice(9, 12)
    for arr in (res.base, res.log_z, res.dist2_q, res.max_dp, res.max_pair, res.paired_prob):
        assert same_bits(arr[a], arr[b])


def test_constraints(ctx):
    """x over six bases, a bracket pair, a '<' and max_bp_span = 20 at n = 60, all positions: every mutant is
    folded under the wild type's string (constraints only remove pairs: the bracket's own bases may mutate)"""
    reset(ctx)
    n = 60
    seq = seq_of(n)
    i, j = next((i, j) for i in range(2, 25) for j in range(i + 8, i + 15) if (seq[i], seq[j]) in CANONICAL)
    c = ["."] * n
    c[i], c[j] = "(", ")"
    c[40:46] = "x" * 6
    c[50] = "<"
    cons = "".join(c)
    res, *_ = run_case(ctx, n, cons=cons, span=20)
    assert len(res) == 180 and np.all(np.isfinite(res.log_z)) and np.any(res.dist2_q > 0)
    assert np.all(res.paired_prob[:, 40:46].view(np.uint32) == 0)
    moved = res.max_pair[res.max_dp > 0]
    assert len(moved) > 0 and np.all(moved[:, 1] - moved[:, 0] < 20)
    assert not np.any((moved >= 40) & (moved < 46)) and not np.any(moved[:, 1] == 50)
    ends = (moved[:, 0] == i) | (moved[:, 1] == i) | (moved[:, 0] == j) | (moved[:, 1] == j)
    assert np.all(moved[ends] == (i, j))  # a bracket's base pairs with its partner or not at all
    free = ctx.mutant_scan(seq, False, False)
    assert not same_bits(free.dist2_q, res.dist2_q)


def test_independent_cross_checks(ctx):
    """mode 0: ln Z = rnamc_log_partition_batch, paired_prob = rnamc_bpp_batch_sparse's, wild type = the plain entries'"""
    reset(ctx)
    n = 76
    seq = seq_of(n)
    _, _, recs = mutants_of(seq)
    res = ctx.mutant_scan(seq, False, False)
    assert same_bits(res.log_z, ctx.log_partition_batch(recs, False, False))
    sparse, zs = ctx.bpp_batch_sparse(recs, False, False, 0.5)
    assert same_bits(res.log_z, zs)
    for m, sp in enumerate(sparse):
        assert same_bits(res.paired_prob[m], sp.paired_prob), m
    wt_sparse, wt_z = ctx.bpp_batch_sparse([seq], False, False, 0.5)
    assert same_bits(res.wt_paired_prob, wt_sparse[0].paired_prob)
    assert np.float32(res.wt_log_z).tobytes() == wt_z[:1].tobytes()
    assert np.float32(res.wt_log_z).tobytes() == ctx.log_partition_batch([seq], False, False)[:1].tobytes()


def test_invariance_and_statistics(ctx, params):
    """the same bytes whatever the grouping, the chunking and the number of contexts; launches_mutant counts the
    compare launch (and the paired launch) of every group, and the wild type's paired launch"""
    from rna_algos_amd.mccaskill_algo import Pool
    reset(ctx)
    n = 76
    base, seq, _ = run_case(ctx, n)
    st = ctx.stats()
    assert st["n_groups"] == 2 and st["launches_mutant"] == 3
    try:
        ctx.set("group_max_seqs", 3)
        same_scan(ctx.mutant_scan(seq, False, False), base)
        st = ctx.stats()
        assert st["n_groups"] == 1 + 76  # the wild type's group, then three mutants a group
        assert st["launches_mutant"] == 1 + 2 * 76 and st["launches_other"] >= st["launches_mutant"] + st["n_groups"]
        reset(ctx)
        ctx.set("mutant_chunk_nt", 2 * n)  # two mutants a chunk: a position's mutants straddle chunks
        same_scan(ctx.mutant_scan(seq, False, False), base)
        st = ctx.stats()
        assert st["n_groups"] == 1 + 114 and st["launches_mutant"] == 1 + 2 * 114
        ctx.set("mutant_chunk_nt", 1)  # below one mutant: a mutant a chunk
        few = ctx.mutant_scan(seq, False, False, positions=[5, 40])
        assert ctx.stats()["n_groups"] == 1 + 6
        reset(ctx)
        same_scan(ctx.mutant_scan(seq, False, False, positions=[5, 40]), few)
    finally:
        reset(ctx)
    pool = Pool(params, devices=[0, 0])
    try:
        same_scan(pool.mutant_scan(seq, False, False), base)
        pool.set("mutant_chunk_nt", 5 * n)
        same_scan(pool.mutant_scan(seq, False, False), base)
        one = pool.mutant_scan(seq, False, False, positions=[])  # no mutant: one shard, the wild type alone
        assert len(one) == 0 and same_bits(one.wt_paired_prob, base.wt_paired_prob)
        assert one.wt_log_z == base.wt_log_z
    finally:
        pool.close()


def test_profiled_call_times_the_mutant_kernels(ctx):
    reset(ctx)
    seq = seq_of(76)
    ctx.set("profile", 1)
    try:
        ctx.mutant_scan(seq, False, False, positions=[3, 30])
        st = ctx.stats()
    finally:
        ctx.set("profile", 0)
    assert st["launches_mutant"] == 3 and 0 < st["ms_mutant"] < 1e3
    ctx.mutant_scan(seq, False, False, positions=[3])
    assert ctx.stats()["ms_mutant"] == 0


def test_chunks_groups_and_profile_together(ctx):
    """several chunks, several groups a chunk and a profiled call at once: 60 bases are 180 mutants; 600
    nucleotides a chunk are 18 chunks of 10 mutants, three mutants a group are four groups a chunk.  The same
    bytes as the call of one chunk and one group, and the statistics of the whole call: the wild type's group and
    its paired launch, then a compare and a paired launch per group"""
    reset(ctx)
    seq = seq_of(60)
    base = ctx.mutant_scan(seq, False, False)
    plain = ctx.stats()
    assert len(base) == 180 and plain["n_groups"] == 2 and plain["launches_mutant"] == 3 and plain["ms_mutant"] == 0
    try:
        ctx.set("mutant_chunk_nt", 600)
        ctx.set("group_max_seqs", 3)
        counts = []
        for profile in (0, 1):
            ctx.set("profile", profile)
            same_scan(ctx.mutant_scan(seq, False, False), base)
            st = ctx.stats()
            assert st["n_groups"] == 1 + 18 * 4 and st["launches_mutant"] == 1 + 2 * 72
            assert st["launches_other"] >= st["launches_mutant"] + st["n_groups"]
            assert st["launches_inside"] >= 73 and st["launches_outside"] >= 73
            assert st["workspace_bytes"] == plain["workspace_bytes"]  # (the context's workspace never shrinks)
            assert (0 < st["ms_mutant"] < 1e3 and st["ms_inside"] > 0 and st["ms_outside"] > 0) if profile else \
                (st["ms_mutant"] == 0 and st["ms_inside"] == 0 and st["ms_outside"] == 0)
            counts.append({k: v for k, v in st.items() if not k.startswith("ms_")})
        assert counts[0] == counts[1]  # (timing a call changes none of its counts)
    finally:
        ctx.set("profile", 0)
        reset(ctx)


def test_tree_order_mode(ctx):
    """summation mode 1: against the dense entry in mode 1 with the same call structure, the wild type alone,
    then the chunk's records"""
    reset(ctx)
    ctx.set("summation_mode", 1)
    try:
        res, *_ = run_case(ctx, 76)
        assert np.any(res.dist2_q > 0)
    finally:
        reset(ctx)


def check_against_the_cpu_oracle(ctx, params, contra=False, short=False):
    import oracle_lib as O
    reset(ctx)
    n = 30
    seq = seq_of(n)
    _, _, recs = mutants_of(seq)

    def oracle(s):
        ref, z = O.bpp(params.ptr, s, contra, short)
        return np.where(ref < 0, np.float32(-1), ref).astype(np.float32), z
    wt, wt_z = oracle(seq)
    tris, zs = zip(*(oracle(r) for r in recs))
    res = ctx.mutant_scan(seq, contra, short)
    check_against(res, n, seq, None, wt, wt_z, list(tris), zs)
    assert np.any(res.dist2_q > 0)
    return res


def test_against_the_cpu_oracle(ctx, params):
    """n = 30, Turner, reference order: the yardstick fed with the CPU oracle's triangles"""
    check_against_the_cpu_oracle(ctx, params)


# ---- allows_short_hairpins = 1 (CONTRAfold): the triangles carry pairs of span 1, 2 and 3, and the
# compare kernel meets moved cells on the first three diagonals

def short_moves(res):
    """the mutants whose largest change is at a pair with j - i < 4"""
    moved = res.max_dp > 0
    return int(np.count_nonzero(moved & (res.max_pair[:, 1] - res.max_pair[:, 0] < 4)))


@pytest.mark.parametrize("n,positions", [(76, None), (91, [0, 45, 90])])
def test_short_hairpins(ctx, params, n, positions):
    """all positions at n = 76 and the ends and middle at n = 91 (two strips), against the yardstick fed by
    the dense entry with the same flag.  The flag is seen -- the assertion used: some mutant's max_pair has
    span < 4 (the yardstick on the CPU oracle's triangles names such a pair for 72 of the 228 mutants at
    n = 76 and for 6 of the 9 at n = 91), which the scan without the flag never names; its paired_prob and
    ln Z differ too."""
    import short_pairs as SP
    reset(ctx)
    SP.assert_input_has_short_pairs(params, [seq_of(n)])
    res, seq, _ = run_case(ctx, n, contra=True, positions=positions, short=True)
    assert np.any(res.dist2_q > 0)
    print("mutants whose max_pair has span < 4:", short_moves(res), "of", len(res))
    assert short_moves(res) > 0
    plain = ctx.mutant_scan(seq, True, False, positions=positions)
    assert short_moves(plain) == 0
    assert not same_bits(res.paired_prob, plain.paired_prob) and not same_bits(res.log_z, plain.log_z)


def test_against_the_cpu_oracle_short_hairpins(ctx, params):
    """n = 30 with O.bpp(..., True, True)"""
    import short_pairs as SP
    SP.assert_input_has_short_pairs(params, [seq_of(30)])
    check_against_the_cpu_oracle(ctx, params, True, True)


def test_errors_leave_the_context_usable(ctx):
    from rna_algos_amd import _lib
    reset(ctx)
    seq = seq_of(37)
    with pytest.raises(_lib.RnamcError) as e:
        ctx.mutant_scan(seq, False, False, constraint="." * 20 + "(" + "." * 16)
    assert e.value.status == _lib.ERR_INVALID_ARG and "position 20" in str(e.value)
    with pytest.raises(_lib.RnamcError) as e:
        ctx.mutant_scan(seq, False, False, positions=[3, 37])
    assert e.value.status == _lib.ERR_INVALID_ARG
    run_case(ctx, 37, positions=[0, 36])


def test_cli_round_trip(params, tmp_path):
    """mutant_scan on a two-record FASTA: the lines of every record re-derived from Context.mutant_scan"""
    import subprocess
    import sys
    from rna_algos_amd import utils
    from rna_algos_amd.bin.mccaskill_algo import fmt_f32
    from rna_algos_amd.mccaskill_algo import Context
    utils.set_default_tables(params)
    seqs = [seq_of(33), seq_of(48)]
    fa = os.path.join(tmp_path, "in.fa")
    with open(fa, "w") as fh:
        for k, s in enumerate(seqs):
            fh.write(f">r{k}\n" + "".join("ACGU"[x] for x in s) + "\n")
    out = os.path.join(tmp_path, "scan.tsv")
    subprocess.check_call([sys.executable, "-m", "rna_algos_amd.bin.mutant_scan", "--synthetic-tables", "1", "-i", fa,
                           "-o", out, "--positions", "4-6,20,0", "--max-bp-span", "25"], cwd=ROOT,
                          stderr=subprocess.DEVNULL, timeout=300)
    fss = utils.FoldScoreSets.new(0.0)
    fss.transfer()
    c = Context(fss, device=0)
    want = []
    try:
        for k, s in enumerate(seqs):
            res = c.mutant_scan(s, False, False, positions=[4, 5, 6, 20, 0], max_bp_span=25)
            corr = res.profile_correlation()
            want.append(f">{k}\n")
            assert len(res) == 15 and np.any(res.dist2_q > 0)
            for m in range(len(res)):
                p = int(res.pos[m])
                want.append("\t".join([str(p), "ACGU"[s[p]], "ACGU"[res.base[m]], fmt_f32(res.log_z[m]),
                                       repr(float(res.delta_log_z[m])), repr(float(res.dist2[m])),
                                       fmt_f32(res.max_dp[m]), str(int(res.max_pair[m, 0])),
                                       str(int(res.max_pair[m, 1])), repr(float(corr[m]))]) + "\n")
    finally:
        c.close()
    assert open(out).read() == "".join(want)
