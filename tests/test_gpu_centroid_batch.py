"""rnamc_centroid_fold_batch / rnamc_centroid_fold_batch_multi on the GPU: mccaskill_algo and the
gamma-centroid fold of every record and threshold in one call, the bpp triangles staying on the
device.

The oracle throughout is O.centroid_fold(packed, n, gamma) applied to a triangle; "equal" means the
dot-bracket equals get_fold_str of the oracle's pairs, n_pairs equals the oracle's count and
expect_accuracy has the oracle's f32 bits.  No tolerances anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

GRID = [2.0 ** k for k in range(-7, 11)]  # src/bin/centroid_fold.rs:9-10
EDGE_LENS = [1, 2, 3, 5, 6, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 300]
EDGE_GAMMAS = [0.5, 2.0, 4.0, 64.0]


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def reset(ctx):
    for k, v in (("summation_mode", 0), ("group_max_seqs", 8192), ("centroid_chunk_bytes", 0)):
        ctx.set(k, v)


def raw(entry, handle, seqs, gammas, contra, short=False, cons=None, span=0, want_bpp=True):
    """the C entry itself -> (rows [s][g] str, n_pairs u32[s, g], acc f32[s, g], logz, triangles or None)"""
    from rna_algos_amd import _lib
    from rna_algos_amd.mccaskill_algo import _constraint_bytes, _pack
    lens, offsets, bases = _pack(seqs)
    g = np.ascontiguousarray(gammas, dtype=np.float32)
    ng = len(g)
    rows = np.full(int(offsets[-1]) * ng, ord("?"), dtype=np.uint8)
    npairs = np.full((len(seqs), ng), 0xdeadbeef, dtype=np.uint32)
    acc = np.full((len(seqs), ng), np.nan, dtype=np.float32)
    logz = np.full(len(seqs), np.nan, dtype=np.float32)
    out_offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens * (lens + 1) // 2, out=out_offsets[1:])
    bpp = np.full(int(out_offsets[-1]), np.nan, dtype=np.float32)
    _lib.check(entry(handle, len(seqs), bases.ctypes.data, offsets.ctypes.data,
                     _constraint_bytes(cons, lens), span, int(contra), int(short), g.ctypes.data, ng,
                     rows.ctypes.data, npairs.ctypes.data, acc.ctypes.data, logz.ctypes.data,
                     bpp.ctypes.data if want_bpp else None,
                     out_offsets.ctypes.data if want_bpp else None))
    strs = []
    for s in range(len(seqs)):
        n, base = int(lens[s]), int(offsets[s]) * ng
        strs.append([bytes(rows[base + k * n:base + (k + 1) * n]).decode() for k in range(ng)])
    tris = [bpp[int(out_offsets[s]):int(out_offsets[s + 1])] for s in range(len(seqs))] if want_bpp else None
    return strs, npairs, acc, logz, tris


def ctx_raw(ctx, seqs, gammas, contra, **kw):
    from rna_algos_amd import _lib
    return raw(_lib.lib().rnamc_centroid_fold_batch, ctx._h, seqs, gammas, contra, **kw)


_oracle_cache = {}


def oracle(tri, n, gamma):
    """(dot-bracket, count, f32 bits of the accuracy) of the CPU oracle on one triangle; computed once
    per (triangle, threshold) and shared"""
    key = (n, float(gamma), tri.tobytes())
    if key not in _oracle_cache:
        pairs, acc = O.centroid_fold(tri, n, gamma)
        s = ["."] * n
        for i, j in pairs:
            s[i], s[j] = "(", ")"
        _oracle_cache[key] = ("".join(s), len(pairs), int(np.float32(acc).view(np.uint32)))
    return _oracle_cache[key]


def assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris):
    for s, seq in enumerate(seqs):
        for k, gamma in enumerate(gammas):
            db, cnt, bits = oracle(tris[s], len(seq), np.float32(gamma))
            assert strs[s][k] == db, (s, len(seq), gamma)
            assert int(npairs[s, k]) == cnt, (s, len(seq), gamma)
            assert int(acc[s, k].view(np.uint32)) == bits, (s, len(seq), gamma, acc[s, k])


def edge_batch():
    from rna_algos_amd.workloads import synthetic_seq
    return [synthetic_seq(n, seed=n) for n in EDGE_LENS]


@pytest.fixture(scope="module")
def edge_result(ctx):
    """the 20-sequence batch of shape edges through the entry with default knobs (shared)"""
    reset(ctx)
    seqs = edge_batch()
    res = ctx_raw(ctx, seqs, EDGE_GAMMAS, False)
    return seqs, res, ctx.stats()


@pytest.mark.parametrize("contra", [False, True])
def test_trnas(ctx, params, trnas, contra):
    """both models, default mode, the reference's 18 thresholds plus 0.5 and 3.7: triangles and log_z equal
    mccaskill_algo_batch's bit for bit, every (s, g) equals the oracle on them, and bpp = NULL changes nothing"""
    from rna_algos_amd.centroid_fold import centroid_fold_batch
    from rna_algos_amd.mccaskill_algo import mccaskill_algo_batch
    reset(ctx)
    seqs = [s for _, s in trnas]
    gammas = GRID + [0.5, 3.7]
    folds, logz, mats = centroid_fold_batch(seqs, gammas, contra, False, params, return_bpp=True)
    ref_mats, ref_logz = mccaskill_algo_batch(seqs, contra, False, params)
    assert np.array_equal(logz.view(np.uint32), ref_logz.view(np.uint32))
    for m, r in zip(mats, ref_mats):
        assert np.array_equal(m.packed.view(np.uint32), r.packed.view(np.uint32))
    strs, npairs, acc, logz2, tris = ctx_raw(ctx, seqs, gammas, contra)
    assert np.array_equal(logz2.view(np.uint32), ref_logz.view(np.uint32))
    for t, r in zip(tris, ref_mats):
        assert np.array_equal(t.view(np.uint32), r.packed.view(np.uint32))
    assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)
    for s in range(len(seqs)):
        for k in range(len(gammas)):
            assert folds[s][k][0] == strs[s][k]
            assert np.float32(folds[s][k][1]).view(np.uint32) == acc[s, k].view(np.uint32)
    strs0, npairs0, acc0, logz0, none = ctx_raw(ctx, seqs, gammas, contra, want_bpp=False)
    assert none is None and strs0 == strs and np.array_equal(npairs0, npairs)
    assert np.array_equal(acc0.view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(logz0.view(np.uint32), logz2.view(np.uint32))
    folds0, _ = centroid_fold_batch(seqs, gammas, contra, False, params)
    assert [[f[0] for f in row] for row in folds0] == strs


def test_shape_edges(ctx, edge_result):
    """n = 1 .. 300 around every wave, workgroup and launch-form boundary in one batch: every (s, g) equals
    the oracle (n = 1 and n = 2 have no cell above the main diagonal: all '.')"""
    seqs, (strs, npairs, acc, _, tris), _ = edge_result
    assert_equal_oracle(seqs, EDGE_GAMMAS, strs, npairs, acc, tris)
    assert strs[0] == ["."] * 4 and strs[1] == [".."] * 4
    assert any("(" in x for row in strs for x in row)


@pytest.mark.parametrize("case", ["groups_of_3", "reversed", "small_chunks"])
def test_shape_edges_independent_of_schedule(ctx, edge_result, case):
    """per-sequence results do not depend on grouping, batch order or chunking (the chunk budget of
    400 000 bytes holds two of the 300-nt items' 180 736-byte matrices: the thresholds of one sequence
    that need the fill land in different chunks, and one group splits into several)"""
    seqs, (strs, npairs, acc, logz, tris), _ = edge_result
    reset(ctx)
    order = list(range(len(seqs)))
    if case == "groups_of_3":
        ctx.set("group_max_seqs", 3)
    elif case == "reversed":
        order.reverse()
    else:
        ctx.set("centroid_chunk_bytes", 400000)
    try:
        strs2, npairs2, acc2, logz2, tris2 = ctx_raw(ctx, [seqs[x] for x in order], EDGE_GAMMAS, False)
    finally:
        reset(ctx)
    for pos, x in enumerate(order):
        assert strs2[pos] == strs[x], EDGE_LENS[x]
        assert np.array_equal(npairs2[pos], npairs[x])
        assert np.array_equal(acc2[pos].view(np.uint32), acc[x].view(np.uint32))
        assert logz2[pos].view(np.uint32) == logz[x].view(np.uint32)
        assert np.array_equal(tris2[pos].view(np.uint32), tris[x].view(np.uint32))


def test_ties(ctx):
    """the traceback compares floats for equality: repeats, alternating GC, a long stem, and poly-A
    (every bpp absent: all rows '.', accuracy 0)"""
    from rna_algos_amd.utils import bytes2seq
    reset(ctx)
    texts = ["GGGAAACCC" * 8, "GC" * 30, "G" * 20 + "A" * 4 + "C" * 20, "A" * 40]
    seqs = [bytes2seq(t.encode()) for t in texts]
    gammas = [1.0, 2.0, 4.0, 1024.0]
    for contra in (False, True):
        strs, npairs, acc, _, tris = ctx_raw(ctx, seqs, gammas, contra)
        assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)
        assert strs[3] == ["." * 40] * 4 and not npairs[3].any()
        assert np.array_equal(acc[3].view(np.uint32), np.zeros(4, np.uint32))


def test_long_sums(ctx):
    """one 700-nt record, alone and inside a batch of short records: sums cut over the waves of a
    workgroup (d > 64) and traceback scans longer than 64"""
    from rna_algos_amd.workloads import synthetic_seq
    reset(ctx)
    long = synthetic_seq(700, seed=700)
    gammas = [2.0, 8.0, 256.0]
    strs, npairs, acc, _, tris = ctx_raw(ctx, [long], gammas, False)
    assert_equal_oracle([long], gammas, strs, npairs, acc, tris)
    batch = [synthetic_seq(n, seed=1000 + n) for n in (40, 90)] + [long] + \
        [synthetic_seq(n, seed=1000 + n) for n in (17, 150)]
    strs2, npairs2, acc2, _, tris2 = ctx_raw(ctx, batch, gammas, False)
    assert strs2[2] == strs[0] and np.array_equal(npairs2[2], npairs[0])
    assert np.array_equal(acc2[2].view(np.uint32), acc[0].view(np.uint32))
    assert_equal_oracle(batch, gammas, strs2, npairs2, acc2, tris2)


def test_tree_order(ctx):
    """summation_mode 1 (both lane settings of its batch form): every (s, g) equals the oracle on the
    triangles the SAME call returned; no cross-call comparison in this mode"""
    from rna_algos_amd.workloads import synthetic_seq
    seqs = [synthetic_seq(n, seed=n) for n in (200, 257, 313, 390, 444, 500, 555, 600)]
    gammas = [2.0, 4.0, 32.0]
    try:
        for lane in (1, 2):
            reset(ctx)
            ctx.set("summation_mode", 1)
            ctx.set("tree_lane", lane)
            strs, npairs, acc, logz, tris = ctx_raw(ctx, seqs, gammas, False)
            assert np.isfinite(logz).all()
            assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)
            assert any("(" in x for row in strs for x in row)
    finally:
        ctx.set("tree_lane", 1)
        reset(ctx)


# ---- beyond d = 1024: the sixteen-wave form of the fill (launch_centroid_batch picks one wave per 64 cells
# for d <= 64, four for d <= 1024, sixteen beyond), k scans of 16 steps and more in the traceback, the
# `active` prefix shrinking on diagonals past 1024, chunk cuts between multi-megabyte items.
# n = 1025 ends at d = 1024, the last four-wave launch; n = 1026 has exactly one cell at d = 1025;
# n = 1100 has 75 sixteen-wave diagonals, on which the shorter items have dropped out of `active`.
BIG_LENS = [1100, 1026, 1025, 700, 90]
BIG_GAMMAS = [2.0, 8.0, 256.0]


def big_batch():
    from rna_algos_amd.workloads import synthetic_seq
    return [synthetic_seq(n, seed=n) for n in BIG_LENS]


def item_floats(n):
    """centroid_item_floats (rnamc_device.h) restated: the n(n+1)/2 floats of an item's packed triangle,
    rounded up to a multiple of 64"""
    return (n * (n + 1) // 2 + 63) // 64 * 64


@pytest.fixture(scope="module")
def big_result(ctx):
    """the five-record batch around d = 1024 through the entry with default knobs (shared, left unchanged)"""
    reset(ctx)
    seqs = big_batch()
    res = ctx_raw(ctx, seqs, BIG_GAMMAS, False)
    return seqs, res, ctx.stats()


def test_launch_form_edge(ctx, big_result):
    """Turner, mode 0, default knobs: every (s, g) of the batch around the four-wave / sixteen-wave edge
    equals the oracle, and every record past 1024 nt has a fold that holds a pair"""
    seqs, (strs, npairs, acc, logz, tris), _ = big_result
    assert np.isfinite(logz).all()
    assert_equal_oracle(seqs, BIG_GAMMAS, strs, npairs, acc, tris)
    for s, n in enumerate(BIG_LENS):
        if n > 1024:
            assert any("(" in x for x in strs[s]), n


def test_long_record_alone_equals_batch(ctx, big_result):
    """the 1100-nt record alone (every launch has one item): the rows, counts and accuracy bits it has
    inside the batch"""
    seqs, (strs, npairs, acc, logz, tris), _ = big_result
    reset(ctx)
    strs1, npairs1, acc1, logz1, tris1 = ctx_raw(ctx, [seqs[0]], BIG_GAMMAS, False)
    assert strs1[0] == strs[0]
    assert np.array_equal(npairs1[0], npairs[0])
    assert np.array_equal(acc1[0].view(np.uint32), acc[0].view(np.uint32))
    assert logz1[0].view(np.uint32) == logz[0].view(np.uint32)
    assert np.array_equal(tris1[0].view(np.uint32), tris[0].view(np.uint32))


def test_contrafold_at_size(ctx):
    """CONTRAfold once past d = 1024, beside a 300-nt record"""
    from rna_algos_amd.workloads import synthetic_seq
    reset(ctx)
    seqs = [synthetic_seq(n, seed=n) for n in (1100, 300)]
    gammas = [4.0, 64.0]
    strs, npairs, acc, logz, tris = ctx_raw(ctx, seqs, gammas, True)
    assert np.isfinite(logz).all()
    assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)
    assert any("(" in x for x in strs[0])


def test_ties_at_size(ctx):
    """repeats and alternating GC past 1024 nt, both models: the traceback's float equality tests with k
    scans longer than 64 and bifurcations parked on the stack"""
    from rna_algos_amd.utils import bytes2seq
    reset(ctx)
    texts = ["GGGAAACCC" * 123, "GC" * 520]
    assert [len(t) for t in texts] == [1107, 1040]
    seqs = [bytes2seq(t.encode()) for t in texts]
    gammas = [1.0, 4.0, 1024.0]
    for contra in (False, True):
        strs, npairs, acc, _, tris = ctx_raw(ctx, seqs, gammas, contra)
        assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)
        assert any("(" in x for row in strs for x in row)


def hairpin(length):
    """G^s A^l C^s of the given length (l = 4 or 5) and the constraint string of its s nested pairs"""
    loop = 4 + length % 2
    s = (length - loop) // 2
    return "G" * s + "A" * loop + "C" * s, "(" * s + "." * loop + ")" * s


def test_every_wave_slice_decides_a_cell(ctx):
    """The maximum over the splits k of a cell is highly redundant on natural inputs (any k in an unpaired
    gap between two domains attains it), so a sixteen-wave join that loses one wave's partial maximum
    passes the batches above.  Here it cannot: record r is two hairpins of 512 + r and 514 nt that abut,
    with a constraint string that leaves only their nested pairs, so at gamma = 1024 the fold is both
    stems and the top cell (0, n-1), at d = n - 1 > 1024, has ONE maximal candidate: the split after the
    first hairpin, k = 511 + r.  Any other split cuts a stem pair of positive gain, a skip loses an outer
    pair, and (0, n-1) itself is no pair.  Wave w takes the splits a = k - i = 1 + w (mod 16): the sixteen
    records put the deciding split in each of the sixteen waves once.  expect_accuracy = M(0, n-1)."""
    from rna_algos_amd.utils import bytes2seq
    reset(ctx)
    seqs, cons, firsts = [], [], []
    for r in range(16):
        a, ca = hairpin(512 + r)
        b, cb = hairpin(514)
        seqs.append(bytes2seq((a + b).encode()))
        cons.append(ca + cb)
        firsts.append(512 + r)
    assert sorted((l1 - 2) % 16 for l1 in firsts) == list(range(16))  # a = l1 - 1 = 1 + w (mod 16)
    assert min(len(s) for s in seqs) - 1 > 1024
    gammas = [1024.0]
    strs, npairs, acc, logz, tris = ctx_raw(ctx, seqs, gammas, False, cons=cons)
    assert np.isfinite(logz).all()
    for s, l1 in enumerate(firsts):
        assert strs[s][0] == cons[s], l1  # every designed pair is in the fold, and nothing else can be
    assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)


def test_chunk_cuts_between_long_items(ctx, big_result):
    """centroid_chunk_bytes = the bytes of two 1100-nt items: 2 * item_floats(1100) * 4 = 2 * 605 568 * 4
    (a chunk takes items while the sum of their centroid_item_floats stays within the budget in floats, so
    this value admits two such items and not a third).  Items go longest record first, thresholds in
    order: the chunks are [1100, 1100], [1100, 1026], ... -- the thresholds of the 1100-nt and of the
    1026-nt record land in different chunks.  Results equal the default-knob run bit for bit."""
    seqs, (strs, npairs, acc, logz, tris), stats = big_result
    assert item_floats(1100) == 605568
    chunk_bytes = 2 * item_floats(1100) * 4
    assert chunk_bytes // 4 >= 2 * item_floats(1100) and chunk_bytes // 4 < 3 * item_floats(1100)
    assert item_floats(1100) + item_floats(1026) <= chunk_bytes // 4 < item_floats(1100) + 2 * item_floats(1026)
    reset(ctx)
    ctx.set("centroid_chunk_bytes", chunk_bytes)
    try:
        strs2, npairs2, acc2, logz2, tris2 = ctx_raw(ctx, seqs, BIG_GAMMAS, False)
        stats2 = ctx.stats()
    finally:
        reset(ctx)
    assert strs2 == strs
    assert np.array_equal(npairs2, npairs)
    assert np.array_equal(acc2.view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(logz2.view(np.uint32), logz.view(np.uint32))
    for a, b in zip(tris2, tris):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the cut happened: every fold of the 1100-nt record is non-empty, so its three items went through the
    # fill, and the third opens a second chunk of 1100 + 1 launches that the default run does not make
    assert all("(" in x for x in strs[0])
    print("launches_other", stats["launches_other"], "chunked", stats2["launches_other"])
    assert stats2["launches_other"] >= stats["launches_other"] + 1101


def test_tree_order_at_size(ctx):
    """summation_mode 1, tree_lane 1, past d = 1024: every (s, g) equals the oracle on the triangles the
    SAME call returned, as test_tree_order"""
    from rna_algos_amd.workloads import synthetic_seq
    seqs = [synthetic_seq(n, seed=n) for n in (1100, 1030)]
    gammas = [2.0, 32.0]
    try:
        reset(ctx)
        ctx.set("summation_mode", 1)
        ctx.set("tree_lane", 1)
        strs, npairs, acc, logz, tris = ctx_raw(ctx, seqs, gammas, False)
        assert np.isfinite(logz).all()
        assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)
        assert all(any("(" in x for x in row) for row in strs)
    finally:
        ctx.set("tree_lane", 1)
        reset(ctx)


def test_trnas_short_hairpins(ctx, params, trnas):
    """allows_short_hairpins = 1 (CONTRAfold): triangles and log_z equal mccaskill_algo_batch(seqs, True,
    True)'s bit for bit, every (s, g) equals the oracle on them, and at gamma = 1024 some fold holds a pair
    with j - i < 4 -- which the CPU oracle's fold of O.bpp(..., True, True) has too (the input condition)"""
    import short_pairs as SP
    from rna_algos_amd.mccaskill_algo import mccaskill_algo_batch
    reset(ctx)
    seqs = [s for _, s in trnas]
    gammas = GRID + [0.5, 3.7]
    assert gammas[17] == 1024.0
    SP.assert_input_has_short_pairs(params, seqs)
    cpu_short = 0
    for s in seqs:
        tri, _ = O.bpp(params.ptr, s, True, True)
        pairs, _ = O.centroid_fold(np.where(tri < 0, np.float32(-1), tri).astype(np.float32), len(s), np.float32(1024.0))
        cpu_short += sum(1 for i, j in pairs if j - i < 4)
    assert cpu_short > 0
    ref_mats, ref_logz = mccaskill_algo_batch(seqs, True, True, params)
    strs, npairs, acc, logz, tris = ctx_raw(ctx, seqs, gammas, True, short=True)
    assert np.array_equal(logz.view(np.uint32), ref_logz.view(np.uint32))
    for t, r in zip(tris, ref_mats):
        assert np.array_equal(t.view(np.uint32), r.packed.view(np.uint32))
        assert SP.short_present(t, r.n) > 0
    assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)
    gpu_short = sum(1 for s in range(len(seqs)) for i, j in SP.pairs_of(strs[s][17]) if j - i < 4)
    assert gpu_short > 0


def test_constraints(ctx, params, trnas):
    """an x run, a bracket pair and max_bp_span = 40 on the tRNAs (mode 0): triangles equal the constrained
    mccaskill_algo_batch's bit for bit, folds equal the oracle's on them, every row is compatible"""
    from rna_algos_amd.mccaskill_algo import is_compatible, mccaskill_algo_batch
    reset(ctx)
    seqs = [s for _, s in trnas]
    cons = []
    for s in seqs:
        c = ["."] * len(s)
        c[10:16] = "x" * 6
        c[2], c[30] = "(", ")"
        cons.append("".join(c))
    gammas = [2.0, 4.0, 1024.0]
    span = 40
    strs, npairs, acc, logz, tris = ctx_raw(ctx, seqs, gammas, False, cons=cons, span=span)
    ref_mats, ref_logz = mccaskill_algo_batch(seqs, False, False, params, constraints=cons, max_bp_span=span)
    assert np.array_equal(logz.view(np.uint32), ref_logz.view(np.uint32))
    for t, r in zip(tris, ref_mats):
        assert np.array_equal(t.view(np.uint32), r.packed.view(np.uint32))
    assert_equal_oracle(seqs, gammas, strs, npairs, acc, tris)
    for s in range(len(seqs)):
        for row in strs[s]:
            assert is_compatible(row, cons[s], span)
    assert any("(" in x for row in strs for x in row)


def test_pool_equals_context(ctx, params):
    """the _multi entry over the default devices equals the single-context entry (12 records, mixed lengths)"""
    from rna_algos_amd import _lib
    from rna_algos_amd.mccaskill_algo import _pool_for
    from rna_algos_amd.workloads import synthetic_seq
    reset(ctx)
    seqs = [synthetic_seq(n, seed=50 + n) for n in (120, 33, 260, 75, 5, 190, 64, 301, 18, 99, 150, 222)]
    gammas = [0.5, 4.0, 128.0]
    pool = _pool_for(params)
    a = ctx_raw(ctx, seqs, gammas, True)
    b = raw(_lib.lib().rnamc_centroid_fold_batch_multi, pool._h, seqs, gammas, True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))
    for x, y in zip(a[4], b[4]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    c = raw(_lib.lib().rnamc_centroid_fold_batch_multi, pool._h, seqs, gammas, True, want_bpp=False)
    assert c[0] == a[0] and np.array_equal(c[1], a[1])


@pytest.mark.parametrize("single", [False, True])
def test_cli_files(params, tmp_path, single):
    """the CLI's files are byte-identical to files written from the host centroid_fold per record
    (write_centroid_fold), for the 18 thresholds and with -g 4"""
    from rna_algos_amd import utils
    from rna_algos_amd.bin import centroid_fold as cli
    from rna_algos_amd.bin.mccaskill_algo import fmt_f32
    from rna_algos_amd.mccaskill_algo import mccaskill_algo_batch
    from rna_algos_amd.workloads import synthetic_seq
    utils.set_default_tables(params)
    fa = os.path.join(tmp_path, "in.fa")
    with open(fa, "w") as fh:
        for k, n in enumerate((30, 77, 131, 260, 520)):
            fh.write(f">r{k}\n" + "".join("ACGU"[b] for b in synthetic_seq(n, seed=7000 + n)) + "\n")
    recs = utils.read_fasta(fa)
    out = os.path.join(tmp_path, "out")
    assert cli.main(["-i", fa, "-o", out] + (["-g", "4"] if single else [])) == 0
    gammas = [4.0] if single else GRID
    assert sorted(os.listdir(out)) == sorted(f"centroid_threshold={fmt_f32(g)}.fa" for g in gammas)
    fss = utils.FoldScoreSets.new(0.0)
    fss.transfer()
    mats, _ = mccaskill_algo_batch([s for _, s in recs], False, False, fss)
    want = os.path.join(tmp_path, "want.fa")
    for g in gammas:
        cli.write_centroid_fold(mats, recs, g, want)
        name = f"centroid_threshold={fmt_f32(g)}.fa"
        assert open(os.path.join(out, name), "rb").read() == open(want, "rb").read(), name


def test_argument_errors_with_a_context(ctx):
    """the argument checks of the CPU tests, on a live context"""
    from rna_algos_amd import _lib
    L = _lib.lib()
    bases = np.zeros(8, np.uint8)
    offsets = np.array([0, 8], np.uint64)
    g = np.array([4.0], np.float32)
    rows = np.zeros(8, np.uint8)
    bpp = np.zeros(36, np.float32)

    def call(ng, bpp_p, oo_p):
        return L.rnamc_centroid_fold_batch(ctx._h, 1, bases.ctypes.data, offsets.ctypes.data, None, 0, 0, 0,
                                           g.ctypes.data, ng, rows.ctypes.data, None, None, None, bpp_p, oo_p)
    assert call(0, None, None) == _lib.ERR_INVALID_ARG
    assert call(1, bpp.ctypes.data, None) == _lib.ERR_INVALID_ARG
    assert call(1, None, offsets.ctypes.data) == _lib.ERR_INVALID_ARG
    assert call(1, None, None) == _lib.OK and bytes(rows) == b"........"  # (poly-A)


def test_no_hidden_host_route(edge_result):
    """the entry does not work by rnamc_centroid_fold_multi per record (n - 1 launches each: 2 397 for this
    batch).  One chunk per group with the default budget: a chunk makes (longest n) + 1 launches (the zeroed
    main diagonals, n - 1 anti-diagonals, the traceback), the group adds one for p_max, and its bpp sweep
    counts its init and finalize kernels under launches_other: (longest n) + 4 per group, 304 for this batch
    (counted from the launch sites; the test prints the figure).  The bound allows 8."""
    _, _, stats = edge_result
    groups = stats["n_groups"]
    assert groups >= 1
    print("launches_other", stats["launches_other"], "groups", groups)
    assert stats["launches_other"] < groups * 1 * (max(EDGE_LENS) + 8)
