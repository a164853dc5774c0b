"""rnamc_bpp_alignment / rnamc_bpp_alignment_multi on the GPU: the rows of a multiple alignment folded
without their gaps, their pair probabilities mapped onto alignment columns and averaged over all rows
(DESIGN.md section 17).

The yardstick is a numpy restatement of the contract in include/rnamc.h -- per row the column map, int64
sums of min(rint(p * 2^44), 2^45) and row counters per column pair, the division by n_rows * 2^44, the
column-profile loop -- fed with the triangles of the dense entry (rnamc_bpp_batch_constrained) on the
same context for the ungapped rows.  Every comparison is bit for bit, no tolerances (but for the one
the contract itself states for a single row)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
Q = float(2 ** 44)
GAP = 4


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def reset(ctx):
    for k, v in (("summation_mode", 0), ("group_max_seqs", 8192), ("centroid_chunk_bytes", 0)):
        ctx.set(k, v)


def seq_of(n, seed=0):
    from rna_algos_amd.workloads import synthetic_seq
    return synthetic_seq(n, seed=1700 + 131 * seed + n)


def rows_of(masks, seed=0):
    """boolean masks (True: a base in that column) -> the alignment, every row's bases synthetic"""
    masks = np.asarray(masks, bool)
    rows = np.full(masks.shape, GAP, np.uint8)
    for s, m in enumerate(masks):
        rows[s, m] = seq_of(int(m.sum()), seed + s)
    return rows


def ungapped(rows):
    return [r[r != GAP] for r in rows]


def tri_off(n, d):
    return d * n - d * (d - 1) // 2


def yardstick(rows, tris):
    """include/rnamc.h restated: the packed triangles of the ungapped rows -> (avg f32[n_cols (n_cols + 1) / 2],
    col_paired f32[n_cols])"""
    n_rows, n_cols = rows.shape
    S = np.zeros(tri_off(n_cols, n_cols), np.int64)
    present = np.zeros(tri_off(n_cols, n_cols), np.uint32)
    for r, tri in zip(rows, tris):
        cmap = np.nonzero(r != GAP)[0].astype(np.int64)  # map_s[k]: the column of the row's k-th base
        n = len(cmap)
        assert tri.shape == (tri_off(n, n),)
        off = n
        for d in range(1, n):
            cells = tri[off:off + n - d]
            off += n - d
            have = cells > -0.5
            q = np.minimum(np.rint(np.where(have, cells, 0).astype(np.float64) * Q), 2.0 * Q)  # (ties to even)
            ci, cj = cmap[:n - d], cmap[d:]
            at = tri_off(n_cols, cj - ci) + ci  # (distinct inside one row: a plain indexed add is exact)
            S[at[have]] += q[have].astype(np.int64)
            present[at[have]] += 1
    val = (S.astype(np.float64) / (np.float64(n_rows) * Q)).astype(np.float32)
    avg = np.where(present > 0, val, np.float32(-1)).astype(np.float32)
    avg[:n_cols] = -1
    paired = np.zeros(n_cols, np.float32)
    for d in range(1, n_cols):
        cells = avg[tri_off(n_cols, d):tri_off(n_cols, d + 1)]
        add = np.where(cells > -0.5, cells, np.float32(0)).astype(np.float32)  # (x + 0 == x: an absent pair adds nothing)
        paired[:n_cols - d] = paired[:n_cols - d] + add
        paired[d:] = paired[d:] + add
    return avg, paired


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_case(ctx, rows, contra=False, short=False, span=0, gammas=(), entry=None):
    recs = ungapped(rows)
    mats, logz = ctx.bpp_batch(recs, contra, short, max_bp_span=span)
    want, want_paired = yardstick(rows, [np.asarray(m.packed) for m in mats])
    res = (entry or ctx.bpp_alignment)(rows, contra, short, gammas, span)
    key = (rows.shape, contra, short, span)
    assert res.n_cols == rows.shape[1] and res.bpp.n == rows.shape[1]
    assert same_bits(np.asarray(res.bpp.packed), want), key
    assert same_bits(res.col_paired, want_paired), key
    assert same_bits(res.log_z, logz), key
    assert res.row_len.tolist() == [len(r) for r in recs]
    p = np.asarray(res.bpp.packed)
    assert np.all((p == -1) | ((p >= 0) & (p <= 1))), key  # no cell outside [0, 1] u {-1}
    assert np.all(p[:rows.shape[1]] == -1)
    return res, want, want_paired


def check_folds(res, gammas):
    """every row string, count and expect_accuracy = rnamc_centroid_fold of the returned triangle"""
    from rna_algos_amd.centroid_fold import centroid_fold, get_fold_str
    assert len(res.folds) == len(gammas)
    for g, (db, acc) in zip(gammas, res.folds):
        want = centroid_fold(res.bpp, res.n_cols, g)
        assert db == get_fold_str(want, res.n_cols), g
        assert db.count("(") == len(want.basepair_pos_pairs) == db.count(")")
        assert np.float32(acc).tobytes() == np.float32(want.expect_accuracy).tobytes(), g


# ---- edges

def test_one_by_one(ctx):
    reset(ctx)
    res, *_ = run_case(ctx, np.array([[2]], np.uint8), gammas=(2.0,))
    assert np.asarray(res.bpp.packed).tolist() == [-1.0] and res.col_paired.tolist() == [0.0]
    assert res.folds[0][0] == "." and res.folds[0][1] == 0


def test_one_base_row_among_longer_rows(ctx):
    reset(ctx)
    masks = np.ones((3, 40), bool)
    masks[1] = False
    masks[1, 17] = True
    res, want, _ = run_case(ctx, rows_of(masks))
    assert res.row_len.tolist() == [40, 1, 40] and np.any(want > 0)


def plain_rule(got, plain):
    """equal to the plain bpp bit for bit where p >= 2^-20, within 2^-45 below; the same key set"""
    assert np.array_equal(got > -0.5, plain > -0.5) and np.count_nonzero(plain > -0.5) > 0
    big = plain >= np.float32(2.0 ** -20)
    assert np.count_nonzero(big) > 0
    assert got[big].tobytes() == plain[big].tobytes()
    small = (plain > -0.5) & ~big
    assert np.all(np.abs(got[small].astype(np.float64) - plain[small].astype(np.float64)) <= 2.0 ** -45)


def test_one_row_without_gaps_is_the_plain_bpp(ctx):
    reset(ctx)
    seq = seq_of(50)
    res, *_ = run_case(ctx, seq[None, :].copy())
    mats, _ = ctx.bpp_batch([seq], False, False)
    plain = np.asarray(mats[0].packed).copy()
    plain[:50] = -1  # (the main diagonal is no pair)
    plain_rule(np.asarray(res.bpp.packed), plain)


def test_identical_gapless_rows_average_to_the_single_row(ctx):
    reset(ctx)
    seq = seq_of(50)
    one, *_ = run_case(ctx, seq[None, :].copy())
    res, *_ = run_case(ctx, np.repeat(seq[None, :], 8, axis=0))
    assert same_bits(np.asarray(res.bpp.packed), np.asarray(one.bpp.packed))  # 8 q / (8 * 2^44) is q / 2^44
    assert same_bits(res.col_paired, one.col_paired)
    mats, _ = ctx.bpp_batch([seq], False, False)
    plain = np.asarray(mats[0].packed).copy()
    plain[:50] = -1
    plain_rule(np.asarray(res.bpp.packed), plain)


# ---- block and wave edges of the accumulate kernel

def test_rows_whose_triangles_straddle_blocks(ctx):
    """rows of 22, 23, 32 and 33 bases in one call: triangles of 253, 276, 528 and 561 cells, around 256 and 512"""
    reset(ctx)
    lens = [22, 23, 32, 33]
    assert [n * (n + 1) // 2 for n in lens] == [253, 276, 528, 561]
    masks = np.zeros((4, 36), bool)
    for s, n in enumerate(lens):
        masks[s, s:s + n] = True  # (leading and trailing gaps)
    res, want, _ = run_case(ctx, rows_of(masks))
    assert np.any(want > 0)


@pytest.mark.parametrize("contra", [False, True])
def test_rows_of_one_wave_and_one_more(ctx, contra):
    reset(ctx)
    masks = np.ones((2, 70), bool)
    masks[0, 64:] = False              # 64 bases, trailing gaps
    masks[1, [3, 20, 21, 40, 69]] = False  # 65 bases, internal gaps
    res, want, _ = run_case(ctx, rows_of(masks), contra=contra)
    assert res.row_len.tolist() == [64, 65] and np.any(want > 0)


# ---- variable lengths in one launch

def variable_rows():
    """12 rows of 1 .. 90 bases over 130 columns: gaps leading, trailing and internal, column 77 all gaps, rows 0
    and 1 without a common column"""
    lens = [1, 2, 5, 9, 17, 30, 41, 52, 64, 77, 83, 90]
    n_cols = 130
    masks = np.zeros((12, n_cols), bool)
    masks[0, 100] = True                      # one base
    masks[1, [3, 60]] = True                  # two bases, far apart; no column of row 0
    for s, n in enumerate(lens[2:], start=2):
        free = [c for c in range(n_cols) if c != 77]
        if s % 3 == 0:
            cols = free[:n]                   # trailing gaps
        elif s % 3 == 1:
            cols = free[len(free) - n:]       # leading gaps
        else:
            cols = [c for c in free if c % 4 != 1][:n]  # internal gaps: every fourth column
        masks[s, cols] = True
    assert masks.sum(axis=1).tolist() == lens and not masks[:, 77].any() and not (masks[0] & masks[1]).any()
    return rows_of(masks)


def test_variable_lengths_in_one_launch(ctx):
    reset(ctx)
    rows = variable_rows()
    res, want, want_paired = run_case(ctx, rows)
    n_cols = rows.shape[1]
    dense = res.bpp.dense()
    assert np.all(dense[77, :] == -1) and np.all(dense[:, 77] == -1)  # the all-gap column has no pair
    assert res.col_paired[77].tobytes() == np.float32(0).tobytes()
    assert np.any(want > 0) and np.any(want_paired > 0)
    assert ctx.stats()["n_groups"] == 1
    assert res.bpp.to_dict(0.25) == {k: v for k, v in res.bpp.to_dict().items() if v >= 0.25}
    i, j, p = res.pairs()
    assert len(p) == np.count_nonzero(want > -0.5) and np.all(i < j) and np.all(j < n_cols)


# ---- finalize edges

@pytest.mark.parametrize("n_cols", [63, 64, 65, 257])
def test_column_counts_around_the_workgroup(ctx, n_cols):
    reset(ctx)
    masks = np.ones((3, n_cols), bool)
    masks[0, :4] = False
    masks[1, n_cols // 2:n_cols // 2 + 6] = False
    masks[2, -3:] = False
    res, want, _ = run_case(ctx, rows_of(masks, seed=n_cols))
    assert np.any(want > 0)
    assert want[-1] == res.bpp[0, n_cols - 1]  # the triangle's last cell


# ---- options

@pytest.mark.parametrize("contra, short", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("span", [0, 7])
def test_options(ctx, contra, short, span):
    """both models, short hairpins, and a span limit of 7 counted in each row's OWN bases: a pair of two columns
    further apart than 7 is present where gaps lie between them"""
    reset(ctx)
    masks = np.ones((3, 52), bool)
    masks[0, 10:22] = False
    masks[1, :6] = False
    masks[1, 30:36] = False
    masks[2, 40:] = False
    rows = rows_of(masks)
    assert [len(r) for r in ungapped(rows)] == [40, 40, 40]
    res, want, _ = run_case(ctx, rows, contra=contra, short=short, span=span)
    assert np.any(want > 0)
    i, j, _ = res.pairs()
    if span:
        assert np.max(j - i) > span  # column distance, across the gaps of row 0
        assert np.max(j - i) < span + 12
    if short:
        assert np.min(j - i) < 4


# ---- invariance

def test_grouping_and_devices_leave_the_bytes_alone(ctx, params):
    from rna_algos_amd.mccaskill_algo import Pool
    reset(ctx)
    masks = np.ones((20, 60), bool)
    for s in range(20):
        masks[s, (3 * s) % 50:(3 * s) % 50 + s % 7] = False
        masks[s, :s % 4] = False
    rows = rows_of(masks)
    gammas = (0.5, 2.0, 8.0)
    base, *_ = run_case(ctx, rows, gammas=gammas)
    assert ctx.stats()["n_groups"] == 1

    def same(res):
        assert same_bits(np.asarray(res.bpp.packed), np.asarray(base.bpp.packed))
        assert same_bits(res.col_paired, base.col_paired) and same_bits(res.log_z, base.log_z)
        assert res.row_len.tolist() == base.row_len.tolist()
        assert [(db, np.float32(a).tobytes()) for db, a in res.folds] == \
            [(db, np.float32(a).tobytes()) for db, a in base.folds]
    try:
        ctx.set("group_max_seqs", 3)
        same(ctx.bpp_alignment(rows, False, False, gammas))
        st = ctx.stats()
        assert st["n_groups"] == 7 and st["launches_other"] >= 7 + 2
        ctx.set("centroid_chunk_bytes", 4096)  # one threshold a chunk
        same(ctx.bpp_alignment(rows, False, False, gammas))
    finally:
        reset(ctx)
    pool = Pool(params, devices=[0, 0])
    try:
        same(pool.bpp_alignment(rows, False, False, gammas))
        one = pool.bpp_alignment(rows[:1], False, False)  # one row: one shard
        alone = ctx.bpp_alignment(rows[:1], False, False)
        assert same_bits(np.asarray(one.bpp.packed), np.asarray(alone.bpp.packed))
        assert same_bits(one.col_paired, alone.col_paired)
    finally:
        pool.close()


@pytest.mark.parametrize("tree_lane", [1, 2])
def test_tree_order_mode(ctx, tree_lane):
    """summation mode 1, wave per cell and (tree_lane = 2) lane per cell, the form of large batches: against the
    dense entry in the same mode on the identical list of records"""
    reset(ctx)
    ctx.set("summation_mode", 1)
    ctx.set("tree_lane", tree_lane)
    try:
        masks = np.ones((5, 80), bool)
        for s in range(5):
            masks[s, 10 * s:10 * s + 2 * s] = False
        res, want, _ = run_case(ctx, rows_of(masks))
        assert np.any(want > 0)
    finally:
        ctx.set("tree_lane", 1)
        reset(ctx)


# ---- consensus folds

def fold_rows():
    """six rows that are one hairpin-rich sequence with a few gaps each: the averaged triangle keeps strong pairs"""
    seq = seq_of(70, seed=5)
    rows = np.repeat(seq[None, :], 6, axis=0)
    for s in range(1, 6):
        rows[s, 11 * s:11 * s + 2] = GAP
    return rows


def test_consensus_folds(ctx):
    reset(ctx)
    gammas = (0.5, 2.0, 8.0)
    rows = fold_rows()
    res, *_ = run_case(ctx, rows, gammas=gammas)
    check_folds(res, gammas)
    assert res.folds[-1][0].count("(") > 0, "the case must have a non-empty fold"
    assert all(len(db) == rows.shape[1] for db, _ in res.folds)
    # without the triangle on the host the folds are the same
    bare = ctx.bpp_alignment(rows, False, False, gammas, return_bpp=False)
    assert bare.bpp is None
    assert [(db, np.float32(a).tobytes()) for db, a in bare.folds] == \
        [(db, np.float32(a).tobytes()) for db, a in res.folds]
    assert same_bits(bare.col_paired, res.col_paired)
    # columns beyond every row: the (max,+) triangle is larger than any row's
    wide = np.full((2, 150), GAP, np.uint8)
    wide[0, 5:5 + 70:1] = rows[0]
    wide[1, 80:150] = rows[0]
    res, *_ = run_case(ctx, wide, gammas=gammas)
    check_folds(res, gammas)


# ---- an independent source

def test_against_the_cpu_oracle(ctx, params):
    """three rows, Turner, reference order: the yardstick fed with the CPU oracle's bpp of every ungapped row"""
    import oracle_lib as O
    reset(ctx)
    masks = np.ones((3, 44), bool)
    masks[0, 5:9] = False
    masks[1, :3] = False
    masks[2, 30:37] = False
    rows = rows_of(masks)
    tris, zs = [], []
    for r in ungapped(rows):
        ref, z = O.bpp(params.ptr, r, False, False)
        tris.append(np.where(ref < 0, np.float32(-1), ref).astype(np.float32))
        zs.append(z)
    want, want_paired = yardstick(rows, tris)
    res = ctx.bpp_alignment(rows, False, False)
    assert np.count_nonzero(want > 0) > 0
    assert same_bits(np.asarray(res.bpp.packed), want)
    assert same_bits(res.col_paired, want_paired)
    assert same_bits(res.log_z, np.asarray(zs, np.float32))


# ---- sanity

def test_log_partition_is_the_rows_own(ctx):
    reset(ctx)
    rows = variable_rows()
    res = ctx.bpp_alignment(rows, True, False, max_bp_span=25)
    want = ctx.log_partition_batch(ungapped(rows), True, False, max_bp_span=25)
    assert same_bits(res.log_z, want)


def test_errors_leave_the_context_usable(ctx):
    from rna_algos_amd import _lib
    reset(ctx)
    rows = fold_rows()
    bad = rows.copy()
    bad[2, :] = GAP
    with pytest.raises(_lib.RnamcError) as e:
        ctx.bpp_alignment(bad, False, False)
    assert e.value.status == _lib.ERR_EMPTY_SEQ and "row 2" in str(e.value)
    bad = rows.copy()
    bad[1, 7] = 5
    with pytest.raises(_lib.RnamcError) as e:
        ctx.bpp_alignment(bad, False, False)
    assert e.value.status == _lib.ERR_INVALID_BASE
    run_case(ctx, rows)


# ---- the CLI

def test_cli_round_trip(params, tmp_path):
    """align_fold on the 4 x 37 fixture in its three formats: bpp.dat holds `.pairs(0.01)` of the API, one
    consensus file per gamma; the Stockholm file through a fresh process, the other two through main()"""
    import subprocess
    import sys
    from rna_algos_amd import utils
    from rna_algos_amd.bin import align_fold as cli
    from rna_algos_amd.bin.mccaskill_algo import HEADER, fmt_f32
    from rna_algos_amd.mccaskill_algo import alignment_fold
    utils.set_default_tables(params)
    gammas = [0.5, 2.0, 8.0]
    flags = ["--synthetic-tables", "1", "-g", "0.5", "2", "8"]
    outs = {}
    for ext in ("sto", "aln", "fa"):
        out = os.path.join(tmp_path, "out_" + ext)
        argv = flags + ["-i", os.path.join(GOLDEN, "align_small." + ext), "-o", out]
        if ext == "sto":
            subprocess.check_call([sys.executable, "-m", "rna_algos_amd.bin.align_fold"] + argv, cwd=ROOT,
                                  stderr=subprocess.DEVNULL, timeout=300)
        else:
            assert cli.main(argv) == 0
        outs[ext] = {f: open(os.path.join(out, f)).read() for f in sorted(os.listdir(out))}
    utils.set_default_tables(params)
    fss = utils.FoldScoreSets.new(0.0)
    fss.transfer()
    rows, _ = utils.read_align(os.path.join(GOLDEN, "align_small.sto"))
    res = alignment_fold(rows, False, False, fss, gammas)
    i, j, p = res.pairs(0.01)
    assert len(p) > 0 and np.all(p >= np.float32(0.01))
    want = {"bpp.dat": HEADER + "\n\n>0\n" + "".join(f"{a},{b},{fmt_f32(q)} " for a, b, q in zip(i, j, p))}
    for g, (db, _) in zip(gammas, res.folds):
        want[f"centroid_threshold={fmt_f32(g)}.fa"] = ">0\n" + db
    assert sorted(want) == ["bpp.dat", "centroid_threshold=0.5.fa", "centroid_threshold=2.fa",
                            "centroid_threshold=8.fa"]
    for ext in outs:
        assert outs[ext] == want, ext
