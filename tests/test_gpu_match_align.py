"""Pairwise alignment on the device (rnamc_match_align_mats, rnamc_durbin_align_batch; DESIGN.md
section 20).  The (max,+) fill and its traceback against the host function rnamc_match_align bit for
bit; lists, marginals, mates, counts and accuracies of whole batches against the numpy-f32
restatement (match_align_ref.py) applied to the dense matrices durbin_algo_batch returns for the same
pairs, which test_gpu_durbin.py pins to the oracle."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import match_align_ref as R

pytestmark = pytest.mark.gpu

GAMMAS = (1.5, 2.0, 8.0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def check_alignments(r, P, gammas, what, host=True):
    """mate, count and accuracy of every gamma against the host function (or the helper)"""
    from rna_algos_amd.pair_align import match_align
    assert r.mate.shape == (len(gammas), P.shape[0]), what
    for g, gamma in enumerate(gammas):
        mate, count, acc = match_align(P, gamma) if host else R.match_align(P, gamma)
        assert np.array_equal(r.mate[g], mate), f"{what} gamma {gamma}: mate"
        assert int(r.n_matched[g]) == count, f"{what} gamma {gamma}: count"
        assert bits(r.expect_accuracy[g]) == bits(acc), f"{what} gamma {gamma}: {r.expect_accuracy[g]} vs {acc}"


def check_lists(r, P, min_prob, what):
    i, j, p = R.listing(P, min_prob)
    assert np.array_equal(r.i, i) and np.array_equal(r.j, j), f"{what}: listed cells"
    assert np.array_equal(bits(r.p), bits(p)), f"{what}: listed probabilities"
    rows, cols = R.marginals(P)
    assert np.array_equal(bits(r.row_matched), bits(rows)), f"{what}: row_matched"
    assert np.array_equal(bits(r.col_matched), bits(cols)), f"{what}: col_matched"


def check_all(r, P, gammas, min_prob, what):
    check_lists(r, P, min_prob, what)
    check_alignments(r, P, gammas, what, host=False)


def same_result(x, y, what):
    for name in ("i", "j", "mate", "n_matched"):
        assert np.array_equal(getattr(x, name), getattr(y, name)), f"{what}: {name}"
    for name in ("p", "row_matched", "col_matched", "expect_accuracy"):
        assert np.array_equal(bits(getattr(x, name)), bits(getattr(y, name))), f"{what}: {name}"


# ---- match_align_mats against the host function

def test_mats_small_sides_bit_exact(built):
    """L in {0, 1, 2, 63, 64, 65} in every ragged combination, random and tie-rich, three gammas"""
    from rna_algos_amd.pair_align import match_align_mats
    rng = np.random.default_rng(30)
    mats = []
    for l1, l2 in itertools.product((0, 1, 2, 63, 64, 65), repeat=2):
        mats.append(R.random_probmat(rng, l1 + 2, l2 + 2, 0.4))
        mats.append(R.quantised_probmat(rng, l1 + 2, l2 + 2))
    res = match_align_mats(mats, GAMMAS, min_prob=0.25)
    assert len(res) == len(mats)
    for k, (r, P) in enumerate(zip(res, mats)):
        what = f"matrix {k} ({P.shape[0]} x {P.shape[1]})"
        check_alignments(r, P, GAMMAS, what)
        check_lists(r, P, 0.25, what)
    # the tie-rich matrices with the gammas that make every candidate exact
    quant = mats[1::2]
    for r, P in zip(match_align_mats(quant, (2.0, 4.0)), quant):
        check_alignments(r, P, (2.0, 4.0), f"quantised {P.shape}")


@pytest.mark.parametrize("side", [1023, 1024, 1025])
def test_mats_diagonals_around_the_lds_limit(built, side):
    """longest diagonals of 1023, 1024 and 1025 cells: the last that stays in LDS and the first two
    that spill, each far beyond one pass of the workgroup; a staircase and a tie-rich matrix"""
    from rna_algos_amd.pair_align import match_align_mats
    rng = np.random.default_rng(31 + side)
    stair, path = R.staircase(side + 2, side + 2, start=2, run=5, gap_a=1, gap_b=0)
    quant = R.quantised_probmat(rng, side + 2, side + 2)
    rs, rq = match_align_mats([stair, quant], (2.0, 4.0), min_prob=0.5)
    assert np.array_equal(rs.mate[0], path) and rs.expect_accuracy[0] == np.float32(np.sum(path >= 0))
    check_alignments(rs, stair, (2.0, 4.0), f"staircase {side}")
    check_alignments(rq, quant, (2.0, 4.0), f"quantised {side}")
    check_lists(rs, stair, 0.5, f"staircase {side}")
    check_lists(rq, quant, 0.5, f"quantised {side}")


def lane_residues(path, n2, lanes):
    """the lane (of `lanes`) that computes every cell of a path: cells of diagonal s = i + j are dealt
    out from its first row max(1, s - L2) on"""
    l2 = n2 - 2
    i = np.nonzero(path >= 0)[0]
    s = i + path[i]
    return set(((i - np.maximum(1, s - l2)) % lanes).tolist())


def test_staircases_through_every_lane(built):
    """paths that put a decisive cell on every lane of a workgroup (and beyond one pass of it): a lane
    slice of the fill that is lost loses a match"""
    from rna_algos_amd.pair_align import match_align_mats
    mats, paths = [], []
    for shape, kw in (((302, 1000), dict(start=1, run=1, gap_a=0, gap_b=1)),
                      ((1102, 3400), dict(start=1, run=1, gap_a=0, gap_b=1)),
                      ((700, 302), dict(start=1, run=2, gap_a=1, gap_b=0)),
                      ((520, 530), dict(start=3, run=7, gap_a=0, gap_b=0))):
        P, path = R.staircase(*shape, **kw)
        mats.append(P)
        paths.append(path)
    assert lane_residues(paths[0], 1000, 256) == set(range(256))
    assert lane_residues(paths[1], 3400, 1024) == set(range(1024))
    assert lane_residues(paths[1], 3400, 64) == set(range(64))
    covered = set()
    for path, P in zip(paths[2:], mats[2:]):
        covered |= lane_residues(path, P.shape[1], 256)
    assert covered == set(range(256))
    for r, P, path in zip(match_align_mats(mats, (2.0,)), mats, paths):
        assert np.array_equal(r.mate[0], path), P.shape
        assert int(r.n_matched[0]) == int(np.sum(path >= 0))
        assert r.expect_accuracy[0] == np.float32(np.sum(path >= 0))
        check_alignments(r, P, (2.0,), f"staircase {P.shape}")


# ---- pair_align_batch against the helper on the dense matrices of durbin_algo_batch

def score_sets():
    from rna_algos_amd.durbin_algo import AlignScores
    rng = np.random.default_rng(11)
    s = AlignScores.new(0.0)
    s.transfer()
    r = AlignScores.new(0.0)
    for name in ("match2match_score", "match2insert_score", "insert_extend_score",
                 "init_match_score", "init_insert_score"):
        r.set(name, rng.uniform(-2, 2))
    r.set("insert_scores", rng.uniform(-1, 1, 4).astype(np.float32))
    r.set("match_scores", rng.uniform(-1, 1, (4, 4)).astype(np.float32))
    return {"transferred": s, "zero": AlignScores.new(0.0), "random": r}


def ragged_set():
    """the sequences and pairs of test_gpu_durbin.py::test_ragged_pairs_and_other_scores_bit_exact"""
    from rna_algos_amd.durbin_algo import with_pseudo_bases
    rng = np.random.default_rng(11)
    lens = [0, 1, 2, 3, 17, 64, 65, 200, 1100, 1300]
    seqs = [with_pseudo_bases(rng.integers(0, 4, n)) for n in lens]
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 3), (3, 7), (4, 4), (5, 6), (6, 5), (7, 4),
             (8, 9), (9, 8), (8, 2), (0, 9)]
    return seqs, pairs


def test_all_pairs_of_the_fixture(trnas):
    from rna_algos_amd.durbin_algo import durbin_algo_batch, with_pseudo_bases
    from rna_algos_amd.pair_align import pair_align_batch, rows_to_mate
    s = score_sets()["transferred"]
    seqs = [with_pseudo_bases(x) for _, x in trnas]
    pairs = list(itertools.combinations(range(len(seqs)), 2))
    assert len(pairs) == 15
    mats = durbin_algo_batch(seqs, pairs, s)
    res = pair_align_batch(seqs, pairs, s, gammas=GAMMAS, min_prob=0.01)
    dense = pair_align_batch(seqs, pairs, s, gammas=GAMMAS, min_prob=0.01, dense=True)
    for (a, b), P, r, d in zip(pairs, mats, res, dense):
        check_all(r, P, GAMMAS, 0.01, f"pair {a},{b}")
        assert r.probs is None and np.array_equal(bits(d.probs), bits(P))
        same_result(r, d, f"pair {a},{b} with the dense matrices")
        assert r.to_dict() == {(int(i), int(j)): P[i, j] for i, j in zip(*np.nonzero(P >= np.float32(0.01)))}
        for g, (row_a, row_b, acc) in enumerate(r.alignments):
            assert np.array_equal(rows_to_mate(row_a, row_b), r.mate[g]) and acc == r.expect_accuracy[g]
            assert row_a.replace("-", "") == "".join("ACGU"[x] for x in seqs[a][1:-1])
            assert row_b.replace("-", "") == "".join("ACGU"[x] for x in seqs[b][1:-1])
        assert int(r.n_matched[2]) > 30  # (tRNAs align: the test is not about empty alignments)


@pytest.mark.parametrize("which", ["transferred", "zero", "random"])
def test_ragged_pairs_and_other_scores(built, which):
    """the empty sequence to a 1100 x 1300 pair (a spilled diagonal), self pairs, both orders of a
    pair; the all-zero scores give symmetric, tie-rich probabilities"""
    from rna_algos_amd.durbin_algo import durbin_algo_batch
    from rna_algos_amd.pair_align import pair_align_batch
    sc = score_sets()[which]
    seqs, pairs = ragged_set()
    mats = durbin_algo_batch(seqs, pairs, sc)
    res = pair_align_batch(seqs, pairs, sc, gammas=GAMMAS, min_prob=0.01, dense=True)
    for (a, b), P, r in zip(pairs, mats, res):
        what = f"scores {which} pair {a},{b} ({P.shape[0]} x {P.shape[1]})"
        assert np.array_equal(bits(r.probs), bits(P)), what
        check_all(r, P, GAMMAS, 0.01, what)


# ---- the contract of the entries

def raw_mats_call(ctx, mats, gammas, min_prob, cap, lists=True):
    """rnamc_match_align_mats as it is: -> (status, total, counts, starts, i, j, p)"""
    from rna_algos_amd import _lib
    n1 = np.array([m.shape[0] for m in mats], dtype=np.uint32)
    n2 = np.array([m.shape[1] for m in mats], dtype=np.uint32)
    offs = np.zeros(len(mats) + 1, dtype=np.uint64)
    np.cumsum(np.array([m.size for m in mats], dtype=np.uint64), out=offs[1:])
    flat = np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in mats])
    g = np.asarray(gammas, dtype=np.float32)
    i, j, p = np.zeros(cap + 1, np.uint32), np.zeros(cap + 1, np.uint32), np.zeros(cap + 1, np.float32)
    start = np.full(len(mats), 2 ** 63, dtype=np.uint64)
    count = np.full(len(mats), 2 ** 63, dtype=np.uint64)
    total = C.c_uint64(2 ** 63)
    rc = _lib.lib().rnamc_match_align_mats(
        ctx._h, len(mats), n1.ctypes.data, n2.ctypes.data, flat.ctypes.data, offs.ctypes.data, C.c_float(min_prob),
        g.ctypes.data if len(g) else None, len(g), i.ctypes.data if lists else None, j.ctypes.data if lists else None,
        p.ctypes.data if lists else None, cap, start.ctypes.data, count.ctypes.data, C.byref(total),
        None, None, None, None, None, None)
    return rc, int(total.value), count, start, i, j, p


def test_counting_mode_capacity_and_bad_arguments(built):
    from rna_algos_amd import _lib
    from rna_algos_amd.durbin_algo import _default_context
    ctx = _default_context()
    rng = np.random.default_rng(33)
    mats = [R.random_probmat(rng, n1, n2, 0.5) for n1, n2 in ((9, 20), (2, 5), (40, 3), (31, 33))]
    want = [R.listing(P, 0.3) for P in mats]
    counts = np.array([len(w[0]) for w in want], dtype=np.uint64)
    # counting: no arrays
    rc, total, count, start, *_ = raw_mats_call(ctx, mats, (), 0.3, 0, lists=False)
    assert rc == _lib.OK and total == int(counts.sum()) and np.array_equal(count, counts)
    # a capacity too small: the error, with the counts and the total set
    rc, total2, count2, *_ = raw_mats_call(ctx, mats, (), 0.3, total - 1)
    assert rc == _lib.ERR_INVALID_ARG and total2 == total and np.array_equal(count2, counts)
    # exactly enough: lists that do not overlap
    rc, total3, count3, start3, i, j, p = raw_mats_call(ctx, mats, (), 0.3, total)
    assert rc == _lib.OK and total3 == total
    spans = sorted((int(s), int(s + c)) for s, c in zip(start3, count3))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total
    for s, c, w in zip(start3, count3, want):
        s, c = int(s), int(c)
        assert np.array_equal(i[s:s + c], w[0]) and np.array_equal(j[s:s + c], w[1])
        assert np.array_equal(bits(p[s:s + c]), bits(w[2]))
    # arguments that fail before any device work
    for bad in (dict(min_prob=-0.1), dict(min_prob=float("nan")), dict(min_prob=float("inf")),
                dict(gammas=(1.0, float("inf"))), dict(gammas=(float("nan"),)), dict(gammas=tuple([2.0] * 65))):
        kw = dict(gammas=(), min_prob=0.3)
        kw.update(bad)
        rc, total4, *_ = raw_mats_call(ctx, mats, kw["gammas"], kw["min_prob"], total)
        assert rc == _lib.ERR_INVALID_ARG and total4 == 2 ** 63, bad
    rc, *_ = raw_mats_call(ctx, mats + [np.zeros((1, 5), np.float32)], (), 0.3, total)
    assert rc == _lib.ERR_EMPTY_SEQ
    rc, *_ = raw_mats_call(ctx, mats, tuple([2.0] * 64), 0.3, total)
    assert rc == _lib.OK


def test_no_gammas_and_the_thresholds(trnas):
    """n_gammas = 0: lists and marginals only; min_prob = 0 lists np.nonzero(m > 0); a min_prob above
    every entry empties the lists and leaves the marginals"""
    from rna_algos_amd.durbin_algo import durbin_algo_batch, with_pseudo_bases
    from rna_algos_amd.pair_align import pair_align_batch
    s = score_sets()["transferred"]
    seqs = [with_pseudo_bases(x) for _, x in trnas]
    pairs = [(0, 1), (2, 2), (5, 3)]
    mats = durbin_algo_batch(seqs, pairs, s)
    zero = pair_align_batch(seqs, pairs, s, gammas=(), min_prob=0.0)
    high = pair_align_batch(seqs, pairs, s, gammas=(), min_prob=1.5)
    for P, z, h in zip(mats, zero, high):
        assert z.mate.shape == (0, P.shape[0]) and len(z.n_matched) == 0 and z.alignments == []
        ii, jj = np.nonzero(P > 0)
        assert np.array_equal(z.i, ii) and np.array_equal(z.j, jj) and np.array_equal(bits(z.p), bits(P[ii, jj]))
        assert len(ii) > 100
        check_lists(z, P, 0.0, "min_prob 0")
        assert len(h.i) == len(h.j) == len(h.p) == 0
        assert np.array_equal(bits(h.row_matched), bits(z.row_matched))
        assert np.array_equal(bits(h.col_matched), bits(z.col_matched))


# ---- independence of the schedule

def test_results_do_not_depend_on_the_schedule(built):
    """the same pairs alone, in the batch, in reversed order, and with the workspace budget lowered so
    that chunk cuts fall between and around the long pair"""
    from rna_algos_amd.mccaskill_algo import Context
    from rna_algos_amd.pair_align import pair_align_batch
    from rna_algos_amd.utils import FoldScoreSets
    sc = score_sets()["transferred"]
    seqs, pairs = ragged_set()
    pairs = pairs[:10] + [(8, 9)] + pairs[12:] + [(7, 7), (5, 4)]
    ctx = Context(FoldScoreSets.new(0.0))
    try:
        base = pair_align_batch(seqs, pairs, sc, gammas=GAMMAS, min_prob=0.02, ctx=ctx)
        rev = pair_align_batch(seqs, pairs[::-1], sc, gammas=GAMMAS, min_prob=0.02, ctx=ctx)[::-1]
        for k, (x, y) in enumerate(zip(base, rev)):
            same_result(x, y, f"pair {k} reversed")
        for k in (0, 4, 9, 10, 14):
            alone = pair_align_batch(seqs, [pairs[k]], sc, gammas=GAMMAS, min_prob=0.02, ctx=ctx)[0]
            same_result(base[k], alone, f"pair {k} alone")
        # 6 f32 matrices of the 1102 x 1302 pair: 34.4 MB.  35 MB: the long pair alone in its chunk, the
        # short ones together before and after it; 1 MB: 202 x 202 and 202 x 19 alone, smaller ones in
        # twos and threes; 4 bytes: every pair alone
        for budget in (35 << 20, 1 << 20, 4):
            ctx.set("group_ws_bytes", budget)
            cut = pair_align_batch(seqs, pairs, sc, gammas=GAMMAS, min_prob=0.02, ctx=ctx, dense=True)
            for k, (x, y) in enumerate(zip(base, cut)):
                same_result(x, y, f"pair {k} with group_ws_bytes {budget}")
    finally:
        ctx.close()


def test_more_pairs_than_one_launch_holds(built):
    """the 380 records of test_durbin_more_pairs_than_one_launch_holds: more than 65535 pairs, the
    grid-y limit of the stage's count, list and marginal kernels"""
    from rna_algos_amd.durbin_algo import AlignScores, durbin_algo_batch, with_pseudo_bases
    from rna_algos_amd.pair_align import pair_align_batch
    rng = np.random.default_rng(5)
    seqs = [with_pseudo_bases(rng.integers(0, 4, int(n))) for n in rng.integers(0, 3, 380)]
    pairs = [(a, b) for a in range(len(seqs)) for b in range(a + 1, len(seqs))]
    assert len(pairs) > 65535 + 4000
    sc = AlignScores.new(0.0)
    sc.transfer()
    res = pair_align_batch(seqs, pairs, sc, gammas=(2.0, 8.0), min_prob=0.05)
    assert len(res) == len(pairs)
    spot = sorted(set(list(range(0, len(pairs), 997)) + [65533, 65534, 65535, 65536, 65537, len(pairs) - 1]))
    mats = durbin_algo_batch(seqs, [pairs[x] for x in spot], sc)
    for x, P in zip(spot, mats):
        check_all(res[x], P, (2.0, 8.0), 0.05, f"pair {x} = {pairs[x]}")
    total = sum(len(r.p) for r in res)
    starts = np.array([r.i.ctypes.data for r in res if len(r.i)], dtype=np.uint64)
    assert total > 10000 and len(np.unique(starts)) == len(starts)


# ---- the command-line tool

def test_cli_text_and_alignments(trnas, tmp_path):
    from rna_algos_amd.bin import durbin_algo as dense_cli
    from rna_algos_amd.bin import pair_align as cli
    from rna_algos_amd.durbin_algo import with_pseudo_bases
    from rna_algos_amd.pair_align import pair_align_batch, rows_to_mate
    from rna_algos_amd.utils import EXAMPLE_FASTA_FILE_PATH
    want = os.path.join(tmp_path, "durbin.dat")
    assert dense_cli.main(["-i", EXAMPLE_FASTA_FILE_PATH, "-o", want]) == 0
    out = os.path.join(tmp_path, "out")
    assert cli.main(["-i", EXAMPLE_FASTA_FILE_PATH, "-o", out, "-g", "2", "-g", "6.5", "--min-prob", "0"]) == 0
    assert open(os.path.join(out, "match.dat")).read() == open(want).read()
    assert sorted(os.listdir(out)) == ["gamma=2.aln", "gamma=6.5.aln", "match.dat"]
    lines = open(os.path.join(out, "gamma=6.5.aln")).read().split("\n")
    assert len(lines) == 15 * 3 + 1 and lines[-1] == ""
    head, row_a, row_b = lines[3 * 7:3 * 7 + 3]
    ids, acc = head[1:].split(" ")
    a, b = (int(x) for x in ids.split(","))
    seqs = [with_pseudo_bases(x) for _, x in trnas]
    s = score_sets()["transferred"]
    r = pair_align_batch(seqs, [(a, b)], s, gammas=(6.5,), min_prob=0.0)[0]
    assert np.array_equal(rows_to_mate(row_a, row_b), r.mate[0])
    assert np.float32(acc) == r.expect_accuracy[0]
    assert row_a.replace("-", "") == "".join("ACGU"[x] for x in seqs[a][1:-1])
