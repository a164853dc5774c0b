"""The pair-HMM on the device against the f64 model of tests/durbin_ref.py, and against its own
schedule ("What the rewrite of k_durbin_sums must keep").  Both entries that
reach the kernels, rnamc_durbin_batch (durbin_algo_batch) and rnamc_durbin_align_batch
(pair_align_batch with dense=True), run the cases of tests/test_durbin_model_cpu.py: within the CPU
bound of the model, the oracle's bits, and exact zeros, exact ones and NaN masks under -inf scores.
Then the dense entry's own chunk loop under every budget, the two entries against each other, and
every entry on a workspace that earlier calls left dirty."""
import contextlib

import numpy as np
import pytest

import oracle_lib as O
import test_durbin_model_cpu as T
from test_gpu_durbin import same_bits
from test_gpu_match_align import bits, check_alignments, ragged_set

pytestmark = pytest.mark.gpu

ENTRIES = ("durbin_algo_batch", "pair_align_batch")


def dense(entry, seqs, pairs, sc, ctx=None):
    """the dense ProbMats of `pairs` through one of the two entries"""
    from rna_algos_amd.durbin_algo import durbin_algo_batch
    from rna_algos_amd.pair_align import pair_align_batch
    if entry == "durbin_algo_batch":
        return durbin_algo_batch(seqs, pairs, sc, ctx)
    return [r.probs for r in pair_align_batch(seqs, pairs, sc, gammas=(), min_prob=0.5, ctx=ctx, dense=True)]


@contextlib.contextmanager
def fresh_context():
    from rna_algos_amd.mccaskill_algo import Context
    from rna_algos_amd.utils import FoldScoreSets
    ctx = Context(FoldScoreSets.new(0.0))
    try:
        yield ctx
    finally:
        ctx.close()


def identical(got, want, what):
    assert len(got) == len(want), what
    for k, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), \
            f"{what}: matrix {k} ({x.shape[0]} x {x.shape[1]}) differs in {int(np.sum(bits(x) != bits(y)))} cells"


def same_bits_and_nans(got, want, what):
    """same_bits where neither is NaN; NaN where the other is, whatever the payload"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN masks"
    same_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), what)


# ---- against the model

def test_small_pairs_against_the_enumeration(built):
    """every pair up to 6 x 6 under the six score sets, one batch per set and entry"""
    seqs, pairs = T.small_set()
    worst = 0.0
    for which, sc in T.score_sets().items():
        truth = T.small_truth(which)
        want = [O.durbin(sc.ptr, seqs[x], seqs[y]) for x, y in pairs]
        for entry in ENTRIES:
            got = dense(entry, seqs, pairs, sc)
            for k, (m, w, (P, _)) in enumerate(zip(got, want, truth)):
                same_bits(m, w, f"{entry} {which} pair {pairs[k]}")
                worst = max(worst, float(np.abs(m.astype(np.float64) - P).max()))
    print(f"worst |device - enumeration| {worst:.4e}")
    assert worst <= T.BOUND


@pytest.mark.parametrize("which", T.BUMP_SETS)
def test_every_parameter_carries(built, which):
    """the 25 bumps of the CPU test through both entries: the device moves every cell as the f64
    model does, within the bound, and returns the oracle's bits under every bumped set"""
    a, b = T.bump_pair()
    sc = T.score_sets()[which]
    base, bumped = T.bump_truth(which)
    worst = 0.0
    for entry in ENTRIES:
        d_base = dense(entry, [a, b], [(0, 1)], sc)[0].astype(np.float64)
        assert np.abs(d_base - base).max() <= T.BOUND
        for p in T.PARAMS:
            up = T.changed(sc, p, add=1.0)
            got = dense(entry, [a, b], [(0, 1)], up)[0]
            same_bits(got, O.durbin(up.ptr, a, b), f"{entry} {which} {p}")
            moved = bumped[p] - base
            assert np.abs(moved).max() >= 0.01, p
            dev = float(np.abs((got.astype(np.float64) - d_base) - moved).max())
            worst = max(worst, dev)
            assert dev <= T.BOUND, (entry, p, dev)
        off = T.copy_scores(sc)
        off.set("insert_switch_score", sc.insert_switch_score + 1.0)
        identical(dense(entry, [a, b], [(0, 1)], off), dense(entry, [a, b], [(0, 1)], sc), "insert_switch_score")
    print(f"{which}: worst |device's change - model's change| {worst:.4e}")


@pytest.mark.parametrize("which", T.BUMP_SETS)
def test_forbidden_matches(built, which):
    seqs, pairs = T.small_set()
    sc = T.forbid_matches(T.score_sets()[which])
    want = [O.durbin(sc.ptr, seqs[x], seqs[y]) for x, y in pairs]
    worst = 0.0
    for entry in ENTRIES:
        for (x, y), m, w, P in zip(pairs, dense(entry, seqs, pairs, sc), want, T.forbidden_truth(which)):
            same_bits(m, w, f"{entry} {which} pair {x},{y}")
            assert np.all(bits(m[T.forbidden_cells(seqs[x], seqs[y])]) == 0), (entry, x, y)
            worst = max(worst, float(np.abs(m.astype(np.float64) - P).max()))
    print(f"{which}: worst |device - enumeration| with two forbidden matches {worst:.4e}")
    assert worst <= T.BOUND


def test_forbidden_inserts(built):
    """equal lengths: the exact identity where the f32 sums are exact, the oracle's bits and the bound
    elsewhere; unequal lengths: NaN on every interior cell, as the oracle and the model"""
    seqs, pairs = T.equal_set()
    exact = T.forbid_inserts(T.dyadic_scores())
    for entry in ENTRIES:
        T.check_forbidden_inserts_equal(dense(entry, seqs, pairs, exact), f"{entry}, scores in eighths")
        for which, sc in T.score_sets().items():
            c = T.forbid_inserts(sc)
            got = dense(entry, seqs, pairs, c)
            T.check_forbidden_inserts_equal(got[:1], f"{entry} {which}, 1 x 1")
            for (x, y), m in zip(pairs, got):
                same_bits(m, O.durbin(c.ptr, seqs[x], seqs[y]), f"{entry} {which} {len(seqs[x]) - 2} nt")
            for m in got[:3]:
                want = np.zeros(m.shape)
                want[1:-1, 1:-1] = np.eye(m.shape[0] - 2)
                assert np.abs(m - want).max() <= T.BOUND and np.array_equal(m != 0, want != 0)
    small, small_pairs = T.small_set()
    ragged = [(x, y) for x, y in small_pairs if len(small[x]) != len(small[y])]
    for which in T.BUMP_SETS:
        c = T.forbid_inserts(T.score_sets()[which])
        for entry in ENTRIES:
            for (x, y), m in zip(ragged, dense(entry, small, ragged, c)):
                interior = np.zeros(m.shape, dtype=bool)
                interior[1:-1, 1:-1] = True
                assert np.array_equal(np.isnan(m), interior), (entry, which, x, y)
                same_bits_and_nans(m, O.durbin(c.ptr, small[x], small[y]), f"{entry} {which} pair {x},{y}")


@pytest.mark.parametrize("l1,l2,which", sorted(T.DRIFT))
def test_drift_with_length(built, l1, l2, which):
    """the lengths of the CPU drift table, to 1100 x 1300 (diagonals beyond one workgroup's 1024
    lanes): the oracle's bits, and so its distance from the f64 model, held to twice the measured"""
    a, b = T.drift_pair(l1, l2)
    sc = T.score_sets()[which]
    P, _ = T.drift_truth(l1, l2, which)
    want = O.durbin(sc.ptr, a, b)
    for entry in ENTRIES:
        got = dense(entry, [a, b], [(0, 1)], sc)[0]
        same_bits(got, want, f"{entry} {l1} x {l2} {which}")
        dev = float(np.abs(got.astype(np.float64) - P).max())
        print(f"{entry} {l1} x {l2} {which}: worst |device - model| {dev:.4e}")
        assert dev <= 2 * T.DRIFT[(l1, l2, which)][0]


def test_far_negative_finite_scores_as_the_oracle(built):
    """out of the documented domain the device is still the reference's arithmetic: values above 1"""
    a, b = T.bump_pair()
    sc = T.far_negative_scores()
    want = O.durbin(sc.ptr, a, b)
    for entry in ENTRIES:
        got = dense(entry, [a, b], [(0, 1)], sc)[0]
        assert np.nanmax(got) > 1
        same_bits_and_nans(got, want, entry)


# ---- the schedule of rnamc_durbin_batch

def test_dense_entry_does_not_depend_on_the_schedule(built):
    """the ragged set of test_gpu_durbin.py through rnamc_durbin_batch's own chunk loop: every pair
    alone, the batch, the batch reversed, and the batch with the workspace budget at 35 MB (the six
    matrices of a 1102 x 1302 pair are 34.4 MB: each long pair alone, the short ones together around
    them), 1 MB (202 x 202 alone, smaller ones in twos and threes) and 4 bytes (every pair alone).
    The dense matrices of rnamc_durbin_align_batch under the same budget are the same bits."""
    sc = T.score_sets()["transferred"]
    seqs, pairs = ragged_set()
    with fresh_context() as ctx:
        base = dense("durbin_algo_batch", seqs, pairs, sc, ctx)
        identical(dense("durbin_algo_batch", seqs, pairs[::-1], sc, ctx)[::-1], base, "reversed")
        identical([dense("durbin_algo_batch", seqs, [p], sc, ctx)[0] for p in pairs], base, "alone")
        identical(dense("pair_align_batch", seqs, pairs, sc, ctx), base, "the other entry")
        for budget in (35 << 20, 1 << 20, 4):
            ctx.set("group_ws_bytes", budget)
            cut = dense("durbin_algo_batch", seqs, pairs, sc, ctx)
            identical(cut, base, f"group_ws_bytes {budget}")
            identical(dense("pair_align_batch", seqs, pairs, sc, ctx), cut, f"the other entry, group_ws_bytes {budget}")


# ---- a workspace that earlier calls left dirty

def short_and_long():
    seqs, pairs = ragged_set()
    short = [p for p in pairs if 8 not in p and 9 not in p] + [(7, 7), (7, 6)]
    assert len(short) == 12 and max(len(seqs[x]) * len(seqs[y]) for x, y in short) == 202 * 202
    return seqs, short, (8, 9)


@pytest.mark.parametrize("entry", ENTRIES)
def test_dirty_workspace(built, params, entry):
    """The context's workspace is shared with the folding entries and never shrinks (ensure_ws only
    grows it), so after a large call no later, smaller call reallocates: it runs on whatever the
    large one left.  Each result is compared bit for bit with the same call on a fresh context (and
    the short pairs with the oracle, which knows no workspace):
    (a) a bpp_batch of four records of about 300 nt, then the pairs;
    (b) the 1102 x 1302 pair, then the short pairs each alone: they land at offset 0, on the finite
        forward sums of the long pair;
    (c) the long pair first and the short ones after it in one call with a budget of 4 bytes, so
        every chunk starts at offset 0 of the same allocation."""
    from rna_algos_amd.mccaskill_algo import Context
    sc = T.score_sets()["transferred"]
    seqs, short, long_pair = short_and_long()
    want = [O.durbin(sc.ptr, seqs[x], seqs[y]) for x, y in short]
    with fresh_context() as ctx:
        clean = dense(entry, seqs, short, sc, ctx)
    for k, (m, w) in enumerate(zip(clean, want)):
        same_bits(m, w, f"fresh context, pair {short[k]}")
    with fresh_context() as ctx:
        clean_long = dense(entry, seqs, [long_pair], sc, ctx)
    # (a)
    rng = np.random.default_rng(50)
    records = [rng.integers(0, 4, n).astype(np.uint8) for n in (300, 290, 310, 257)]
    ctx = Context(params, device=0)
    try:
        ctx.bpp_batch(records, False, False)
        identical(dense(entry, seqs, short, sc, ctx), clean, "(a) after bpp_batch")
        ctx.bpp_batch(records, True, False)
        identical(dense(entry, seqs, [long_pair], sc, ctx), clean_long, "(a) the long pair after bpp_batch")
    finally:
        ctx.close()
    # (b)
    with fresh_context() as ctx:
        identical(dense(entry, seqs, [long_pair], sc, ctx), clean_long, "(b) the long pair")
        for k, p in enumerate(short):
            identical(dense(entry, seqs, [p], sc, ctx), clean[k:k + 1], f"(b) pair {p} alone after the long pair")
    # (c)
    with fresh_context() as ctx:
        ctx.set("group_ws_bytes", 4)
        got = dense(entry, seqs, [long_pair] + short, sc, ctx)
        identical(got[:1], clean_long, "(c) the long pair")
        identical(got[1:], clean, "(c) the short pairs after the long pair, one chunk each")


def test_existing_entries_unaffected(built, params, trnas):
    """rnamc_bpp_batch before and after the two pair-HMM entries on the same context: identical bits"""
    from rna_algos_amd.durbin_algo import with_pseudo_bases
    from rna_algos_amd.mccaskill_algo import Context
    sc = T.score_sets()["transferred"]
    records = [s for _, s in trnas]
    seqs = [with_pseudo_bases(s) for s in records]
    ctx = Context(params, device=0)
    try:
        before, zb = ctx.bpp_batch(records, True, False)
        for entry in ENTRIES:
            dense(entry, seqs, [(0, 1), (2, 5), (4, 3)], sc, ctx)
        after, za = ctx.bpp_batch(records, True, False)
        assert all(np.array_equal(bits(x.packed), bits(y.packed)) for x, y in zip(before, after))
        assert np.array_equal(bits(zb), bits(za))
    finally:
        ctx.close()


# ---- the alignment stage on the matrices of the exhaustive search

def test_match_align_on_the_enumerated_matrices(built):
    """the matrices of tests/test_match_align_enum_cpu.py, whose host results are held to the maximum
    over every monotone matching, through rnamc_match_align_mats: the host's bits"""
    import test_match_align_enum_cpu as E
    from rna_algos_amd.pair_align import match_align_mats
    for mats, gammas in ((E.quantised_mats(), (2.0, 4.0)), (E.random_mats(), (1.5, 8.0, 1.0, 0.5))):
        for r, P in zip(match_align_mats(mats, gammas), mats):
            check_alignments(r, P, gammas, f"{P.shape} gammas {gammas}")
            for g, gamma in enumerate(gammas):
                best = E.best_score(P, gamma)
                assert abs(float(r.expect_accuracy[g]) - best) <= (0 if gamma in (2.0, 4.0) else 1e-5)
                assert abs(E.mate_score(P, gamma, r.mate[g], int(r.n_matched[g])) - best) <= \
                    (0 if gamma in (2.0, 4.0) else 1e-5)
