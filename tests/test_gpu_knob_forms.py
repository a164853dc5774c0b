"""Reference-order sweep under the knobs that select another kernel instantiation, another
block-to-role mapping or another stream schedule (rnamc_sweep.cpp, rnamc_kernels.hip): whatever the
knobs say, the result is the CPU oracle's, bit for bit (assert_same of tests/test_gpu_parity.py: the
same absent set, identical f32, 1 ulp where the reference takes its libm exp branch; log_partition
bit for bit).  The oracle's result does not depend on the knobs: one oracle run per (batch, model
variant), shared by every case.  Every case takes a context of its own (tests/soak.py draws some of
these knobs at random; this is the collected, deterministic part)."""
import contextlib

import numpy as np
import pytest

import oracle_lib as O
from knob_table import DEFAULT_GROUP_MAX_NT
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

VARIANTS = [(False, False), (True, False), (True, True)]
VARIANT_IDS = ["turner", "contra", "contra-short"]
variants = pytest.mark.parametrize("contra,short", VARIANTS, ids=VARIANT_IDS)


def ragged_lens():
    """41 lengths of 1 .. 330: the lengths around the block sizes, the longest, 22 long ones (so that the
    upper diagonals hold enough cells for the dual_min_cells / dual_max_diag windows of case d) and 8
    shorter ones"""
    rng = np.random.default_rng(20261)
    lens = [1, 2, 5, 64, 65, 128, 129, 192, 256, 257, 330]
    lens += [int(x) for x in rng.integers(245, 331, 22)] + [int(x) for x in rng.integers(10, 245, 8)]
    return lens


def wide_lens():
    return [int(x) for x in np.random.default_rng(20262).integers(170, 261, 420)]


def make_seqs(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, int(n)).astype(np.uint8) for n in lens]


class Batch:
    """sequences and, per model variant, the oracle's result (computed at first use, once)"""

    def __init__(self, params, seqs):
        self.params, self.seqs, self.lens = params, seqs, [len(s) for s in seqs]
        self._ref = {}

    def ref(self, contra, short):
        if (contra, short) not in self._ref:
            self._ref[(contra, short)] = O.bpp_batch(self.params.ptr, self.seqs, contra, short, n_threads=16)
        return self._ref[(contra, short)]


@pytest.fixture(scope="module")
def ragged(params):
    return Batch(params, make_seqs(ragged_lens(), 11))


@pytest.fixture(scope="module")
def wide(params):
    lens = wide_lens()
    # the non-split k_inside<*, false> and the fused k_inside2 run only where a launch holds 65 536 cells
    assert sum(n - 2 for n in lens) >= 65536
    assert inside_fused_diagonals(lens, 64), "no diagonal of the wide batch takes the fused launch"
    return Batch(params, make_seqs(lens, 12))


@pytest.fixture(scope="module")
def equal6(params):
    return Batch(params, make_seqs([120] * 6, 13))


@contextlib.contextmanager
def context(params, **knobs):
    from rna_algos_amd.mccaskill_algo import Context
    ctx = Context(params, device=0)
    try:
        for k, v in knobs.items():
            ctx.set(k, v)
        yield ctx
    finally:
        ctx.close()


def check(batch, contra, short, mats, logz, what):
    ref, ref_logz = batch.ref(contra, short)
    assert len(mats) == len(ref)
    for s, m, r in zip(batch.seqs, mats, ref):
        assert_same(m.packed, r, f"{what}: n={len(s)}")
    assert np.array_equal(np.asarray(logz, dtype=np.float32).view(np.uint32),
                          np.asarray(ref_logz).view(np.uint32)), f"{what}: log_partition differs"


def run_check(batch, contra, short, **knobs):
    with context(batch.params, **knobs) as ctx:
        mats, logz = ctx.bpp_batch(batch.seqs, contra, short)
        st = ctx.stats()
    check(batch, contra, short, mats, logz, str(knobs))
    return st


# ---- the launch rules of rnamc_sweep.cpp, restated: which form a diagonal takes -------------------

def groups_of(lens, max_seqs=8192, max_nt=DEFAULT_GROUP_MAX_NT):
    """BatchPlan::cut: longest first, a new group when the next sequence would exceed a limit (a
    sequence longer than the nucleotide limit still gets a group of its own)"""
    groups, cur = [], []
    for n in sorted(lens, reverse=True):
        if cur and (len(cur) >= max_seqs or sum(cur) + n > max_nt):
            groups.append(cur)
            cur = []
        cur.append(n)
    groups.append(cur)
    return groups


def dmin_outside(contra, short):
    return 1 if (contra and short) else 4


def outside_forms(group, dmin_out, dual_outside=1, dual_min_cells=256 * 1024, dual_max_diag=1 << 30):
    """per outside diagonal of a group, from the top: True where the launch is two kernels on two streams"""
    gmax = group[0]
    forms = []
    for d in range(gmax, dmin_out - 1, -1):
        na = sum(1 for n in group if n > max(d - 1, 0))
        forms.append(bool(dual_outside) and d < gmax and gmax - d <= dual_max_diag
                     and (gmax - d) * na >= dual_min_cells)
    return forms


def inside_fused_diagonals(lens, block):
    """diagonals d of the one group of `lens` whose folds take the two-diagonal launch with heads, and
    where the fold blocks and the head blocks of k_inside2 differ in number"""
    gmax = max(lens)
    out = []
    for d in range(2, gmax - 2):
        active = sum(1 for n in lens if n > d)
        if (gmax - d) * active >= 65536 and -(-(gmax - d) // block) != -(-(gmax - d - 2) // block):
            out.append(d)
    return out


def is_latency_group(group, contra, lat_max_cells):
    return len(group) * group[0] <= (lat_max_cells // 2 if contra else lat_max_cells)


def test_ragged_batch_meets_block_multiples(ragged):
    """with 64 and 128 threads a block, some diagonals of the ragged group are exact multiples of the
    block (the head role of k_outside then has one block more than the other two: Bh = B + 1) and
    some are not"""
    gmax = max(ragged.lens)
    assert gmax == 330 and len(ragged.lens) == 41
    for block in (64, 128):
        rem = {(gmax - d) % block == 0 for d in range(4, gmax)}
        assert rem == {True, False}


# ---- a. block_threads ----------------------------------------------------------------------------

@variants
@pytest.mark.parametrize("block", [64, 128, 192])
def test_block_threads_ragged(ragged, contra, short, block):
    """block counts of k_inside, k_pair_tail and k_outside and the cells per block of the split form
    ((block / 64) * 21) follow block_threads; throughput forms (latency_mode 0), the outside sweep by
    its default rule (one kernel: the group never reaches dual_min_cells), as two kernels on every
    diagonal (ROLES 5 + 2) and as one (ROLES 7)"""
    run_check(ragged, contra, short, latency_mode=0, block_threads=block)
    run_check(ragged, contra, short, latency_mode=0, block_threads=block, dual_min_cells=0)
    run_check(ragged, contra, short, latency_mode=0, block_threads=block, dual_outside=0)


@variants
@pytest.mark.parametrize("block", [64, 128, 192])
def test_block_threads_wide(wide, contra, short, block):
    """420 sequences: the low diagonals hold more than 65 536 cells, where the folds leave the split
    form for k_inside<*, false> and the fused k_inside2 (fixture `wide` asserts it)"""
    st = run_check(wide, contra, short, block_threads=block)
    assert st["n_groups"] == 1


# ---- b. order_inside -----------------------------------------------------------------------------

@variants
@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("order", [1, 2])
def test_order_inside_wide(wide, contra, short, order, block):
    """The permutation of k_inside2 acts in fused launches with heads only: diagonals with
    (gmax - d) * active >= 65 536 (inside_is_split), i.e. the low diagonals of the wide batch.  With
    64 threads a block blocks_sums = ceil((gmax - d) / 64) and blocks_head = ceil((gmax - d - 2) / 64)
    are both above 1 and differ where (gmax - d) mod 64 is 1 or 2 (asserted by the fixture): mode 2
    then deals triples and ends in its fold-only tail (S > m); where they are equal it ends with the
    triples.  (launch_inside2 never makes blocks_head exceed blocks_sums: the head-only tail of mode 2
    is out of its reach.)  With 256 threads both are 1 or 2."""
    run_check(wide, contra, short, order_inside=order, block_threads=block)


# ---- c. order_outside ----------------------------------------------------------------------------

@variants
@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("order", [0, 2, 3, 4])
def test_order_outside_ragged(ragged, contra, short, order, block):
    """The permutation of k_outside over B = ceil((gmax - d) / block) blocks of each of the first two
    roles and Bh = ceil((gmax - d + 1) / block) head blocks, in the one-kernel form (ROLES 7: Bh is B
    or B + 1) and in the two-kernel form (ROLES 5 with all three ranges, ROLES 2 with Bh = 0: the only
    launch where mode 4 takes its B > Bh branch)."""
    run_check(ragged, contra, short, latency_mode=0, order_outside=order, block_threads=block, dual_outside=0)
    run_check(ragged, contra, short, latency_mode=0, order_outside=order, block_threads=block, dual_min_cells=0)


@variants
@pytest.mark.parametrize("block,order", [(64, 4), (128, 3), (192, 0), (256, 2)])
def test_order_outside_wide(wide, contra, short, block, order):
    """Large launches.  At the default dual_min_cells (262 144) the 420-sequence group stays in the
    one-kernel form throughout ((gmax - d) * active is at most 258 * 420); with dual_min_cells = 65 536
    the sweep starts as one kernel and turns into two kernels partway down by itself, which the
    per-kernel accounting shows."""
    run_check(wide, contra, short, block_threads=block, order_outside=order)
    forms = outside_forms(groups_of(wide.lens)[0], dmin_outside(contra, short), dual_min_cells=65536)
    assert forms[0] is False and forms[-1] is True
    st = run_check(wide, contra, short, block_threads=block, order_outside=order, dual_min_cells=65536, profile=2)
    assert st["launches_outside_main"] == st["launches_outside_tail"] == sum(forms) > 0
    assert st["launches_outside_small"] == len(forms) - sum(forms) > 0


# ---- d. dual_max_diag ----------------------------------------------------------------------------

@variants
@pytest.mark.parametrize("min_cells,max_diag", [(2000, 90), (0, 37)])
def test_dual_max_diag_both_transitions(ragged, contra, short, min_cells, max_diag):
    """One sweep that goes one kernel -> two kernels on two streams -> one kernel again: the top
    diagonals run single while (gmax - d) * active < dual_min_cells, the middle runs dual, and from
    gmax - d > dual_max_diag on the sweep is back on one stream behind the wait for the second
    stream's event (the `if (dual)` branch of the one-kernel launch in rnamc_sweep.cpp).  The form of
    every diagonal follows from the lengths (outside_forms); the per-kernel accounting (profile 2)
    must count exactly those."""
    group = groups_of(ragged.lens)[0]
    forms = outside_forms(group, dmin_outside(contra, short), dual_min_cells=min_cells, dual_max_diag=max_diag)
    changes = [a != b for a, b in zip(forms, forms[1:])]
    assert sum(changes) == 2 and forms[0] is False and forms[-1] is False and sum(forms) >= 5
    st = run_check(ragged, contra, short, latency_mode=0, profile=2, dual_min_cells=min_cells,
                   dual_max_diag=max_diag)
    assert st["n_groups"] == 1
    assert st["launches_outside_main"] == st["launches_outside_tail"] == sum(forms) > 0
    assert st["launches_outside_small"] == len(forms) - sum(forms) > 0
    # every outside diagonal of the group is in exactly one class (a two-kernel diagonal in two)
    assert st["launches_outside_small"] + st["launches_outside_main"] == group[0] + 1 - dmin_outside(contra, short)


# ---- e. lat_max_cells ----------------------------------------------------------------------------

@variants
def test_lat_max_cells_boundary(equal6, contra, short):
    """latency_mode 1 takes the latency forms for a group of nseq * gmax <= lat_max_cells (CONTRAfold:
    lat_max_cells / 2).  One group of 6 x 120 nt: at the boundary the launch counts are those of the
    forced latency forms (latency_mode 2), one below those of the batch forms (latency_mode 0).
    (lat_merge 0 throughout — it acts in the latency forms only: their merged schedule is one launch per
    diagonal and sweep, which is also what the batch forms of a Turner group this small take; un-merged,
    the 2-loop blocks are launches of their own and the counts tell the forms apart.)"""
    cells = 6 * 120
    at = 2 * cells if contra else cells
    counts = lambda st: (st["launches_inside"], st["launches_outside"])
    forced_lat = counts(run_check(equal6, contra, short, lat_merge=0, latency_mode=2))
    forced_batch = counts(run_check(equal6, contra, short, lat_merge=0, latency_mode=0))
    assert forced_lat != forced_batch
    assert counts(run_check(equal6, contra, short, lat_merge=0, latency_mode=1, lat_max_cells=at)) == forced_lat
    assert counts(run_check(equal6, contra, short, lat_merge=0, latency_mode=1, lat_max_cells=at - 1)) == forced_batch


@variants
def test_lat_max_cells_mixed_groups(ragged, contra, short):
    """One call whose groups fall on both sides of the boundary: groups of 5, lat_max_cells = 5 * 150 —
    the groups of long sequences take the batch forms, those of short ones the latency forms, back
    to back on the same streams and workspace.  At default knobs, and with lat_merge 0, where the launch
    counts tell the forms apart (see test_lat_max_cells_boundary): neither all latency nor all batch."""
    groups = groups_of(ragged.lens, max_seqs=5)
    kinds = [is_latency_group(g, contra, 750) for g in groups]
    assert True in kinds and False in kinds
    counts = lambda st: (st["launches_inside"], st["launches_outside"])
    st = run_check(ragged, contra, short, latency_mode=1, group_max_seqs=5, lat_max_cells=750)
    assert st["n_groups"] == len(groups)
    mixed = run_check(ragged, contra, short, lat_merge=0, latency_mode=1, group_max_seqs=5, lat_max_cells=750)
    assert mixed["n_groups"] == len(groups)
    all_lat = run_check(ragged, contra, short, lat_merge=0, latency_mode=2, group_max_seqs=5)
    all_batch = run_check(ragged, contra, short, lat_merge=0, latency_mode=0, group_max_seqs=5)
    assert counts(mixed) != counts(all_lat) and counts(mixed) != counts(all_batch)


# ---- f. lat_split --------------------------------------------------------------------------------

@variants
@pytest.mark.parametrize("lat_pairs", [0, 1])
def test_lat_split(ragged, contra, short, lat_pairs):
    """lat_split: probs_multibranch and the multibranch half of the pair probabilities of a diagonal as
    two k_outside_lat launches, the 2-loop half beside them on the second stream (k_pair_lat, or the
    head role of k_outside with lat_pairs 0) — the un-merged two-stream schedule.  The accounting of
    profile 2 files the first launch as "tail", which no other latency-form schedule does."""
    st = run_check(ragged, contra, short, latency_mode=2, group_max_seqs=5, lat_split=1, lat_pairs=lat_pairs,
                   profile=2)
    assert st["launches_outside_tail"] == st["launches_outside_main"] > 0
    assert st["launches_outside_small"] > 0
    st = run_check(ragged, contra, short, latency_mode=2, group_max_seqs=5, lat_pairs=lat_pairs, profile=2)
    assert st["launches_outside_tail"] == 0


# ---- g. group_max_nt -----------------------------------------------------------------------------

@variants
@pytest.mark.parametrize("max_nt", [1, 500, 3000])
def test_group_max_nt(ragged, contra, short, max_nt):
    """the nucleotide cut of BatchPlan::cut: the oracle's bits, and as many groups as the greedy
    longest-first cut gives (a sequence longer than the limit gets a group of its own)"""
    groups = groups_of(ragged.lens, max_nt=max_nt)
    assert len(groups) == 41 if max_nt == 1 else 1 < len(groups) < 41
    st = run_check(ragged, contra, short, group_max_nt=max_nt)
    assert st["n_groups"] == len(groups)


def tree_pair_bound(n):
    """two forms of the tree-order mode against each other (tests/test_gpu_tree.py)"""
    return 2 * (2e-5 + 2e-7 * n)


@variants
def test_group_max_nt_tree_order(ragged, contra, short):
    """The same cuts in tree-order mode, against the tree-order result at the default group_max_nt:
    identical key sets, |dp| within the bound two forms of the mode have against each other (a
    sequence swept in another group meets other launch shapes: threads per cell follow the group's
    cells, the outside sweep pairs diagonals from the group's longest sequence down).  A sequence that
    is alone in its group under two cuts is swept by the same launches in both: equal bits."""
    def tree(max_nt):
        with context(ragged.params, summation_mode=1, group_max_nt=max_nt) as ctx:
            mats, logz = ctx.bpp_batch(ragged.seqs, contra, short)
            return [np.asarray(m.packed).copy() for m in mats], np.asarray(logz).copy(), ctx.stats()["n_groups"]
    base, zbase, g0 = tree(DEFAULT_GROUP_MAX_NT)
    assert g0 == 1
    cut = {}
    for max_nt in (1, 500, 3000):
        got, z, g = tree(max_nt)
        assert g == len(groups_of(ragged.lens, max_nt=max_nt))
        cut[max_nt] = got
        for n, a, b0, za, zb in zip(ragged.lens, got, base, z, zbase):
            assert np.array_equal(a >= -0.5, b0 >= -0.5), (max_nt, n)
            both = a >= -0.5
            dp = float(np.max(np.abs(a[both].astype(np.float64) - b0[both]))) if both.any() else 0.0
            assert dp <= tree_pair_bound(n), (max_nt, n, dp)
            assert abs(float(za) - float(zb)) <= 2 * (2e-5 + 3e-6 * abs(float(zb))), (max_nt, n)
    # (the library sorts stably: positions of the sorted order <-> members of the groups)
    order = sorted(range(len(ragged.lens)), key=lambda x: -ragged.lens[x])
    same, pos = [], 0
    for g in groups_of(ragged.lens, max_nt=500):
        if len(g) == 1:
            same.append(order[pos])
        pos += len(g)
    assert len(same) >= 5
    for x in same:
        assert np.array_equal(cut[1][x].view(np.uint32), cut[500][x].view(np.uint32)), ragged.lens[x]


# ---- h. pairwise cover ---------------------------------------------------------------------------

PAIRWISE_DOMAINS = {
    "block_threads": (64, 128, 192, 256), "order_inside": (0, 1, 2), "order_outside": (0, 1, 2, 3, 4),
    "fuse_inside": (0, 1), "dual_outside": (0, 1), "dual_min_cells": (0, 4096, 262144),
    "latency_mode": (0, 1, 2), "lat_pairs": (0, 1), "lat_merge": (0, 1), "lat_split": (0, 1),
    "lat_zr_ahead": (0, 1), "lat_inside": (0, 2), "lat_e_waves": (0, 64, 2048), "group_max_seqs": (3, 17, 8192),
}
PAIRWISE_COLUMNS = ("block_threads", "order_inside", "order_outside", "fuse_inside", "dual_outside",
                    "dual_min_cells", "latency_mode", "lat_pairs", "lat_merge", "lat_split", "lat_zr_ahead",
                    "lat_inside", "lat_e_waves", "group_max_seqs")
# every pair of values of two different columns stands together in some row
# (tests/test_knob_table_cpu.py verifies it)
PAIRWISE_TABLE = (
    (64, 2, 3, 1, 0, 0, 2, 0, 0, 1, 0, 2, 2048, 3),
    (192, 2, 2, 0, 1, 4096, 0, 1, 1, 0, 1, 0, 0, 8192),
    (128, 0, 4, 0, 0, 262144, 1, 0, 1, 1, 0, 0, 64, 17),
    (256, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 2, 64, 17),
    (128, 0, 0, 0, 1, 262144, 2, 1, 0, 0, 1, 0, 2048, 3),
    (256, 1, 0, 1, 0, 4096, 0, 0, 1, 1, 0, 2, 0, 8192),
    (64, 0, 4, 0, 1, 0, 0, 0, 0, 0, 1, 2, 0, 8192),
    (192, 1, 1, 1, 0, 262144, 2, 1, 1, 1, 0, 0, 2048, 3),
    (192, 0, 2, 1, 0, 4096, 1, 0, 0, 0, 0, 2, 64, 3),
    (64, 1, 3, 0, 1, 262144, 1, 1, 1, 1, 1, 0, 64, 8192),
    (128, 2, 1, 0, 1, 262144, 0, 0, 0, 1, 0, 2, 0, 17),
    (256, 2, 4, 0, 0, 4096, 2, 1, 0, 0, 1, 0, 2048, 17),
    (128, 1, 2, 1, 1, 0, 2, 0, 1, 1, 0, 0, 2048, 8192),
    (256, 0, 3, 1, 1, 4096, 0, 1, 0, 0, 0, 0, 0, 3),
    (192, 2, 0, 0, 1, 0, 1, 1, 0, 1, 1, 0, 64, 17),
    (64, 0, 1, 0, 0, 4096, 1, 0, 1, 0, 0, 0, 2048, 8192),
    (64, 2, 2, 0, 1, 262144, 2, 0, 0, 0, 1, 0, 0, 17),
    (192, 1, 4, 1, 1, 0, 0, 0, 1, 0, 1, 0, 2048, 3),
    (128, 2, 3, 0, 1, 4096, 1, 0, 0, 0, 1, 0, 0, 17),
    (256, 0, 2, 1, 1, 262144, 0, 0, 1, 0, 0, 0, 64, 8192),
    (64, 2, 0, 0, 1, 4096, 2, 0, 0, 1, 0, 2, 64, 8192),
    (192, 1, 3, 0, 1, 4096, 2, 0, 1, 1, 0, 2, 0, 3),
)


def pairwise_rows():
    return [dict(zip(PAIRWISE_COLUMNS, row)) for row in PAIRWISE_TABLE]


@pytest.mark.parametrize("row", range(len(PAIRWISE_TABLE)))
def test_pairwise_cover(ragged, row):
    """every pair of values of the reference-order knobs in some row; the row index picks the model
    variant round-robin"""
    contra, short = VARIANTS[row % 3]
    run_check(ragged, contra, short, **pairwise_rows()[row])
