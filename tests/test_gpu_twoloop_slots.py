"""Every two-loop slot (a, b), a + b <= 30, in every form of the sweeps that walk them.

The inputs (tests/twoloop_inputs.py; their conditions are pinned on the CPU by
test_twoloop_inputs_cpu.py) make ONE slot carry the result: family S folds into two stems around the
(a, b) loop with P(both pairs) >= 0.4, at four placements (row mod 4, distance to both ends); family E
puts the loop's outer pair at (0, n - 1), every outside guard on its boundary; family N is S's shape
without the constraint, so the per-diagonal lists hold many competing cells.  On random inputs a lone
3 x 17 loop moves no probability by anything near the suite's absolute bounds.

  * reference order: every probability and ln Z against O.bpp_masked by the parity rule
    (test_gpu_parity.assert_same), batch sweep and latency forms, two group shapes;
  * tree order: key sets, the existing absolute bounds, and a RELATIVE bound on the pairs the slot
    decides — |p_gpu / p_f64 - 1| <= 16 ulp_f32(S), S = max(1, |ln Z|, |score of the full structure|):
    a tree-order probability is the exp of a sum and difference of f32 log-domain values of at most that
    magnitude (16 ulp: the rule of test_tree_vs_committed_exact_f64) — in the wave-per-cell kernels
    (tree_tpc, tree_two, tree_ahead) and the lane-per-cell batch (tree_gen_batch 1 and 3).  Measured on
    one MI355X: worst relative deviation 0.16 - 0.19 of that bound under Turner, 0.68 under CONTRAfold,
    in every form (DESIGN.md section 4c has the table).  A call whose longest sequence has fewer than
    194 bases is swept unbanded and never as a lane-per-cell batch, whatever the knobs say, so those
    forms fold the records beside one 200-base neighbour (twoloop_inputs.family_x);
  * max-plus sweep and traceback: the optimum against O.mfe_exact, family S returns the full structure;
  * sampler: the frequency of "both pairs" against the slot use u.
"""
import time

import numpy as np
import pytest

import twoloop_inputs as T
from test_gpu_mfe import check_optimum
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

DEFAULTS = {"summation_mode": 0, "latency_mode": 1, "lat_pairs": 1, "lat_merge": 1, "group_max_seqs": 8192,
            "tree_lane": 1, "tree_tpc": 0, "tree_two": 1, "tree_ahead": 1, "tree_gen_batch": 3}


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def configure(ctx, **knobs):
    for k, v in dict(DEFAULTS, **knobs).items():
        ctx.set(k, v)


class Batch:
    """records of one call with the oracle's answers laid out as the call's output is: one flat
    array, record after record (built once per module and model, never modified)"""

    def __init__(self, recs, contra, short, exact=False, reference=False):
        self.recs = recs
        self.seqs = [r.seq for r in recs]
        self.cons = [r.cons for r in recs] if any(r.cons is not None for r in recs) else None
        sizes = np.array([r.n * (r.n + 1) // 2 for r in recs], np.int64)
        self.starts = np.concatenate([[0], np.cumsum(sizes)])
        self.n = np.array([r.n for r in recs], np.float64)
        if reference:
            res = [T.reference(r.family, contra, short)[r.idx] for r in recs]
            self.ref = np.concatenate([b for b, _ in res])
            self.ref_z = np.array([z for _, z in res], np.float32)
        if exact:
            res = [T.exact(r.family, contra, short)[r.idx] for r in recs]
            self.exact = np.concatenate([b for b, _ in res])
            self.exact_z = np.array([z for _, z in res], np.float64)
            self.present = self.exact >= -0.5
            self.bound_p = np.repeat(2e-5 + 2e-7 * self.n, sizes)
            self.bound_z = 2e-5 + 3e-6 * np.abs(self.exact_z)
            # the pairs the slot decides: family S (i, j) and every outer-stem pair, family E (0, n - 1)
            full = np.array([T.full_scores(r.family, contra, short)[r.idx] for r in recs])
            scale = np.maximum(1.0, np.maximum(np.abs(self.exact_z), np.abs(full))).astype(np.float32)
            where, owner = [], []
            for x, r in enumerate(recs):
                pairs = r.outer if r.family == "S" else [(0, r.n - 1)] if r.family == "E" else []
                where += [self.starts[x] + T.index(r.n, p, q) for p, q in pairs]
                owner += [x] * len(pairs)
            self.decisive = np.array(where, np.int64)
            self.owner = np.array(owner, np.int64)
            self.bound_rel = 16.0 * np.spacing(scale)[self.owner].astype(np.float64)
            assert np.all(self.exact[self.decisive] > 0)

    def flat(self, mats):
        out = np.concatenate([np.asarray(m.packed) for m in mats])
        assert out.size == self.starts[-1]
        return out

    def record_of(self, flat_index):
        return self.recs[int(np.searchsorted(self.starts, flat_index, side="right")) - 1]


_batches = {}


def batch(name, contra, short, **kw):
    """the Batch of a named set of records, built on first use"""
    key = (name, contra, short, tuple(sorted(kw.items())))
    if key not in _batches:
        S, E, N = T.family_s(), T.family_e(), T.family_n()
        recs = {"S+E": S + E,
                "all": S + E + N,
                "all+X": S + E + N + T.family_x(),  # (last: the other records keep their places)
                "S": S, "N": N,
                "S pl=0": [r for r in S if r.pl == 0]}[name]
        _batches[key] = Batch(recs, contra, short, **kw)
    return _batches[key]


# ---------------------------------------------------------------------------------------------------
REFERENCE_FORMS = [("batch sweep", dict(latency_mode=0)),
                   ("latency forms", dict(latency_mode=2)),
                   ("latency forms, lat_pairs 0", dict(latency_mode=2, lat_pairs=0)),
                   ("latency forms, lat_merge 0", dict(latency_mode=2, lat_merge=0))]


@pytest.mark.parametrize("group_max_seqs", [8192, 7])
@pytest.mark.parametrize("contra,short", T.MODELS)
def test_reference_order_every_slot(ctx, contra, short, group_max_seqs):
    """families S and E: the reference-order 2-loop blocks, their latency forms (one wave per listed
    cell, merged or not), in one group and in groups of 7 (records meet different group shapes)"""
    b = batch("S+E", contra, short, reference=True, exact=True)
    try:
        for form, knobs in REFERENCE_FORMS:
            what = f"contra={contra} short={short} group_max_seqs={group_max_seqs} {form}"
            configure(ctx, group_max_seqs=group_max_seqs, **knobs)
            t0 = time.perf_counter()
            mats, lz = ctx.bpp_batch(b.seqs, contra, short, b.cons)
            dt = time.perf_counter() - t0
            lp = ctx.log_partition_batch(b.seqs, contra, short, b.cons)
            got = b.flat(mats)
            if not np.array_equal(got, b.ref):  # (name the record; the rule itself is assert_same's)
                for x in np.unique(np.searchsorted(b.starts, np.flatnonzero(got != b.ref), side="right") - 1):
                    lo, hi = b.starts[x], b.starts[x + 1]
                    assert_same(got[lo:hi], b.ref[lo:hi], f"{what} {b.recs[x]}")
            bad = np.flatnonzero(lz.view(np.uint32) != b.ref_z.view(np.uint32))
            assert bad.size == 0, f"{what}: ln Z of {bad.size} records, first {b.recs[bad[0]]}: " \
                f"gpu={lz[bad[0]]!r} ref={b.ref_z[bad[0]]!r}"
            assert lp.tobytes() == lz.tobytes(), f"{what}: log_partition_batch differs from the call's ln Z"
            print(f"{what}: {len(b.recs)} records, bpp_batch {dt:.2f} s")
    finally:
        configure(ctx)


# ---------------------------------------------------------------------------------------------------
def check_tree(b, mats, lz, what, problems):
    """key sets, the absolute bounds of test_tree_vs_exact_f64 and the relative bound on the decisive
    pairs -> (worst |dp| / bound, worst |d ln Z| / bound, worst relative deviation / bound)"""
    got = b.flat(mats).astype(np.float64)
    keys = got >= -0.5
    if not np.array_equal(keys, b.present):
        w = np.flatnonzero(keys != b.present)
        problems.append(f"{what}: key sets differ in {w.size} places, first in {b.record_of(w[0])}")
        return np.inf, np.inf, np.inf
    dp = np.where(keys, np.abs(got - b.exact), 0.0) / b.bound_p
    dz = np.abs(np.asarray(lz, np.float64) - b.exact_z) / b.bound_z
    rel = np.abs(got[b.decisive] / b.exact[b.decisive] - 1.0) / b.bound_rel
    if dp.max() > 1.0:
        w = int(np.argmax(dp))
        problems.append(f"{what}: |dp| = {dp[w] * b.bound_p[w]:.3e} > {b.bound_p[w]:.3e} in {b.record_of(w)}")
    if dz.max() > 1.0:
        w = int(np.argmax(dz))
        problems.append(f"{what}: |d ln Z| = {dz[w] * b.bound_z[w]:.3e} > {b.bound_z[w]:.3e} in {b.recs[w]}")
    if rel.max() > 1.0:
        w = int(np.argmax(rel))
        q = b.decisive[w]
        problems.append(f"{what}: decisive pair of {b.recs[b.owner[w]]}: p = {got[q]!r}, f64 {b.exact[q]!r}, "
                        f"relative deviation {rel[w] * b.bound_rel[w]:.3e} > {b.bound_rel[w]:.3e}; "
                        f"{int((rel > 1.0).sum())} pairs beyond the bound")
    return float(dp.max()), float(dz.max()), float(rel.max())


@pytest.mark.parametrize("tree_tpc", [0, 64, 256, 1024])
@pytest.mark.parametrize("contra,short", T.MODELS)
def test_tree_order_wave_per_cell(ctx, contra, short, tree_tpc):
    """tree_lane 0: the wave-per-cell kernels of rnamc_tree.hip at every threads-per-cell choice, one
    and two diagonals a launch, with and without the look-ahead — every record of the three families
    (a call takes hundredths of a second: no sub-sample of the slots).  Alone the records are swept
    unbanded; beside the 200-base neighbour (twoloop_inputs.family_x) banded, where tree_two allows
    it: only there do the look-ahead and the far parts of a block exist."""
    problems = []
    try:
        for name in ("all", "all+X"):
            b = batch(name, contra, short, exact=True)
            for tree_two in (0, 1):
                for tree_ahead in (0, 1):
                    what = f"contra={contra} short={short} {name} tree_tpc={tree_tpc} tree_two={tree_two} " \
                        f"tree_ahead={tree_ahead}"
                    configure(ctx, summation_mode=1, tree_lane=0, tree_tpc=tree_tpc, tree_two=tree_two,
                              tree_ahead=tree_ahead)
                    t0 = time.perf_counter()
                    mats, lz = ctx.bpp_batch(b.seqs, contra, short, b.cons)
                    dt = time.perf_counter() - t0
                    wp, wz, wr = check_tree(b, mats, lz, what, problems)
                    print(f"{what}: {len(b.recs)} records in {dt:.2f} s, worst |dp| {wp:.3f}, |d ln Z| {wz:.3f}, "
                          f"relative deviation of the decisive pairs {wr:.3f} of their bounds")
    finally:
        configure(ctx)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("contra,short", T.MODELS)
def test_tree_order_lane_batch(ctx, contra, short):
    """tree_lane 2: the lane-per-cell batch (lane_generic_run4, lane_generic_edge, the explicit small
    loops, k_tlane_gen three diagonals a launch and one) over every record of the three families in one
    call — with the 200-base neighbour, without which a call of records this short never takes the
    form; tree_gen_batch 1 and 3 sum the same terms in the same order within a cell"""
    b = batch("all+X", contra, short, exact=True)
    problems, flats = [], []
    try:
        for tree_gen_batch in (3, 1):
            what = f"contra={contra} short={short} lane batch tree_gen_batch={tree_gen_batch}"
            configure(ctx, summation_mode=1, tree_lane=2, tree_gen_batch=tree_gen_batch)
            t0 = time.perf_counter()
            mats, lz = ctx.bpp_batch(b.seqs, contra, short, b.cons)
            dt = time.perf_counter() - t0
            wp, wz, wr = check_tree(b, mats, lz, what, problems)
            flats.append((b.flat(mats), np.array(lz)))
            st = ctx.stats()
            print(f"{what}: {len(b.recs)} records in {dt:.2f} s, worst |dp| {wp:.3f}, |d ln Z| {wz:.3f}, "
                  f"relative deviation of the decisive pairs {wr:.3f} of their bounds; launches inside / outside "
                  f"{st['launches_inside']} / {st['launches_outside']}")
    finally:
        configure(ctx)
    (p3, z3), (p1, z1) = flats
    if not (np.array_equal(p3, p1) and np.array_equal(z3, z1)):
        w = np.flatnonzero(p3 != p1)
        problems.append(f"tree_gen_batch 1 and 3 differ in {w.size} entries" +
                        (f", first in {b.record_of(w[0])}" if w.size else " (ln Z)"))
    assert not problems, "\n".join(problems)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contra,short", T.MODELS)
def test_mfe_every_slot(ctx, params, contra, short):
    """the max-plus sweep's slot bounds and the traceback's min(RNAMC_MAX_2LOOP_LEN, j - i - 3) scan:
    family S under its constraint returns the full structure, family N (no constraint) its optimum"""
    from rna_algos_amd.mccaskill_algo import is_compatible
    worst = 0.0
    for name in ("S", "N"):
        b = batch(name, contra, short)
        t0 = time.perf_counter()
        dbs, sc, dp = ctx.mfe_batch(b.seqs, contra, short, b.cons)
        dt = time.perf_counter() - t0
        best = T.optimum(name, contra, short)
        wrong = []
        for r, db, s, v, w in zip(b.recs, dbs, sc, dp, best):
            assert len(db) == r.n and is_compatible(db, r.cons), (r, db)
            worst = max(worst, check_optimum(params, r.seq, db, s, v, w, contra, short, repr(r)))
            if name == "S" and db != r.full:
                wrong.append((r, db))
        assert not wrong, (len(wrong), wrong[:5])
        print(f"contra={contra} short={short} family {name}: {len(b.recs)} records in {dt:.2f} s")
    print(f"contra={contra} short={short}: worst error {worst:.3f} of the bound")


# ---------------------------------------------------------------------------------------------------
N_SAMPLES = 2000


@pytest.mark.parametrize("contra", [False, True])
def test_sampler_chooses_every_slot(ctx, contra):
    """the walker (rnamc_walk.h) must choose slot (a, b) with its probability: per record of family S,
    placement pl = 0, the frequency of "(i, j) and (k, l) both present" against the slot use u within
    6 sigma (binomial) + 2 e + 1e-3, e = |reference order - exact| of that record (the formula of
    test_sampler_marginals_past_cached_decisions); every sampled structure satisfies the constraint"""
    from rna_algos_amd.mccaskill_algo import is_compatible
    b = batch("S pl=0", contra, False, reference=True, exact=True)
    u = np.array(T.slot_use("S", contra, False))[[r.idx for r in b.recs]]
    t0 = time.perf_counter()
    rows, _, _ = ctx.sample_batch(b.seqs, N_SAMPLES, contra, False, seed=41, constraints=b.cons)
    dt = time.perf_counter() - t0
    worst, problems = 0.0, []
    for x, (r, smp) in enumerate(zip(b.recs, rows)):
        lo, hi = b.starts[x], b.starts[x + 1]
        keys = b.present[lo:hi]
        assert np.array_equal(b.ref[lo:hi] >= -0.5, keys), r
        e = float(np.max(np.abs(b.ref[lo:hi].astype(np.float64) - b.exact[lo:hi])[keys]))
        for db in np.unique(smp, axis=0):
            assert is_compatible(bytes(db), r.cons), (r, bytes(db))
        i, j, k, l = r.ijkl
        op, cl = ord("("), ord(")")
        f = float(np.mean((smp[:, i] == op) & (smp[:, j] == cl) & (smp[:, k] == op) & (smp[:, l] == cl)))
        bound = 6 * np.sqrt(u[x] * (1 - u[x]) / N_SAMPLES) + 2 * e + 1e-3
        worst = max(worst, abs(f - u[x]) / bound)
        if not abs(f - u[x]) <= bound:
            problems.append(f"{r}: frequency {f:.4f}, u = {u[x]:.4f}, bound {bound:.4f}")
    print(f"contra={contra}: {len(b.recs)} records x {N_SAMPLES} samples in {dt:.2f} s, worst |f - u| = "
          f"{worst:.2f} of the bound")
    assert not problems, "\n".join(problems[:20])
