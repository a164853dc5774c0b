"""Tables replaced on live contexts, and the table members no other GPU test changes.

A context derives three things from the tables it holds: the Turner hairpin initiation table (hp_init), the
tree-order 2-loop length tables (TreeTabs) and the fold-scores cache.  rnamc_ctx_set_params must drop each;
if it kept one, no call would fail: every result would be computed from a mixture of two table sets.  The
sets of table_sets.py change one block each (test_table_sets_cpu.py pins, from the oracle alone, that every
one of them moves what is compared here), so the piece that was kept is singled out.  As in
test_gpu_growth.py, "right" is the bits of the same call on a freshly created context; the oracle anchors the
live context as well, because a fresh context that is wrong in the same way would agree with it."""
import functools
import math
import threading

import numpy as np
import pytest

import oracle_lib as O
import table_sets as T
from entry_families import freeze, records, table_families
from test_gpu_mfe import check_optimum, sscore, tol as mfe_tol
from test_gpu_parity import assert_same
from test_gpu_sample import pairs_of
from test_gpu_tree import bpp_bound, deviation, logz_bound
from test_oracle_cpu import count_structures

pytestmark = pytest.mark.gpu

SMALL, LARGE = T.SMALL, T.LARGE
# (table set, summation_mode, tree_lane): tree_lane 2 makes the LARGE call take the lane-per-cell form, which
# reads the gslot / glen / g4len / elen members of TreeTabs
CASES = [(name, mode, lane) for name in sorted(T.SETS) for mode, lane in ((0, None), (1, None), (1, 2))
         if lane is None or name in ("B_len", "B_all")]


def tables(name):
    return T.A() if name == "A" else T.SETS[name]()


def context(name, mode=0, lane=None):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(tables(name), device=0)
    c.set("summation_mode", mode)
    if lane is not None:
        c.set("tree_lane", lane)
    return c


_fresh = {}


def fresh(name, mode, lane, model, family, call, shape):
    """the frozen result of `call` on a context created with the tables `name` (computed once)"""
    key = (name, mode, lane, model, family, shape)
    if key not in _fresh:
        c = context(name, mode, lane)
        try:
            _fresh[key] = freeze(call(c, shape))
        finally:
            c.close()
            assert not c._h
    return _fresh[key]


@functools.lru_cache(None)
def oracle(name, model, k):
    """record k of SMALL under the tables `name` -> (reference bpp f32, its ln Z, exact bpp, exact ln Z, best score)"""
    P, seq = tables(name), records(SMALL)[k]
    return O.bpp(P.ptr, seq, *model) + O.exact_bpp(P.ptr, seq, *model) + (O.mfe_exact(P.ptr, seq, *model),)


def anchor(ctx, name, model, mode, what):
    """the live context against the oracle under the tables `name`, which it must hold now"""
    P, seqs = tables(name), records(SMALL)
    mats, logz = ctx.bpp_batch(seqs, *model)
    dbs, scores, dps = ctx.mfe_batch(seqs, *model)
    for k, seq in enumerate(seqs):
        ref, ref_z, exact, exact_z, best = oracle(name, model, k)
        if mode == 0:
            assert np.float32(logz[k]) == ref_z, (what, k)
            assert_same(mats[k].packed, ref, f"{what} record {k}")
        else:
            same, dp = deviation(mats[k].packed, exact)
            assert same and dp <= bpp_bound(len(seq)), (what, k, dp)
            assert abs(float(logz[k]) - exact_z) <= logz_bound(exact_z), (what, k, float(logz[k]), exact_z)
        check_optimum(P, seq, dbs[k], scores[k], dps[k], best, *model, f"{what} record {k}")
        own = sscore(P, seq, dbs[k], *model)
        assert abs(float(scores[k]) - own) <= mfe_tol(own, dbs[k]), (what, k, float(scores[k]), own)


@pytest.mark.parametrize("name,mode,lane", CASES)
def test_replaced_tables_equal_a_fresh_context(name, mode, lane):
    """One context created with A: LARGE under A (hp_init grows to 201 entries), the tables replaced by B, SMALL
    (a hp_init that was kept is long enough and silently A's) and LARGE under B, A again, SMALL and LARGE."""
    for model in T.MODELS[name]:
        families = [f for f in table_families(*model) if mode == 0 or f[1]]
        want = {(f, shape, t): fresh(t, mode, lane, model, f, call, shape)
                for f, _, call in families for shape in (SMALL, LARGE) for t in ("A", name)}
        for f, _, _ in families:
            for shape in (SMALL, LARGE):
                assert want[f, shape, "A"] != want[f, shape, name], (f, shape, model, "the tables do not matter here")
        ctx = context("A", mode, lane)
        try:
            def run(t, shape):
                for f, _, call in families:
                    assert freeze(call(ctx, shape)) == want[f, shape, t], (f, shape, t, name, mode, lane, model)
            run("A", LARGE)
            ctx.sync_params(tables(name))
            run(name, SMALL)
            anchor(ctx, name, model, mode, f"{name} after A, mode {mode}, model {model}")
            run(name, LARGE)
            ctx.sync_params(T.A())
            run("A", SMALL)
            anchor(ctx, "A", model, mode, f"A after {name}, mode {mode}, model {model}")
            run("A", LARGE)
        finally:
            ctx.close()
        assert not ctx._h


def assert_fold_scores(got, P, seq, model, what):
    """as test_gpu_parity.py::test_fold_scores_match_reference_maps: same keys, f32 bits and order"""
    _, hp, mb, ac, tl = got
    rhp, rmb, rac, rtl = O.fold_scores(P.ptr, seq, *model)
    for g, r, m in ((hp, rhp, "hairpin"), (mb, rmb, "mbclose"), (ac, rac, "accessible")):
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, m)
        assert np.array_equal(g.view(np.uint32)[~np.isnan(r)], r.view(np.uint32)[~np.isnan(r)]), (what, m)
    assert tl.shape == rtl.shape and tl.tobytes() == rtl.tobytes(), (what, "twoloop")


@pytest.mark.parametrize("between", ["nothing", "fold_sums"])
@pytest.mark.parametrize("name,model", [("B_all", (False, False)), ("B_all", (True, False)), ("B_hp", (False, False))])
def test_fold_scores_cache_is_dropped_with_the_tables(name, model, between):
    """the cache is keyed by bases and flags only: the same sequence and flags after other tables.  Under B_hp
    only the host copy of hp_init differs, which the cached path does not rebuild"""
    seq = records((1, 76))[0]
    a, b = O.fold_scores(T.A().ptr, seq, *model), O.fold_scores(tables(name).ptr, seq, *model)
    assert a[0].tobytes() != b[0].tobytes()  # (the hairpin maps)
    ctx = context("A")
    try:
        assert_fold_scores(ctx.fold_scores_packed(seq, *model), T.A(), seq, model, "A")
        ctx.sync_params(tables(name))
        if between == "fold_sums":
            got = ctx.fold_sums(seq, *model)
            ref = O.fold_sums(tables(name).ptr, seq, *model)
            for f in O.FOLD_SUMS_FIELDS:
                assert np.array_equal(got.dense[f].view(np.uint32), ref[f].view(np.uint32)), f
        assert_fold_scores(ctx.fold_scores_packed(seq, *model), tables(name), seq, model, f"{name} after A")
        ctx.sync_params(T.A())
        assert_fold_scores(ctx.fold_scores_packed(seq, *model), T.A(), seq, model, f"A after {name}")
    finally:
        ctx.close()


@functools.lru_cache(None)
def pool_seqs():
    return records((4, 90)) + records(SMALL) + records((2, 150))


def pool_calls(pool, model):
    seq = records((1, 93))[0]
    return {
        "bpp_batch": pool.bpp_batch(pool_seqs(), *model),
        "bpp_batch_sparse": pool.bpp_batch_sparse(pool_seqs(), *model, 0.01),
        "centroid_fold_batch": pool.centroid_fold_batch(pool_seqs(), [0.5, 2.0, 8.0], *model),
        "bpp_windowed": pool.bpp_windowed(seq, 60, *model, stride=3),
        "mutant_scan": pool.mutant_scan(seq[:40], *model, positions=list(range(0, 40, 5))),
    }


@pytest.mark.parametrize("model", [(False, False), (True, False)])
def test_pool_replaces_the_tables_of_every_context(model):
    from rna_algos_amd.mccaskill_algo import Pool, shard_plan
    plan = shard_plan([len(s) for s in pool_seqs()], 2)
    assert set(plan.tolist()) == {0, 1}
    want = {}
    for t in ("A", "B_all"):
        p = Pool(tables(t), devices=[0, 0])
        try:
            want[t] = {k: freeze(v) for k, v in pool_calls(p, model).items()}
        finally:
            p.close()
    assert all(want["A"][k] != want["B_all"][k] for k in want["A"])
    pool = Pool(T.A(), devices=[0, 0])
    try:
        assert len(pool) == 2
        for t in ("A", "B_all", "A"):
            pool.sync_params(tables(t))
            got = pool_calls(pool, model)
            for k, v in got.items():
                assert freeze(v) == want[t][k], (k, t, model)
            mats, logz = got["bpp_batch"]
            for s, (seq, m) in enumerate(zip(pool_seqs(), mats)):  # (records of both shards)
                ref, ref_z = O.bpp(tables(t).ptr, seq, *model)
                assert np.float32(logz[s]) == ref_z, (t, s, int(plan[s]))
                assert_same(m.packed, ref, f"pool under {t}, record {s} of shard {int(plan[s])}")
    finally:
        pool.close()


def test_borrowed_context_syncs_through_its_pool():
    """a Context borrowed from a Pool has no key of its own: after pool.sync_params(B) its sync_params(A)
    uploads A (it compares with the pool's key, not with a copy from before), to every context of the pool"""
    from rna_algos_amd.mccaskill_algo import Context, Pool
    pool = Pool(T.A(), devices=[0, 0])
    try:
        c0 = Context.of_pool(pool, 0)
        pool.sync_params(T.B_all())
        c0.sync_params(T.A())
        for who in (c0, pool):
            mats, logz = who.bpp_batch(pool_seqs(), False, False)
            for s, (seq, m) in enumerate(zip(pool_seqs(), mats)):
                ref, ref_z = O.bpp(T.A().ptr, seq, False, False)
                assert np.float32(logz[s]) == ref_z, (type(who).__name__, s)
                assert_same(m.packed, ref, f"{type(who).__name__} record {s}")
        # and the other way round: the borrowed context's sync is seen by the pool's next comparison
        c0.sync_params(T.B_all())
        pool.sync_params(T.B_all())
        mats, logz = pool.bpp_batch(pool_seqs(), False, False)
        for s, (seq, m) in enumerate(zip(pool_seqs(), mats)):
            ref, ref_z = O.bpp(T.B_all().ptr, seq, False, False)
            assert np.float32(logz[s]) == ref_z, s
            assert_same(m.packed, ref, f"pool under B_all, record {s}")
        c0.close()  # (leaves the pool's context alone)
        assert pool.bpp_batch(pool_seqs()[:1], False, False)[1].shape == (1,)
    finally:
        pool.close()


def test_get_fold_sums_hold_the_context_lock(params, monkeypatch):
    """get_fold_sums / get_fold_sums_contra keep _ctx_lock until the sweep has run: while Context.fold_sums runs,
    another thread cannot take the lock (so cannot replace the tables of the shared context)"""
    from rna_algos_amd import mccaskill_algo as M
    real, seen = M.Context.fold_sums, []

    def watched(self, *args):
        def attempt():
            got = M._ctx_lock.acquire(blocking=False)
            if got:
                M._ctx_lock.release()
            seen.append(got)
        t = threading.Thread(target=attempt)
        t.start()
        t.join()
        return real(self, *args)

    monkeypatch.setattr(M.Context, "fold_sums", watched)
    seq = records(SMALL)[0]
    a = M.get_fold_sums(seq, params)
    b = M.get_fold_sums_contra(seq, False, params)
    assert seen == [False, False]
    for got, contra in ((a, False), (b, True)):
        ref = O.fold_sums(params.ptr, seq, contra, False)
        assert np.array_equal(got.sums_external.view(np.uint32), ref["sums_external"].view(np.uint32))


def test_one_set_edited_in_place_between_module_level_calls(params):
    """the training-loop pattern: ONE FoldScoreSets object changes between calls of the module-level functions;
    every result is the oracle's under the tables as they are at the time of the call"""
    from rna_algos_amd import mccaskill_algo as M
    from rna_algos_amd.centroid_fold import centroid_fold, centroid_fold_batch, get_fold_str
    model = (True, False)
    P = T.copy_of(T.A())
    seqs = records(SMALL) + records((2, 60))
    seq = seqs[-1]

    def edit():
        P.interior_scores_len[3] += np.float32(0.25)
        P.accumulate()

    def check_bpp(mats, logz, what):
        for s, (x, m) in enumerate(zip(seqs, mats)):
            ref, ref_z = O.bpp(P.ptr, x, *model)
            assert np.float32(logz[s]) == ref_z, (what, s)
            assert_same(np.asarray(m.packed), ref, f"{what} record {s}")

    try:
        before = O.bpp(P.ptr, seq, *model)[0]
        check_bpp(*M.mccaskill_algo_batch(seqs, *model, P), "mccaskill_algo_batch")
        bpp, scores = M.mccaskill_algo(seq, *model, P)
        at_call = O.fold_scores(P.ptr, seq, *model)
        edit()
        assert not np.array_equal(O.bpp(P.ptr, seq, *model)[0], before)  # (the edit matters)
        assert O.fold_scores(P.ptr, seq, *model)[3].tobytes() != at_call[3].tobytes()
        got = M.get_fold_sums_contra(seq, False, P)
        ref = O.fold_sums(P.ptr, seq, *model)
        for f in O.FOLD_SUMS_FIELDS:
            assert np.array_equal(got.dense[f].view(np.uint32), ref[f].view(np.uint32)), f
        # the maps of the call BEFORE the edit, materialised only now: the tables of that call
        assert len(scores.twoloop_scores) == len(at_call[3])
        for e in at_call[3]:
            key = (int(e["i"]), int(e["j"]), int(e["k"]), int(e["l"]))
            assert np.float32(scores.twoloop_scores[key]) == e["score"], key
        for (i, j), v in scores.accessible_scores.items():
            assert np.float32(v) == at_call[2][M.bpp_index(len(seq), i, j)]
        assert set(scores.accessible_scores) == set(bpp)
        # (materialising put the tables of the earlier call on the device: the next call brings P back)
        sparse, logz = M.mccaskill_algo_batch_sparse(seqs, *model, P, 0.0)
        check_bpp([s.dense() for s in sparse], logz, "mccaskill_algo_batch_sparse")
        edit()
        folds, logz, mats = centroid_fold_batch(seqs, [2.0], *model, P, return_bpp=True)
        check_bpp(mats, logz, "centroid_fold_batch")
        for x, m, f in zip(seqs, mats, folds):
            assert f[0][0] == get_fold_str(centroid_fold(m, len(x), 2.0), len(x))
        edit()
        bpp, _ = M.mccaskill_algo(seq, *model, P)
        ref, _ = O.bpp(P.ptr, seq, *model)
        assert len(bpp) == int((ref >= -0.5).sum())
        for (i, j), v in bpp.items():
            r = ref[M.bpp_index(len(seq), i, j)]
            assert np.float32(v) == r or (r >= 0.9999 and abs(np.float32(v) - r) <= np.spacing(r)), (i, j, v, r)
    finally:
        with M._ctx_lock:  # later tests share the module's pool
            M._pool_for(params)


def test_non_default_hairpin_limits_and_special_list_in_every_caller():
    """B_lim (limits 4 / 12 / 13, 64 special hairpins of lengths 5 .. 16, a -inf entry and its duplicate) through
    every caller of Turner::hairpin: the reference-order sweep in both forms, the tree-order sweep wave per
    cell and lane per cell, the max-plus sweep and its walker, the sampler's walker, the host scorers"""
    P = T.B_lim()
    seqs = [T.planted()[0], T.long_loops()]
    neighbour = records(LARGE)[0]
    model = (False, False)
    ref = [O.bpp(P.ptr, s, *model) for s in seqs]
    exact = [O.exact_bpp(P.ptr, s, *model) for s in seqs]
    ctx = context("B_lim")
    try:
        for latency_mode in (0, 1):
            ctx.set("latency_mode", latency_mode)
            for batch in ([seqs[0]], [seqs[1]], seqs):
                mats, logz = ctx.bpp_batch(batch, *model)
                for s, m, z in zip(batch, mats, logz):
                    r, rz = ref[0] if s is seqs[0] else ref[1]
                    assert np.float32(z) == rz, (latency_mode, len(s))
                    assert_same(m.packed, r, f"latency_mode {latency_mode} n={len(s)}")
        ctx.set("summation_mode", 1)
        for lane, batches in ((1, [[seqs[0]], [seqs[1]]]), (2, [[seqs[0], neighbour], [seqs[1], neighbour]])):
            ctx.set("tree_lane", lane)
            for batch in batches:
                mats, logz = ctx.bpp_batch(batch, *model)
                x, xz = exact[0] if batch[0] is seqs[0] else exact[1]
                same, dp = deviation(mats[0].packed, x)
                print(f"tree_lane {lane} n={len(batch[0])}: |dp| {dp:.2e} of {bpp_bound(len(batch[0])):.2e}, "
                      f"|d ln Z| {abs(float(logz[0]) - xz):.2e} of {logz_bound(xz):.2e}")
                assert same and dp <= bpp_bound(len(batch[0])), (lane, len(batch[0]), dp)
                assert abs(float(logz[0]) - xz) <= logz_bound(xz), (lane, len(batch[0]))
        ctx.set("tree_lane", 1)
        ctx.set("summation_mode", 0)
        dbs, scores, dps = ctx.mfe_batch(seqs, *model)
        for s, db, w, v in zip(seqs, dbs, scores, dps):
            check_optimum(P, s, db, w, v, O.mfe_exact(P.ptr, s, *model), *model, f"B_lim n={len(s)}")
            own = sscore(P, s, db, *model)
            assert abs(float(w) - own) <= mfe_tol(own, db), (len(s), float(w), own)
        rows, weights, logz = ctx.sample_batch(seqs, 300, *model, seed=5)
        for s, r, w, z, (_, rz) in zip(seqs, rows, weights, logz, ref):
            assert np.float32(z) == rz
            u, inv = np.unique(r, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            for x, row in enumerate(u):
                own = sscore(P, s, bytes(row).decode(), *model)
                assert math.isfinite(own)
                # (the bound of test_gpu_sample.py::check_weights_and_validity_trnas)
                bound = 4 * (len(pairs_of(row)) + 1) * float(np.spacing(np.float32(max(1.0, abs(own)))))
                got = w[inv == x]
                assert np.all(got == got[0]) and abs(float(got[0]) - own) <= bound, (bytes(row), float(got[0]), own)
        for s in seqs:
            assert_fold_scores(ctx.fold_scores_packed(s, *model), P, s, model, f"B_lim n={len(s)}")
    finally:
        ctx.close()


@functools.lru_cache(None)
def log_count(k, short):
    return math.log(count_structures(tuple(int(x) for x in T.zero_records()[k]), short))


@pytest.mark.parametrize("short", [False, True])
def test_zero_tables_tree_order_counts_structures(short):
    """all-zero tables, CONTRAfold: every structure weighs 1, so exp(ln Z) is the number of structures, a known
    answer that needs no oracle.  (The reference order gets no such bound: its own arithmetic sits up to 4.6e-4
    from ln(count); its anchor stays the oracle's bits.)"""
    P = T.ZERO()
    neighbour = records(LARGE)[0]
    ctx = context("A", 1)
    worst = 0.0
    try:
        ctx.sync_params(P)
        for lane, beside in ((1, []), (2, [neighbour])):
            ctx.set("tree_lane", lane)
            for k, seq in enumerate(T.zero_records()):
                mats, logz = ctx.bpp_batch([seq] + beside, True, short)
                lc = log_count(k, short)
                worst = max(worst, abs(float(logz[0]) - lc) / logz_bound(lc))
                assert abs(float(logz[0]) - lc) <= logz_bound(lc), (lane, len(seq), float(logz[0]), lc)
                ref, _ = O.bpp(P.ptr, seq, True, short)
                p = np.asarray(mats[0].packed)
                assert np.array_equal(p >= -0.5, ref >= -0.5), (lane, len(seq))
                d = mats[0].dense().astype(np.float64)
                d[d < -0.5] = 0.0
                assert np.all((d + d.T).sum(axis=1) <= 1 + 1e-5), (lane, len(seq), (d + d.T).sum(axis=1).max())
    finally:
        ctx.close()
    print(f"short={short}: worst |ln Z - ln count| = {worst:.3f} of the tree-order bound")
