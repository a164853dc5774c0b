"""Constrained folding at scale against the pair-mask CPU oracles (oracle/README.md).  DESIGN.md
section 11 defines every constraint rule as "removes pairs", so the right answer of a constrained
call is the oracle's loops run with the forbidden pairs' sums_close keys absent:
  * reference order: every probability and ln Z bit for bit against O.bpp_masked, in the batch sweep
    and the latency forms, alone and beside unconstrained neighbours, and rnamc_log_partition_batch;
  * tree order: key sets, |dp| and |d ln Z| against O.exact_bpp_masked within the bounds of
    test_tree_vs_exact_f64, lone (wave per cell), with the VALU mid-field and as a lane-per-cell batch;
  * the sampler at n = 640 (decision scans beyond the cached 8 x 64 candidates): pair frequencies
    against the (masked) exact probabilities, every sampled pair allowed by the mask.
The masks come from constraint_masks.allowed_matrix, a restatement of the rules that shares nothing
with compile_constraint / pair_allowed."""
import numpy as np
import pytest

import oracle_lib as O
from constraint_masks import allowed_matrix, binds, exact, mixed_case, reference, warm
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

MODELS = [(False, False), (True, False), (True, True)]  # (contra, allows_short_hairpins)
KNOBS = (("summation_mode", 0), ("latency_mode", 1), ("tree_lane", 1), ("tree_mid_mx", 1))


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def reset(ctx):
    for k, v in KNOBS:
        ctx.set(k, v)


def neighbours(n):
    """two unconstrained records for a batch around the mixed case of length n (the call's span
    limit applies to them too)"""
    return [O.splitmix_seq(40, 5100 + n), O.splitmix_seq(n // 2 + 3, 5200 + n)]


def first_mismatch(ctx, params, seq, contra, short, cons, span, mask):
    """the first differing cell of each DP matrix (smallest span for the inside matrices, largest for
    the outside ones) between a lone constrained call and the masked oracle"""
    names = ["sums_close", "sums_accessible", "sums_external", "sums_1ormore", "mbclose", "pm", "pm2"]
    n = len(seq)
    ctx.bpp_batch([seq], contra, short, [cons], span)
    _, _, mats = O.bpp_masked(params.ptr, seq, contra, short, mask, dump=True)
    iu = np.triu_indices(n)
    msgs = []
    for w, name in enumerate(names):
        gv, rv = ctx.debug_fetch(0, w, n)[iu], mats[w][iu]
        bad = ~((gv == rv) | (np.isnan(gv) & np.isnan(rv)))
        if bad.any():
            k = np.nonzero(bad)[0]
            spans = iu[1][k] - iu[0][k]
            kk = k[np.argmin(spans)] if w < 5 else k[np.argmax(spans)]
            msgs.append(f"{name}: {bad.sum()} bad, e.g. ({iu[0][kk]},{iu[1][kk]}) gpu={gv[kk]!r} ref={rv[kk]!r}")
    return "; ".join(msgs) or "every fetched matrix equal"


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 130, 257, 400])
@pytest.mark.parametrize("contra,short", MODELS)
def test_reference_order_bit_identical_to_masked_oracle(ctx, params, contra, short, n):
    seq, cons, span, mask = mixed_case(n)
    ref, ref_z = reference(n, contra, short, True)
    ok, kc, kp = binds(ref, reference(n, contra, short, False)[0])
    assert ok, f"the constraint does not bind: {kc} of {kp} keys"
    others = neighbours(n)
    other_refs = [O.bpp_masked(params.ptr, s, contra, short, allowed_matrix("." * len(s), span)) for s in others]
    batch = [others[0], seq, others[1]]
    batch_cons = [None, cons, None]
    try:
        for latency_mode in (0, 2):
            ctx.set("latency_mode", latency_mode)
            what = f"n={n} contra={contra} short={short} latency_mode={latency_mode}"
            mats, lz = ctx.bpp_batch(batch, contra, short, batch_cons, span)
            one, lz1 = ctx.bpp_batch([seq], contra, short, [cons], span)
            lp = ctx.log_partition_batch(batch, contra, short, batch_cons, span)
            lp1 = ctx.log_partition_batch([seq], contra, short, [cons], span)
            got = [(mats[1], lz[1], "in a batch"), (one[0], lz1[0], "alone")]
            detail = ""
            if any(np.float32(z) != ref_z or not np.array_equal(m.packed, ref) for m, z, _ in got):
                detail = first_mismatch(ctx, params, seq, contra, short, cons, span, mask)
            for m, z, form in got:
                assert np.float32(z).tobytes() == ref_z.tobytes(), f"{what} {form}: ln Z gpu={z!r} ref={ref_z!r} :: {detail}"
                assert_same(m.packed, ref, f"{what} {form} :: {detail}")
            for m, z, (r, rz), s in zip((mats[0], mats[2]), (lz[0], lz[2]), other_refs, others):
                assert np.float32(z).tobytes() == rz.tobytes(), f"{what}: neighbour n={len(s)} ln Z"
                assert_same(m.packed, r, f"{what}: neighbour n={len(s)}")
            assert lp.tobytes() == lz.tobytes() and lp1.tobytes() == lz1.tobytes(), what
    finally:
        reset(ctx)


# ---------------------------------------------------------------------------------------------------
def deviation(a, b):
    """-> (key sets equal, max |a - b| over the pairs both hold)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ka, kb = a >= -0.5, b >= -0.5
    both = ka & kb
    return bool(np.array_equal(ka, kb)), float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


TREE_CASES = [(c, s, n) for c, s in MODELS for n in (130, 257, 640) if not (s and n == 640)]


@pytest.mark.parametrize("contra,short,n", TREE_CASES)
def test_tree_order_vs_masked_exact(ctx, params, contra, short, n):
    seq, cons, span, mask = mixed_case(n)
    warm((exact, n, contra, short, True), (reference, n, contra, short, False))
    xb, xz = exact(n, contra, short, True)
    ok, kc, kp = binds(xb, reference(n, contra, short, False)[0])
    assert ok, f"the constraint does not bind: {kc} of {kp} keys"
    other = neighbours(n)[1]
    ob, oz = O.exact_bpp_masked(params.ptr, other, contra, short, allowed_matrix("." * len(other), span))
    forms = [("lone", dict(tree_lane=0), [seq], [cons]),
             ("lone, VALU mid-field", dict(tree_lane=0, tree_mid_mx=0), [seq], [cons]),
             ("lane batch", dict(tree_lane=2), [other, seq], [None, cons])]
    bound_p, bound_z = 2e-5 + 2e-7 * n, 2e-5 + 3e-6 * abs(xz)
    report, failures = [], []
    try:
        for name, knobs, seqs, cs in forms:
            reset(ctx)
            ctx.set("summation_mode", 1)
            for k, v in knobs.items():
                ctx.set(k, v)
            mats, lz = ctx.bpp_batch(seqs, contra, short, cs, span)
            same, dp = deviation(mats[-1].packed, xb)
            dz = abs(float(lz[-1]) - xz)
            report.append(f"{name}: |dp| {dp:.2e} ({dp / bound_p:.2f} of the bound), |d ln Z| {dz:.2e} "
                          f"({dz / bound_z:.2f})")
            if not (same and dp <= bound_p and dz <= bound_z):
                failures.append((name, same, dp, dz))
            if len(seqs) == 2:
                same, dp = deviation(mats[0].packed, ob)
                dz = abs(float(lz[0]) - oz)
                if not (same and dp <= 2e-5 + 2e-7 * len(other) and dz <= 2e-5 + 3e-6 * abs(oz)):
                    failures.append((name + ", neighbour", same, dp, dz))
    finally:
        reset(ctx)
    print(f"contra={contra} short={short} n={n}: " + "; ".join(report))
    assert not failures, (failures, bound_p, bound_z)


# ---------------------------------------------------------------------------------------------------
def pair_counts(rows):
    """(n_samples, n) rows of b'(', b')', b'.' -> n x n counts of the pairs (i < j).  Within one row
    and one nesting depth opening and closing brackets alternate, so sorted by (row, depth,
    position) the k-th opening bracket pairs with the k-th closing one."""
    n_samples, n = rows.shape
    op, cl = rows == ord("("), rows == ord(")")
    assert np.all(op | cl | (rows == ord(".")))
    depth = np.cumsum(op.astype(np.int32) - cl.astype(np.int32), axis=1)
    assert np.all(depth >= 0) and np.all(depth[:, -1] == 0), "unbalanced"
    ro, po = np.nonzero(op)
    rc, pc = np.nonzero(cl)
    do, dc = depth[ro, po], depth[rc, pc] + 1
    o = np.lexsort((po, do, ro))
    c = np.lexsort((pc, dc, rc))
    i, j = po[o], pc[c]
    assert np.array_equal(ro[o], rc[c]) and np.array_equal(do[o], dc[c]) and np.all(i < j)
    counts = np.zeros((n, n), np.int64)
    np.add.at(counts, (i, j), 1)
    return counts


def dense(packed, n):
    m = np.zeros((n, n), np.float64)
    off = 0
    for d in range(n):
        idx = np.arange(n - d)
        m[idx, idx + d] = np.maximum(np.asarray(packed[off:off + n - d], np.float64), 0.0)
        off += n - d
    return m


def test_pair_counts_helper():
    rows = np.frombuffer(b"((.)).()" + b".(()())." + b"........", np.uint8).reshape(3, 8)
    want = np.zeros((8, 8), np.int64)
    for i, j in [(0, 4), (1, 3), (6, 7), (1, 6), (2, 3), (4, 5)]:
        want[i, j] += 1
    assert np.array_equal(pair_counts(rows), want)


@pytest.mark.parametrize("constrained", [False, True])
@pytest.mark.parametrize("contra", [False, True])
def test_sampler_marginals_past_cached_decisions(ctx, params, contra, constrained):
    n, N = 640, 5000
    seq, cons, span, mask = mixed_case(n)
    warm((reference, n, contra, False, constrained), (exact, n, contra, False, constrained),
         (reference, n, contra, False, False))
    rb, _ = reference(n, contra, False, constrained)
    xb, _ = exact(n, contra, False, constrained)
    same, e = deviation(rb, xb)
    assert same
    if constrained:
        ok, kc, kp = binds(rb, reference(n, contra, False, False)[0])
        assert ok, f"the constraint does not bind: {kc} of {kp} keys"
        rows, _, _ = ctx.sample_batch([seq], N, contra, False, seed=23, constraints=[cons], max_bp_span=span)
    else:
        rows, _, _ = ctx.sample_batch([seq], N, contra, False, seed=23)
    counts = pair_counts(rows[0])
    if constrained:
        assert not np.any((counts > 0) & (mask == 0)), "a sampled pair is forbidden by the mask"
    p = dense(xb, n)
    keys = dense(np.where(rb >= -0.5, 1.0, 0.0), n) > 0
    assert not np.any((counts > 0) & ~keys), "a sampled pair is not in the oracle's key set"
    f = counts / N
    bound = 6 * np.sqrt(np.clip(p * (1 - p), 0, None) / N) + 2 * e + 1e-3
    excess = np.abs(f - p) / bound
    print(f"contra={contra} constrained={constrained}: e = {e:.2e}, worst |f - p| / bound = {excess.max():.2f}, "
          f"max |f - p| = {np.abs(f - p).max():.2e}")
    assert np.all(np.abs(f - p) <= bound), float(excess.max())
