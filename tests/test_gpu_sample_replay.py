"""Every decision of the GPU sampler replayed on the CPU (tests/sample_replay.py).

The grammar is unambiguous and the oracle's fold sums are the device's bit for bit (asserted first in
every test), so each sampled row names its decisions, and each decision is judged against the
contract of include/rnamc.h: Philox4x32-10 keyed by the seed on the counter (decision index, t, s, 0),
u from word 0, candidates in the documented order, the first inclusive prefix above u * total, within
EPS = 2^-17 of the total (derived in sample_replay).  The f32 sum of the walker's local scores is
rebuilt in decision order and must equal the returned log-weight bit for bit.  Each test prints the
largest distance of a decision from its exact f64 interval, as a fraction of the total.

test_sample_replay_cpu.py shows what this audit rejects."""
import numpy as np
import pytest

import oracle_lib as O
import sample_replay as SR

pytestmark = pytest.mark.gpu

MODELS = [(False, False), (True, False), (True, True)]
HIGH_SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def assert_device_sums(ctx, params, seq, contra, short, sums=None):
    """the device's seven inside matrices are the oracle's, bit for bit"""
    ref = sums if sums is not None else O.fold_sums(params.ptr, seq, contra, short)
    got = ctx.fold_sums(seq, contra, short)
    for f in O.FOLD_SUMS_FIELDS:
        assert np.array_equal(got.dense[f].view(np.uint32), ref[f].view(np.uint32)), f


def audit(r, rows, weights, seed, s, ts, tally):
    """rows[t], weights[t] of batch index s, for t in ts: every decision passes, every log-weight is
    the replay's f32 sum"""
    rng = SR.Rng(seed)
    for t in ts:
        t = int(t)
        bad, lw = r.audit_row(rows[t], rng, s, t, tally)
        assert not bad, (f"s = {s}, t = {t}: {len(bad)} decisions outside the interval; first (dec, type, i, j, "
                         f"cnt, pick), u, excess: {bad[0]}; row {bytes(rows[t]).decode()}")
        assert lw.tobytes() == weights[t].tobytes(), (s, t, float(lw), float(weights[t]), bytes(rows[t]).decode())


def report(name, tally):
    print(f"{name}: {tally.decisions} decisions audited, largest excess over the exact interval "
          f"{tally.excess:.3e} of the total (eps = {SR.EPS:.3e}); cnt > 512: {tally.wide_names()}; "
          f"C alternatives: {tally.c_alt}")


@pytest.mark.parametrize("contra,short", MODELS)
def test_trnas(ctx, params, trnas, contra, short):
    """six tRNAs in one batch (s = 0..5), 200 samples each; every alternative of C is audited at
    least 20 times"""
    seqs = [s for _, s in trnas]
    reps = [SR.Replay(params, s, contra, short) for s in seqs]
    assert_device_sums(ctx, params, seqs[0], contra, short, reps[0].sums)
    rows, w, _ = ctx.sample_batch(seqs, 200, contra, short, seed=21)
    tally = SR.Tally()
    for s, r in enumerate(reps):
        audit(r, rows[s], w[s], 21, s, range(200), tally)
    report("tRNAs", tally)
    assert min(tally.c_alt.values()) >= 20, tally.c_alt


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("n", SR.BOUNDARY_LENGTHS)
def test_boundary_lengths(ctx, params, n, contra):
    """X(n - 1) has n candidates: 64 and 65 sit on both sides of one wave step, 512 and 513 on both sides
    of the eight steps whose terms stay in registers; 5 is the shortest sequence that can pair"""
    seq = SR.boundary_seq(n)
    r = SR.Replay(params, seq, contra)
    assert_device_sums(ctx, params, seq, contra, False, r.sums)
    rows, w, _ = ctx.sample_batch([seq], 100, contra, False, seed=31 + n)
    tally = SR.Tally()
    audit(r, rows[0], w[0], 31 + n, 0, range(100), tally)
    report(f"n = {n}", tally)
    assert n in tally.cnts and tally.decisions >= 100
    if n >= 64:
        assert len(np.unique(rows[0], axis=0)) > 1


@pytest.mark.parametrize("contra", [False, True])
def test_wide_multiloop(ctx, params, contra):
    """the designed input of sample_replay.wide_multiloop: scans of more than 512 candidates (terms
    evaluated again in each pass, the prefix carried across more than eight steps) in every cell type
    that has them.  Under CONTRAfold the interior nests instead of branching, so no O cell that wide
    arises there (the reference sampler draws none in 100 samples); the Turner case carries O."""
    seq = SR.wide_multiloop()
    r = SR.Replay(params, seq, contra)
    assert_device_sums(ctx, params, seq, contra, False, r.sums)
    rows, w, _ = ctx.sample_batch([seq], 100, contra, False, seed=41)
    tally = SR.Tally()
    audit(r, rows[0], w[0], 41, 0, range(100), tally)
    report("wide multiloop", tally)
    wide = tally.wide_names()
    if contra:
        del wide["O"]
    assert min(wide.values()) >= 20, wide


def test_ragged_batch(ctx, params):
    """five sequences whose length order is not their input order, swept in groups of two and in one
    group: the same bytes, and every decision drawn with the caller's batch index"""
    lens = [40, 90, 25, 130, 60]
    seqs = [O.splitmix_seq(n, 6100 + n) for n in lens]
    for contra in (False, True):
        reps = [SR.Replay(params, s, contra) for s in seqs]
        assert_device_sums(ctx, params, seqs[3], contra, False, reps[3].sums)
        ctx.set("group_max_seqs", 2)
        try:
            small = ctx.sample_batch(seqs, 60, contra, False, seed=51)
        finally:
            ctx.set("group_max_seqs", 8192)
        whole = ctx.sample_batch(seqs, 60, contra, False, seed=51)
        for a, b in zip(small[0], whole[0]):
            assert a.tobytes() == b.tobytes()
        assert small[1].tobytes() == whole[1].tobytes()
        tally = SR.Tally()
        for s, r in enumerate(reps):
            audit(r, small[0][s], small[1][s], 51, s, range(60), tally)
        report("ragged batch", tally)
        assert tally.decisions >= 5 * 60


def test_many_samples(ctx, params):
    """20 000 samples of a 30-mer, more (sequence, sample) items than the kernel has waves: the first
    200, the last 200 and 200 drawn by a fixed seed"""
    N = 20_000
    seq = O.splitmix_seq(30, 7130)
    ts = np.unique(np.concatenate([np.arange(200), np.arange(N - 200, N),
                                   np.random.default_rng(5).choice(N, 200, replace=False)]))
    for contra in (False, True):
        r = SR.Replay(params, seq, contra)
        assert_device_sums(ctx, params, seq, contra, False, r.sums)
        rows, w, _ = ctx.sample_batch([seq], N, contra, False, seed=61)
        tally = SR.Tally()
        audit(r, rows[0], w[0], 61, 0, ts, tally)
        report("many samples", tally)
        assert len(np.unique(rows[0][ts], axis=0)) > 1 and tally.decisions >= len(ts)


def test_high_seed_bits(ctx, params, trnas):
    """a seed with its high word set: the key's second word is the seed's high half (the same audit
    with the high word dropped rejects these samples).  Sample t = 57 of the CONTRAfold run is the one
    this audit caught: at C(9, 66) u * total lies 4e-9 of the total under the prefix of candidate 3, and
    the f32 scan put the prefix of candidate 4, a -inf term, above it: the kernel without the weight
    test in its pass 2 paired C-C at (10, 62)"""
    seq = trnas[1][1]
    for contra in (False, True):
        r = SR.Replay(params, seq, contra)
        assert_device_sums(ctx, params, seq, contra, False, r.sums)
        rows, w, _ = ctx.sample_batch([seq], 200, contra, False, seed=HIGH_SEED)
        tally = SR.Tally()
        audit(r, rows[0], w[0], HIGH_SEED, 0, range(200), tally)
        report("high seed bits", tally)
        low = SR.Rng(HIGH_SEED, drop_high=True)
        assert sum(len(r.audit_row(rows[0][t], low, 0, t)[0]) for t in range(20)) > 0


def test_constrained(ctx, params):
    """constraint_masks.mixed_case(120): the terms come from the oracle's sums with the forbidden pairs'
    keys absent, and no sampled pair is a forbidden one"""
    import constraint_masks as CM
    seq, cons, span, mask = CM.mixed_case(120)
    for contra in (False, True):
        assert_device_sums(ctx, params, seq, contra, False)
        r = SR.Replay(params, seq, contra, False, mask)
        rows, w, _ = ctx.sample_batch([seq], 200, contra, False, seed=71, constraints=[cons], max_bp_span=span)
        tally = SR.Tally()
        audit(r, rows[0], w[0], 71, 0, range(200), tally)
        report("constrained", tally)
        for row in np.unique(rows[0], axis=0):
            pt = SR.partners(row)
            assert all(mask[i, pt[i]] for i in range(120) if pt[i] > i)
        assert len(np.unique(rows[0], axis=0)) > 1
