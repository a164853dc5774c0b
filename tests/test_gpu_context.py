"""Structural context profiles on the device (rnamc_context_profile_batch)
against the f64 replay of the sums from the CPU oracle's matrices and against the exhaustive
enumeration (tests/context_ref.py)."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [(False, False), (True, False), (True, True)]  # (contra, allows_short_hairpins)
LENGTHS = (1, 4, 5, 33, 34, 64, 65, 130, 257)  # below, at and past the 2-loop window, a wave, a 256-thread block
# Largest |device - replay| over exactly the inputs of replay_inputs() (rows 0 .. 4), measured on an
# MI355X: 6.07e-8.  The bound is four times that: what is left between the two
# is expf in f32 against exp in f64 and the rounding of the exponent to f32, which grows with the
# magnitudes that cancel in it, i.e. with ln Z.
MEASURED = 6.1e-8
BOUND = 4 * MEASURED


def _tables(name):
    import table_sets
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(1) if name == "synthetic1" else table_sets.ZERO()


@functools.lru_cache(None)
def replay_inputs():
    """[(tables name, label, seq, constraint, mask)]: the lengths under both table sets (zero tables
    up to 65), and records of the families S and E of twoloop_inputs on the level a + b = 30, its
    ends a = 0 and b = 0 included"""
    import twoloop_inputs as T
    out = [("synthetic1", f"n={n}", O.splitmix_seq(n, 9000 + n), None, None) for n in LENGTHS]
    out += [("zero", f"n={n}", O.splitmix_seq(n, 9000 + n), None, None) for n in LENGTHS if n <= 65]
    for a in (0, 1, 15, 29, 30):
        b = 30 - a
        recs = [T.Rec("S", a, b, pl, (pl + b) % 3, T.S_SHAPE) for pl in T.PLACEMENTS] + [T.Rec("E", a, b, 0, 0, T.E_SHAPE)]
        out += [("synthetic1", repr(r), r.seq, r.cons, r.mask) for r in recs]
    return out


@functools.lru_cache(None)
def replays(contra, short):
    import context_ref as R
    return [R.replay_profile(seq, contra, short, _tables(tn), mask) for tn, _, seq, _, mask in replay_inputs()]


@functools.lru_cache(None)
def device_profiles(contra, short):
    """[(profile, paired_prob of the sparse entry)] per replay input, one call per table set"""
    from rna_algos_amd.mccaskill_algo import Context
    inputs = replay_inputs()
    out = [None] * len(inputs)
    for tn in ("synthetic1", "zero"):
        idx = [x for x, inp in enumerate(inputs) if inp[0] == tn]
        ctx = Context(_tables(tn), device=0)
        try:
            seqs = [inputs[x][2] for x in idx]
            cons = [inputs[x][3] for x in idx]
            prof, _ = ctx.context_profile_batch(seqs, contra, short, cons)
            sp, _ = ctx.bpp_batch_sparse(seqs, contra, short, 0.0, cons)
        finally:
            ctx.close()
        for x, p, q in zip(idx, prof, sp):
            out[x] = (p.copy(), q.paired_prob.copy())
    return out


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


@pytest.mark.parametrize("model", MODELS)
def test_device_matches_replay(built, model):
    worst = 0.0
    for inp, r, (p, paired) in zip(replay_inputs(), replays(*model), device_profiles(*model)):
        err = float(np.abs(p[:5] - r[:5]).max())
        print(model, inp[0], inp[1], "max |device - replay| %.2e" % err, "by row",
              ["%.1e" % v for v in np.abs(p[:5] - r[:5]).max(axis=1)], "row maxima", np.round(p.max(axis=1), 3))
        worst = max(worst, err)
        assert p.shape == (6, len(inp[2])) and np.isfinite(p).all() and (p >= 0).all()
        assert np.array_equal(p[5], paired), inp[:2]  # row 5: the sparse entry's paired_prob, bit for bit
    print("worst |device - replay|", worst, "bound", BOUND)
    assert worst <= BOUND


@pytest.mark.parametrize("model", MODELS)
def test_rows_sum_to_one(built, model):
    for inp, r, (p, _) in zip(replay_inputs(), replays(*model), device_profiles(*model)):
        dev = float(np.abs(p.astype(np.float64).sum(axis=0) - 1).max())
        own = float(np.abs(r.sum(axis=0) - 1).max())
        print(model, inp[0], inp[1], "|sum - 1| device %.2e replay %.2e" % (dev, own))
        assert dev <= own + 6 * BOUND, (inp[:2], dev, own)


def test_every_class_is_exercised(built):
    """not vacuous: over the replay inputs every row reaches 0.05 somewhere, bulges and internal loops
    at the ends of the 2-loop window (a + b = 30 with an empty side, and without) included"""
    tops = np.max([r.max(axis=1) for m in MODELS for r in replays(*m)], axis=0)
    assert (tops >= 0.05).all(), tops
    import context_ref as R
    for (tn, label, _, _, _), r in zip(replay_inputs(), replays(False, False)):
        if label.startswith("S(a=0, b=30") or label.startswith("S(a=30, b=0"):
            assert r[R.BULGE].max() > 0.05, label
        if label.startswith("S(a=15, b=15"):
            assert r[R.INTERNAL].max() > 0.05, label


@pytest.mark.parametrize("tables_name", ["synthetic1", "zero"])
def test_device_matches_enumeration(built, tables_name):
    """the CPU test's inputs and the CPU test's bound"""
    import test_context_cpu as cpu
    from rna_algos_amd.mccaskill_algo import Context
    from rna_algos_amd.utils import bytes2seq
    seqs = [bytes2seq(s) for s, _ in cpu.FIXED] + [O.splitmix_seq(n, seed) for n, seed, _ in cpu.SPLITMIX]
    models = [m for _, m in cpu.FIXED] + [m for _, _, m in cpu.SPLITMIX]
    b = cpu.bound(tables_name)
    c = Context(_tables(tables_name), device=0)
    try:
        for x, ((label, e, _, _), seq, (contra, short)) in enumerate(zip(cpu.cases(tables_name), seqs, models)):
            prof, _ = c.context_profile_batch([seq], contra, short)
            err = float(np.abs(prof[0] - e).max())
            print(tables_name, label, "max |device - enumeration| %.2e" % err, "bound %.2e" % b)
            assert err <= b, (label, err, b)
    finally:
        c.close()


def _batch24():
    return [O.splitmix_seq(int(n), 5200 + int(n)) for n in np.linspace(20, 130, 24).astype(int)]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("model", MODELS)
def test_schedule_independence_bit_for_bit(built, params, model):
    from rna_algos_amd.mccaskill_algo import Context, Pool
    contra, short = model
    seqs = _batch24()
    c = Context(params, device=0)
    try:
        base, z = c.context_profile_batch(seqs, contra, short)
        assert c.stats()["n_groups"] == 1
        for knob, value, groups in (("group_ws_bytes", 4, 24), ("group_max_seqs", 3, 8)):
            k = Context(params, device=0)
            try:
                k.set(knob, value)
                got, gz = k.context_profile_batch(seqs, contra, short)
                assert k.stats()["n_groups"] == groups
            finally:
                k.close()
            assert _same(base, got) and np.array_equal(z, gz), knob
        k = Context(params, device=0)
        try:
            k.set("group_ws_bytes", 1 << 21)  # groups of a few records, more of the short ones
            got, _ = k.context_profile_batch(seqs, contra, short)
            assert 1 < k.stats()["n_groups"] < 24
        finally:
            k.close()
        assert _same(base, got)
        rev, _ = c.context_profile_batch(seqs[::-1], contra, short)
        assert _same(base, rev[::-1])
        one, _ = c.context_profile_batch(seqs[:1], contra, short)
        assert _same(base[:1], one)
        again, _ = c.context_profile_batch(seqs, contra, short)
        assert _same(base, again)
    finally:
        c.close()
    p = Pool(params, devices=[0])
    try:
        pooled, pz = p.context_profile_batch(seqs, contra, short)
    finally:
        p.close()
    assert _same(base, pooled) and np.array_equal(z, pz)


@pytest.mark.parametrize("model", MODELS)
def test_constraints_and_span_limit(built, params, model):
    """an x run, a bracket pair and a span limit at n = 65 against the masked replay"""
    import context_ref as R
    from constraint_masks import allowed_matrix
    from rna_algos_amd.mccaskill_algo import Context
    contra, short = model
    n, span = 65, 50
    seq = O.splitmix_seq(n, 6565)
    canon = {(0, 3), (1, 2), (2, 1), (2, 3), (3, 0), (3, 2)}
    i, j = next((i, j) for i in range(5, 20) for j in range(i + 30, i + 45) if (int(seq[i]), int(seq[j])) in canon)
    cons = ["."] * n
    cons[i], cons[j] = "(", ")"
    for x in range(i + 8, i + 14):
        cons[x] = "x"
    cons = "".join(cons)
    mask = np.ascontiguousarray(allowed_matrix(cons, span), np.uint8)
    r = R.replay_profile(seq, contra, short, params, mask)
    free = R.replay_profile(seq, contra, short, params)
    assert np.abs(r - free).max() > 0.05  # the constraint binds
    c = Context(params, device=0)
    try:
        prof, _ = c.context_profile_batch([seq], contra, short, [cons], span)
        sp, _ = c.bpp_batch_sparse([seq], contra, short, 0.0, [cons], span)
    finally:
        c.close()
    err = float(np.abs(prof[0][:5] - r[:5]).max())
    print(model, cons, "max |device - replay| %.2e" % err)
    assert err <= BOUND
    assert np.array_equal(prof[0][5], sp[0].paired_prob) and (prof[0][5][i + 8:i + 14] == 0).all()


def test_mode_independence(built, ctx):
    """the reference-order sweep whatever summation_mode says: the same bits"""
    seqs = _batch24()[::4] + [O.splitmix_seq(257, 9257)]
    try:
        ctx.set("summation_mode", 0)
        a, za = ctx.context_profile_batch(seqs, False, False)
        ctx.set("summation_mode", 1)
        b, zb = ctx.context_profile_batch(seqs, False, False)
    finally:
        ctx.set("summation_mode", 0)
    assert _same(a, b) and np.array_equal(za, zb)


@pytest.mark.parametrize("model", MODELS)
def test_existing_entries_unaffected(built, ctx, model):
    """rnamc_bpp_batch before and after a profile call on the same context: identical bits, same grouping"""
    contra, short = model
    seqs = _batch24()
    before, zb = ctx.bpp_batch(seqs, contra, short)
    groups = ctx.stats()["n_groups"]
    ctx.context_profile_batch(seqs, contra, short)
    assert ctx.stats()["n_groups"] == groups and ctx.stats()["launches_context"] > 0
    after, za = ctx.bpp_batch(seqs, contra, short)
    st = ctx.stats()
    assert st["n_groups"] == groups and st["launches_context"] == 0 and st["ms_context"] == 0
    assert all(np.array_equal(x.packed.view(np.uint32), y.packed.view(np.uint32)) for x, y in zip(before, after))
    assert np.array_equal(zb, za)


def test_profiling(built, params):
    from rna_algos_amd.mccaskill_algo import Context
    seqs = _batch24()
    c = Context(params, device=0)
    try:
        c.context_profile_batch(seqs, False, False)
        st = c.stats()
        # per group: the copy of sums_multibranch, six profile kernels, the paired kernel
        assert st["launches_context"] == 8 and st["ms_context"] == 0 and st["launches_other"] >= 8 + 2
        c.set("profile", 1)
        c.set("group_max_seqs", 8)
        c.context_profile_batch(seqs, False, False)
        st = c.stats()
        assert st["n_groups"] == 3 and st["launches_context"] == 24 and 0 < st["ms_context"] < 1e3
        assert st["ms_inside"] > 0 and st["ms_outside"] > 0
    finally:
        c.close()


def test_python_mirror_and_cli(built, params, trnas, tmp_path):
    from rna_algos_amd import mccaskill_algo as M
    from rna_algos_amd.bin import context_profile as cli
    from rna_algos_amd.mccaskill_algo import Context
    seqs = [s for _, s in trnas]
    c = Context(params, device=0)
    try:
        want, wz = c.context_profile_batch(seqs, True, False)
    finally:
        c.close()
    got, gz = M.context_profile_batch(seqs, True, False, params)
    assert _same(want, got) and np.array_equal(wz, gz)
    one, z1 = M.context_profile(seqs[2], True, False, params)
    assert np.array_equal(one, want[2]) and z1 == float(wz[2])
    for p in want:
        assert abs(p.astype(np.float64).sum(axis=0) - 1).max() < 1e-2 and p[4].max() >= 0
    out = tmp_path / "profile.txt"
    fa = os.path.join(ROOT, "tests", "golden", "sampled_trnas.fa")
    assert cli.main(["-i", fa, "-o", str(out), "-c", "--synthetic-tables", "1"]) == 0
    assert _same(want, cli.parse_profiles(out.read_text()))
