"""Hard constraints on the GPU (include/rnamc.h): neutral constraints change nothing bit for bit;
constrained ln Z, pair probabilities and MFE against the enumeration of the compatible nested
structures; the 'x' identity P(p unpaired) = Z_{x@p} / Z at scale; everything forbidden; the
consistency of keys, samples and MFE structures with the constraint; sampled frequencies against
constraint_probability; batch invariance; error paths; the CLIs."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from constraint_masks import allowed_matrix, enumerate_constrained, pairs_of, sscore, tol
from test_constraints_cpu import allowed, random_constraint

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [(False, False), (True, False), (True, True)]  # (contra, allows_short_hairpins)


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


def mode(ctx, summation, **knobs):
    ctx.set("summation_mode", summation)
    for k, v in knobs.items():
        ctx.set(k, v)


def reset(ctx):
    for k, v in (("summation_mode", 0), ("latency_mode", 1), ("tree_lane", 1), ("group_max_seqs", 8192)):
        ctx.set(k, v)


def plain_bpp(ctx, seqs):
    """rnamc_bpp_batch itself (the entry without constraints)"""
    from rna_algos_amd import _lib

    def run(contra, short):
        lens = np.array([len(s) for s in seqs], np.uint64)
        offs = np.zeros(len(seqs) + 1, np.uint64)
        np.cumsum(lens, out=offs[1:])
        oo = np.zeros(len(seqs) + 1, np.uint64)
        np.cumsum(lens * (lens + 1) // 2, out=oo[1:])
        bases = np.concatenate([np.asarray(s, np.uint8) for s in seqs])
        out = np.empty(int(oo[-1]), np.float32)
        lz = np.empty(len(seqs), np.float32)
        _lib.check(_lib.lib().rnamc_bpp_batch(ctx._h, len(seqs), bases.ctypes.data, offs.ctypes.data,
                                              int(contra), int(short), out.ctypes.data, oo.ctypes.data,
                                              lz.ctypes.data))
        return out, lz
    return run


def packed(mats):
    return np.concatenate([m.packed for m in mats])


def mfe_score_tol(w, n_pairs):
    return 4 * (n_pairs + 1) * float(np.spacing(np.float32(max(1.0, abs(w)))))


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contra,short", MODELS)
def test_neutral_constraints_bit_identical(ctx, params, trnas, contra, short):
    from rna_algos_amd.mccaskill_algo import Pool
    seqs = [np.asarray(s, np.uint8) for _, s in trnas] + [O.splitmix_seq(1024, 1024)]
    nmax = max(len(s) for s in seqs)
    dots = ["." * len(s) for s in seqs]
    # "<" on the first base and ">" on the last forbid nothing, yet make the call constrained: the
    # words are installed and pair_allowed runs at every site (reference batch and latency forms,
    # max-plus sweep, tree order lone and lane-per-cell) -- so do mixed batches of it and no string
    ends = ["<" + "." * (len(s) - 2) + ">" for s in seqs]
    mixed = [e if k % 2 else None for k, e in enumerate(ends)]
    neutral = [(None, 0), (dots, 0), (None, nmax), (dots, nmax), ([None] * len(seqs), 0),
               (ends, 0), (ends, nmax), (mixed, 0)]
    settings = [(0, dict(latency_mode=0)), (0, dict(latency_mode=2)), (1, dict(tree_lane=0)),
                (1, dict(tree_lane=2))]
    try:
        for summation, knobs in settings:
            mode(ctx, summation, **knobs)
            ref_b, ref_z = plain_bpp(ctx, seqs)(contra, short)
            for cons, span in neutral:
                mats, lz = ctx.bpp_batch(seqs, contra, short, cons, span)
                assert packed(mats).tobytes() == ref_b.tobytes(), (summation, knobs, span)
                assert lz.tobytes() == ref_z.tobytes()
            reset(ctx)
        dbs0, sc0, dp0 = ctx.mfe_batch(seqs, contra, short)
        rows0, w0, z0 = ctx.sample_batch(seqs, 50, contra, short, seed=9)
        lp0 = ctx.log_partition_batch(seqs, contra, short)
        for cons, span in neutral:
            dbs, sc, dp = ctx.mfe_batch(seqs, contra, short, cons, span)
            assert dbs == dbs0 and sc.tobytes() == sc0.tobytes() and dp.tobytes() == dp0.tobytes()
            rows, w, z = ctx.sample_batch(seqs, 50, contra, short, seed=9, constraints=cons, max_bp_span=span)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(rows, rows0))
            assert w.tobytes() == w0.tobytes() and z.tobytes() == z0.tobytes()
            assert ctx.log_partition_batch(seqs, contra, short, cons, span).tobytes() == lp0.tobytes()
        pool = Pool(params, devices=[0])
        try:
            ref_m, ref_pz = pool.bpp_batch(seqs, contra, short)
            for cons, span in neutral:
                mats, lz = pool.bpp_batch(seqs, contra, short, cons, span)
                assert packed(mats).tobytes() == packed(ref_m).tobytes()
                assert lz.tobytes() == ref_pz.tobytes()
        finally:
            pool.close()
    finally:
        reset(ctx)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contra,short", MODELS)
def test_exhaustive_small(ctx, params, contra, short):
    from rna_algos_amd.mccaskill_algo import is_compatible
    rng = random.Random(700 + 10 * contra + short)
    cases = []
    for k in range(10):
        n = 8 + (k * 5) % 15  # 8 .. 22
        seq = O.splitmix_seq(n, 8800 + k)
        cons = random_constraint(rng, n) if k % 3 != 2 else None
        span = rng.choice([0, 0, rng.randint(4, n)])
        cases.append((seq, cons, span))
    cases.append((O.splitmix_seq(12, 8899), "(" + "." * 10 + ")", 0))  # a constraint pair at any bases
    try:
        for seq, cons, span in cases:
            n = len(seq)
            lz_e, probs, best, ws, dbs = enumerate_constrained(params, seq, cons, span, contra, short)
            for summation in (0, 1):
                mode(ctx, summation)
                mats, lz = ctx.bpp_batch([seq], contra, short, None if cons is None else [cons], span)
                d = mats[0].dense().astype(np.float64)
                if summation == 0:
                    assert abs(float(lz[0]) - lz_e) <= 2e-3, (cons, span, lz, lz_e)
                else:
                    assert abs(float(lz[0]) - lz_e) <= 1e-5 * max(1.0, abs(lz_e)), (cons, span, lz, lz_e)
                for i in range(n):
                    for j in range(i + 1, n):
                        p = probs.get((i, j), 0.0)
                        if p > 0:
                            assert d[i, j] >= 0, (summation, cons, span, i, j, p)
                            assert abs(d[i, j] - p) <= (2e-3 if summation == 0 else 2e-6), (summation, i, j, d[i, j], p)
                        else:
                            assert d[i, j] < -0.5 or d[i, j] <= 1e-30, (summation, cons, span, i, j, d[i, j])
                            if summation == 0:
                                assert d[i, j] < -0.5
            reset(ctx)
            dbm, sc, dp = ctx.mfe_batch([seq], contra, short, None if cons is None else [cons], span)
            db = dbm[0]
            assert is_compatible(db, cons, span), (db, cons, span)
            t = tol(best, db)
            assert abs(float(sc[0]) - best) <= t and abs(float(dp[0]) - best) <= t, (db, sc, dp, best)
            assert abs(sscore(params, seq, db, contra, short) - best) <= t
            lp = ctx.log_partition_batch([seq], contra, short, None if cons is None else [cons], span)
            assert abs(float(lp[0]) - lz_e) <= 2e-3
    finally:
        reset(ctx)


# ---------------------------------------------------------------------------------------------------
def x_at(n, p):
    return "." * p + "x" + "." * (n - 1 - p)


@pytest.mark.parametrize("contra", [False, True])
def test_x_identity_tree_order_at_scale(ctx, params, contra):
    """n = 900, tree order: exp(ln Z_{x@p} - ln Z) against the f64 unpaired probabilities of the
    exact evaluation, lone sequences and a lane-per-cell batch"""
    n = 900
    seq = O.splitmix_seq(n, 9009)
    xb, xz = O.exact_bpp(params.ptr, seq, contra, False)
    full = np.zeros((n, n))
    idx = 0
    for d in range(n):  # packed diagonal-major triangle -> dense
        row = np.asarray(xb[idx:idx + n - d], np.float64)
        full[np.arange(n - d), np.arange(n - d) + d] = np.where(row > 0, row, 0.0)
        idx += n - d
    sym = full + full.T
    unpaired = 1.0 - sym.sum(axis=1)
    pos = [int(x) for x in np.linspace(3, n - 4, 16)]
    worst = {}
    try:
        mode(ctx, 1, tree_lane=0)
        _, z0 = ctx.bpp_batch([seq], contra, False)
        got = []
        for p in pos:
            _, zc = ctx.bpp_batch([seq], contra, False, [x_at(n, p)])
            got.append(math.exp(float(zc[0]) - float(z0[0])))
        worst["lone"] = max(abs(g - unpaired[p]) for g, p in zip(got, pos))
        mode(ctx, 1, tree_lane=2)
        _, zs = ctx.bpp_batch([seq] * (len(pos) + 1), contra, False, [None] + [x_at(n, p) for p in pos])
        got = [math.exp(float(zs[k + 1]) - float(zs[0])) for k in range(len(pos))]
        worst["lane"] = max(abs(g - unpaired[p]) for g, p in zip(got, pos))
    finally:
        reset(ctx)
    print(f"contra={contra}: max |P(x@p) - (1 - sum_j p(p, j))| at n = {n}: lone {worst['lone']:.2e}, "
          f"lane batch {worst['lane']:.2e}")
    assert max(worst.values()) <= 1e-3, worst


@pytest.mark.parametrize("contra", [False, True])
def test_x_identity_trnas_reference_order(ctx, trnas, contra):
    worst = 0.0
    for _, seq in trnas:
        n = len(seq)
        mats, lz = ctx.bpp_batch([seq], contra, False)
        d = mats[0].dense().astype(np.float64)
        d = np.where(d > 0, d, 0.0)
        sym = d + d.T
        pos = list(range(0, n, 3))
        lzc = ctx.log_partition_batch([seq] * len(pos), contra, False, [x_at(n, p) for p in pos])
        for p, zc in zip(pos, lzc):
            worst = max(worst, abs(math.exp(float(zc) - float(lz[0])) - (1.0 - sym[p].sum())))
    print(f"contra={contra}: tRNAs, reference order: max |P(x@p) - (1 - sum_j p(p, j))| {worst:.2e}")
    assert worst <= 5e-3


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contra,short", MODELS)
def test_everything_forbidden(ctx, params, contra, short):
    seqs = [np.asarray(s, np.uint8) for s in (O.splitmix_seq(40, 1), O.splitmix_seq(200, 2))]
    unp = float(params.field("contra.external_score_unpair")[0])
    variants = [(["x" * len(s) for s in seqs], 0), (None, 1)]
    if not contra:
        variants.append((None, 4))
    try:
        for cons, span in variants:
            for summation in (0, 1):
                mode(ctx, summation)
                mats, lz = ctx.bpp_batch(seqs, contra, short, cons, span)
                for s, m, z in zip(seqs, mats, lz):
                    assert np.all(m.packed == -1.0), (summation, span)
                    want = len(s) * unp if contra else 0.0
                    assert abs(float(z) - want) <= 4 * len(s) * float(np.spacing(np.float32(max(1.0, abs(want)))))
            reset(ctx)
            dbs, sc, _ = ctx.mfe_batch(seqs, contra, short, cons, span)
            assert dbs == ["." * len(s) for s in seqs]
            rows, _, _ = ctx.sample_batch(seqs, 20, contra, short, seed=4, constraints=cons, max_bp_span=span)
            for r in rows:
                assert np.all(r == ord("."))
    finally:
        reset(ctx)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contra,short", MODELS)
def test_consistency(ctx, params, trnas, contra, short):
    from rna_algos_amd.mccaskill_algo import is_compatible
    rng = random.Random(31 + contra + 2 * short)
    seqs = [np.asarray(s, np.uint8) for _, s in trnas] + [O.splitmix_seq(1024, 77)]
    cons = [random_constraint(rng, len(s)) for s in seqs]
    for span in (0, 60):
        _, lz0 = ctx.bpp_batch(seqs, contra, short)
        for summation in (0, 1):
            mode(ctx, summation)
            mats, lz = ctx.bpp_batch(seqs, contra, short, cons, span)
            for s, c, m, z, z0 in zip(seqs, cons, mats, lz, lz0):
                present = np.triu(m.dense() >= -0.5, 1)
                assert not np.any(present & ~allowed_matrix(c, span)), (len(s), summation, span)
                if span:
                    ii, jj = np.nonzero(present)
                    assert np.all(jj - ii + 1 <= span)
                if summation == 0:
                    assert float(z) <= float(z0) + 1e-4 * max(1.0, abs(float(z0)))
            reset(ctx)
        dbs, sc, _ = ctx.mfe_batch(seqs, contra, short, cons, span)
        rows, w, _ = ctx.sample_batch(seqs, 200, contra, short, seed=5, constraints=cons, max_bp_span=span)
        for s, c, db, best, r, ws in zip(seqs, cons, dbs, sc, rows, w):
            assert is_compatible(db, c, span)
            for row in np.unique(r, axis=0):
                assert is_compatible(bytes(row).decode(), c, span)
            assert float(best) >= float(ws.max()) - mfe_score_tol(float(best), len(s) // 2)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contra", [False, True])
def test_sampling_frequency(ctx, params, trnas, contra):
    from rna_algos_amd.mccaskill_algo import constraint_probability, is_compatible
    seq = np.asarray(trnas[0][1], np.uint8)
    n = len(seq)
    N = 20000
    rows, _, _ = ctx.sample_batch([seq], N, contra, False, seed=17)
    u, cnt = np.unique(rows[0], axis=0, return_counts=True)
    dbs = [bytes(x).decode() for x in u]
    mats, _ = ctx.bpp_batch([seq], contra, False)
    d = mats[0].dense()
    i0, j0 = max(((i, j) for i in range(n) for j in range(i + 1, n)), key=lambda ij: d[ij])
    cases = [("." * 30 + "x" * 8 + "." * (n - 38), 0),
             ("." * i0 + "(" + "." * (j0 - i0 - 1) + ")" + "." * (n - 1 - j0), 0),
             (None, 40)]
    for c, span in cases:
        P = constraint_probability(seq, c, contra, False, params, span)
        f = sum(k for db, k in zip(dbs, cnt) if is_compatible(db, c, span)) / N
        assert abs(f - P) <= 5 * math.sqrt(P * (1 - P) / N) + 2e-3, (c, span, f, P)


# ---------------------------------------------------------------------------------------------------
def test_batch_invariance(ctx, params, trnas):
    from rna_algos_amd.mccaskill_algo import Pool
    rng = random.Random(5)
    seqs = [np.asarray(s, np.uint8) for _, s in trnas] + [O.splitmix_seq(300, 3)]
    cons = []
    for k, s in enumerate(seqs):
        cons.append([random_constraint(rng, len(s)), "." * len(s), None][k % 3])
    for contra in (False, True):
        mats, lz = ctx.bpp_batch(seqs, contra, False, cons)
        for k, s in enumerate(seqs):
            m1, z1 = ctx.bpp_batch([s], contra, False, [cons[k]])
            assert m1[0].packed.tobytes() == mats[k].packed.tobytes() and z1.tobytes() == lz[k:k + 1].tobytes()
        ctx.set("group_max_seqs", 1)
        try:
            m2, z2 = ctx.bpp_batch(seqs, contra, False, cons)
        finally:
            ctx.set("group_max_seqs", 8192)
        assert packed(m2).tobytes() == packed(mats).tobytes() and z2.tobytes() == lz.tobytes()
        pool = Pool(params, devices=[0, 0])
        try:
            m3, z3 = pool.bpp_batch(seqs, contra, False, cons)
        finally:
            pool.close()
        assert packed(m3).tobytes() == packed(mats).tobytes() and z3.tobytes() == lz.tobytes()
        assert ctx.log_partition_batch(seqs, contra, False, cons).tobytes() == lz.tobytes()


def test_error_paths(ctx, trnas):
    from rna_algos_amd import _lib
    seqs = [np.asarray(s, np.uint8) for _, s in trnas[:3]]
    good = ["." * len(s) for s in seqs]
    ref, refz = ctx.bpp_batch(seqs, False, False, good, 50)
    for bad in ("|", "(", ")", "A"):
        cons = list(good)
        cons[1] = bad + cons[1][1:]
        for call in (lambda: ctx.bpp_batch(seqs, False, False, cons),
                     lambda: ctx.mfe_batch(seqs, False, False, cons),
                     lambda: ctx.sample_batch(seqs, 3, False, False, constraints=cons),
                     lambda: ctx.log_partition_batch(seqs, False, False, cons)):
            with pytest.raises(_lib.RnamcError) as e:
                call()
            assert e.value.status == _lib.ERR_INVALID_ARG and "record 1" in str(e.value)
    with pytest.raises(_lib.RnamcError):
        ctx.bpp_batch(seqs, False, False, [good[0], good[1][:-1], good[2]])
    m, z = ctx.bpp_batch(seqs, False, False, good, 50)
    assert packed(m).tobytes() == packed(ref).tobytes() and z.tobytes() == refz.tobytes()


def test_pool_error_paths(params, trnas):
    """the pool entry validates every record's constraint before it shards (rnamc_pool.cpp), and
    the pool works normally afterwards"""
    from rna_algos_amd import _lib
    from rna_algos_amd.mccaskill_algo import Pool
    seqs = [np.asarray(s, np.uint8) for _, s in trnas[:3]]
    cons = ["<" + "." * (len(s) - 2) + ">" for s in seqs]
    pool = Pool(params, devices=[0, 0])
    try:
        ref, refz = pool.bpp_batch(seqs, False, False, cons, 60)
        for bad in ("|", "(", ")", "A"):
            b = list(cons)
            b[1] = bad + b[1][1:]
            _lib.lib().rnamc_constraint_check(b"|", 1, 0, None, None)  # (another message first)
            with pytest.raises(_lib.RnamcError) as e:
                pool.bpp_batch(seqs, False, False, b, 60)
            assert e.value.status == _lib.ERR_INVALID_ARG
            assert "record 1" in str(e.value), str(e.value)
        m, z = pool.bpp_batch(seqs, False, False, cons, 60)
        assert packed(m).tobytes() == packed(ref).tobytes() and z.tobytes() == refz.tobytes()
    finally:
        pool.close()


def test_shared_context_threads(ctx, trnas):
    """calls on one context from two threads are serialised: a constrained and an unconstrained
    caller, interleaved, get exactly what each gets alone"""
    import threading
    seqs = [np.asarray(s, np.uint8) for _, s in trnas]
    short = [s[:40] for s in seqs]  # (shorter records than the constrained caller's)
    cons = ["." * 10 + "x" * 12 + "." * (len(s) - 22) for s in seqs]
    want_c = ctx.bpp_batch(seqs, False, False, cons, 50)
    want_u = ctx.bpp_batch(short, False, False)
    errors = []

    def worker(f, want):
        try:
            for _ in range(8):
                m, z = f()
                if packed(m).tobytes() != packed(want[0]).tobytes() or z.tobytes() != want[1].tobytes():
                    errors.append("result differs from the lone call")
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(lambda: ctx.bpp_batch(seqs, False, False, cons, 50), want_c)),
          threading.Thread(target=worker, args=(lambda: ctx.bpp_batch(short, False, False), want_u))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---------------------------------------------------------------------------------------------------
def test_clis(tmp_path):
    from rna_algos_amd.mccaskill_algo import is_compatible
    from rna_algos_amd.utils import read_fasta
    fa = os.path.join(ROOT, "tests", "golden", "sampled_trnas.fa")
    recs = read_fasta(fa)
    rng = random.Random(3)
    cons = [random_constraint(rng, len(s)) for _, s in recs]
    cf = tmp_path / "cons.fa"
    cf.write_text("".join(f">c{k}\n{c}\n" for k, c in enumerate(cons)))
    env = dict(os.environ)

    def run(mod, *args):
        out = tmp_path / f"{mod}.txt"
        r = subprocess.run([sys.executable, "-m", f"rna_algos_amd.bin.{mod}", "-i", fa, "-o", str(out),
                            "--synthetic-tables", "1", *args], cwd=ROOT, capture_output=True, text=True,
                           timeout=600, env=env)
        assert r.returncode == 0, r.stderr
        return out.read_text()

    span = 70
    txt = run("mfe_fold", "--constraints", str(cf), "--max-bp-span", str(span))
    lines = txt.splitlines()
    for k, c in enumerate(cons):
        assert lines[2 * k] == f">{k}"
        assert is_compatible(lines[2 * k + 1].split("\t")[0], c, span)
    txt = run("sample_fold", "-n", "20", "--constraints", str(cf), "--max-bp-span", str(span))
    rec = -1
    for line in txt.splitlines():
        if line.startswith(">"):
            rec = int(line[1:])
            continue
        db, lp = line.split("\t")
        assert is_compatible(db, cons[rec], span) and float(lp) <= 1e-5
    txt = run("mccaskill_algo", "--constraints", str(cf), "--max-bp-span", str(span))
    for k, block in enumerate(txt.split("\n\n>")[1:]):
        head, _, body = block.partition("\n")
        assert int(head) == k
        for t in body.split():
            i, j, p = t.split(",")
            assert allowed(cons[k], span, int(i), int(j)) and 0 <= float(p) <= 1.001
    txt = run("accessibility", "-w", "10")
    rec, seen = -1, 0
    for line in txt.splitlines():
        if line.startswith(">"):
            rec = int(line[1:])
            continue
        a, p = line.split("\t")
        assert 0.0 <= float(p) <= 1.0
        seen += 1
    assert seen == sum(len(s) - 9 for _, s in recs)
