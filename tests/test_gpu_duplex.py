"""RNA-RNA duplex folding on the GPU (rnamc_duplex_batch) against the independent
f64 reference of tests/duplex_ref.py: exhaustive enumeration on small strands, the loop limit, the
recurrences at size, schedule independence bit for bit, internal consistency, the shared workspace,
and the CLI end to end.

Bounds against f64 are the project's tree-order bounds (tests/test_gpu_tree.py), n = nA + nB:
|dP|, |dpa|, |dpb| <= 2e-5 + 2e-7 n and |d ln Z| <= 2e-5 + 3e-6 |ln Z|.  The max-plus value is a
chain of at most min(nA, nB) + 1 f32 additions, each rounded once: its bound is that many half-ulps of
the largest partial value, (min(nA, nB) + 1) * 2^-24 * max(1, max |M|, max |outer + M|)."""
import os

import numpy as np
import pytest

import duplex_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABS = ("synthetic", "zero")

# ten strands of 1 .. 8 bases: single bases, mixed strands, GU-rich, all-canonical runs, and strands
# without a partner in some of the others (A x G, AAAA x CCC)
STRANDS = ["G", "C", "A", "ACGUACGU", "GGAUCCAU", "GUGUGU", "CCC", "AAAA", "UGCAUGC", "GGGGGGGG"]
SIZES = [(22, 300), (150, 150), (300, 22), (1, 70), (33, 33)]


def tol_p(n):
    return 2e-5 + 2e-7 * n


def tol_z(z):
    return 2e-5 + 3e-6 * abs(z)


def tol_best(na, nb, *mats):
    top = max([1.0] + [float(np.max(np.abs(m[np.isfinite(m)]))) for m in mats if np.isfinite(m).any()])
    return (min(na, nb) + 1) * 2.0 ** -24 * top


@pytest.fixture(scope="module")
def tables(params):
    from rna_algos_amd.utils import FoldScoreSets
    return {"synthetic": params, "zero": FoldScoreSets.new(0.0)}


@pytest.fixture(scope="module")
def ctxs(tables):
    from rna_algos_amd.mccaskill_algo import Context
    out = {tab: Context(tables[tab], device=0) for tab in TABS}
    yield out
    for c in out.values():
        c.close()


def fold(ctx, seqs, pairs, contra, **kw):
    from rna_algos_amd import _lib
    from rna_algos_amd.duplex import _duplex_batch
    return _duplex_batch(_lib.lib().rnamc_duplex_batch, ctx._h, seqs, pairs, contra, **kw)


def check_against(f, ref, label):
    """ln Z, P, pa, pb of one DuplexFold against a reference object (Enumeration or Recurrences)"""
    n = f.n_a + f.n_b
    if ref.log_z == -np.inf:
        assert f.log_z == -np.inf and not f.probs.any() and not f.bound_a.any() and not f.bound_b.any(), label
        return
    dz = abs(f.log_z - ref.log_z)
    dp = float(np.max(np.abs(f.probs - ref.P)))
    da = float(np.max(np.abs(f.bound_a - ref.pa)))
    db = float(np.max(np.abs(f.bound_b - ref.pb)))
    print(f"{label}: lnZ {ref.log_z:.6f} dlnZ {dz:.3g} (bound {tol_z(ref.log_z):.3g})  dP {dp:.3g} dpa {da:.3g} "
          f"dpb {db:.3g} (bound {tol_p(n):.3g})")
    assert dz <= tol_z(ref.log_z), label
    assert dp <= tol_p(n) and da <= tol_p(n) and db <= tol_p(n), label
    assert not np.isnan(f.probs).any()


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("tab", TABS)
def test_enumeration(tables, ctxs, tab, contra):
    """all ordered pairs of the ten strands in ONE call against the exhaustive enumeration"""
    from rna_algos_amd.duplex import duplex_score
    seqs = [R.encode(s) for s in STRANDS]
    pairs = [(x, y) for x in range(len(seqs)) for y in range(len(seqs))]
    folds = fold(ctxs[tab], seqs, pairs, contra)
    shapes = set()
    for (x, y), f in zip(pairs, folds):
        label = f"{STRANDS[x]} x {STRANDS[y]} {tab} contra={contra}"
        sc = R.Scores(tables[tab], seqs[x], seqs[y], contra)
        en = R.Enumeration(sc)
        shapes.add((f.n_a, f.n_b))
        check_against(f, en, label)
        if en.count == 0:
            assert f.best_score == -np.inf and f.pairs() == [] and set(f.structure) <= set(".&"), label
            continue
        tb = tol_best(f.n_a, f.n_b, np.array(en.weights))
        assert abs(f.best_score - en.best) <= tb, label
        chain = tuple(f.pairs())
        got = duplex_score(seqs[x], seqs[y], list(chain), contra, tables[tab])
        assert abs(got - f.best_score) <= tb, label
        # the maximiser the tie rule names (where f32 can tell the maximisers from the rest)
        if en.margin > 4 * tb:
            assert chain == en.pick, (label, chain, en.pick)
        else:
            assert abs(sc.chain_score(list(chain)) - en.best) <= 4 * tb, label
        if tab == "zero":
            assert abs(f.log_z - np.log(en.count)) <= tol_z(np.log(en.count)), label
            if en.count * tol_z(np.log(en.count)) < 0.4:  # (the bound on ln Z pins the integer)
                assert round(float(np.exp(np.float64(f.log_z)))) == en.count, label
            first = min((i, j) for i in range(f.n_a) for j in range(f.n_b) if sc.outer[i, j] > -np.inf)
            assert chain == (first,), label
    assert {(1, 1), (1, 8), (8, 1)} <= shapes
    assert folds[pairs.index((2, 0))].log_z == -np.inf  # A x G
    assert folds[pairs.index((7, 6))].log_z == -np.inf  # AAAA x CCC


@pytest.mark.parametrize("contra", [False, True])
def test_loop_limit(tables, ctxs, contra):
    """every pair canonical, zero tables: ln Z counts the duplexes, and a chain with a + b = 31 .. 34 unpaired
    bases between two pairs would change the count"""
    cases = [("GG", "C" * 36), ("C" * 36, "GG"), ("GGG", "C" * 40)]
    seqs = [R.encode(s) for ab in cases for s in ab]
    folds = fold(ctxs["zero"], seqs, [(0, 1), (2, 3), (4, 5)], contra)
    for (sa, sb), f in zip(cases, folds):
        sc = R.Scores(tables["zero"], R.encode(sa), R.encode(sb), contra)
        en = R.Enumeration(sc)
        assert not any(k - i - 1 + j - l - 1 > 30 for ch in en.chains for (i, j), (k, l) in zip(ch, ch[1:]))
        # the count with the limit off by one either way differs by more than the bound on ln Z
        label = f"{len(sa)}x{len(sb)} zero contra={contra}"
        assert abs(f.log_z - np.log(en.count)) <= tol_z(np.log(en.count)), label
        assert round(float(np.exp(np.float64(f.log_z))) / en.count, 3) == 1.0
        check_against(f, en, label)
    # GG x C*36 by hand: single pairs, and two pairs with at most 30 bases of B between them
    want = 2 * 36 + sum(1 for j1 in range(36) for j2 in range(j1) if j1 - j2 - 1 <= 30)
    assert abs(folds[0].log_z - np.log(want)) <= tol_z(np.log(want))
    assert want == 692
    assert abs(np.log(want + 4) - np.log(want)) > 4 * tol_z(np.log(want))  # b = 31 admitted: 4 more duplexes


def sized_seqs():
    """the strands of the five shapes (seeded) and the pair list of the mixed batch"""
    seqs, pairs = [], []
    for x, (na, nb) in enumerate(SIZES):
        seqs += [O.splitmix_seq(na, 1000 + x), O.splitmix_seq(nb, 2000 + x)]
        pairs.append((2 * x, 2 * x + 1))
    return seqs, pairs


_MIXED = {}


def mixed_batch(ctxs, tab, contra):
    """the five shapes in ONE call (ragged pairs, idle steps), once per table set and model"""
    if (tab, contra) not in _MIXED:
        seqs, pairs = sized_seqs()
        _MIXED[(tab, contra)] = fold(ctxs[tab], seqs, pairs, contra)
    return _MIXED[(tab, contra)]


@pytest.mark.parametrize("shape", range(len(SIZES)), ids=[f"{a}x{b}" for a, b in SIZES])
@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("tab", TABS)
def test_recurrences_at_size(tables, ctxs, tab, contra, shape):
    from rna_algos_amd.duplex import duplex_score
    seqs, pairs = sized_seqs()
    a, b = seqs[pairs[shape][0]], seqs[pairs[shape][1]]
    f = mixed_batch(ctxs, tab, contra)[shape]
    sc = R.Scores(tables[tab], a, b, contra)
    rc = R.Recurrences(sc)
    label = f"{len(a)}x{len(b)} {tab} contra={contra}"
    check_against(f, rc, label)
    tb = tol_best(len(a), len(b), rc.Mx, sc.outer + rc.Mx)
    print(f"{label}: best {rc.best:.6f} d {abs(f.best_score - rc.best):.3g} (bound {tb:.3g})")
    assert abs(f.best_score - rc.best) <= tb, label
    chain = f.pairs()
    assert chain and abs(duplex_score(a, b, chain, contra, tables[tab]) - rc.best) <= tb, label
    assert abs(sc.chain_score(chain) - rc.best) <= tb, label


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("tab", TABS)
def test_consistency(ctxs, tab, contra):
    for f in mixed_batch(ctxs, tab, contra):
        P = f.probs.astype(np.float64)
        n = f.n_a + f.n_b
        total = P.sum()
        # pa / pb are the f64 row / column sums rounded once to f32
        tol_sum = n * 2.0 ** -23 * max(1.0, total)
        assert abs(f.bound_a.astype(np.float64).sum() - total) <= tol_sum
        assert abs(f.bound_b.astype(np.float64).sum() - total) <= tol_sum
        assert np.max(np.abs(f.bound_a - P.sum(axis=1))) <= tol_p(n)
        assert np.max(np.abs(f.bound_b - P.sum(axis=0))) <= tol_p(n)
        assert P.min() >= 0.0 and P.max() <= 1.0 + 1e-6
        # every pair of the best duplex has at least that duplex's probability, exp(best - ln Z): positive
        # wherever f32 can hold it (under the zero tables at 150 x 150 it is e^-137, below the smallest f32:
        # there 0 is the correctly rounded value)
        floor = np.exp(np.float64(f.best_score) - np.float64(f.log_z))
        assert f.pairs() and all(P[i, j] >= 0.0 for i, j in f.pairs())
        if floor >= 2.0 ** -120:
            assert all(P[i, j] >= floor * (1.0 - 1e-4) for i, j in f.pairs())


def same(x, y):
    return (np.float32(x.log_z).tobytes() == np.float32(y.log_z).tobytes() and
            np.float32(x.best_score).tobytes() == np.float32(y.best_score).tobytes() and
            x.structure == y.structure and np.array_equal(x.bound_a, y.bound_a) and
            np.array_equal(x.bound_b, y.bound_b) and
            (x.probs is None or y.probs is None or np.array_equal(x.probs, y.probs)))


def first_canonical(a, b):
    """the first cell in row-major order whose bases can pair"""
    return min((i, j) for i in range(len(a)) for j in range(len(b)) if R.canonical(int(a[i]), int(b[j])))


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("tab", TABS)
def test_schedule_independence(tables, tab, contra):
    """the same pairs alone, inside a shuffled batch of 40, every pair its own chunk, through the pool,
    and without the matrices: identical bits.  Alone and as chunks of their own, 22 x 300 steps along A
    and 300 x 22 along B; in the batch both step along A.  Under the zero tables every duplex weighs 1,
    every candidate of the traceback ties, and the structure must be the tie rule's pick whatever the
    schedule: the single pair at the first canonical cell."""
    from rna_algos_amd import _lib
    from rna_algos_amd.duplex import _duplex_batch
    from rna_algos_amd.mccaskill_algo import Context, Pool
    rng = np.random.default_rng(7)
    # every pair has between 3 301 and 6 600 cells: no two of them fit the chunk budget set below
    probes = [(O.splitmix_seq(22, 31), O.splitmix_seq(300, 32)), (O.splitmix_seq(300, 33), O.splitmix_seq(22, 34)),
              (O.splitmix_seq(58, 35), O.splitmix_seq(60, 36)), (O.splitmix_seq(80, 37), O.splitmix_seq(45, 38))]
    ctx = Context(tables[tab], device=0)
    try:
        alone = [fold(ctx, [a, b], [(0, 1)], contra)[0] for a, b in probes]
        assert all(np.isfinite(f.log_z) for f in alone)
        # a shuffled batch of 40 pairs holding the probes
        seqs, pairs = [], []
        for a, b in probes:
            seqs += [a, b]
            pairs.append((len(seqs) - 2, len(seqs) - 1))
        while len(pairs) < 40:
            seqs += [O.splitmix_seq(int(rng.integers(58, 81)), 100 + len(seqs)),
                     O.splitmix_seq(int(rng.integers(58, 81)), 200 + len(seqs))]
            pairs.append((len(seqs) - 2, len(seqs) - 1))
        cells = [len(seqs[a]) * len(seqs[b]) for a, b in pairs]
        assert max(cells) == 6600 and 2 * min(cells) > 6600
        order = rng.permutation(len(pairs))
        shuffled = [pairs[x] for x in order]
        where = {int(x): pos for pos, x in enumerate(order)}
        batch = fold(ctx, seqs, shuffled, contra)
        for x, f in enumerate(alone):
            assert same(f, batch[where[x]]), ("batch", x)
        if tab == "zero":
            for (a, b), f in zip(shuffled, batch):
                assert f.pairs() == [first_canonical(seqs[a], seqs[b])] and f.best_score == 0.0
        # no matrix leaves the device: the other outputs keep their bits
        lean = fold(ctx, seqs, shuffled, contra, want_probs=False)
        assert all(f.probs is None for f in lean)
        assert all(same(f, g) for f, g in zip(batch, lean))
        # 4 bytes hold no pair: refused with RNAMC_ERR_OOM before any launch
        ctx.set("group_ws_bytes", 4)
        with pytest.raises(_lib.RnamcError) as e:
            fold(ctx, seqs, shuffled, contra)
        assert e.value.status == _lib.ERR_OOM and "group_ws_bytes" in str(e.value)
        # the lowest setting the call accepts: exactly the matrices of the largest pair (F and G in f64,
        # the max-plus matrix in f32: five floats a cell, and one of padding).  Any two pairs of the batch
        # are more than that: every pair is its own chunk, with its own stepping direction.
        ctx.set("group_ws_bytes", 4 * (5 * 6600 + 1))
        chunked = fold(ctx, seqs, shuffled, contra)
        ctx.set("group_ws_bytes", 64 << 30)
        assert all(same(f, g) for f, g in zip(batch, chunked))
        # every visible device
        pool = Pool(tables[tab])
        try:
            multi = _duplex_batch(_lib.lib().rnamc_duplex_batch_multi, pool._h, seqs, shuffled, contra)
        finally:
            pool.close()
        assert all(same(f, g) for f, g in zip(batch, multi))
    finally:
        ctx.close()


@pytest.mark.parametrize("tab", TABS)
def test_existing_entries_unaffected(tables, trnas, tab):
    """rnamc_bpp_batch before, between and after duplex calls on ONE context (the workspace is shared):
    the bits of a fresh context"""
    from rna_algos_amd.mccaskill_algo import Context
    seqs = [s for _, s in trnas]
    fresh = Context(tables[tab], device=0)
    try:
        want, want_z = fresh.bpp_batch(seqs, False, False)
    finally:
        fresh.close()
    ctx = Context(tables[tab], device=0)
    try:
        a, b = O.splitmix_seq(40, 5), O.splitmix_seq(120, 6)
        runs = [ctx.bpp_batch(seqs, False, False)]
        first = fold(ctx, [a, b], [(0, 1)], False)[0]
        runs.append(ctx.bpp_batch(seqs, False, False))
        again = fold(ctx, [a, b], [(0, 1)], False)[0]
        third = fold(ctx, [b, a], [(0, 1)], True)[0]
        runs.append(ctx.bpp_batch(seqs, False, False))
        assert same(first, again) and np.isfinite(third.log_z)
        for mats, logz in runs:
            assert np.array_equal(logz, want_z)
            assert all(np.array_equal(m.packed, w.packed) for m, w in zip(mats, want))
    finally:
        ctx.close()


def test_python_mirror_and_cli(params, tmp_path, monkeypatch):
    """the CLI end to end on the FASTA fixtures; its lines parsed back equal duplex_fold_batch's results,
    and duplex_scan / duplex_fold agree with the batch"""
    from rna_algos_amd import utils
    from rna_algos_amd.bin import duplex_fold as cli
    from rna_algos_amd.duplex import duplex_fold, duplex_fold_batch, duplex_scan
    monkeypatch.setattr(utils, "_default", utils._default)  # the CLI names its tables: put them back afterwards
    qf = os.path.join(ROOT, "tests", "golden", "duplex_queries.fa")
    tf = os.path.join(ROOT, "tests", "golden", "duplex_targets.fa")
    for contra in (False, True):
        out, pdir = tmp_path / f"out{int(contra)}.tsv", tmp_path / f"probs{int(contra)}"
        argv = ["-q", qf, "-t", tf, "-o", str(out), "--probs", str(pdir), "--synthetic-tables", "1"]
        assert cli.main(argv + (["-c"] if contra else [])) == 0
        queries, targets = utils.read_fasta(qf), utils.read_fasta(tf)
        tables = utils.FoldScoreSets.new(0.0)
        tables.transfer(utils.FoldScoreSets.synthetic(1))
        seqs = [s for _, s in queries] + [s for _, s in targets]
        pairs = [(q, len(queries) + t) for q in range(len(queries)) for t in range(len(targets))]
        folds = duplex_fold_batch(seqs, pairs, contra, tables)
        rows = [cli.parse_line(ln) for ln in out.read_text().splitlines()]
        assert len(rows) == len(pairs) == 12
        for (q, t), f, row in zip(pairs, folds, rows):
            t -= len(queries)
            chain = f.pairs()
            assert row[:2] == (queries[q][0], targets[t][0])
            assert np.float32(row[2]) == np.float32(f.log_z) and np.float32(row[3]) == np.float32(f.best_score)
            assert row[4:6] == (chain[0] if chain else (-1, -1)) and row[6] == f.structure
            assert np.array_equal(np.load(pdir / f"{q}_{t}.npy"), f.probs)
        scan = duplex_scan(queries[0][1], [s for _, s in targets], contra, tables)
        assert len(scan) == 4 and scan.folds[0].probs is None
        assert [np.float32(f.log_z) for f in scan.folds] == [np.float32(f.log_z) for f in folds[:4]]
        top = scan.top(2)
        assert top[0][0] == int(np.argmax([f.log_z for f in folds[:4]])) and top[0][1].log_z >= top[1][1].log_z
        one = duplex_fold(queries[0][1], targets[0][1], contra, tables)
        assert one.structure == folds[0].structure and np.array_equal(one.probs, folds[0].probs)
