"""Tree-order summation (summation_mode 1) on helix-rich inputs, every form of the sweep against the
f64 evaluation of the recurrences (oracle/mccaskill_exact.c).

The inputs (tests/helix_inputs.py; their conditions are pinned on the CPU by
test_tree_helices_cpu.py) drive sums_1ormore_basepairs through 170 nats (strong tables) / 132 nats
(mild tables) inside one aligned chunk of 32 k — the unit over which the matrix-core mid-field
(k_tree_mid_mx, rnamc_tree_mx.h) shares one power-of-two scale per operand row.  Random sequences,
which every other tree-order test folds, reach 33-62.  Along the G-run that two helices share, one
operand rises and the other falls by a stack score per k, so the terms that carry the multiloop sit
far below BOTH operands' chunk maxima: a scale per chunk alone lets them underflow in f32.  Measured
with the strong tables, Turner model, before the kernel learnt to notice and redo such tiles in its
exact form: max |dp| 0.34 - 0.60 and |d ln Z| 1.0 - 1.4 in every matrix-core form (131.6 "expected
pairs" in a helix that holds 33.8), 6.4e-4 and 5.8e-4 in the VALU forms; since then 6.4e-4 - 6.9e-4 and
5.8e-4 in all of them (DESIGN.md section 4c has the table).

Bounds (none of them derived from a form with a mid-field):
  |d ln Z| <= 2e-5 + 3e-6 |ln Z|                                   (test_gpu_tree.py)
  max |dp| <= max(2e-5 + 2e-7 n, 16 ulp_f32(|ln Z|))               (test_gpu_tree.py, both terms:
      ln Z reaches 384 at n = 207 and 1070 at n = 430 under the strong tables — one f32 ulp of it is
      3e-5 / 1.2e-4, and a probability is the exp of a difference of such values)
  banded form against the unbanded control: 2 x that bound         (test_tree_banded_mid_field)
  expected pairs of either helix of a split-run input: 0.05 of the exact count.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helix_inputs as H
import oracle_lib as O

pytestmark = pytest.mark.gpu

TABLES = ("strong", "mild")
MODELS = (False, True)  # uses_contra_model
DEFAULTS = {"tree_band": 64, "tree_lane": 1, "tree_mid_mx": 1}


@pytest.fixture(scope="module")
def tables(built):
    return {"strong": H.strong_tables(), "mild": H.mild_tables()}


@pytest.fixture(scope="module")
def contexts(tables):
    from rna_algos_amd.mccaskill_algo import Context
    cs = {k: Context(v, device=0) for k, v in tables.items()}
    yield cs
    for c in cs.values():
        c.set("summation_mode", 0)
        c.close()


@pytest.fixture(scope="module")
def exact(tables):
    """{(tables, contra, name): (packed f64 probabilities, ln Z)} — computed once, never modified"""
    jobs = [(t, contra, name, s) for t in TABLES for contra in MODELS for name, s in H.family()]
    with ThreadPoolExecutor(max_workers=8) as ex:
        res = list(ex.map(lambda j: O.exact_bpp(tables[j[0]].ptr, j[3], j[1]), jobs))
    for xb, _ in res:
        xb.setflags(write=False)
    return {(t, contra, name): r for (t, contra, name, _), r in zip(jobs, res)}


def run(ctx, seqs, contra, mode, **knobs):
    ctx.set("summation_mode", mode)
    for k, v in knobs.items():
        ctx.set(k, v)
    try:
        return ctx.bpp_batch(seqs, contra, False)
    finally:
        ctx.set("summation_mode", 0)
        for k in knobs:
            ctx.set(k, DEFAULTS[k])


def deviation(a, b):
    """-> (key sets equal, max |a - b| over the pairs both hold)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ka, kb = a >= -0.5, b >= -0.5
    both = ka & kb
    return bool(np.array_equal(ka, kb)), float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def bound_p(n, lnz):
    return max(2e-5 + 2e-7 * n, 16.0 * float(np.spacing(np.float32(abs(lnz)))))


def bound_z(lnz):
    return 2e-5 + 3e-6 * abs(lnz)


def check_against_exact(form, names, seqs, mats, logz, exact, key, problems):
    """the per-form assertions against f64; -> (worst |dp|, worst |d ln Z|, worst |dp| / bound)"""
    worst_p = worst_z = worst_rel = 0.0
    for name, s, m, z in zip(names, seqs, mats, logz):
        xb, xz = exact[key + (name,)]
        same, dp = deviation(m.packed, xb)
        dz = abs(float(z) - xz)
        bp = bound_p(len(s), xz)
        worst_p, worst_z, worst_rel = max(worst_p, dp), max(worst_z, dz), max(worst_rel, dp / bp)
        if not same:
            problems.append(f"{form} {name}: key set differs from the exact one")
        if not dp <= bp:
            problems.append(f"{form} {name}: |dp| = {dp:.3e} > {bp:.3e}")
        if not dz <= bound_z(xz):
            problems.append(f"{form} {name}: |d ln Z| = {dz:.3e} > {bound_z(xz):.3e} (ln Z = {xz:.3f})")
        if name.startswith("split_a"):
            a = int(name[len("split_a"):])
            g1, g2, gc = H.split_run_pair_counts(m.packed, a)
            x1, x2, xc = H.split_run_pair_counts(xb, a)
            if not (abs(g1 - x1) <= 0.05 and abs(g2 - x2) <= 0.05):
                problems.append(f"{form} {name}: expected pairs of the helices {g1:.3f} / {g2:.3f}, "
                                f"exact {x1:.3f} / {x2:.3f}")
            if not abs(gc - xc) <= bp:
                problems.append(f"{form} {name}: closing pair p = {gc:.6f}, exact {xc:.6f}")
    return worst_p, worst_z, worst_rel


def check_against_control(form, names, seqs, mats, control, exact, key, problems):
    for name, s, m, c in zip(names, seqs, mats, control):
        same, dp = deviation(m.packed, c.packed)
        bp = 2.0 * bound_p(len(s), exact[key + (name,)][1])
        if not (same and dp <= bp):
            problems.append(f"{form} {name}: against the unbanded control keys equal = {same}, |dp| = {dp:.3e} > {bp:.3e}")


def same_bits(ma, za, mb, zb):
    return all(np.array_equal(np.asarray(a.packed), np.asarray(b.packed)) for a, b in zip(ma, mb)) and \
        np.array_equal(np.asarray(za), np.asarray(zb))


# (form, knobs): the wave-per-cell launches of a group with the matrix-core mid-field
# (k_tree_mid_mx<4>: the family's 15 sequences stay far below 4 096 tiles a launch) and with the VALU
# mid-field (k_tree_mid), at both band widths; the batch form (lane per cell, band 32, the mid-field
# in front of every band from band 1 on)
BANDED_FORMS = [
    ("wave band64 mx", dict(tree_lane=0, tree_band=64)),
    ("wave band32 mx", dict(tree_lane=0, tree_band=32)),
    ("wave band64 valu", dict(tree_lane=0, tree_band=64, tree_mid_mx=0)),
    ("wave band32 valu", dict(tree_lane=0, tree_band=32, tree_mid_mx=0)),
    ("lane batch mx", dict(tree_lane=2)),
    ("lane batch valu", dict(tree_lane=2, tree_mid_mx=0)),
]


@pytest.mark.parametrize("contra", MODELS)
@pytest.mark.parametrize("tab", TABLES)
def test_every_form_against_exact_f64(contexts, exact, tab, contra):
    """Pins k_tree_mid_mx<4> (group and lone calls), k_tree_mid and the lane-per-cell batch form with
    either mid-field, against the unbanded sweep (no mid-field kernel: the control) and against f64,
    on the whole family: chunk spread 170 nats (strong tables) / 132 (mild) for the run inputs, 88 /
    54 for (GC)^120, 55-62 / 31-34 for the SplitMix controls.  Split-run inputs additionally: the
    expected pair count of each helix and the closing pair.  Each form twice: bit-identical."""
    ctx, key = contexts[tab], (tab, contra)
    names = [n for n, _ in H.family()]
    seqs = [s for _, s in H.family()]
    problems = []
    control, zc = run(ctx, seqs, contra, 1, tree_lane=0, tree_band=0)
    wp, wz, wr = check_against_exact("control", names, seqs, control, zc, exact, key, problems)
    print(f"{tab} contra={contra} control (unbanded): worst |dp| = {wp:.3e} ({wr:.2f} x bound), |d ln Z| = {wz:.3e}")
    for form, knobs in BANDED_FORMS:
        m, z = run(ctx, seqs, contra, 1, **knobs)
        wp, wz, wr = check_against_exact(form, names, seqs, m, z, exact, key, problems)
        print(f"{tab} contra={contra} {form}: worst |dp| = {wp:.3e} ({wr:.2f} x bound), |d ln Z| = {wz:.3e}")
        check_against_control(form, names, seqs, m, control, exact, key, problems)
        m2, z2 = run(ctx, seqs, contra, 1, **knobs)
        if not same_bits(m, z, m2, z2):
            problems.append(f"{form}: a repeat of the call is not bit-identical")
    # default knobs, every sequence alone: the wave-per-cell chain with k_tree_mid_mx<4> a band ahead on
    # the side stream
    lone = [run(ctx, [s], contra, 1) for s in seqs]
    m, z = [r[0][0] for r in lone], [r[1][0] for r in lone]
    wp, wz, wr = check_against_exact("lone default", names, seqs, m, z, exact, key, problems)
    print(f"{tab} contra={contra} lone default: worst |dp| = {wp:.3e} ({wr:.2f} x bound), |d ln Z| = {wz:.3e}")
    check_against_control("lone default", names, seqs, m, control, exact, key, problems)
    again = run(ctx, [seqs[0]], contra, 1)
    if not same_bits([m[0]], [z[0]], again[0], [again[1][0]]):
        problems.append("lone default: a repeat of the call is not bit-identical")
    assert not problems, "\n".join(problems)


BIG = ("split_a10", "split_a26", "split_a27", "split_a28", "core_a10", "core_a26", "hairpins_60x2", "gc_120")
COPIES = 64


@pytest.mark.parametrize("contra", MODELS)
@pytest.mark.parametrize("tab", TABLES)
def test_large_batch_tile_per_wave(contexts, exact, tab, contra):
    """Pins k_tree_mid_mx<1> (a tile per wave; chosen when tiles x sequences of a launch >= 4 096): 8
    inputs x 64 copies, n <= 248, default knobs — 118 000 nt, so the call takes the batch form at band
    32.  Chunk spread of the inputs as above (170 / 132 nats; (GC)^120 88 / 54).  Copies of one sequence
    agree bit for bit; every distinct result within the bounds against f64."""
    ctx, key = contexts[tab], (tab, contra)
    fam = dict(H.family())
    seqs = [fam[name] for _ in range(COPIES) for name in BIG]  # interleaved: copies land in different places
    assert max(len(s) for s in seqs) <= 260 and sum(len(s) for s in seqs) >= 65536
    # the launch rule of launch_tree_mid_mx (the stats do not say which form ran): 32-row blocks x 2
    # column tiles (x 2 products outside) x the sequences longer than the band's first diagonal.  Inside,
    # bands 1 .. 4 (d = 32 .. 159: the pairs of both helices) take the tile-per-wave form; outside, every
    # band up to band 6 (d = 192 .. 223: the closing stacks of the split-run inputs).
    gmax = max(len(s) for s in seqs)
    tiles = lambda dlo, outside: ((gmax - dlo + 31) // 32) * 2 * (2 if outside else 1) * sum(len(s) > dlo for s in seqs)
    assert all(tiles(32 * x, False) >= 4096 for x in range(1, 5))
    assert all(tiles(32 * x, True) >= 4096 for x in range(1, 7))
    m, z = run(ctx, seqs, contra, 1)
    problems = []
    for x, name in enumerate(BIG):
        for c in range(1, COPIES):
            y = c * len(BIG) + x
            if not (np.array_equal(np.asarray(m[x].packed), np.asarray(m[y].packed)) and z[x] == z[y]):
                problems.append(f"{name}: copy {c} differs from copy 0")
                break
    first = len(BIG)
    wp, wz, wr = check_against_exact("big batch", BIG, seqs[:first], m[:first], z[:first], exact, key, problems)
    print(f"{tab} contra={contra} 512-sequence batch: worst |dp| = {wp:.3e} ({wr:.2f} x bound), |d ln Z| = {wz:.3e}")
    control, _ = run(ctx, seqs[:first], contra, 1, tree_lane=0, tree_band=0)
    check_against_control("big batch", BIG, seqs[:first], m[:first], control, exact, key, problems)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("contra", MODELS)
@pytest.mark.parametrize("tab", TABLES)
def test_reference_order_parity_on_helices(contexts, tables, tab, contra):
    """The parity gate (summation_mode 0, the reference-order kernels of rnamc_kernels.hip) on the same
    inputs and tables: bit-identical to the CPU oracle — no low-complexity test ran it with stacks of
    5.5 nats and chunk spreads of 170 nats before."""
    ctx = contexts[tab]
    seqs = [s for _, s in H.family()]
    ref, refz = O.bpp_batch(tables[tab].ptr, seqs, contra, False, n_threads=8)
    m, z = run(ctx, seqs, contra, 0)
    for (name, s), a, r, za, zr in zip(H.family(), m, ref, z, refz):
        neg = r < 0
        assert np.array_equal(np.asarray(a.packed)[~neg], r[~neg]), name
        assert np.array_equal(np.asarray(a.packed) < -0.5, r < -0.5), name
        assert np.float32(za) == np.float32(zr), name


def test_sparse_entry_inherits_the_sweep(tables):
    """A downstream entry on a split-run input (chunk spread 170 nats, strong tables; whatever
    mid-field form the pool's call takes): mccaskill_algo_batch_sparse at 0.01 in tree order lists
    exactly the pairs of the dense result of the same call path with p >= 0.01, with their bits."""
    from rna_algos_amd import mccaskill_algo as M
    p = tables["strong"]
    s = H.split_run(26)
    pool = M._pool_for(p)
    pool.set("summation_mode", 1)
    try:
        sp, zs = M.mccaskill_algo_batch_sparse([s], False, False, p, 0.01)
        de, zd = M.mccaskill_algo_batch([s], False, False, p)
    finally:
        pool.set("summation_mode", 0)
    packed = np.asarray(de[0].packed)
    idx = np.nonzero((packed > -0.5) & (packed >= np.float32(0.01)))[0]
    n = len(s)
    starts = np.array([d * n - d * (d - 1) // 2 for d in range(n + 1)], dtype=np.int64)
    d = np.searchsorted(starts, idx, side="right") - 1
    i = idx - starts[d]
    assert len(idx) > 50  # both helices and the closing stack are listed
    assert np.array_equal(sp[0].i, i.astype(np.uint32)) and np.array_equal(sp[0].j, (i + d).astype(np.uint32))
    assert np.array_equal(np.asarray(sp[0].p).view(np.uint32), packed[idx].view(np.uint32))
    assert np.float32(zs[0]) == np.float32(zd[0])
