"""Tree-order summation mode (rnamc_ctx_set "summation_mode" 1, rna_algos_amd/csrc/rnamc_tree.hip)
through the C ABI.

This mode cannot be bit-compared with the reference: its logsumexp is an order-dependent,
approximate left fold (src/utils.rs:579-627).  What is asserted instead:
  * against the f64 evaluation of the SAME recurrences (oracle/mccaskill_exact.c, exact
    logsumexp) and against the exhaustive f64 enumeration (oracle/bruteforce.c): identical key
    sets, |dp| and |d ln Z| within the f32 rounding of an order-free sum (bounds below) — the
    mode is one to two orders of magnitude CLOSER to the exact value than the reference's own
    arithmetic is, which the tests also assert;
  * against the reference-order mode of the same library (the parity gate): identical key sets,
    max |dp| and |d ln Z| printed and bounded by the reference's own distance from the exact
    value (measured: DESIGN.md section 4b);
  * determinism run to run, every kernel variant against the others, ragged batches, edge cases.
"""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

VARIANTS = [(False, False), (True, False), (True, True)]


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.set("summation_mode", 0)
    c.close()


def run(ctx, seqs, contra, short, mode, **knobs):
    ctx.set("summation_mode", mode)
    for k, v in knobs.items():
        ctx.set(k, v)
    try:
        return ctx.bpp_batch(seqs, contra, short)
    finally:
        ctx.set("summation_mode", 0)
        for k in knobs:
            ctx.set(k, {"tree_two": 1, "tree_tpc": 0, "tree_band": 64, "tree_ahead": 1, "tree_lane": 1,
                        "tree_mid_sync": 1, "tree_mid_mx": 1, "tree_gen_batch": 3, "tree_lane_band": 32, "tree_dual": 1}[k])


def deviation(a, b):
    """-> (key sets equal, max |a - b| over the pairs both hold)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ka, kb = a >= -0.5, b >= -0.5
    both = ka & kb
    return bool(np.array_equal(ka, kb)), float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def bpp_bound(n):
    """|dp| against the f64 evaluation: the f32 rounding of an order-free sum, which grows with the magnitude
    of ln Z (~ n)"""
    return 2e-5 + 2e-7 * n


def logz_bound(exact_logz):
    """|d ln Z| against the f64 evaluation"""
    return 2e-5 + 3e-6 * abs(exact_logz)


def lengths_mix():
    return [O.splitmix_seq(n, 100 + n) for n in (1, 2, 3, 4, 5, 6, 7, 9, 12, 17, 21, 33, 47, 64, 65,
                                                 100, 129, 200, 257, 300)]


@pytest.mark.parametrize("contra,short", VARIANTS)
def test_tree_vs_exact_f64(ctx, params, trnas, contra, short):
    seqs = [r[1] for r in trnas] + lengths_mix()
    mt, zt = run(ctx, seqs, contra, short, 1)
    mr, zr = run(ctx, seqs, contra, short, 0)
    worst_t = worst_r = worst_z = 0.0
    for s, a, r, za, zb in zip(seqs, mt, mr, zt, zr):
        xb, xz = O.exact_bpp(params.ptr, s, contra, short)
        same, dt = deviation(a.packed, xb)
        assert same, f"n={len(s)}: key set differs from the exact evaluation"
        _, dr = deviation(r.packed, xb)
        assert dt <= bpp_bound(len(s)), f"n={len(s)}: |dp| = {dt:.3e} against the f64 evaluation"
        assert abs(float(za) - xz) <= logz_bound(xz), f"n={len(s)}: ln Z {float(za)} vs {xz}"
        worst_t, worst_r, worst_z = max(worst_t, dt), max(worst_r, dr), max(worst_z, abs(float(za) - xz))
    print(f"contra={contra} short={short}: max |dp| tree {worst_t:.2e}, reference-order {worst_r:.2e}; "
          f"max |d ln Z| tree {worst_z:.2e}")
    assert worst_t < worst_r, "tree-order mode should sit closer to the exact value than the reference fold"


@pytest.mark.parametrize("contra,short", VARIANTS)
def test_tree_vs_bruteforce(ctx, params, contra, short):
    # the oracle's own bound against the enumeration is 2e-3 (approximate logsumexp); the
    # tree-order mode has no such approximation
    for n, seed in [(8, 1), (11, 2), (14, 3), (16, 4), (18, 5), (19, 6), (21, 7)]:
        if short and n > 19:
            continue  # (enumeration time)
        s = O.splitmix_seq(n, seed)
        ez, full, cnt = O.bruteforce(params.ptr, s, contra, short)
        m, z = run(ctx, [s], contra, short, 1)
        assert abs(float(z[0]) - ez) <= 1e-5 * max(1.0, abs(ez))
        d = m[0].dense().astype(np.float64)
        for i in range(n):
            for j in range(i, n):
                if full[i, j] > 0:
                    assert d[i, j] >= 0 and abs(d[i, j] - full[i, j]) <= 2e-6, (n, i, j, d[i, j], full[i, j])
                else:
                    assert d[i, j] < -0.5 or d[i, j] <= 1e-30


@pytest.mark.parametrize("contra", [False, True])
def test_tree_vs_reference_order_keys_and_deviation(ctx, params, trnas, contra):
    """tRNAs and n = 1024: key sets identical to the parity gate's; the deviation is the
    reference fold's own error (the tree-order result sits next to the exact value)."""
    seqs = [r[1] for r in trnas] + [O.splitmix_seq(1024, 1024)]
    mt, zt = run(ctx, seqs, contra, False, 1)
    mr, zr = run(ctx, seqs, contra, False, 0)
    for s, a, r, za, zb in zip(seqs, mt, mr, zt, zr):
        same, dp = deviation(a.packed, r.packed)
        assert same
        dz = abs(float(za) - float(zb))
        print(f"contra={contra} n={len(s)}: tree vs reference-order max |dp| = {dp:.3e}, |d ln Z| = {dz:.3e}")
        # measured: 1e-3 (tRNAs), 1.2e-2 / 1.7e-3 (n = 1024 CONTRAfold / Turner); bound with margin
        assert dp <= (2e-3 if len(s) < 200 else 3e-2)
        assert dz <= (3e-3 if len(s) < 200 else 4e-2)
        p = np.asarray(a.packed)
        pres = p[p >= -0.5]
        assert pres.min() >= -0.001 and pres.max() < 1.001  # the reference's own assertion


def load_exact(name):
    """f64 fixture of tests/make_golden.py `exact` (oracle/mccaskill_exact.c): ln Z, the probability of
    every 97th present pair (packed diagonal-major index), the sha256 of the key set."""
    import hashlib
    import os
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    return f, hashlib


EXACT_FIXTURES = ["exact_n1024_seed1024_contra", "exact_n1024_seed1024_turner", "exact_n2048_seed2048_turner",
                  "exact_n4096_seed4096_turner"]


@pytest.mark.parametrize("name", EXACT_FIXTURES)
def test_tree_vs_committed_exact_f64(ctx, params, name):
    """The tree-order mode pinned AT SCALE (round-3 verdict, missing 4): n = 1024 both models, n = 2048
    and n = 4096 Turner against committed f64 evaluations of the recurrences — many bands of the
    banded sweep, ring wrap-arounds at depth, every kernel of the mode.  Key set equal; up to
    n = 1024 the bounds of test_tree_vs_exact_f64 (|dp| <= 2e-5 + 2e-7 n, |d ln Z| <= 2e-5 + 3e-6 |ln Z|).
    Beyond, what bounds an f32 log-domain DP is the resolution of its values, not the summation
    order: ln Z = 1431 (n = 2048) / 2957 (n = 4096) carry ulps of 1.2e-4 / 2.4e-4, and a probability
    is the exp of a difference of such values — measured 7.2e-4 / 8.3e-4 at n = 2048; the bound is
    16 ulps of ln Z for both, and the reference-order result of the same library must sit FURTHER
    from the exact value (it does, by an order of magnitude: its fold is approximate on top).
    Each fixture is folded as a LONE sequence: the wave-per-cell chain of rnamc_tree.hip, not the batch
    form, which test_gpu_tree_batch_scale.py holds to the same fixtures."""
    import os
    if not os.path.exists(os.path.join(os.path.dirname(__file__), "golden", name + ".npz")):
        pytest.skip(f"{name}.npz not generated (python tests/make_golden.py exact|exact4096)")
    f, hashlib = load_exact(name)
    n, seed, contra = int(f["n"][0]), int(f["seed"][0]), bool(f["contra"][0])
    s = O.splitmix_seq(n, seed)
    m, z = run(ctx, [s], contra, False, 1)
    p = np.asarray(m[0].packed)
    pres = np.flatnonzero(p >= -0.5)
    assert pres.size == int(f["present"][0])
    assert hashlib.sha256(pres.astype(np.uint32).tobytes()).digest() == bytes(f["keyset_sha256"]), "key set differs"
    dp = float(np.max(np.abs(p[f["index"]].astype(np.float64) - f["prob"])))
    dz = abs(float(z[0]) - float(f["log_partition"][0]))
    print(f"{name}: tree-order vs committed f64: max |dp| = {dp:.3e} over {f['index'].size} pairs, "
          f"|d ln Z| = {dz:.3e} (ln Z = {float(f['log_partition'][0]):.4f})")
    xz = float(f["log_partition"][0])
    ulp = float(np.spacing(np.float32(abs(xz))))
    if n <= 1024:
        assert dp <= 2e-5 + 2e-7 * n
        assert dz <= 2e-5 + 3e-6 * abs(xz)
    else:
        assert dp <= 16 * ulp and dz <= 16 * ulp, (dp, dz, ulp)
    mr, zr = run(ctx, [s], contra, False, 0)
    pr = np.asarray(mr[0].packed)
    dpr = float(np.max(np.abs(pr[f["index"]].astype(np.float64) - f["prob"])))
    dzr = abs(float(zr[0]) - xz)
    print(f"{name}: reference-order vs committed f64: max |dp| = {dpr:.3e}, |d ln Z| = {dzr:.3e}  (ulp of ln Z {ulp:.2e})")
    assert dp < dpr and dz < dzr, "tree-order mode should sit closer to the exact value than the reference fold"
    # sum over the sampled pairs as a second, aggregate check: what may be systematic is the error of
    # ln Z itself (every log-probability carries it with the same sign), nothing beyond it
    bias = abs(float(p[f["index"]].astype(np.float64).sum()) - float(f["prob"].sum()))
    assert bias <= (dz + 4 * ulp) * float(f["prob"].sum()) + 1e-5 * f["index"].size ** 0.5 + 1e-4, bias


def test_tree_n4096_turner(ctx, params):
    """BASELINE.json configs[2] in tree-order mode: key set of the parity gate, deviation
    printed and bounded, row sums, deterministic."""
    s = O.splitmix_seq(4096, 4096)
    mt, zt = run(ctx, [s], False, False, 1)
    mt2, zt2 = run(ctx, [s], False, False, 1)
    assert np.array_equal(mt[0].packed, mt2[0].packed) and zt[0] == zt2[0], "not deterministic"
    mr, zr = run(ctx, [s], False, False, 0)
    same, dp = deviation(mt[0].packed, mr[0].packed)
    dz = abs(float(zt[0]) - float(zr[0]))
    print(f"n=4096 Turner: tree vs reference-order max |dp| = {dp:.3e}, |d ln Z| = {dz:.3e} "
          f"(ln Z {float(zt[0]):.4f} vs {float(zr[0]):.4f})")
    assert same, "key sets differ"
    assert dp <= 3e-2 and dz <= 1e-1  # measured 6.6e-3 / 2.6e-2
    d = mt[0].dense().astype(np.float64)
    d[d < 0] = 0
    rows = d.sum(axis=1) + d.sum(axis=0)
    assert rows.max() <= 1.0 + 5e-3


def test_tree_n16384_banded_and_oom(params):
    """n = 16 384 (a sequence's 27 dense matrices: 29 GB, more than 2^32 floats): the banded sweep
    addresses its operands by a 64-bit base per matrix + 32-bit offsets inside it, sums_external's
    vectors are walked in global memory (they do not fit the LDS) — key set = every canonical pair of
    span >= 5 (Turner: static), probabilities in range, row sums <= 1, the banded sweep equal to the
    unbanded one to rounding, and several times faster.  n = 65 535 (what T = u16 admits) would
    need 464 GB: refused with RNAMC_ERR_OOM, and the context works afterwards."""
    import time
    import torch
    from rna_algos_amd import _lib
    from rna_algos_amd.mccaskill_algo import Context
    n = 16384
    s = O.splitmix_seq(n, n)
    dev = torch.device("cuda:0")
    b = torch.from_numpy(np.ascontiguousarray(s)).to(dev)
    off = np.array([0, n], dtype=np.uint64)
    oo = np.array([0, n * (n + 1) // 2], dtype=np.uint64)
    z = torch.empty(1, dtype=torch.float32, device=dev)
    c = Context(params, device=0)
    c.set("summation_mode", 1)
    outs, secs = {}, {}
    try:
        for band in (64, 0):
            c.set("tree_band", band)
            o = torch.empty(n * (n + 1) // 2, dtype=torch.float32, device=dev)
            for rep in range(2):  # (the first call allocates the 29-GB workspace)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c.bpp_batch_device(1, b.data_ptr(), off, False, False, o.data_ptr(), oo, z.data_ptr(), 0)
                torch.cuda.synchronize()
                secs[band] = time.perf_counter() - t0
            outs[band] = (o, float(z[0]))
        print(f"tree-order n={n}: banded {secs[64] * 1e3:.0f} ms, unbanded {secs[0] * 1e3:.0f} ms, ln Z {outs[64][1]:.3f}")
        ob, zb = outs[64]
        ou, zu = outs[0]
        kb, ku = ob >= -0.5, ou >= -0.5
        assert bool(torch.equal(kb, ku))
        assert float((ob[kb] - ou[kb]).abs().max()) <= 2 * (2e-5 + 2e-7 * n)
        assert abs(zb - zu) <= 3e-6 * abs(zu)
        assert secs[64] < 0.6 * secs[0]
        # key set: canonical pairs of span >= 5, diagonal-major
        st = torch.from_numpy(s.astype(np.int64)).to(dev)
        chk = 0
        for d in (0, 3, 4, 5, 100, 4095, 8192, 12000, n - 2, n - 1):
            seg = ob[d * n - d * (d - 1) // 2: d * n - d * (d - 1) // 2 + n - d]
            t = st[:n - d] + st[d:]
            want = ((t == 3) | (t == 5)) & (d >= 4)
            assert bool(torch.equal(seg >= -0.5, want)), d
            chk += int(want.sum())
        assert chk > 0
        pres = ob[kb]
        # (ln Z = 11 612: one f32 ulp is 9.8e-4, and a probability is the exp of a difference of such
        # values — the reference's own bound 1.001 does not survive f32 at this length in any order)
        ulp = float(np.spacing(np.float32(abs(zb))))
        assert float(pres.min()) >= -0.001 and float(pres.max()) < 1.0 + 16 * ulp
        # row sums on a slice of rows (dense unpacking of 16384^2 would take 1 GB: do it by diagonals)
        rows = torch.zeros(n, dtype=torch.float64, device=dev)
        p0 = torch.clamp(ob, min=0).double()
        for d in range(4, n):
            base = d * n - d * (d - 1) // 2
            seg = p0[base:base + n - d]
            rows[:n - d] += seg
            rows[d:] += seg
        assert float(rows.max()) <= 1.0 + 32 * ulp
        # 464 GB of workspace: refused, nothing broken
        del ob, ou, outs, p0
        torch.cuda.empty_cache()
        big = 65535
        sb = torch.zeros(big, dtype=torch.uint8, device=dev)
        obig = torch.empty(8, dtype=torch.float32, device=dev)  # (never written: the call fails before any launch)
        offb = np.array([0, big], dtype=np.uint64)
        oob = np.array([0, big * (big + 1) // 2], dtype=np.uint64)
        with pytest.raises(_lib.RnamcError) as ei:
            c.bpp_batch_device(1, sb.data_ptr(), offb, False, False, obig.data_ptr(), oob, z.data_ptr(), 0)
        assert ei.value.status == _lib.ERR_OOM
        m, zz = c.bpp_batch([O.splitmix_seq(300, 3)], False, False)
        assert np.isfinite(float(zz[0]))
    finally:
        c.set("summation_mode", 0)
        c.close()


@pytest.mark.parametrize("contra,short", VARIANTS)
def test_tree_kernel_variants_agree(ctx, params, contra, short):
    """one / two diagonals per launch, 64 / 128 / 256 / 1024 threads per cell: the same sums in other
    orders — equal to f32 rounding, and each within the bound against the exact evaluation."""
    seqs = [O.splitmix_seq(n, 7 * n) for n in (5, 6, 37, 150, 301, 410)]
    exact = [O.exact_bpp(params.ptr, s, contra, short) for s in seqs]
    base = None
    for two in (1, 0):
        for tpc in (0, 64, 128, 256, 1024):
            m, z = run(ctx, seqs, contra, short, 1, tree_two=two, tree_tpc=tpc)
            for s, a, za, (xb, xz) in zip(seqs, m, z, exact):
                same, dt = deviation(a.packed, xb)
                assert same and dt <= 2e-5 + 2e-7 * len(s), (two, tpc, len(s), dt)
                assert abs(float(za) - xz) <= 2e-5 + 3e-6 * abs(xz)
            if base is None:
                base = m
            else:
                for s, a, b0 in zip(seqs, m, base):
                    assert deviation(a.packed, b0.packed)[1] <= 2 * (2e-5 + 2e-7 * len(s))


@pytest.mark.parametrize("contra,short", VARIANTS)
def test_tree_banded_mid_field(ctx, params, contra, short):
    """Banded sweep (k_tree_mid sums the mid-field of the three cubic products one band ahead on a
    second stream, the launches add the edge) against the unbanded sweep of the same mode: the
    same terms in another grouping — equal to f32 rounding; lone sequences and a ragged group,
    band widths 32 and 64, lengths around the first banded diagonal (3 * band) and band ends."""
    lens = (95, 96, 97, 98, 127, 128, 129, 130, 191, 192, 193, 200, 257, 300, 383, 410, 640)
    seqs = [O.splitmix_seq(n, 13 * n + 5) for n in lens]
    base, zbase = run(ctx, seqs, contra, short, 1, tree_band=0)
    tol = lambda n: 2 * (2e-5 + 2e-7 * n)
    for band, ahead in ((32, 1), (64, 1), (64, 0)):
        # (tree_ahead: the far part of a launch's 2-loop blocks summed by the previous launch)
        m, z = run(ctx, seqs, contra, short, 1, tree_band=band, tree_ahead=ahead)
        for s, a, b0, za, zb in zip(seqs, m, base, z, zbase):
            same, dp = deviation(a.packed, b0.packed)
            assert same and dp <= tol(len(s)), (band, len(s), dp)
            assert abs(float(za) - float(zb)) <= 3e-6 * max(1.0, abs(float(zb))), (band, len(s))
        for x in (7, 13, 16):  # alone: other launch shapes (no ragged prefix)
            m1, z1 = run(ctx, [seqs[x]], contra, short, 1, tree_band=band)
            same, dp = deviation(m1[0].packed, base[x].packed)
            assert same and dp <= tol(len(seqs[x])), (band, len(seqs[x]), dp)
    # against the exact f64 evaluation too (the bound of test_tree_kernel_variants_agree)
    m, z = run(ctx, [seqs[15]], contra, short, 1, tree_band=32)
    xb, xz = O.exact_bpp(params.ptr, seqs[15], contra, short)
    same, dt = deviation(m[0].packed, xb)
    assert same and dt <= 2e-5 + 2e-7 * 410 and abs(float(z[0]) - xz) <= 2e-5 + 3e-6 * abs(xz)
    # deterministic run to run (fixed merge order of the eight waves of a tile)
    m2, z2 = run(ctx, [seqs[15]], contra, short, 1, tree_band=32)
    assert np.array_equal(np.asarray(m2[0].packed), np.asarray(m[0].packed))


def test_tree_ragged_batch_and_lone_calls(ctx, params):
    """a ragged group (sequences leave the sweep at different diagonals) against the same
    sequences one by one: the same sums, possibly paired into launches differently (the
    outside sweep pairs diagonals from the group's longest sequence down) — equal to rounding"""
    seqs = [O.splitmix_seq(n, 31 * n + 1) for n in (300, 299, 150, 77, 76, 5, 4, 3, 1, 222, 64)]
    for contra, short in VARIANTS:
        mb, zb = run(ctx, seqs, contra, short, 1, tree_tpc=256)
        for x, s in enumerate(seqs):
            m1, z1 = run(ctx, [s], contra, short, 1, tree_tpc=256)
            same, dp = deviation(m1[0].packed, mb[x].packed)
            # (in the group a sequence may be swept banded, with its 2-loop blocks' far parts formed
            # a launch ahead; alone, a short one is not: the same terms grouped differently)
            assert same and dp <= 2 * (2e-5 + 2e-7 * len(s)), (contra, short, len(s), dp)
            assert abs(float(z1[0]) - float(zb[x])) <= 1e-6 * max(1.0, abs(float(zb[x])))


@pytest.mark.parametrize("contra,short", VARIANTS)
def test_tree_lane_per_cell_batch(ctx, params, contra, short):
    """The batch form of the mode (rnamc_tree_lane.h: a lane per cell, diagonal-major operands, one
    diagonal per launch, bands spread into the row- / column-major copies of the mid-field kernels):
    a ragged batch, lengths 1 .. 900 around the band boundaries, against the f64 evaluation of the
    recurrences at those lengths (the mode's own bound; 1024 .. 4096 nt: test_gpu_tree_batch_scale.py)
    and against the wave-per-cell launches of the same mode (the
    same terms grouped differently: rounding); band 32, the mid-field kernels a band ahead on the side
    stream instead of in front of the band, and the VALU form of the mid-field products instead of the
    matrix-core form (rnamc_tree_mx.h) too."""
    lens = (900, 640, 410, 300, 257, 194, 193, 192, 129, 128, 127, 65, 64, 37, 5, 4, 2, 1)
    seqs = [O.splitmix_seq(n, 17 * n + 3) for n in lens]
    exact = [O.exact_bpp(params.ptr, s, contra, short) for s in seqs]
    base, zbase = run(ctx, seqs, contra, short, 1, tree_lane=0)
    first = None
    for knobs in ({"tree_lane": 2}, {"tree_lane": 2, "tree_band": 32}, {"tree_lane": 2, "tree_mid_sync": 0},
                  {"tree_lane": 2, "tree_mid_mx": 0}):
        m, z = run(ctx, seqs, contra, short, 1, **knobs)
        worst = 0.0
        for s, a, za, b0, zb, (xb, xz) in zip(seqs, m, z, base, zbase, exact):
            same, dt = deviation(a.packed, xb)
            _, dw = deviation(b0.packed, xb)
            # (the bound of the wave-per-cell launches, 2e-5 + 2e-7 n ~ 7 ulp of ln Z, with half as much
            # again: another grouping of the same f32 sums lands on either side of it — printed below)
            assert same and dt <= 1.5 * (2e-5 + 2e-7 * len(s)), (knobs, len(s), dt, dw)
            assert abs(float(za) - xz) <= 2e-5 + 3e-6 * abs(xz), (knobs, len(s))
            same, dp = deviation(a.packed, b0.packed)
            assert same and dp <= 2 * (2e-5 + 2e-7 * len(s)), (knobs, len(s), dp)
            worst = max(worst, dt / (2e-5 + 2e-7 * len(s)))
        print(f"contra={contra} short={short} {knobs}: worst |dp| against f64 = {worst:.2f} x (2e-5 + 2e-7 n)")
        if first is None:
            first = m
    # the same batch again: bit-identical (fixed merge orders), and the stats say which form ran
    m2, _ = run(ctx, seqs, contra, short, 1, tree_lane=2)
    for a, b0 in zip(m2, first):
        assert np.array_equal(np.asarray(a.packed), np.asarray(b0.packed))
    # one sequence of the batch alone in the batch form (other launch shapes, no ragged prefix)
    m1, z1 = run(ctx, [seqs[1]], contra, short, 1, tree_lane=2)
    same, dp = deviation(m1[0].packed, first[1].packed)
    assert same and dp <= 2 * (2e-5 + 2e-7 * len(seqs[1]))


@pytest.mark.parametrize("contra", [False, True])
def test_tree_batch_form_many_sequences(ctx, params, contra):
    """The batch form at the size where its other launch shapes apply: 160 ragged sequences (300 .. 700 nt) —
    a tile per wave in the matrix-core mid-field (k_tree_mid_mx<1>: at least 4 096 tiles a launch), the
    generic 2-loop sums three diagonals a launch (k_tlane_gen) against one diagonal a launch, 256 listed
    cells to a workgroup in the just-in-time role — against the wave-per-cell launches of the same mode
    (rounding) and, for the two shortest (300 nt or little more), against the f64 evaluation of the
    recurrences; the batch form against f64 at the benchmark's lengths: test_gpu_tree_batch_scale.py."""
    rng = np.random.default_rng(2026)
    lens = sorted((int(x) for x in rng.integers(300, 701, size=160)), reverse=True)
    seqs = [O.splitmix_seq(n, 31 * n + k) for k, n in enumerate(lens)]
    base, zbase = run(ctx, seqs, contra, False, 1, tree_lane=0)
    m, z = run(ctx, seqs, contra, False, 1)
    st = ctx.stats()
    m1, z1 = run(ctx, seqs, contra, False, 1, tree_gen_batch=1)
    worst = 0.0
    for s, a, a1, b0, za, zb in zip(seqs, m, m1, base, z, zbase):
        same, dp = deviation(a.packed, b0.packed)
        assert same and dp <= 2 * (2e-5 + 2e-7 * len(s)), (len(s), dp)
        assert abs(float(za) - float(zb)) <= 3e-6 * abs(float(zb)), (len(s), float(za), float(zb))
        # the same sums a diagonal at a time: the same terms in the same order within a cell
        assert np.array_equal(np.asarray(a.packed), np.asarray(a1.packed)), len(s)
        worst = max(worst, dp / (2e-5 + 2e-7 * len(s)))
    for k in (len(seqs) - 1, len(seqs) - 2):
        xb, xz = O.exact_bpp(params.ptr, seqs[k], contra, False)
        same, dt = deviation(m[k].packed, xb)
        assert same and dt <= 1.5 * (2e-5 + 2e-7 * len(seqs[k])), (len(seqs[k]), dt)
        assert abs(float(z[k]) - xz) <= 2e-5 + 3e-6 * abs(xz)
    print(f"contra={contra}: 160 sequences, batch form against wave-per-cell launches: worst |dp| = {worst:.2f} x "
          f"(2e-5 + 2e-7 n); launches inside / outside {st['launches_inside']} / {st['launches_outside']}")


@pytest.mark.parametrize("contra,short", VARIANTS)
def test_tree_batch_form_two_groups_side_by_side(ctx, params, contra, short):
    """Every other group of a batch-form call through the DEVICE-resident entry sweeps on a second stream with
    its own half of the workspace (tree_dual; the host-buffer entry stages group by group and keeps one
    stream): the same bits as one group after the other, whatever the number of groups (odd, even, a lone
    last one) — and the same again with the call repeated (the halves are reused across groups)."""
    import torch
    lens = (600, 555, 430, 410, 390, 300, 260, 257, 200, 150, 99, 64, 7)
    seqs = [O.splitmix_seq(n, 7 * n + 11) for n in lens]
    ln = np.array(lens, dtype=np.uint64)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(ln, out=off[1:])
    oo = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(ln * (ln + np.uint64(1)) // np.uint64(2), out=oo[1:])
    dev = torch.device("cuda:0")
    d_b = torch.from_numpy(np.concatenate(seqs)).to(dev)

    def call(dual):
        d_o = torch.full((int(oo[-1]),), -7.0, dtype=torch.float32, device=dev)
        d_z = torch.zeros(len(seqs), dtype=torch.float32, device=dev)
        ctx.set("summation_mode", 1)
        ctx.set("tree_lane", 2)
        ctx.set("tree_dual", dual)
        try:
            ctx.bpp_batch_device(len(seqs), d_b.data_ptr(), off, contra, short, d_o.data_ptr(), oo, d_z.data_ptr(), 0)
            torch.cuda.synchronize()
            groups = ctx.stats()["n_groups"]
        finally:
            ctx.set("summation_mode", 0)
            ctx.set("tree_lane", 1)
            ctx.set("tree_dual", 1)
        return d_o.cpu().numpy(), d_z.cpu().numpy(), groups

    host, zhost = run(ctx, seqs, contra, short, 1, tree_lane=2)
    for per_group in (2, 3, 5):
        ctx.set("group_max_seqs", per_group)
        try:
            one, z_one, g1 = call(0)
            two, z_two, g2 = call(1)
            again, z_again, _ = call(1)
        finally:
            ctx.set("group_max_seqs", 8192)
        assert g1 == g2 == -(-len(seqs) // per_group)
        assert np.array_equal(one, two) and np.array_equal(one, again)
        assert np.array_equal(z_one, z_two) and np.array_equal(z_one, z_again)
        assert not np.any(one == -7.0)
    # (and the host-buffer entry's result of the same batch in ONE group: other launch shapes, rounding)
    for x, m in enumerate(host):
        same, dp = deviation(one[int(oo[x]):int(oo[x + 1])], m.packed)
        assert same and dp <= 2 * (2e-5 + 2e-7 * lens[x])


def test_tree_edge_cases(ctx, params):
    a = np.zeros(40, dtype=np.uint8)  # homopolymer: nothing pairs
    for contra, short in VARIANTS:
        m, z = run(ctx, [a, a[:1], a[:4]], contra, short, 1)
        mr, zr = run(ctx, [a, a[:1], a[:4]], contra, short, 0)
        for x in range(3):
            assert np.all(np.asarray(m[x].packed) == -1.0)
            assert abs(float(z[x]) - float(zr[x])) <= 1e-4 * max(1.0, abs(float(zr[x])))
    from rna_algos_amd import _lib
    with pytest.raises(_lib.RnamcError):
        run(ctx, [np.zeros(0, dtype=np.uint8)], False, False, 1)


def test_mode_knob_and_fold_scores_unaffected(ctx, params, trnas):
    """rnamc_fold_scores always takes the reference-order sweep, whatever the mode says; an
    unknown mode value is refused."""
    from rna_algos_amd import _lib
    with pytest.raises(_lib.RnamcError):
        ctx.set("summation_mode", 2)
    s = trnas[0][1]
    ctx.set("summation_mode", 1)
    try:
        n, hp, mb, ac, tl = ctx.fold_scores_packed(s, False, False)
    finally:
        ctx.set("summation_mode", 0)
    rhp, rmb, rac, rtl = O.fold_scores(params.ptr, s, False, False)
    assert np.array_equal(np.isnan(mb), np.isnan(rmb)) and np.array_equal(tl, rtl)


def test_tree_side_stream_owns_a_queue(params):
    """The banded sweep's side stream (mid-field products, lowest priority) must own a hardware
    queue.  When it was created at the first tree-order call and that call followed a host-entry
    batch (own, high-priority and copy streams in use: the process's first low-priority queue came
    fourth or later), its 100-600-us kernels shared the queue of the sweep's 11-us launches on the
    caller's stream: n = 4096 took 157 ms instead of 49.5 ms, which is what bench.py's batch run
    reported (profiles/r03_tree_side_stream_order.txt).  rnamc_ctx_create makes the stream now.
    Checked here against the sweep WITHOUT a side stream (tree_band = 0), in the order that failed:
    host entry first, then the device-resident tree-order calls on the null stream.  Banded:
    18.5 ms, unbanded: 29 ms; with the late-created stream the banded sweep took 77 ms (test fails)."""
    import time
    import torch
    from rna_algos_amd.mccaskill_algo import Context
    rng = np.random.default_rng(31)
    batch = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(300, 600, 300)]
    n = 2048
    s = O.splitmix_seq(n, n)
    dev = torch.device("cuda:0")
    b = torch.from_numpy(np.ascontiguousarray(s)).to(dev)
    o = torch.empty(n * (n + 1) // 2, dtype=torch.float32, device=dev)
    z = torch.empty(1, dtype=torch.float32, device=dev)
    off = np.array([0, n], dtype=np.uint64)
    oo = np.array([0, n * (n + 1) // 2], dtype=np.uint64)
    c = Context(params, device=0)
    c.bpp_batch(batch, False, False)  # host entry first: H2D, two-kernel sweeps, drain thread, D2H

    def tree_ms(band):
        c.set("summation_mode", 1)
        c.set("tree_band", band)
        try:
            ms = []
            for r in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c.bpp_batch_device(1, b.data_ptr(), off, False, False, o.data_ptr(), oo, z.data_ptr(), 0)
                torch.cuda.synchronize()
                if r:  # (the first call allocates the workspace)
                    ms.append((time.perf_counter() - t0) * 1e3)
        finally:
            c.set("summation_mode", 0)
            c.set("tree_band", 64)
        return float(np.median(ms))

    banded = tree_ms(64)
    verdict = c.stats()["tree_side_stream"]
    unbanded = tree_ms(0)
    c.close()
    print(f"tree-order n={n} after a host-entry batch, device-resident entry: banded {banded:.1f} ms, "
          f"unbanded {unbanded:.1f} ms, side-stream probe {verdict}")
    # Round 4: the library PROBES whether its side stream runs beside the caller's stream (once per
    # context and stream) and sweeps unbanded when it does not, so the gate is the probe's verdict;
    # the wall-clock comparison (timing on a shared GPU) is reported, and only sanity-bounded.
    assert verdict == 1, "the side stream does not run beside the caller's stream on this box"
    assert banded < 2.0 * unbanded


def test_tree_side_stream_fallback(ctx, params):
    """what the library does when its probe says the side stream is serialised behind the caller's
    stream (forced here through the knob): the sweep runs unbanded — the same result to rounding —
    and the stats say so"""
    s = O.splitmix_seq(700, 77)
    base, zb = run(ctx, [s], False, False, 1)
    assert ctx.stats()["tree_side_stream"] == 1
    ctx.set("tree_side_stream", 2)
    try:
        m, z = run(ctx, [s], False, False, 1)
        assert ctx.stats()["tree_side_stream"] == 2
    finally:
        ctx.set("tree_side_stream", 0)
    same, dp = deviation(m[0].packed, base[0].packed)
    assert same and dp <= 2 * (2e-5 + 2e-7 * 700) and abs(float(z[0]) - float(zb[0])) <= 3e-6 * abs(float(zb[0]))
    m2, _ = run(ctx, [s], False, False, 1)  # probed again: banded
    assert ctx.stats()["tree_side_stream"] == 1 and np.array_equal(np.asarray(m2[0].packed), np.asarray(base[0].packed))
