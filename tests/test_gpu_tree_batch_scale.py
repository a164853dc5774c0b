"""The tree-order BATCH form (rnamc_tree_lane.h, rnamc_tree_mx.h, the lane_mode branch of
run_batch_tree) at the lengths it was built for: 1024 .. 4096 nt against the committed f64 fixtures
(tests/make_golden.py `exact`, `exact4096`, `exact_mid`), alone and among the benchmark's own records.

What runs only past the sizes of test_gpu_tree.py's batch-form tests (at most 900 nt) and is reached here:
k_tree_mid_mx<1> (a tile per wave) with k ranges of up to 64 chunks, both mid-field forms within one sweep,
scale exponents beyond 2^11, the event ring wrapping four times, partial tiles past 1024 (n = 1531 =
47 * 32 + 27), three groups of gigabytes side by side.

Bounds: the project's own (test_gpu_tree.py), nothing new —
  n <= 1024: |dp| <= 1.5 (2e-5 + 2e-7 n) (the batch-form bound of test_tree_lane_per_cell_batch),
             |d ln Z| <= 2e-5 + 3e-6 |ln Z|;
  n >  1024: 16 f32 ulps of ln Z for both (test_tree_vs_committed_exact_f64);
  one form against another of the same mode: twice the bound of one form against f64 — 2 (2e-5 + 2e-7 n)
  up to 1024 as in test_tree_batch_form_many_sequences, 32 ulps of ln Z beyond — and
  |d ln Z| <= 3e-6 |ln Z|;
  the batch form lies closer to the fixture than the reference-order result of the same record.
Every measured fraction of a bound is printed ("Benchmark lengths, pinned").
"""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_tree import EXACT_FIXTURES, bpp_bound, deviation, load_exact, logz_bound, run

pytestmark = pytest.mark.gpu

FIXTURES = ["exact_n1024_seed1024_contra", "exact_n1024_seed1024_turner", "exact_n1531_seed1531_contra",
            "exact_n1531_seed1531_turner", "exact_n2048_seed2048_contra_short", "exact_n2048_seed2048_turner",
            "exact_n4096_seed4096_turner"]
assert set(EXACT_FIXTURES) <= set(FIXTURES)
# (label, knobs on top of tree_lane = 2); the first two are all that n = 4096 runs
FORMS = [("default", {}), ("tree_mid_mx=0", {"tree_mid_mx": 0}), ("tree_lane_band=64", {"tree_lane_band": 64}),
         ("tree_mid_sync=0", {"tree_mid_sync": 0}), ("tree_gen_batch=1", {"tree_gen_batch": 1})]
MODELS = [("turner", False, False), ("contra", True, False), ("contra_short", True, True)]
BATCH_HEAD = 64  # the first records of the benchmark batch: 70 239 nt, lengths 256 .. 2034


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.set("summation_mode", 0)
    c.close()


class Fixture:
    def __init__(self, name):
        self.name = name
        self.f, self.hashlib = load_exact(name)
        f = self.f
        self.n, self.seed, self.contra = int(f["n"][0]), int(f["seed"][0]), bool(f["contra"][0])
        self.short = bool(f["short"][0]) if "short" in f.files else False  # (absent in the older files: 0)
        self.xz = float(f["log_partition"][0])
        self.ulp = float(np.spacing(np.float32(abs(self.xz))))
        self.seq = O.splitmix_seq(self.n, self.seed)

    def model(self):
        return self.contra, self.short


def dp_bound(n, xz):
    return 1.5 * bpp_bound(n) if n <= 1024 else 16 * float(np.spacing(np.float32(abs(xz))))


def dz_bound(n, xz):
    return logz_bound(xz) if n <= 1024 else 16 * float(np.spacing(np.float32(abs(xz))))


def form_bound(n, lnz):
    """one form of the mode against another, the same terms grouped differently"""
    return 2 * bpp_bound(n) if n <= 1024 else 32 * float(np.spacing(np.float32(abs(lnz))))


def against_fixture(fx, label, packed, z, ref_packed, ref_z):
    """The assertions of test_tree_vs_committed_exact_f64 on one result, by the bounds of the batch form;
    -> the measured fractions of the two bounds"""
    f = fx.f
    p = np.asarray(packed)
    pres = np.flatnonzero(p >= -0.5)
    assert pres.size == int(f["present"][0]), (fx.name, label)
    assert fx.hashlib.sha256(pres.astype(np.uint32).tobytes()).digest() == bytes(f["keyset_sha256"]), \
        f"{fx.name} {label}: key set differs"
    dp = float(np.max(np.abs(p[f["index"]].astype(np.float64) - f["prob"])))
    dz = abs(float(z) - fx.xz)
    bp, bz = dp_bound(fx.n, fx.xz), dz_bound(fx.n, fx.xz)
    pr = np.asarray(ref_packed)
    dpr = float(np.max(np.abs(pr[f["index"]].astype(np.float64) - f["prob"])))
    dzr = abs(float(ref_z) - fx.xz)
    print(f"{fx.name} [{label}]: |dp| = {dp:.3e} = {dp / bp:.3f} x bound, |d ln Z| = {dz:.3e} = {dz / bz:.3f} x bound "
          f"(reference-order {dpr:.3e} / {dzr:.3e})")
    assert dp <= bp, (fx.name, label, dp, bp)
    assert dz <= bz, (fx.name, label, dz, bz)
    assert dp < dpr and dz < dzr, (fx.name, label, "not closer to the exact value than the reference fold")
    # (the aggregate check of test_tree_vs_committed_exact_f64: nothing systematic beyond the error of ln Z)
    bias = abs(float(p[f["index"]].astype(np.float64).sum()) - float(f["prob"].sum()))
    assert bias <= (dz + 4 * fx.ulp) * float(f["prob"].sum()) + 1e-5 * f["index"].size ** 0.5 + 1e-4, (fx.name, label, bias)
    return dp / bp, dz / bz


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_alone_in_batch_form(ctx, params, name):
    """(a) One record a call, the batch form forced (tree_lane = 2): the shared-tile mid-field with the
    fixture's own k ranges, every knob that regroups the sums, against f64, against the wave-per-cell
    launches of the same record, and twice for the bits."""
    fx = Fixture(name)
    contra, short = fx.model()
    mr, zr = run(ctx, [fx.seq], contra, short, 0)
    mw, zw = run(ctx, [fx.seq], contra, short, 1, tree_lane=0)
    pw = np.asarray(mw[0].packed)
    dpw = float(np.max(np.abs(pw[fx.f["index"]].astype(np.float64) - fx.f["prob"])))
    print(f"{name} [wave-per-cell]: |dp| = {dpw:.3e} = {dpw / dp_bound(fx.n, fx.xz):.3f} x bound, "
          f"|d ln Z| = {abs(float(zw[0]) - fx.xz):.3e} = {abs(float(zw[0]) - fx.xz) / dz_bound(fx.n, fx.xz):.3f} x bound")
    results = {}
    for label, knobs in (FORMS if fx.n < 4096 else FORMS[:2]):
        m, z = run(ctx, [fx.seq], contra, short, 1, tree_lane=2, **knobs)
        against_fixture(fx, label, m[0].packed, z[0], mr[0].packed, zr[0])
        same, dw = deviation(m[0].packed, pw)
        assert same and dw <= form_bound(fx.n, fx.xz), (name, label, dw)
        assert abs(float(z[0]) - float(zw[0])) <= 3e-6 * abs(float(zw[0])), (name, label)
        results[label] = (np.asarray(m[0].packed), z[0])
    if "tree_gen_batch=1" in results:  # (the same terms in the same order within a cell)
        assert np.array_equal(results["tree_gen_batch=1"][0], results["default"][0])
    m2, z2 = run(ctx, [fx.seq], contra, short, 1, tree_lane=2)
    assert np.array_equal(np.asarray(m2[0].packed), results["default"][0]) and z2[0] == results["default"][1], \
        "not deterministic"


def bench_batch(contra, short):
    """-> (sequences, {index in the batch: Fixture}): the benchmark's first records, then the model's
    fixture records of at most 2048 nt"""
    from rna_algos_amd import workloads as W
    seqs = W.batch(BATCH_HEAD)
    assert sum(len(s) for s in seqs) == 70239 and min(len(s) for s in seqs) == 256 and max(len(s) for s in seqs) == 2034
    fixtures = {}
    for name in FIXTURES:
        fx = Fixture(name)
        if fx.model() == (contra, short) and fx.n <= 2048:
            fixtures[len(seqs)] = fx
            seqs.append(fx.seq)
    return seqs, fixtures


def mid_field_forms(lens, band=32):
    """Which form of the matrix-core mid-field each launch of a ONE-group batch-form sweep takes.  This
    RESTATES the rule of launch_tree_mid_mx (rnamc_tree_mx.h) and the launches of run_batch_tree
    (rnamc_sweep_tree.cpp, tree_mid_sync = 1) — no statistic of the library reports the form:
        nbi = ceil((gmax - dlo) / 32), ntc = ceil((31 + band width) / 32), tiles = nbi ntc (x 2 outside),
        a tile per wave when tiles * active(dlo) >= 4096, else four waves share a tile.
    -> {"inside" / "outside": ([dlo of the tile-per-wave launches], [dlo of the shared-tile launches])}"""
    gmax = max(lens)
    out = {"inside": ([], []), "outside": ([], [])}
    for x in range((gmax + band - 1) // band):
        dlo, dhi = x * band, min(gmax - 1, x * band + band - 1)
        nbi, ntc = (gmax - dlo + 31) // 32, (31 + (dhi - dlo + 1) + 31) // 32
        active = sum(1 for n in lens if n > dlo)
        if x >= 1:  # inside: the band's mid-field in front of the band
            out["inside"][0 if nbi * ntc * active >= 4096 else 1].append(dlo)
        if (x + 1) * band < gmax:  # outside: operands of every band above this one
            out["outside"][0 if 2 * nbi * ntc * active >= 4096 else 1].append(dlo)
    return out


def same_keys(a, b):
    return np.array_equal(np.asarray(a) >= -0.5, np.asarray(b) >= -0.5)


@pytest.mark.parametrize("model,contra,short", MODELS)
def test_bench_records_with_fixtures(ctx, params, model, contra, short):
    """(b) The route of `bench.py --summation tree`: the host-buffer entry at default knobs on a call of
    more than 65 536 nt, one group, ragged — the sweep starts with a tile per wave and ends with shared
    tiles.  The fixture records against f64; every record against the wave-per-cell launches of the same
    call, key sets against the reference-order result too."""
    seqs, fixtures = bench_batch(contra, short)
    lens = [len(s) for s in seqs]
    m, z = run(ctx, seqs, contra, short, 1)
    st = ctx.stats()
    assert st["n_groups"] == 1
    # a launch per diagonal (and the generic 2-loop sums): the batch form, taken by the call's size alone;
    # the wave-per-cell chain pairs its diagonals
    assert st["launches_inside"] >= max(lens) and st["launches_outside"] >= max(lens), st
    forms = mid_field_forms(lens)
    counts = {k: (len(v[0]), len(v[1])) for k, v in forms.items()}
    print(f"{model}: mid-field launches tile-per-wave / shared tile: inside {counts['inside']}, outside {counts['outside']}; "
          f"tile-per-wave up to dlo = {max(forms['inside'][0] + forms['outside'][0])}")
    assert min(counts["inside"] + counts["outside"]) >= 5, counts
    if model == "turner":
        assert counts == {"inside": (22, 41), "outside": (35, 28)}, counts
        assert max(forms["inside"][0] + forms["outside"][0]) == 1088
    mw, zw = run(ctx, seqs, contra, short, 1, tree_lane=0)
    stw = ctx.stats()
    assert stw["launches_inside"] < max(lens), stw
    mr, zr = run(ctx, seqs, contra, short, 0)
    worst = 0.0
    for x, (a, w, r) in enumerate(zip(m, mw, mr)):
        n = lens[x]
        same, dp = deviation(a.packed, w.packed)
        assert same and dp <= form_bound(n, float(zw[x])), (model, x, n, dp)
        assert abs(float(z[x]) - float(zw[x])) <= 3e-6 * abs(float(zw[x])), (model, x, n, float(z[x]), float(zw[x]))
        assert same_keys(a.packed, r.packed), (model, x, n)
        worst = max(worst, dp / form_bound(n, float(zw[x])))
    print(f"{model}: {len(seqs)} records, batch form against wave-per-cell launches: worst |dp| = {worst:.3f} x bound")
    assert fixtures
    for x, fx in fixtures.items():
        against_fixture(fx, f"among {BATCH_HEAD} benchmark records", m[x].packed, z[x], mr[x].packed, zr[x])


@pytest.fixture(scope="module")
def three_groups(ctx):
    """The Turner batch in three groups through the host-buffer entry (which stages group by group and keeps
    one stream): computed once, left unchanged -> (sequences, sequences per group, triangles, ln Z)"""
    seqs, _ = bench_batch(False, False)
    per_group = (len(seqs) + 2) // 3
    ctx.set("group_max_seqs", per_group)
    try:
        host, zhost = run(ctx, seqs, False, False, 1)
        st = ctx.stats()
    finally:
        ctx.set("group_max_seqs", 8192)
    assert st["n_groups"] == 3 and st["launches_inside"] >= max(len(s) for s in seqs), st
    return seqs, per_group, host, np.asarray(zhost)


@pytest.mark.parametrize("dual", [0, 1])
def test_bench_records_three_groups_side_by_side(ctx, params, three_groups, dual):
    """(b) The Turner batch through the device-resident entry in three groups of gigabytes each, one after the
    other (tree_dual = 0) and every other group on a second stream with its own half of the workspace
    (tree_dual = 1): each bit-identical to the host-buffer entry's result with the same groups — hence to
    one another — and every output slot written."""
    import torch
    seqs, per_group, host, zhost = three_groups
    ln = np.array([len(s) for s in seqs], dtype=np.uint64)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(ln, out=off[1:])
    oo = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(ln * (ln + np.uint64(1)) // np.uint64(2), out=oo[1:])
    dev = torch.device("cuda:0")
    d_b = torch.from_numpy(np.concatenate(seqs)).to(dev)
    d_o = torch.full((int(oo[-1]),), -7.0, dtype=torch.float32, device=dev)
    d_z = torch.zeros(len(seqs), dtype=torch.float32, device=dev)
    ctx.set("group_max_seqs", per_group)
    ctx.set("summation_mode", 1)
    ctx.set("tree_dual", dual)
    try:
        ctx.bpp_batch_device(len(seqs), d_b.data_ptr(), off, False, False, d_o.data_ptr(), oo, d_z.data_ptr(), 0)
        torch.cuda.synchronize()
        st = ctx.stats()
    finally:
        ctx.set("summation_mode", 0)
        ctx.set("tree_dual", 1)
        ctx.set("group_max_seqs", 8192)
    assert st["n_groups"] == 3 and st["launches_inside"] >= int(ln.max()), st
    assert not bool((d_o == -7.0).any())
    out = d_o.cpu().numpy()
    assert np.array_equal(d_z.cpu().numpy(), zhost)
    for x, a in enumerate(host):
        assert np.array_equal(np.asarray(a.packed), out[int(oo[x]):int(oo[x + 1])]), x


def test_bench_records_span_limit_and_constraint(ctx, params):
    """(c) The Turner batch under max_bp_span = 150 with 40 bases of the 2048 record forbidden to pair: the
    batch form against the wave-per-cell launches of the same call, to rounding, key sets equal; no pair
    beyond the limit (a pair (i, j) is admitted while j - i + 1 <= 150: no diagonal j - i >= 150), none on
    the forbidden stretch.  A FORM-AGAINST-FORM check only: the masked f64 oracle at this length is hours."""
    seqs, fixtures = bench_batch(False, False)
    x2048 = next(x for x, fx in fixtures.items() if fx.n == 2048)
    lo, hi, span = 1000, 1040, 150
    cons = [None] * len(seqs)
    cons[x2048] = "." * lo + "x" * (hi - lo) + "." * (2048 - hi)

    def call(**knobs):
        ctx.set("summation_mode", 1)
        for k, v in knobs.items():
            ctx.set(k, v)
        try:
            return ctx.bpp_batch(seqs, False, False, cons, span)
        finally:
            ctx.set("summation_mode", 0)
            for k in knobs:
                ctx.set(k, {"tree_lane": 1}[k])

    m, z = call()
    mw, zw = call(tree_lane=0)
    held = 0
    for x, (a, w) in enumerate(zip(m, mw)):
        n = len(seqs[x])
        same, dp = deviation(a.packed, w.packed)
        assert same and dp <= form_bound(n, float(zw[x])), (x, n, dp)
        assert abs(float(z[x]) - float(zw[x])) <= 3e-6 * abs(float(zw[x])), (x, n)
        p = np.asarray(a.packed)
        first = span * n - span * (span - 1) // 2  # (diagonal-major: diagonal 150 starts here)
        assert np.all(p[first:] < -0.5), (x, n)
        held += int(np.count_nonzero(p[first - (n - (span - 1)):first] >= -0.5))
    assert held > 0, "no pair on the longest admitted diagonal: the limit does not bind"
    d = m[x2048].dense()
    assert np.all(d[lo:hi, :] < -0.5) and np.all(d[:, lo:hi] < -0.5)
    assert np.any(d[lo - 1, :] >= -0.5) and np.any(d[:, hi] >= -0.5)


def test_spread_copies_are_bit_identical(ctx, params):
    """k_tlane_spread on rows and bands four times longer than the other batch-form tests reach: after a
    batch-form call the row- and column-major copies that the mid-field kernels read hold the bits of their
    diagonal-major sources — Q1 (both copies, every diagonal), and of the outside sweep W and R (every band
    but the lowest, which has no reader).  Read through rnamc_debug_fetch_tree (slots: enum TreeMat) from the
    Turner batch of (b): a ragged group, records of 2048, 1531 (partial tiles) and 256 nt.  An error of one
    ulp in a copy moves the probabilities by less than the summation order does; only the bits show it."""
    T_Q1R, T_Q1C, T_ZRE, T_ZRM, T_Q1_D, T_ZRM_D, T_W_D = 2, 3, 4, 5, 32, 33, 34
    seqs, fixtures = bench_batch(False, False)
    run(ctx, seqs, False, False, 1)
    assert ctx.stats()["n_groups"] == 1
    picks = [x for x, fx in fixtures.items() if fx.n > 1024] + [int(np.argmin([len(s) for s in seqs]))]
    for x in picks:
        n = len(seqs[x])
        mats = {slot: ctx.debug_fetch_tree(x, slot)[0].view(np.uint32) for slot in (T_Q1R, T_Q1C, T_ZRE, T_ZRM, T_Q1_D, T_ZRM_D, T_W_D)}
        d, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        cell = i + d < n
        d, i = d[cell], i[cell]
        j = i + d
        src = mats[T_Q1_D][d, i]
        assert np.isfinite(src.view(np.float32)).any()
        for name, got in (("row-major Q1", mats[T_Q1R][i, j]), ("column-major Q1", mats[T_Q1C][j, i])):
            bad = np.flatnonzero(got != src)
            assert bad.size == 0, (n, name, bad.size, int(i[bad[0]]), int(j[bad[0]]))
        up = d >= 32  # (the bands above the lowest; tree_lane_band = 32)
        for name, got, s in (("row-major W", mats[T_ZRE][i, j], mats[T_W_D][d, i]),
                             ("column-major R", mats[T_ZRM][j, i], mats[T_ZRM_D][d, i])):
            assert np.isfinite(s[up].view(np.float32)).any()
            bad = np.flatnonzero((got != s) & up)
            assert bad.size == 0, (n, name, bad.size, int(i[bad[0]]), int(j[bad[0]]))
