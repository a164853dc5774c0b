"""CPU suite, part 1: pins the oracle (oracle/*.c) — the restatement of the reference's
McCaskill path that every GPU parity test compares against.

PARITY UNPINNED by the reference itself (no Rust toolchain here, tables live in the absent
rna-ss-params crate, the reference's only test is a range assertion), so the oracle is
pinned by: (1) an exhaustive f64 structure enumeration, (2) an all-zero-table structure
count computed by an independent integer DP, (3) the reference's own range assertion on
its own fixture, (4) committed self-golden vectors (drift guard)."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def unpack(packed, n):
    m = np.full((n, n), -1.0, dtype=np.float64)
    off = 0
    for d in range(n):
        idx = np.arange(n - d)
        m[idx, idx + d] = packed[off:off + n - d]
        off += n - d
    return m


def canon(a, b):
    return (a + b == 3) or (a + b == 5)


@pytest.mark.parametrize("contra,short", [(0, 0), (1, 0), (1, 1)])
def test_bruteforce_random(params, contra, short):
    rng = np.random.default_rng(100 + contra * 2 + short)
    worst_p = worst_z = 0.0
    for trial in range(25):
        n = int(rng.integers(1, 17 if not short else 13))
        seq = rng.integers(0, 4, n).astype(np.uint8)
        out, logz = O.bpp(params.ptr, seq, contra, short)
        lz, full, cnt = O.bruteforce(params.ptr, seq, contra, short)
        m = unpack(out, n)
        for i in range(n):
            for j in range(i, n):
                if m[i, j] < -0.5:
                    assert full[i, j] == 0.0, (seq, i, j)
                else:
                    worst_p = max(worst_p, abs(m[i, j] - full[i, j]))
        worst_z = max(worst_z, abs(lz - float(logz)))
    # logsumexp / expf are CONTRAfold's cubic approximations: ~1e-4 is their floor
    assert worst_p < 2e-3 and worst_z < 2e-3, (worst_p, worst_z)


@pytest.mark.parametrize("contra", [0, 1])
def test_bruteforce_multiloops(params, contra):
    """GC-rich sequences of length 18..21: every loop type incl. multiloops occurs."""
    rng = np.random.default_rng(5)
    for trial in range(4):
        n = int(rng.integers(18, 22))
        seq = rng.choice(np.array([1, 2, 2, 1, 3, 0], dtype=np.uint8), n)
        out, logz = O.bpp(params.ptr, seq, contra, 0)
        lz, full, cnt = O.bruteforce(params.ptr, seq, contra, 0)
        assert cnt > 50
        m = unpack(out, n)
        pres = m >= -0.5
        assert np.array_equal(pres, np.triu(full > 0)), "key set differs from enumeration"
        assert np.abs(m[pres] - full[pres]).max() < 2e-3
        assert abs(lz - float(logz)) < 2e-3


def count_structures(seq, short):
    """Independent integer DP: number of structures the CONTRAfold recurrences admit
    (canonical pairs; span >= 5 unless short; hairpin loop <= 30; a closed loop with one
    inner pair needs <= 30 unpaired bases, else >= 2 branches)."""
    import functools
    n = len(seq)
    L = 30

    def ok(i, j):
        return canon(int(seq[i]), int(seq[j])) and (short or j - i + 1 >= 5)

    @functools.lru_cache(None)
    def closed(i, j):  # structures of [i..j] in which (i,j) is paired
        if not ok(i, j):
            return 0
        tot = 1 if j - i - 1 <= L else 0
        for k in range(i + 1, j - 1):
            if k - i - 1 > L:
                break
            for l in range(j - 1, k, -1):
                if (j - l - 1) + (k - i - 1) > L:
                    break
                tot += closed(k, l)
        tot += multi(i + 1, j - 1, 2)
        return tot

    @functools.lru_cache(None)
    def multi(i, j, need):  # [i..j] holds >= need branches (need in 0,1,2), rest unpaired
        if i > j:
            return 1 if need == 0 else 0
        tot = multi(i + 1, j, need)  # i unpaired
        for l in range(i + 1, j + 1):
            c = closed(i, l)
            if c:
                tot += c * multi(l + 1, j, max(need - 1, 0))
        return tot

    return multi(0, n - 1, 0)


@pytest.mark.parametrize("short", [0, 1])
def test_zero_tables_count_structures(built, short):
    """FoldScoreSets::new(0.) without transfer: every structure weighs 1, so
    exp(sums_external[0][n-1]) is the number of admissible structures."""
    from rna_algos_amd.utils import FoldScoreSets
    zero = FoldScoreSets.new(0.0)
    rng = np.random.default_rng(9)
    for n in (6, 11, 17, 24, 40):
        seq = rng.choice(np.array([1, 2, 2, 1, 3, 0], dtype=np.uint8), n)
        _, logz = O.bpp(zero.ptr, seq, 1, short)
        cnt = count_structures(tuple(int(x) for x in seq), bool(short))
        assert abs(float(logz) - np.log(cnt)) < 2e-3 * max(1.0, np.log(cnt)), (n, cnt, logz)
        if n <= 17:
            _, _, bf = O.bruteforce(zero.ptr, seq, 1, short)
            assert bf == cnt


@pytest.mark.parametrize("contra", [0, 1])
def test_reference_range_assertion_on_trnas(params, trnas, contra):
    """tests/tests.rs:7-43: every bpp value of the 6 tRNAs lies in [-0.001, 1.001)."""
    for _, s in trnas:
        out, _ = O.bpp(params.ptr, s, contra, 0)
        vals = out[out >= -0.5]
        assert vals.size > 0
        assert np.all((vals >= -0.001) & (vals < 1.001))
        # a probability matrix: no base pairs with total mass much above 1
        m = unpack(out, len(s))
        m[m < 0] = 0
        assert (m.sum(0) + m.sum(1)).max() < 1.01


def test_golden_trna_vectors(params, trnas):
    g = np.load(os.path.join(GOLD, "trna_bpp_synthetic_seed1.npz"))
    for idx, (_, s) in enumerate(trnas):
        for contra, name in ((0, "turner"), (1, "contra")):
            out, lz = O.bpp(params.ptr, s, contra, 0)
            assert np.array_equal(out, g[f"trna{idx}_{name}"])
            assert np.float32(lz) == g[f"trna{idx}_{name}_logz"][0]


def test_golden_checksum_n1024(params):
    """configs[1] (n = 1024, seed 1024): ~20 s of oracle time per model; CONTRAfold only here."""
    g = json.load(open(os.path.join(GOLD, "checksums_n1024.json")))["cases"]["n1024_seed1024_contra"]
    s = O.splitmix_seq(1024, 1024)
    out, lz = O.bpp(params.ptr, s, 1, 0)
    a = out.copy()
    a[a >= 0.9999] = 1.0
    assert hashlib.sha256(a.tobytes()).hexdigest() == g["sha256"]
    assert int(np.float32(lz).view(np.uint32)) == g["log_partition_bits"]


def test_edge_cases(params):
    # n < 5 under Turner: nothing is written, Z = 0, empty map
    for n in (1, 2, 4):
        out, lz = O.bpp(params.ptr, np.zeros(n, np.uint8), 0, 0)
        assert np.all(out == -1.0) and lz == 0.0
    # homopolymer: no canonical pair
    out, lz = O.bpp(params.ptr, np.zeros(30, np.uint8), 0, 0)
    assert np.all(out == -1.0) and lz == 0.0
    out, lz = O.bpp(params.ptr, np.zeros(30, np.uint8), 1, 0)
    assert np.all(out == -1.0)
    eu = float(params.external_score_unpair[0])
    assert abs(float(lz) - 30 * eu) < 1e-4
    # invalid input -> status, not a crash
    with pytest.raises(RuntimeError):
        O.bpp(params.ptr, np.zeros(0, np.uint8), 0, 0)
    with pytest.raises(RuntimeError):
        O.bpp(params.ptr, np.array([0, 1, 9], np.uint8), 0, 0)


def test_thread_pool_batch_equals_sequential(params):
    rng = np.random.default_rng(2)
    seqs = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(5, 90, 12)]
    outs, logz = O.bpp_batch(params.ptr, seqs, 1, 0, n_threads=4)
    for s, o, lz in zip(seqs, outs, logz):
        ref, ref_lz = O.bpp(params.ptr, s, 1, 0)
        assert np.array_equal(o, ref) and lz == ref_lz


@pytest.mark.parametrize("contra,short", [(0, 0), (1, 0), (1, 1)])
def test_fold_scores_key_sets(params, trnas, contra, short):
    """FoldScores as the reference's inside pass fills it (src/mccaskill_algo.rs:302-304,
    320, 333-338 / 407-409, 431, 457-462): key-set invariants and loop-shape limits."""
    rng = np.random.default_rng(77)
    seqs = [trnas[0][1], rng.integers(0, 4, 40).astype(np.uint8), np.array([1, 2], np.uint8)]
    for seq in seqs:
        n = len(seq)
        hp, mb, ac, tl = O.fold_scores(params.ptr, seq, contra, short)
        _, _, mats = O.bpp_dump(params.ptr, seq, contra, short)
        close = mats[0]
        hp_m, mb_m, ac_m = (unpack(np.where(np.isnan(x), -1e30, x), n) > -1e29 for x in (hp, mb, ac))
        iu = np.triu_indices(n)
        member = close > -np.inf
        assert (mb_m[iu] == member[iu]).all() and (ac_m[iu] == member[iu]).all()
        for i in range(n):
            for j in range(i, n):
                act = canon(seq[i], seq[j]) and ((contra and short) or j - i + 1 >= 5)
                want_hp = act and (not contra or j - i - 1 <= 30)
                assert hp_m[i, j] == want_hp, (i, j)
        # multibranch_close values are the ones the outside pass read (dump slot 4)
        mbv = unpack(np.where(np.isnan(mb), -1.0, mb), n)
        assert (mbv[member] == mats[4][member]).all()
        # twoloop keys: closing pair may close, enclosed pair has a sums_close entry,
        # strictly nested, at most 30 unpaired bases; no duplicates
        keys = set()
        for e in tl:
            i, j, k, l = int(e["i"]), int(e["j"]), int(e["k"]), int(e["l"])
            assert i < k < l < j and (k - i - 1) + (j - l - 1) <= 30
            assert canon(seq[i], seq[j]) and ((contra and short) or j - i + 1 >= 5)
            assert member[k, l]
            keys.add((i, j, k, l))
        assert len(keys) == len(tl)
        # completeness: every admissible (i,j,k,l) is there
        want = 0
        for i in range(n):
            for j in range(i + 3, n):
                if not (canon(seq[i], seq[j]) and ((contra and short) or j - i + 1 >= 5)):
                    continue
                for k in range(i + 1, min(j - 1, i + 32)):
                    for l in range(j - 1, k, -1):
                        if (k - i - 1) + (j - l - 1) > 30:
                            break
                        want += bool(member[k, l])
        assert want == len(tl)


def test_exact_evaluation_against_bruteforce(params):
    """oracle/mccaskill_exact.c (the restatement's loops with Score = double and an exact
    logsumexp; the checker of the HIP path's tree-order mode) against the exhaustive f64
    enumeration: the two must agree to f64-level accuracy of f32 tables, and the f32
    reference-order restatement must sit farther from both (its logsumexp is a cubic fit)."""
    for n, seed in [(9, 11), (13, 12), (16, 13), (18, 14)]:
        for contra, short in [(False, False), (True, False), (True, True)]:
            s = O.splitmix_seq(n, seed)
            ez, full, cnt = O.bruteforce(params.ptr, s, contra, short)
            xb, xz = O.exact_bpp(params.ptr, s, contra, short)
            rb, rz = O.bpp(params.ptr, s, contra, short)
            assert abs(xz - ez) <= 1e-6 * max(1.0, abs(ez))
            o = 0
            for d in range(n):
                for i in range(n - d):
                    v = xb[o]
                    if full[i, i + d] > 0:
                        assert v >= 0 and abs(v - full[i, i + d]) <= 1e-6
                    else:
                        assert v < 0 or v <= 1e-30
                    assert (rb[o] >= -0.5) == (v >= -0.5)  # same key set as the reference restatement
                    o += 1


def test_logsumexp_pieces_never_lower_the_sum_by_more_than_rounding():
    """What the sure-far classification of the latency forms rests on (rnamc_latency.h,
    far_limit): a fold step returns  lo + r(z)  with  r(z) >= z - eps  for every cubic piece of
    ln_exp_1p (src/utils.rs:602-627), i.e. never less than the larger operand minus a rounding-
    sized eps, so that over a block of at most 256 steps the running sum cannot drop by the margin
    (1 while |values| < 2^12).  Swept over every piece in f32, operation for operation."""
    F = np.float32
    brk = [0.0, 0.66153675, 1.6320158, 2.4912589, 3.3792500, 4.426169, 5.789071, 7.8162727, 11.862479]
    coef = [(-0.0065591595, 0.12764427, 0.49965546, 0.6931542),
            (-0.015515756, 0.14467756, 0.48829398, 0.6958093),
            (-0.012890925, 0.13010283, 0.51503986, 0.6795586),
            (-0.0072142647, 0.087754086, 0.6208708, 0.5909676),
            (-0.0031455354, 0.046722945, 0.7592532, 0.43487945),
            (-0.0010110698, 0.018594341, 0.88317305, 0.25236955),
            (-0.000196278, 0.0046084408, 0.9634432, 0.09831489),
            (-0.0000113994, 0.0003734731, 0.9959107, 0.0149855051)]
    worst = 0.0
    for p, (a, b, c, d) in enumerate(coef):
        z = np.linspace(brk[p], brk[p + 1], 200001, dtype=np.float64).astype(F)
        z = z[(z >= F(brk[p])) & (z < F(brk[p + 1]))]
        r = ((F(a) * z + F(b)) * z + F(c)) * z + F(d)  # f32, no fusion: numpy rounds every op
        assert r.dtype == np.float32
        worst = max(worst, float(np.max(z.astype(np.float64) - r.astype(np.float64))))
        # and against the exact ln(1 + e^z): the reference's approximation error
        exact = np.log1p(np.exp(z.astype(np.float64)))
        assert np.max(np.abs(r.astype(np.float64) - exact)) < 2e-5
    # r(z) - z >= ln(1 + e^-z) - approximation error > 0 up to the last piece's end, where
    # ln(1 + e^-11.86) = 7e-6: the pieces may undershoot z by at most their own error
    assert worst * 256 < 1.0, worst
    print(f"max (z - r(z)) over all pieces: {worst:.3e}  (x 256 steps = {worst * 256:.3e} < margin 1)")


def test_fold_sums_stage_is_the_inside_pass_of_the_whole_path():
    """rnamc_oracle_fold_sums (get_fold_sums{,_contra}, src/mccaskill_algo.rs:282 / 380) returns
    what the whole path's inside pass leaves (bpp_dump's intermediates), with FoldSums::new's
    initial values (213-226) where the reference writes nothing."""
    from rna_algos_amd.utils import FoldScoreSets
    P = FoldScoreSets.synthetic(1)
    rng = np.random.default_rng(3)
    for contra, short in ((False, False), (True, False), (True, True)):
        for n in (1, 4, 5, 33, 90):
            seq = rng.integers(0, 4, n).astype(np.uint8)
            fs = O.fold_sums(P.ptr, seq, contra, short)
            _, logz, mats = O.bpp_dump(P.ptr, seq, contra, short)
            for name, w in (("sums_close", 0), ("sums_accessible", 1), ("sums_external", 2),
                            ("sums_1ormore_basepairs", 3)):
                assert np.array_equal(fs[name].view(np.uint32), mats[w].view(np.uint32)), (name, n, contra)
            assert fs["sums_external"][0, n - 1] == logz
            low = np.tril_indices(n, -1)
            assert np.all(fs["sums_external"][low] == 0.0)
            for name in O.FOLD_SUMS_FIELDS[1:]:
                assert np.all(np.isneginf(fs[name][low])), name
            if not contra:  # Turner never writes the multibranch flavour, nor spans below 5
                assert np.all(np.isneginf(fs["sums_rightmost_basepairs_multibranch"]))
                iu = np.triu_indices(n)
                short_span = (iu[1] - iu[0]) < 4
                assert np.all(fs["sums_external"][iu][short_span] == 0.0)


EXACT_ALL = ["exact_n1024_seed1024_contra", "exact_n1024_seed1024_turner", "exact_n1531_seed1531_contra",
             "exact_n1531_seed1531_turner", "exact_n2048_seed2048_contra_short", "exact_n2048_seed2048_turner",
             "exact_n4096_seed4096_turner"]


@pytest.mark.parametrize("name", ["exact_n1024_seed1024_contra", "exact_n1531_seed1531_contra"])
def test_exact_fixture_reproduces(params, name):
    """tests/golden/exact_n1024_seed1024_contra.npz and exact_n1531_seed1531_contra.npz (the f64 pins of the
    tree-order mode at scale, tests/make_golden.py `exact`, `exact_mid`) are what oracle/mccaskill_exact.c
    gives today: drift guard of the fixtures and of their container (every 97th present pair, key-set
    sha256).  ~30 s and ~2.5 minutes.  The reference-order oracle's deviation at n = 1531, measured here:
    max |dp| 7.8e-3, |d ln Z| 2.3e-2 — inside the band asserted at n = 1024."""
    f = np.load(os.path.join(GOLD, name + ".npz"))
    n, seed = int(f["n"][0]), int(f["seed"][0])
    short = int(f["short"][0]) if "short" in f.files else 0
    assert int(f["contra"][0]) == 1 and short == 0
    xb, xz = O.exact_bpp(params.ptr, O.splitmix_seq(n, seed), 1, 0)
    pres = np.flatnonzero(xb >= -0.5)
    assert hashlib.sha256(pres.astype(np.uint32).tobytes()).digest() == bytes(f["keyset_sha256"])
    assert np.array_equal(pres[::97], f["index"])
    assert np.allclose(xb[f["index"]], f["prob"], rtol=0, atol=1e-13) and abs(xz - float(f["log_partition"][0])) < 1e-9
    # and the f32 reference-order oracle sits where DESIGN.md section 4b says it does against it
    out, lz = O.bpp(params.ptr, O.splitmix_seq(n, seed), 1, 0)
    dp = float(np.max(np.abs(out[f["index"]].astype(np.float64) - f["prob"])))
    print(f"{name}: reference-order oracle against f64: max |dp| = {dp:.3e}, |d ln Z| = {abs(float(lz) - xz):.3e}")
    assert 1e-4 < dp < 5e-2 and abs(float(lz) - xz) < 5e-2, (dp, float(lz), xz)


@pytest.mark.parametrize("name", EXACT_ALL)
def test_exact_fixtures_load(name):
    """Every f64 fixture loads, and its container is consistent with itself — no oracle run: `index` is every
    97th entry of a key set of the recorded `present` size (strictly increasing slots of the packed triangle,
    ceil(present / 97) of them, the first one the key set's first), the probabilities are probabilities, `short`
    is 0 where absent."""
    f = np.load(os.path.join(GOLD, name + ".npz"))
    n, present = int(f["n"][0]), int(f["present"][0])
    assert f"_n{n}_seed{int(f['seed'][0])}_" in name
    assert ("contra" in name) == bool(f["contra"][0])
    assert (int(f["short"][0]) if "short" in f.files else 0) == (1 if name.endswith("_short") else 0)
    idx = f["index"].astype(np.int64)
    assert idx.size == len(range(0, present, 97)) and f["prob"].shape == idx.shape
    assert np.all(np.diff(idx) >= 97) and idx[-1] < n * (n + 1) // 2
    # (96 present slots lie between two picks, fewer than 97 behind the last)
    assert (idx.size - 1) * 97 < present <= idx.size * 97
    # the first present slot of the diagonal-major triangle: the first pair of the shortest admitted span
    s = O.splitmix_seq(n, int(f["seed"][0]))
    dmin = 1 if name.endswith("_short") else 4  # (f["index"][0] lies on the first diagonal that holds a pair)
    t = s[:n - dmin].astype(np.int64) + s[dmin:]
    first = dmin * n - dmin * (dmin - 1) // 2 + int(np.flatnonzero((t == 3) | (t == 5))[0])
    assert idx[0] == first, (int(idx[0]), first)
    assert f["keyset_sha256"].shape == (32,) and f["keyset_sha256"].dtype == np.uint8
    assert np.all(f["prob"] >= 0.0) and np.all(f["prob"] <= 1.0 + 1e-12) and float(f["max_prob"][0]) <= 1.0 + 1e-12
    assert np.isfinite(float(f["log_partition"][0])) and float(f["sum_present"][0]) >= float(f["prob"].sum())
