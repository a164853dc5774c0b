"""Conditions on the inputs of test_gpu_tree_helices.py, checked with the CPU oracle alone (no GPU):
they keep the GPU tests meaningful when somebody shortens an input or swaps a table.

The figure is helix_inputs.chunk_spread of sums_1ormore_basepairs (Turner model): the largest
max - min over the finite entries of a row or column inside an aligned chunk of 32 k — what the
per-chunk scale of the matrix-core mid-field (rnamc_tree_mx.h) has to carry.  Measured here:
split-run, bare-core and hairpin inputs 170-172 nats under strong_tables(), 132 under
mild_tables(); the SplitMix controls 55 / 62 and 31 / 34; (GC)^120 88 and 54.
"""
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import helix_inputs as H
import oracle_lib as O


@pytest.fixture(scope="module")
def strong(built):
    return H.strong_tables()


@pytest.fixture(scope="module")
def mild(built):
    return H.mild_tables()


@pytest.fixture(scope="module")
def spread(strong, mild):
    """{name: (chunk spread under strong_tables(), under mild_tables())}, Turner model"""
    fam = H.family()
    jobs = [(p, s) for _, s in fam for p in (strong, mild)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        res = list(ex.map(lambda j: H.q1_spread(j[0], j[1]), jobs))
    return {name: (res[2 * x], res[2 * x + 1]) for x, (name, _) in enumerate(fam)}


# (GC)^120 pairs in every register but has no run of one base: a helix grows by a stacked pair every
# SECOND k, so its spread is half a run's and the 150 / 120-nat conditions cannot hold for it; it is
# in the family for its many competing helices and is held to "above every control" instead.
RUNS = [(name, s) for name, s in H.helix_family() if name != "gc_120"]


def test_family_shape():
    """every member at most 450 nt and long enough to be swept banded at band 64 (n >= 192); the
    split-run inputs put the G-run's midpoint 0, 1, 2 and 16 positions behind a chunk boundary and
    its start on eight different residues mod 32"""
    for name, s in H.family():
        assert 192 <= len(s) <= 450, name
    mids = {(H.split_run_parts(a)[1] + 32) % H.CHUNK for a in H.SPLIT_A}
    assert {0, 1, 2, 16} <= mids
    assert len({H.split_run_parts(a)[1] % H.CHUNK for a in H.SPLIT_A}) == 8
    names = [name for name, _ in H.family()]
    assert len(set(names)) == len(names)


def test_strong_tables_only_change_turner_stacks(strong, mild):
    a, b = strong.field("turner.stack_scores"), mild.field("turner.stack_scores")
    for x, y in H.CANONICAL:
        for u, v in H.CANONICAL:
            assert a[x][y][u][v] == H.STRONG_STACK and b[x][y][u][v] < H.STRONG_STACK
    sa, sb = strong._buf.copy(), mild._buf.copy()
    off, cnt = strong._fields["turner.stack_scores"]
    sa[off:off + 4 * cnt] = 0
    sb[off:off + 4 * cnt] = 0
    assert (sa == sb).all()  # the CONTRAfold block and every other Turner table untouched
    assert strong.content_key() != mild.content_key()


def test_helix_inputs_reach_the_spread(spread):
    """chunk spread of sums_1ormore_basepairs: >= 150 nats under strong_tables(), >= 120 under
    mild_tables() for every input with a shared or hairpinned run"""
    for name, s in RUNS:
        a, b = spread[name]
        print(f"{name} n={len(s)}: chunk spread {a:.1f} nats strong, {b:.1f} mild")
        assert a >= 150.0, (name, a)
        assert b >= 120.0, (name, b)


def test_controls_stay_below_70_nats(spread):
    """the SplitMix controls stay at or below 70 nats under both tables (the fast path of the
    mid-field must keep them); (GC)^120 sits above them under strong_tables()"""
    worst = 0.0
    for name, s in H.controls():
        a, b = spread[name]
        print(f"{name} n={len(s)}: chunk spread {a:.1f} nats strong, {b:.1f} mild")
        assert a <= 70.0 and b <= 70.0, (name, a, b)
        worst = max(worst, a)
    a, b = spread["gc_120"]
    print(f"gc_120: chunk spread {a:.1f} nats strong, {b:.1f} mild")
    assert a > worst and a > 70.0


def test_split_run_holds_both_helices(strong):
    """exact f64 result, Turner model, strong tables: at least 25 expected pairs in each of the two
    helices that share the G-run (measured 33.8 / 30.2 at a = 0 to 38.7 / 25.3 at a = 28), the closing
    A-U pair at p = 0.97 — the multiloop whose branch point walks the run dominates Z"""
    for a in H.SPLIT_A:
        xb, _ = O.exact_bpp(strong.ptr, H.split_run(a), False)
        h1, h2, pc = H.split_run_pair_counts(xb, a)
        print(f"a={a}: helix 1 {h1:.2f} pairs, helix 2 {h2:.2f}, closing pair p = {pc:.4f}")
        assert h1 >= 25.0 and h2 >= 25.0, (a, h1, h2)
        assert pc >= 0.9, (a, pc)


def test_exact_reference_of_the_longest_input_is_quick(strong):
    """exact_bpp of the longest input in under 5 s (measured 2.9 s at n = 430): the GPU tests compute
    it once per model and table set"""
    s = max((s for _, s in H.family()), key=len)
    assert len(s) == 430
    t0 = time.perf_counter()
    O.exact_bpp(strong.ptr, s, False)
    dt = time.perf_counter() - t0
    print(f"exact_bpp n={len(s)}: {dt:.2f} s")
    assert dt < 5.0
