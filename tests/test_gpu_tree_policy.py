"""Tree-order sweep under the knobs that choose its launch shapes (TreePolicy and the route into the
lane-per-cell batch form: rnamc_tree.hip tree_grid / tree_tpc / launch_tree_mid, rnamc_sweep_tree.cpp).
Against the f64 evaluation of the recurrences (oracle/mccaskill_exact.c), computed once per sequence
and model variant, with the bounds of tests/test_gpu_tree.py: identical key sets,
|dp| <= 2e-5 + 2e-7 n (1.5 x that for the lane-per-cell form), |d ln Z| <= 2e-5 + 3e-6 |ln Z|; two forms
of the mode agree to 2 x the first bound.  Where a knob only deals the same per-cell arithmetic to
other waves or workgroups the bits must not change at all; each such case says from the launch rule
at which shape the other form engages.  Every call takes a context of its own (tests/soak_tree.py
draws some tree knobs at random; this is the collected, deterministic part)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

VARIANTS = [(False, False), (True, False), (True, True)]
variants = pytest.mark.parametrize("contra,short", VARIANTS, ids=["turner", "contra", "contra-short"])

# (length, serial): 98 = 3 * 32 + 2 is the shortest banded sweep at band 32 (194 / 193 / 192 for band 64:
# tests/test_gpu_tree.py)
LONE = [(37, 0), (98, 0), (130, 0), (257, 0), (301, 0), (410, 0), (640, 0)]
# more than 8 sequences: xcd_chunk's rotation by sequence wraps
RAGGED = LONE[::-1] + [(410, 1), (301, 1), (130, 1), (37, 1)]
XCD_EDGE = [(260, 0), (320, 0)]
THREE = [(410, 0), (301, 0), (257, 0)]


def seq_of(key):
    n, serial = key
    return O.splitmix_seq(n, 41 * n + 7 + 1000 * serial)


@pytest.fixture(scope="module")
def exact(params):
    """{(length, serial, contra, short): (f64 bpp, f64 ln Z)}, every sequence of the module once"""
    keys = sorted(set(LONE + RAGGED + XCD_EDGE), reverse=True)
    jobs = [(k, v) for k in keys for v in VARIANTS]
    O.lib()  # (loaded before the threads start)
    with ThreadPoolExecutor(max_workers=16) as pool:  # (the oracle call releases the interpreter lock)
        res = list(pool.map(lambda j: O.exact_bpp(params.ptr, seq_of(j[0]), j[1][0], j[1][1]), jobs))
    return {(k[0], k[1], v[0], v[1]): r for (k, v), r in zip(jobs, res)}


def bpp_bound(n):
    return 2e-5 + 2e-7 * n


def logz_bound(exact_logz):
    return 2e-5 + 3e-6 * abs(exact_logz)


def tree(params, keys, contra, short, **knobs):
    """one tree-order call on a fresh context -> (packed f32 per sequence, ln Z f32[])"""
    from rna_algos_amd.mccaskill_algo import Context
    ctx = Context(params, device=0)
    try:
        ctx.set("summation_mode", 1)
        for k, v in knobs.items():
            ctx.set(k, v)
        mats, logz = ctx.bpp_batch([seq_of(k) for k in keys], contra, short)
        return [np.asarray(m.packed).copy() for m in mats], np.asarray(logz).copy()
    finally:
        ctx.close()


def deviation(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ka, kb = a >= -0.5, b >= -0.5
    both = ka & kb
    return bool(np.array_equal(ka, kb)), float(np.max(np.abs(a[both] - b[both]))) if both.any() else 0.0


def hold_to_exact(exact, keys, contra, short, got, what, factor=1.0):
    mats, logz = got
    for k, a, z in zip(keys, mats, logz):
        xb, xz = exact[(k[0], k[1], contra, short)]
        same, dp = deviation(a, xb)
        assert same, f"{what}: n={k[0]}: key set differs from the f64 evaluation"
        assert dp <= factor * bpp_bound(k[0]), f"{what}: n={k[0]}: |dp| = {dp:.3e}"
        assert abs(float(z) - xz) <= logz_bound(xz), f"{what}: n={k[0]}: ln Z {float(z)!r} vs {xz!r}"


def hold_to_each_other(keys, got, base, what):
    for k, a, b0 in zip(keys, got[0], base[0]):
        same, dp = deviation(a, b0)
        assert same and dp <= 2 * bpp_bound(k[0]), f"{what}: n={k[0]}: |dp| = {dp:.3e} between two forms"


def bits(got):
    return [a.view(np.uint32) for a in got[0]] + [np.asarray(got[1], dtype=np.float32).view(np.uint32)]


def assert_same_bits(got, base, what):
    for x, (a, b0) in enumerate(zip(bits(got), bits(base))):
        assert np.array_equal(a, b0), f"{what}: {int((a != b0).sum())} words differ in output {x}"


CALLS = [[k] for k in LONE] + [RAGGED]


# ---- b. tree_waves x tree_short: the automatic threads-per-cell rule -------------------------------

@variants
@pytest.mark.parametrize("band,ahead", [(0, 1), (64, 1), (64, 0)])
def test_threads_per_cell_rule(params, exact, contra, short, band, ahead):
    """tree_tpc() with tree_tpc = 0 picks, per launch of `cells` cells (all sequences) whose sums have
    `terms` terms: 64 threads a cell if terms <= tree_short or 2 cells > tree_waves, else 128 if
    4 cells > tree_waves, else 256 (terms <= 2048 here).  Unbanded, a lone 410-nt inside sweep has
    cells = 410 - d and terms = d (outside: terms = cells):
      tree_waves 256, tree_short 32:  inside d < 282 -> 64, 282 <= d < 346 -> 128, d >= 346 -> 256;
                                      outside d >= 378 -> 64 (terms <= 32), 346 <= d < 378 -> 256,
                                      282 <= d < 346 -> 128, below -> 64
      tree_waves 64:   cells > 32 -> 64, 16 < cells <= 32 -> 128, cells <= 16 -> 256 (where terms > tree_short)
      tree_waves 1024: cells > 256 (d < 154) -> 128, else 256 (where terms > tree_short)
      defaults (5120, 256): 64 while terms <= 256, then 256 — 128 never.
    Launches of banded diagonals (thr != 0) count terms = 1024 whatever d is, so there the rule is the
    one of the cells alone; with the ahead role (tree_ahead 1) every launch after the first takes the
    one-wave form that reads its far parts from the ring (launch_tree_inside / launch_tree_outside,
    `use_far`): the rule then governs
    the first launch of each sweep alone, whose sums of a handful of terms come out the same in any
    form, so band 64 is run without the ahead role too.  Each setting is held to the f64 evaluation and
    to the default policy; where the rule governs the sweep (unbanded, and banded without the ahead
    role) some setting must change bits of the lone 410-nt sequence against the default policy (the
    knob reached the launch)."""
    common = dict(tree_tpc=0, tree_band=band, tree_ahead=ahead)
    changed = False
    for keys in CALLS:
        base = tree(params, keys, contra, short, **common)
        hold_to_exact(exact, keys, contra, short, base, f"default policy {common}")
        for waves in (64, 256, 1024):
            for short_terms in (1, 32, 256):
                what = f"tree_waves={waves} tree_short={short_terms} {common}"
                got = tree(params, keys, contra, short, tree_waves=waves, tree_short=short_terms, **common)
                hold_to_exact(exact, keys, contra, short, got, what)
                hold_to_each_other(keys, got, base, what)
                if keys == [(410, 0)]:
                    changed |= any(not np.array_equal(a, b0) for a, b0 in zip(bits(got), bits(base)))
    if band == 0 or ahead == 0:
        assert changed, "no tree_waves / tree_short setting changed a bit of the lone 410-nt sweep"


# ---- c. tree_ahead_waves: one ahead wave per cell or per row --------------------------------------

@variants
@pytest.mark.parametrize("tpc", [0, 64])
@pytest.mark.parametrize("band", [32, 64])
def test_ahead_wave_assignment(params, exact, contra, short, band, tpc):
    """The ahead role (banded sweeps: extra workgroups of a launch sum the far part of the next launch's
    2-loop blocks) takes one wave per CELL while (cells + 2 rows) * sequences <= tree_ahead_waves
    (tree_grid, Ahead.flags bit 1), one wave per row — both cells of the row, one after the other —
    beyond.  Default 16 384: every launch of the lone calls is per cell.  0: every launch per row.  300: a
    launch of the inside sweep of a lone n-nt sequence has cells = n - d and rows = n - d - 2, so it runs
    per row while 3 (n - d) - 4 > 300 and per cell for n - d <= 101: the 410-nt sweep switches at
    d = 310, the 640-nt one at d = 540, sequences of up to 101 nt are per cell throughout, and in the
    ragged batch the count is multiplied by the sequences still active.  A cell's far part is the same
    pair_far call and the same wave reduction in either assignment (k_tree_inside2 / k_tree_outside2,
    the `split` branch): bit-identical to the default."""
    common = dict(tree_band=band, tree_ahead=1, tree_tpc=tpc)
    for keys in CALLS:
        base = tree(params, keys, contra, short, **common)
        hold_to_exact(exact, keys, contra, short, base, str(common))
        for ahead_waves in (0, 300):
            got = tree(params, keys, contra, short, tree_ahead_waves=ahead_waves, **common)
            assert_same_bits(got, base, f"tree_ahead_waves={ahead_waves} {common} n={[k[0] for k in keys]}")


# ---- d. tree_xcd_rows: workgroup ids dealt by XCD --------------------------------------------------

@variants
@pytest.mark.parametrize("tpc", [0, 64])
@pytest.mark.parametrize("band", [0, 64])
def test_xcd_rows(params, exact, contra, short, band, tpc):
    """tree_xcd_rows 1 permutes the workgroup ids of a one-wave-per-cell launch (xcd_chunk, rotated by
    the sequence's index) and pads both roles' grids to multiples of 64 workgroups, wherever the launch
    has main_blocks = ceil(cells / 4) >= 64, i.e. at least 253 cells on the diagonal: the low diagonals
    of every sequence here (n = 260: main_blocks 64 or 65 on the first launches, 63 from 252 cells on;
    n = 320: 79 or 80 at the start), padded ids past the diagonal's end and past the ahead role's rows
    leave at once.  Every cell is still computed by one workgroup with the same arithmetic:
    bit-identical to tree_xcd_rows 0."""
    common = dict(tree_band=band, tree_tpc=tpc)
    for keys in [[(301, 0)], [(410, 0)], [(640, 0)], [(260, 0)], [(320, 0)], RAGGED]:
        base = tree(params, keys, contra, short, tree_xcd_rows=0, **common)
        hold_to_exact(exact, keys, contra, short, base, str(common))
        got = tree(params, keys, contra, short, tree_xcd_rows=1, **common)
        assert_same_bits(got, base, f"tree_xcd_rows=1 {common} n={[k[0] for k in keys]}")


# ---- e. tree_mid_wgs: tiles per workgroup of the VALU mid-field kernel -----------------------------

@variants
@pytest.mark.parametrize("band", [32, 64])
def test_mid_field_workgroups(params, exact, contra, short, band):
    """k_tree_mid (tree_mid_mx 0) walks the tiles_i * tiles_z tiles of a band with
    min(tiles, ceil(tree_mid_wgs / sequences)) workgroups, each staging one tile after the other through
    the same LDS.  By default (256 workgroups below 6 144 nt) a workgroup of the lone calls gets one
    tile: a 410-nt band of 64 diagonals has at most 52 x 2 x 2 tiles (the batch of three: 86 workgroups a
    sequence, up to three tiles each).  1 / 3 / 7 make one workgroup walk all / a third / a seventh of
    them.  Every tile writes its own cells from its own operands:
    bit-identical to the default, and from run to run."""
    common = dict(tree_mid_mx=0, tree_band=band)
    for keys in ([(257, 0)], [(410, 0)], THREE):
        base = tree(params, keys, contra, short, **common)
        hold_to_exact(exact, keys, contra, short, base, str(common))
        for wgs in (1, 3, 7):
            what = f"tree_mid_wgs={wgs} {common} n={[k[0] for k in keys]}"
            got = tree(params, keys, contra, short, tree_mid_wgs=wgs, **common)
            assert_same_bits(got, base, what)
            again = tree(params, keys, contra, short, tree_mid_wgs=wgs, **common)
            assert_same_bits(again, got, what + " (second run)")


# ---- f. tree_lane_min_nt: the automatic route into the lane-per-cell batch form --------------------

@variants
def test_lane_route_by_nucleotides(params, exact, contra, short):
    """tree_lane 1 (the default) takes the lane-per-cell batch form for calls of several sequences and
    at least tree_lane_min_nt nucleotides (rnamc_sweep_tree.cpp, `lane_mode`): at the call's total the
    bits are those of tree_lane 2, one above those of tree_lane 0; a lone sequence keeps the
    wave-per-cell chain whatever the knob says."""
    total = sum(k[0] for k in THREE)
    forced = tree(params, THREE, contra, short, tree_lane=2)
    never = tree(params, THREE, contra, short, tree_lane=0)
    hold_to_exact(exact, THREE, contra, short, forced, "tree_lane=2", factor=1.5)
    hold_to_exact(exact, THREE, contra, short, never, "tree_lane=0")
    assert any(not np.array_equal(a, b0) for a, b0 in zip(bits(forced), bits(never))), \
        "the two forms cannot be told apart on this call"
    assert_same_bits(tree(params, THREE, contra, short, tree_lane_min_nt=total), forced, "at the total")
    assert_same_bits(tree(params, THREE, contra, short, tree_lane_min_nt=total + 1), never, "one above")
    lone = [(410, 0)]
    base = tree(params, lone, contra, short, tree_lane=0)
    for min_nt in (0, 410):
        assert_same_bits(tree(params, lone, contra, short, tree_lane_min_nt=min_nt), base, f"lone, {min_nt}")
