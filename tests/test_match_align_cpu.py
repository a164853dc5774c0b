"""The gamma-centroid alignment of a match-probability matrix without a GPU:
rnamc_match_align, the host function that defines what the device stage reproduces, against the
numpy-f32 restatement of include/rnamc.h in match_align_ref.py — mate, count and accuracy bit for
bit — and the gapped-row form of an alignment there and back."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import match_align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (2, 3, 4, 9, 66)


def same(got, want, what):
    mate, count, acc = got
    wmate, wcount, wacc = want
    assert np.array_equal(mate, wmate), what
    assert count == wcount == int(np.sum(wmate >= 0)), what
    assert np.float32(acc).view(np.uint32) == np.float32(wacc).view(np.uint32), f"{what}: {acc} vs {wacc}"
    assert mate[0] == -1 and mate[-1] == -1


def test_random_ragged_matrices_bit_exact(built):
    from rna_algos_amd.pair_align import match_align
    rng = np.random.default_rng(20)
    for n1, n2 in itertools.product(SIDES, SIDES):
        for density in (0.3, 1.0):
            P = R.random_probmat(rng, n1, n2, density)
            for gamma in (1.5, 2.0, 6.0, 64.0):
                same(match_align(P, gamma), R.match_align(P, gamma), f"{n1} x {n2} gamma {gamma}")


def test_quantised_matrices_the_equality_order_decides(built):
    """multiples of 1/4 and gammas 2 and 4: every candidate is exact and ties are everywhere"""
    from rna_algos_amd.pair_align import match_align
    rng = np.random.default_rng(21)
    tied = 0
    for n1, n2 in itertools.product(SIDES, SIDES):
        P = R.quantised_probmat(rng, n1, n2)
        for gamma in (2.0, 4.0):
            want = R.match_align(P, gamma)
            same(match_align(P, gamma), want, f"quantised {n1} x {n2} gamma {gamma}")
            M = R.fill(P, gamma)
            tied += int(np.sum((M[1:, 1:] == M[:-1, 1:]) & (M[1:, 1:] == M[1:, :-1])))
    assert tied > 1000  # (cells where both skips tie: the order of the tests is what is checked)


def test_all_zero_matrix_and_empty_sequences(built):
    from rna_algos_amd.pair_align import match_align
    for n1, n2 in ((9, 66), (2, 2), (2, 9), (9, 2), (3, 3)):
        mate, count, acc = match_align(np.zeros((n1, n2), np.float32), 2.0)
        assert count == 0 and np.all(mate == -1) and len(mate) == n1
        assert np.float32(acc).view(np.uint32) == 0  # +0
    rng = np.random.default_rng(22)
    for n1, n2 in ((2, 9), (9, 2), (2, 2)):  # an empty sequence, whatever the matrix holds
        P = rng.random((n1, n2)).astype(np.float32)
        mate, count, acc = match_align(P, 8.0)
        assert count == 0 and np.all(mate == -1) and np.float32(acc).view(np.uint32) == 0


def test_gamma_at_most_one_matches_nothing(built):
    from rna_algos_amd.pair_align import match_align
    rng = np.random.default_rng(23)
    P = R.random_probmat(rng, 66, 9, 1.0)
    P[3, 4] = 1.0
    for gamma in (1.0, 0.5, 0.0, -3.0):
        got = match_align(P, gamma)
        same(got, R.match_align(P, gamma), f"gamma {gamma}")
        assert got[1] == 0 and np.float32(got[2]).view(np.uint32) == 0


@pytest.mark.parametrize("shape,kw", [((66, 66), dict(start=1, run=3, gap_a=1, gap_b=2)),
                                      ((66, 9), dict(start=5, run=2, gap_a=3, gap_b=0)),
                                      ((9, 66), dict(start=2, run=1, gap_a=0, gap_b=7)),
                                      ((4, 4), dict(start=1, run=1, gap_a=0, gap_b=0))])
def test_staircase_is_recovered(built, shape, kw):
    """p = 1 on a monotone path with gaps, gamma 2: the optimum is exactly that path"""
    from rna_algos_amd.pair_align import match_align
    P, path = R.staircase(*shape, **kw)
    mate, count, acc = match_align(P, 2.0)
    assert np.array_equal(mate, path)
    assert count == int(np.sum(path >= 0)) > 0 and acc == np.float32(count)
    same((mate, count, acc), R.match_align(P, 2.0), "staircase")


def test_gapped_rows_round_trip(built):
    from rna_algos_amd.pair_align import match_align, mate_to_rows, rows_to_mate
    rng = np.random.default_rng(24)
    for n1, n2 in itertools.product(SIDES, SIDES):
        P = R.random_probmat(rng, n1, n2, 0.5)
        mate, count, _ = match_align(P, 3.0)
        row_a, row_b = mate_to_rows(mate, n2)
        assert (row_a, row_b) == R.gapped_rows(mate, n2)
        assert len(row_a) == len(row_b) == (n1 - 2) + (n2 - 2) - count
        assert row_a.replace("-", "") == "N" * (n1 - 2) and row_b.replace("-", "") == "N" * (n2 - 2)
        assert not any(x == "-" and y == "-" for x, y in zip(row_a, row_b))
        assert np.array_equal(rows_to_mate(row_a, row_b), mate)
    # unmatched bases of a come before those of b between two matches; bases are spelled out
    a = np.array([4, 0, 1, 2, 3, 4], np.uint8)
    b = np.array([4, 3, 3, 2, 4], np.uint8)
    rows = mate_to_rows(np.array([-1, -1, -1, -1, 3, -1], np.int32), 5, a, b)
    assert rows == ("ACG--U", "---UUG")


def test_bad_arguments(built):
    from rna_algos_amd import _lib
    L = _lib.lib()
    P = np.zeros((3, 3), np.float32)
    mate = np.zeros(3, np.int32)
    n, acc = C.c_uint32(0), C.c_float(0)
    ok = (P.ctypes.data, 3, 3, C.c_float(2.0), mate.ctypes.data, C.byref(n), C.byref(acc))
    assert L.rnamc_match_align(*ok) == _lib.OK
    assert L.rnamc_match_align(None, *ok[1:]) == _lib.ERR_INVALID_ARG
    assert L.rnamc_match_align(ok[0], 1, *ok[2:]) == _lib.ERR_INVALID_ARG
    assert L.rnamc_match_align(*ok[:4], None, *ok[5:]) == _lib.ERR_INVALID_ARG
    assert L.rnamc_match_align(*ok[:6], None) == _lib.OK  # (the accuracy is optional)


def test_sources_and_bindings_name_the_entries(built):
    mk = open(os.path.join(ROOT, "rna_algos_amd", "csrc", "Makefile")).read()
    assert "rnamc_match.hip" in mk and "rnamc_entries_match.cpp" in mk
    hpp = open(os.path.join(ROOT, "include", "rna_algos", "durbin_algo.hpp")).read()
    for name in ("rnamc_match_align", "rnamc_match_align_mats", "rnamc_durbin_align_batch"):
        assert name in hpp, name
