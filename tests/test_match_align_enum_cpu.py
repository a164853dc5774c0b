"""The gamma-centroid alignment against exhaustive search.  The other tests
of rnamc_match_align hold it to a restatement of its own recurrence and to staircases; here every
monotone matching of a small ProbMat is scored in f64 as the sum of (gamma * p - 1) over its matched
cells, and the (max,+) fill must find the maximum and the traceback an alignment that attains it."""
import itertools

import numpy as np

import match_align_ref as R

SIDES = range(0, 6)  # L1, L2: up to 252 matchings of a 5 x 5 interior


def matchings(l1, l2):
    """every monotone matching of an l1 x l2 interior as (rows, columns), matrix coordinates"""
    for k in range(min(l1, l2) + 1):
        for rows in itertools.combinations(range(1, l1 + 1), k):
            for cols in itertools.combinations(range(1, l2 + 1), k):
                yield rows, cols


def score(P, gamma, rows, cols):
    return sum(float(gamma) * float(P[i, j]) - 1.0 for i, j in zip(rows, cols))


def best_score(P, gamma):
    return max(score(P, gamma, rows, cols) for rows, cols in matchings(P.shape[0] - 2, P.shape[1] - 2))


def mate_score(P, gamma, mate, count):
    """the alignment `mate` describes, checked to be a monotone matching and scored in f64"""
    rows = [i for i in range(len(mate)) if mate[i] >= 0]
    cols = [int(mate[i]) for i in rows]
    assert len(rows) == count and all(1 <= i <= P.shape[0] - 2 for i in rows)
    assert all(1 <= j <= P.shape[1] - 2 for j in cols) and all(x < y for x, y in zip(cols, cols[1:]))
    return score(P, gamma, rows, cols)


def quantised_mats():
    rng = np.random.default_rng(40)
    return [R.quantised_probmat(rng, l1 + 2, l2 + 2) for l1, l2 in itertools.product(SIDES, SIDES) for _ in range(2)]


def random_mats():
    rng = np.random.default_rng(41)
    return [R.random_probmat(rng, l1 + 2, l2 + 2, density)
            for l1, l2 in itertools.product(SIDES, SIDES) for density in (0.4, 1.0)]


def test_quantised_matrices_reach_the_maximum_exactly(built):
    """cells in quarters, gammas 2 and 4: every candidate of the fill and every score of the search is
    exact, so the accuracy IS the maximum and the returned alignment scores exactly that"""
    from rna_algos_amd.pair_align import match_align
    positive = 0
    for P in quantised_mats():
        for gamma in (2.0, 4.0):
            mate, count, acc = match_align(P, gamma)
            best = best_score(P, gamma)
            assert float(acc) == best, (P.shape, gamma, acc, best)
            assert mate_score(P, gamma, mate, count) == best, (P.shape, gamma)
            positive += best > 0
    assert positive > 60  # (the search is not about empty alignments)


def test_random_matrices_reach_the_maximum(built):
    """gammas 1.5 and 8 on random cells: at most five matched cells, so at most ten f32 roundings of
    partial sums below 8 * 5: the accuracy and the score of the returned alignment are within 1e-5 of
    the maximum"""
    from rna_algos_amd.pair_align import match_align
    positive = 0
    for P in random_mats():
        for gamma in (1.5, 8.0):
            mate, count, acc = match_align(P, gamma)
            best = best_score(P, gamma)
            assert abs(float(acc) - best) <= 1e-5, (P.shape, gamma, acc, best)
            assert abs(mate_score(P, gamma, mate, count) - best) <= 1e-5, (P.shape, gamma)
            positive += best > 0
    assert positive > 60


def test_gamma_at_most_one_is_the_empty_alignment(built):
    """gamma * p - 1 <= 0 for every cell: no matching scores above the empty one, which is returned"""
    from rna_algos_amd.pair_align import match_align
    for P in random_mats() + quantised_mats():
        for gamma in (1.0, 0.5):
            assert best_score(P, gamma) == 0.0
            mate, count, acc = match_align(P, gamma)
            assert count == 0 and np.all(mate == -1) and np.float32(acc).view(np.uint32) == 0
