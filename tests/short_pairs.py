"""Shared by the GPU tests that run allows_short_hairpins = 1 (CONTRAfold): with the flag the ensemble
holds pairs of span 1, 2 and 3 (j - i < 4), which no other setting produces.  A test first states, from
the oracle alone, that its input has such pairs in number (expected_short_pairs >= 1), then that the
result of the code under test contains them."""
import numpy as np

import oracle_lib as O

MODEL = (True, True)  # (uses_contra_model, allows_short_hairpins); (False, True) is (False, False) by construction


def diag_off(n, d):
    """first cell of diagonal d in a packed diagonal-major triangle of n rows"""
    return d * n - d * (d - 1) // 2


def short_cells(n):
    """the packed cells of span 1, 2 and 3"""
    return slice(diag_off(n, min(1, n)), diag_off(n, min(4, n)))


def expected_short_pairs(params, seq):
    """expected number of pairs with j - i < 4 per structure in the exact (f64) ensemble of the oracle"""
    ex, _ = O.exact_bpp(params.ptr, seq, True, True)
    cells = ex[short_cells(len(seq))]
    return float(cells[cells > 0].sum())


def assert_input_has_short_pairs(params, seqs):
    for seq in seqs:
        e = expected_short_pairs(params, seq)
        assert e >= 1.0, (len(seq), e)


def pairs_of(dot_bracket):
    """the (i, j) of a balanced dot-bracket string"""
    stack, out = [], []
    for q, ch in enumerate(dot_bracket):
        if ch == "(":
            stack.append(q)
        elif ch == ")":
            out.append((stack.pop(), q))
        else:
            assert ch == "."
    assert not stack
    return out


def short_present(packed, n):
    """number of present cells (p > -0.5) of span 1, 2, 3 in a packed triangle"""
    return int(np.count_nonzero(np.asarray(packed)[short_cells(n)] > -0.5))
