"""CPU: the argument checks of rnamc_mfe_batch (they come before any use of the context or the
device), the mfe_fold CLI's argument parsing, and the f64 restatement (mfe_ref) against the
exhaustive maximum over every nested structure, scored by rnamc_structure_score."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from mfe_ref import mfe_ref

MODELS = [(False, False), (True, False), (True, True)]  # (contra, allows_short_hairpins)
CANON = {(0, 3), (3, 0), (1, 2), (2, 1), (2, 3), (3, 2)}


def call(n_seqs, bases, offsets, structs=True, ctx=True):
    from rna_algos_amd import _lib
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    rows = np.zeros(max(int(offsets[-1]) if offsets.size else 1, 1), np.uint8)
    dummy = np.zeros(64, np.uint8)  # never dereferenced: every check below returns first
    return _lib.lib().rnamc_mfe_batch(dummy.ctypes.data if ctx else None, n_seqs,
                                      bases.ctypes.data if bases.size else None, offsets.ctypes.data,
                                      0, 0, rows.ctypes.data if structs else None, None, None)


def test_argument_checks(built):
    from rna_algos_amd import _lib
    ok = [0, 1, 2, 3, 0, 1]
    assert call(1, ok, [0, 6], ctx=False) == _lib.ERR_INVALID_ARG
    assert call(2, ok, [0, 4, 2]) == _lib.ERR_INVALID_ARG          # decreasing offsets
    assert call(2, ok, [0, 3, 3]) == _lib.ERR_EMPTY_SEQ
    assert call(1, np.zeros(65536, np.uint8), [0, 65536]) == _lib.ERR_SEQ_TOO_LONG
    assert call(1, [0, 1, 4, 2], [0, 4]) == _lib.ERR_INVALID_BASE
    assert call(1, ok, [0, 6], structs=False) == _lib.ERR_INVALID_ARG
    # order: the empty sequence is found before a bad base of a later one, and both before NULL
    # structs
    assert call(2, [0, 1, 9], [0, 0, 3], structs=False) == _lib.ERR_EMPTY_SEQ
    assert call(1, [9], [0, 1], structs=False) == _lib.ERR_INVALID_BASE
    assert call(0, np.zeros(0, np.uint8), [0], structs=False) == _lib.OK


def test_cli_arguments():
    from rna_algos_amd.bin import mfe_fold
    a = mfe_fold.parse_args(["-i", "in.fa", "-o", "out.txt"])
    assert (a.input_file_path, a.output_file_path, a.uses_contra_model, a.allows_short_hairpins,
            a.synthetic_tables) == ("in.fa", "out.txt", False, False, None)
    a = mfe_fold.parse_args(["-i", "x", "-o", "y", "-c", "-s", "--synthetic-tables", "3"])
    assert a.uses_contra_model and a.allows_short_hairpins and a.synthetic_tables == 3
    with pytest.raises(SystemExit):
        mfe_fold.parse_args(["-o", "y"])


def nested_structures(seq):
    n = len(seq)
    memo = {}

    def rec(i, j):
        if i > j:
            return [""]
        if (i, j) in memo:
            return memo[(i, j)]
        out = ["." + s for s in rec(i + 1, j)]
        for k in range(i + 1, j + 1):
            if (int(seq[i]), int(seq[k])) in CANON:
                for a in rec(i + 1, k - 1):
                    for b in rec(k + 1, j):
                        out.append("(" + a + ")" + b)
        memo[(i, j)] = out
        return out

    return rec(0, n - 1)


def structure_score(params, seq, db, contra, short):
    from rna_algos_amd import _lib
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    out = C.c_double()
    _lib.check(_lib.lib().rnamc_structure_score(params.ptr, seq.ctypes.data, len(seq), db.encode(),
                                                int(contra), int(short), C.byref(out)))
    return out.value


@pytest.mark.parametrize("contra,short", MODELS)
def test_mfe_ref_against_enumeration(params, contra, short):
    for k in range(6):
        seq = O.splitmix_seq(9 + k, 5100 + k)
        best = max(structure_score(params, seq, db, contra, short) for db in nested_structures(seq))
        m, db = mfe_ref(params, seq, contra, short)
        assert abs(m - best) <= 1e-4 * max(1.0, abs(best)), (k, m, best)
        assert abs(structure_score(params, seq, db, contra, short) - m) <= 1e-4 * max(1.0, abs(m))
