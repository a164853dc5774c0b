"""rnamc_bpp_batch_sparse without a GPU: the declarations, the argument checks that precede any
device work, the Python helper class, the CLI's flag and the Rust shim's new function."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rnamc_bpp_batch_sparse", "rnamc_bpp_batch_sparse_multi"]


def _args(min_prob=0.0, lists=3, start=True, base=0, cons=None):
    bases = np.full(8, base, np.uint8)
    offsets = np.array([0, 8], np.uint64)
    start_a, count = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    pi, pj, pp = np.zeros(36, np.uint32), np.zeros(36, np.uint32), np.zeros(36, np.float32)
    total = C.c_uint64(0)
    keep = (bases, offsets, start_a, count, pi, pj, pp, total)
    ptrs = [pi.ctypes.data, pj.ctypes.data, pp.ctypes.data][:lists] + [None] * (3 - lists)
    return keep, [1, bases.ctypes.data, offsets.ctypes.data, cons, 0, 0, 0, min_prob,
                  start_a.ctypes.data if start else None, count.ctypes.data, *ptrs, 36, C.byref(total), None, None]


def test_declared_bound_and_exported(built):
    from rna_algos_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rnamc.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == 18 and "float min_prob" in m.group(1)
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert "#define RNAMC_ABI_VERSION 3u" in hdr


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_is_invalid(built, name):
    from rna_algos_amd import _lib
    keep, args = _args()
    assert getattr(_lib.lib(), name)(None, *args) == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks_precede_the_handle(built, name):
    """a bad min_prob, an incomplete set of arrays, arrays without pair_start, a NULL pairs_total and a bad
    base are refused before the context or pool is looked at: the handle is a block of zeros, never read"""
    from rna_algos_amd import _lib
    entry = getattr(_lib.lib(), name)
    dummy = C.create_string_buffer(1 << 16)
    handle = C.cast(dummy, C.c_void_p)
    for bad in (float("nan"), float("inf"), -0.25):
        keep, args = _args(min_prob=bad)
        assert entry(handle, *args) == _lib.ERR_INVALID_ARG, bad
    for lists in (1, 2):
        keep, args = _args(lists=lists)
        assert entry(handle, *args) == _lib.ERR_INVALID_ARG
    keep, args = _args(start=False)
    assert entry(handle, *args) == _lib.ERR_INVALID_ARG
    keep, args = _args()
    args[14] = None  # pairs_total
    assert entry(handle, *args) == _lib.ERR_INVALID_ARG
    keep, args = _args(base=7)
    assert entry(handle, *args) == _lib.ERR_INVALID_BASE


@pytest.mark.parametrize("name", NAMES)
def test_bad_constraint_fails_before_the_handle(built, name):
    """every constraint is compiled before the context or pool is looked at: an unbalanced bracket is
    refused, with its record and position, on a handle that is a block of zeros"""
    from rna_algos_amd import _lib
    L = _lib.lib()
    dummy = C.create_string_buffer(1 << 16)
    keep, args = _args(cons=b"((......")
    assert getattr(L, name)(C.cast(dummy, C.c_void_p), *args) == _lib.ERR_INVALID_ARG
    assert b"constraint of record 0" in L.rnamc_last_error()


def test_helper_class_round_trip():
    from rna_algos_amd.mccaskill_algo import SparseBpp, bpp_index, bpp_len
    n = 7
    i = np.array([0, 2, 1, 0], np.uint32)  # packed order: span ascending, then i
    j = np.array([3, 5, 5, 6], np.uint32)
    p = np.array([0.5, 0.125, 0.25, 1.0], np.float32)
    paired = np.arange(n, dtype=np.float32)
    sp = SparseBpp(n, i, j, p, paired)
    assert len(sp) == 4 and sp.n == n and sp.paired_prob is paired
    assert sp.to_dict() == {(0, 3): 0.5, (2, 5): 0.125, (1, 5): 0.25, (0, 6): 1.0}
    m = sp.dense()
    assert m.n == n and m.packed.dtype == np.float32 and m.packed.shape == (bpp_len(n),)
    want = np.full(bpp_len(n), -1.0, np.float32)
    for a, b, q in zip(i, j, p):
        want[bpp_index(n, int(a), int(b))] = q
    assert np.array_equal(m.packed, want)
    assert m.sparse() == sp.to_dict()
    empty = SparseBpp(1, i[:0], j[:0], p[:0], paired[:1])
    assert empty.to_dict() == {} and np.array_equal(empty.dense().packed, np.array([-1.0], np.float32))


def test_mirrors_exist():
    from rna_algos_amd import mccaskill_algo as M
    assert callable(M.mccaskill_algo_batch_sparse)
    assert callable(M.Context.bpp_batch_sparse) and callable(M.Pool.bpp_batch_sparse)
    assert M.SPARSE_PAIRS_PER_NT >= 1


def test_cli_min_bpp_is_parsed():
    from rna_algos_amd.bin import mccaskill_algo as cli
    assert cli.parse_args(["-i", "in.fa", "-o", "out"]).min_bpp is None
    assert cli.parse_args(["-i", "in.fa", "-o", "out", "--min-bpp", "0.01"]).min_bpp == 0.01
    assert cli.parse_args(["-i", "in.fa", "-o", "out", "--min-bpp", "0"]).min_bpp == 0.0
    for bad in ("-0.5", "nan", "inf"):
        with pytest.raises(SystemExit):
            cli.parse_args(["-i", "in.fa", "-o", "out", "--min-bpp", bad])


def test_cli_sparse_text_is_ascending():
    from rna_algos_amd.bin.mccaskill_algo import sparse2str
    from rna_algos_amd.mccaskill_algo import SparseBpp
    sp = SparseBpp(7, np.array([0, 2, 1, 0], np.uint32), np.array([3, 5, 5, 6], np.uint32),
                   np.array([0.5, 0.125, 0.25, 1.0], np.float32), np.zeros(7, np.float32))
    assert sparse2str(sp) == "0,3,0.5 0,6,1 1,5,0.25 2,5,0.125 "


def test_rust_shim_has_the_function():
    src = open(os.path.join(ROOT, "bindings", "rust", "mccaskill_algo.rs")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "pub fn mccaskill_algo_batch_sparse<T>" in code
    assert "fn rnamc_bpp_batch_sparse_multi(" in code
