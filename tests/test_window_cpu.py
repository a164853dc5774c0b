"""Windowed local folding without a GPU: rnamc_window_plan against a brute-force window list, the
argument checks of rnamc_bpp_windowed / _multi that precede any device work, the Python result
class and the local_fold CLI's arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rnamc_bpp_windowed", "rnamc_bpp_windowed_multi"]


def brute_windows(n, w, s):
    """the window list as include/rnamc.h words it -> (starts, window length)"""
    if n <= w:
        return [0], n
    starts = []
    x = 0
    while x + w <= n:
        starts.append(x)
        x += s
    if starts[-1] + w < n:
        starts.append(n - w)
    return starts, w


def plan_raw(n, w, s, span, cap=None):
    """rnamc_window_plan itself -> (status, count, band, starts)"""
    from rna_algos_amd import _lib
    L = _lib.lib()
    count, band = C.c_uint64(2 ** 63), C.c_uint32(0xffffffff)
    if cap is None:
        st = L.rnamc_window_plan(n, w, s, span, C.byref(count), C.byref(band), None, 0)
        return st, count.value, band.value, None
    starts = np.full(max(cap, 1), 2 ** 63, np.uint64)
    st = L.rnamc_window_plan(n, w, s, span, C.byref(count), C.byref(band), starts.ctypes.data, cap)
    return st, count.value, band.value, starts


@pytest.mark.parametrize("n", [1, 4, 5, 64, 65, 300])
@pytest.mark.parametrize("w", [1, 5, 64, 65, 400])
def test_window_plan_matches_brute_force(built, n, w):
    from rna_algos_amd import _lib
    from rna_algos_amd.mccaskill_algo import window_plan
    for s in (1, 3, w, w + 7):
        want, wl = brute_windows(n, w, s)
        for span in (0, 1, 7, w, w + 1):
            st, count, band, _ = plan_raw(n, w, s, span)
            assert st == _lib.OK and count == len(want), (n, w, s, span)
            assert band == min(x for x in (w, n, span) if x), (n, w, s, span)
            st, count, band2, starts = plan_raw(n, w, s, span, cap=len(want))
            assert st == _lib.OK and count == len(want) and band2 == band
            assert starts[:count].tolist() == want, (n, w, s)
            if n > w:
                assert int(starts[count - 1]) + w == n
            assert all(0 <= a and a + wl <= n for a in want)
            if len(want) > 1:  # too small: INVALID_ARG, the count still set, nothing written
                st, count, _, small = plan_raw(n, w, s, span, cap=len(want) - 1)
                assert st == _lib.ERR_INVALID_ARG and count == len(want)
                assert np.all(small == 2 ** 63)
        got, band = window_plan(n, w, s, 7)
        assert got.dtype == np.uint64 and got.tolist() == want and band == min(w, n, 7)


def test_window_plan_argument_errors(built):
    from rna_algos_amd import _lib
    assert plan_raw(10, 0, 1, 0)[0] == _lib.ERR_INVALID_ARG
    assert plan_raw(10, 5, 0, 0)[0] == _lib.ERR_INVALID_ARG
    assert plan_raw(10, 65536, 1, 0)[0] == _lib.ERR_INVALID_ARG
    assert plan_raw(0, 5, 1, 0)[0] == _lib.ERR_EMPTY_SEQ
    assert plan_raw(2 ** 31, 5, 1, 0)[0] == _lib.ERR_INVALID_ARG
    st, count, band, _ = plan_raw(2 ** 31 - 1, 65535, 2 ** 32 - 1, 0)
    assert st == _lib.OK and count == 2 and band == 65535
    assert _lib.lib().rnamc_window_plan(10, 5, 1, 0, None, None, None, 0) == _lib.ERR_INVALID_ARG


def test_declared_bound_and_exported(built):
    from rna_algos_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rnamc.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, arity in (("rnamc_window_plan", 8), ("rnamc_bpp_windowed", 12), ("rnamc_bpp_windowed_multi", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert "#define RNAMC_ABI_VERSION 3u" in hdr


def _args(n=8, base=0, cons=None, window=5, stride=1, band=True, bases=True):
    b = np.full(max(n, 1), base, np.uint8)
    out = np.zeros(max(n, 1) * 8, np.float32)
    return (b, out), [b.ctypes.data if bases else None, n, cons, window, stride, 0, 0, 0,
                      out.ctypes.data if band else None, None, None]


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_is_invalid(built, name):
    from rna_algos_amd import _lib
    keep, args = _args()
    assert getattr(_lib.lib(), name)(None, *args) == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks_precede_the_handle(built, name):
    """window 0, stride 0, a window above 65 535, n = 0, a bad base, a bracket in the constraint and a NULL
    band_prob or bases are refused before the context or pool is looked at: the handle is a block of zeros"""
    from rna_algos_amd import _lib
    L = _lib.lib()
    entry = getattr(L, name)
    dummy = C.create_string_buffer(1 << 16)
    handle = C.cast(dummy, C.c_void_p)
    for kw, want in ((dict(window=0), _lib.ERR_INVALID_ARG), (dict(stride=0), _lib.ERR_INVALID_ARG),
                     (dict(window=65536), _lib.ERR_INVALID_ARG), (dict(n=0), _lib.ERR_EMPTY_SEQ),
                     (dict(base=4), _lib.ERR_INVALID_BASE), (dict(band=False), _lib.ERR_INVALID_ARG),
                     (dict(bases=False), _lib.ERR_INVALID_ARG)):
        keep, args = _args(**kw)
        assert entry(handle, *args) == want, kw
    for cons, pos in ((b"...(....", 3), (b".....)..", 5), (b"..|.....", 2), (b".x<>.\0..", 5)):
        keep, args = _args(cons=cons)
        assert entry(handle, *args) == _lib.ERR_INVALID_ARG, cons
        assert b"position %d" % pos in L.rnamc_last_error(), cons


def test_window_chunk_knob_is_declared():
    src = open(os.path.join(ROOT, "rna_algos_amd", "csrc", "rnamc_ctx.cpp")).read()
    assert '"window_chunk_nt"' in src
    assert '"window_chunk_nt"' in open(os.path.join(ROOT, "include", "rnamc.h")).read()


def test_result_class_on_a_hand_made_band():
    from rna_algos_amd.mccaskill_algo import WindowedBpp
    band = np.full((6, 4), -1.0, np.float32)
    band[0, 3] = 0.5
    band[2, 1] = 0.25
    band[1, 1] = 0.0078125
    band[1, 3] = 1.0
    band[0, 2] = 0.0
    res = WindowedBpp(band, np.zeros(6, np.float32), np.zeros(3, np.float32), np.array([0, 1, 2], np.uint64))
    assert res.n == 6 and res.band_width == 4 and res.band is band
    i, j, p = res.pairs()
    assert i.tolist() == [1, 2, 0, 0, 1] and j.tolist() == [2, 3, 2, 3, 4]  # span ascending, then i
    assert p.dtype == np.float32 and p.tolist() == [0.0078125, 0.25, 0.0, 0.5, 1.0]
    i, j, p = res.pairs(0.01)
    assert i.tolist() == [2, 0, 1] and j.tolist() == [3, 3, 4] and p.tolist() == [0.25, 0.5, 1.0]
    assert res.to_dict() == {(1, 2): 0.0078125, (2, 3): 0.25, (0, 2): 0.0, (0, 3): 0.5, (1, 4): 1.0}
    assert res.to_dict(0.5) == {(0, 3): 0.5, (1, 4): 1.0}
    assert res.to_dict(2.0) == {}


def test_mirrors_exist():
    from rna_algos_amd import mccaskill_algo as M
    assert callable(M.mccaskill_algo_windowed) and callable(M.window_plan)
    assert callable(M.Context.bpp_windowed) and callable(M.Pool.bpp_windowed)
    src = open(os.path.join(ROOT, "bindings", "rust", "mccaskill_algo.rs")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for name in ("rnamc_window_plan", "rnamc_bpp_windowed", "rnamc_bpp_windowed_multi"):
        assert "fn " + name + "(" in code
    hpp = open(os.path.join(ROOT, "include", "rna_algos", "mccaskill_algo.hpp")).read()
    assert "rnamc_bpp_windowed_multi" in hpp


def test_local_fold_arguments():
    from rna_algos_amd.bin import local_fold as cli
    a = cli.parse_args(["-i", "in.fa", "-o", "out.dat", "-w", "200"])
    assert (a.window, a.max_bp_span, a.stride, a.min_bpp) == (200, 0, 1, 0.01)
    assert not a.uses_contra_model and not a.allows_short_hairpins and a.constraints is None
    a = cli.parse_args(["-i", "in.fa", "-o", "out.dat", "-w", "200", "-l", "150", "--stride", "10", "--min-bpp", "0",
                        "-c", "-s", "--constraints", "c.fa", "--synthetic-tables", "3"])
    assert (a.window, a.max_bp_span, a.stride, a.min_bpp) == (200, 150, 10, 0.0)
    assert a.uses_contra_model and a.allows_short_hairpins and a.constraints == "c.fa" and a.synthetic_tables == 3
    for bad in (["-w", "0"], ["-w", "65536"], ["-w", "9", "--stride", "0"], ["-w", "9", "--min-bpp", "nan"],
                ["-w", "9", "-l", "-1"], []):
        with pytest.raises(SystemExit):
            cli.parse_args(["-i", "in.fa", "-o", "out.dat"] + bad)


def test_local_fold_rejects_brackets_and_formats_triples():
    from rna_algos_amd.bin import _constraints, local_fold as cli
    from rna_algos_amd.mccaskill_algo import WindowedBpp
    cli.check_no_brackets(["..x<>..", "...."])
    with pytest.raises(_constraints.ConstraintFileError, match="record 1, position 2"):
        cli.check_no_brackets(["....", "..(.)."])
    band = np.full((5, 4), -1.0, np.float32)
    band[0, 3], band[2, 1], band[1, 1] = 0.5, 0.25, 0.001
    res = WindowedBpp(band, np.zeros(5, np.float32), np.zeros(1, np.float32), np.zeros(1, np.uint64))
    assert cli.pairs2str(res, 0.01) == "2,3,0.25 0,3,0.5 "
    assert cli.pairs2str(res, 0.0) == "1,2,0.001 2,3,0.25 0,3,0.5 "
