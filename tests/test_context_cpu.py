"""Structural context profiles without a GPU: the f64 replay of the sums
against the exhaustive enumeration, the argument checks that precede any device work, the
declarations, and the CLI's text format."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rnamc_context_profile_batch", "rnamc_context_profile_batch_multi")
TURNER, CONTRA, SHORT = (False, False), (True, False), (True, True)
SEVENTEEN = "GGACAAAGACAAAGACC"
# (record, (contra, allows_short_hairpins)); the six SplitMix records go round the three models
FIXED = [(SEVENTEEN, TURNER), (SEVENTEEN, CONTRA), ("GGCGAAAGCAGCGAAAGCACC", TURNER),
         ("GGCGAAAGCAGCGAAAGCACC", CONTRA), ("GGACGACGAACC", SHORT)]
SPLITMIX = [(14, 7101, TURNER), (15, 7102, CONTRA), (16, 7103, SHORT), (14, 7104, CONTRA), (15, 7105, SHORT),
            (16, 7106, TURNER)]
# the constrained case: a bracket pair, an x run and a span limit on the 17-mer
CONS, SPAN = ".(........xx...).", 15


def _tables(name):
    import table_sets
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(1) if name == "synthetic1" else table_sets.ZERO()


def _bpp_err(packed, pp):
    import context_ref as R
    d = R._dense(packed, pp.shape[0])
    d[d < 0] = 0
    np.fill_diagonal(d, 0)
    return float(np.abs(d - pp).max())


@functools.lru_cache(None)
def cases(tables_name):
    """[(label, enumerated profile, replayed profile, |oracle bpp - enumerated bpp|)], computed once"""
    import context_ref as R
    from rna_algos_amd.utils import bytes2seq
    T = _tables(tables_name)
    recs = [(s, bytes2seq(s), m) for s, m in FIXED]
    recs += [(f"splitmix({n},{seed})", O.splitmix_seq(n, seed), m) for n, seed, m in SPLITMIX]
    out = []
    for label, seq, (contra, short) in recs:
        e, pp, _ = R.enumerate_profile(seq, contra, short, T)
        r = R.replay_profile(seq, contra, short, T)
        packed, _ = O.bpp(T.ptr, seq, contra, short)
        out.append(((label, contra, short), e, r, _bpp_err(packed, pp)))
    return out


def bound(tables_name):
    """8 x the largest |oracle bpp - enumerated bpp| of the same inputs (the measured ratio of the
    profile's error to it was at most 3.3; the margin covers inputs not tried)"""
    return 8.0 * max(c[3] for c in cases(tables_name))


@pytest.mark.parametrize("tables_name", ["synthetic1", "zero"])
def test_replay_matches_enumeration(built, tables_name):
    b = bound(tables_name)
    assert 0 < b < 1e-3
    worst = 0.0
    for label, e, r, _ in cases(tables_name):
        err = float(np.abs(r - e).max())
        print(tables_name, label, "max |replay - enumeration| %.2e" % err, "bound %.2e" % b)
        worst = max(worst, err)
        assert err <= b, (label, err, b)
        assert np.abs(e.sum(axis=0) - 1).max() < 1e-12
    print("worst", worst, "ratio to the bpp error", worst / (b / 8))


@pytest.mark.parametrize("model", [TURNER, CONTRA, SHORT])
def test_sparse_replay_equals_the_dense_one_and_model_error_is_within_the_gpu_bound(built, model):
    """replay_profile walks the closing pairs with p > 0 alone; replay_profile_dense is its first form off
    the list of every 2-loop.  Equal to 1e-12 on every input of the GPU test and of this file (another
    order of the same f64 sums: 1.4e-14 measured).  And D, the largest |device_arith replay - f64
    replay| over rows 0 .. 4, on the GPU test's inputs up to n = 130 stays within that test's bound of
    four times the 6.07e-8 measured on the device: the model of the device's arithmetic and the old
    measurement cannot drift apart unnoticed."""
    import context_ref as R
    import test_gpu_context as G
    from rna_algos_amd.utils import bytes2seq
    contra, short = model
    inputs = [(tn, label, seq, mask) for tn, label, seq, _, mask in G.replay_inputs()]
    for tn in ("synthetic1", "zero"):
        inputs += [(tn, s, bytes2seq(s), None) for s in sorted({s for s, _ in FIXED})]
        inputs += [(tn, f"splitmix({n},{seed})", O.splitmix_seq(n, seed), None) for n, seed, _ in SPLITMIX]
    from constraint_masks import allowed_matrix
    inputs.append(("zero", CONS, bytes2seq(SEVENTEEN), allowed_matrix(CONS, SPAN)))
    worst, pairs = 0.0, []
    for tn, label, seq, mask in inputs:
        T = _tables(tn)
        dense = R.replay_profile_dense(seq, contra, short, T, mask)
        r, d = R.replay_both(seq, contra, short, T, mask)
        err = float(np.abs(r - dense).max())
        worst = max(worst, err)
        assert err <= 1e-12, (tn, label, err)
        if len(seq) <= 130:
            pairs.append((r, d))
    D = R.model_error(pairs)
    print(model, "worst |sparse - dense| %.2e" % worst, "D %.2e" % D, "bound %.2e" % G.BOUND)
    assert 0 < D <= G.BOUND


def test_device_arithmetic_model_rounds_as_stated():
    """the two primitives of device_arith: quanta to nearest with ties to even, the cap, nothing for a
    term that is not positive; the exponent rounded to f32 before the f32 exponential"""
    import context_ref as R
    q = R._quant(np.array([0.5, 1.5, 2.5, 2.0 ** 46, -1.0, 0.0, np.nan]) / R.QUANTUM)
    assert q.tolist() == [0, 2, 2, 2 ** 45, 0, 0, 0]
    x = 1.0 + 2.0 ** -30  # rounds to 1 in f32
    assert R._exp32(np.array([x]))[0] == float(np.exp(np.float32(1.0)))
    assert R.MIN_P == 2.0 ** -45 and R.QUANTUM == 2.0 ** 44


def test_every_row_carries_mass_under_the_zero_tables(built):
    """not vacuous: by the enumeration every one of the six rows reaches 0.05 at some base of the 17-mer"""
    (label, e, _, _) = cases("zero")[0]
    assert label[0] == SEVENTEEN
    print(np.round(e.max(axis=1), 3))
    assert (e.max(axis=1) >= 0.05).all(), e.max(axis=1)


@pytest.mark.parametrize("model", [TURNER, CONTRA])
def test_constrained_replay_matches_filtered_enumeration(built, model):
    import context_ref as R
    from constraint_masks import allowed_matrix
    from rna_algos_amd.utils import bytes2seq
    contra, short = model
    T = _tables("zero")
    seq = bytes2seq(SEVENTEEN)
    mask = allowed_matrix(CONS, SPAN)
    e, pp, _ = R.enumerate_profile(seq, contra, short, T, CONS, SPAN)
    free, _, _ = R.enumerate_profile(seq, contra, short, T)
    assert np.abs(e - free).max() > 0.05  # the constraint binds
    assert pp[0, 16] == 0 and e[R.STEM, 10] == 0 and e[R.STEM, 11] == 0
    r = R.replay_profile(seq, contra, short, T, mask)
    packed, _ = O.bpp_masked(T.ptr, seq, contra, short, mask)
    b = 8.0 * _bpp_err(packed, pp)
    err = float(np.abs(r - e).max())
    print("max |replay - enumeration| %.2e" % err, "bound %.2e" % b)
    assert 0 < b < 1e-3 and err <= b


def test_classify():
    import context_ref as R
    B, E, H, I, M, S = range(6)
    assert R.classify("..((...))..") == [E, E, S, S, H, H, H, S, S, E, E]
    assert R.classify("(.((...)))") == [S, B, S, S, H, H, H, S, S, S]
    assert R.classify("(.(...)..)") == [S, I, S, H, H, H, S, I, I, S]
    assert R.classify("(.(...)(...).)") == [S, M, S, H, H, H, S, S, H, H, H, S, M, S]


def test_declared_bound_and_exported(built):
    from rna_algos_amd import _lib
    from rna_algos_amd import mccaskill_algo as M
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rnamc.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == 10
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 10
    assert "rnamc_context_profile_stats" in _lib.SYMBOLS and hasattr(L, "rnamc_context_profile_stats")
    assert M.CONTEXTS == ("bulge", "exterior", "hairpin", "internal", "multibranch", "stem")
    for obj in (M.Context, M.Pool):
        assert callable(getattr(obj, "context_profile_batch"))
    assert callable(M.context_profile_batch) and callable(M.context_profile)
    mk = open(os.path.join(ROOT, "rna_algos_amd", "csrc", "Makefile")).read()
    assert "rnamc_context.hip" in mk and "rnamc_entries_context.cpp" in mk
    shim = open(os.path.join(ROOT, "bindings", "rust", "mccaskill_algo.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "rna_algos", "mccaskill_algo.hpp")).read()
    for name in NAMES:
        assert "fn " + name + "(" in shim
    assert "rnamc_context_profile_batch(" in hpp


def _args(n=8, base=0, cons=None, span=0, bases=True, profile=True, n_seqs=1):
    b = np.full(max(n, 1), base, np.uint8)
    off = np.array([0, n], np.uint64)
    out = np.zeros(6 * max(n, 1), np.float32)
    return (b, off, out), [n_seqs, b.ctypes.data if bases else None, off.ctypes.data, cons, span, 0, 0,
                           out.ctypes.data if profile else None, None]


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_is_invalid(built, name):
    from rna_algos_amd import _lib
    keep, args = _args()
    assert getattr(_lib.lib(), name)(None, *args) == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks_precede_the_handle(built, name):
    """a bad base, an empty record, a record above 65 535, NULL bases, a NULL profile and a malformed
    constraint are refused before the context or pool is looked at: the handle is a block of zeros"""
    from rna_algos_amd import _lib
    L = _lib.lib()
    entry = getattr(L, name)
    dummy = C.create_string_buffer(1 << 16)
    handle = C.cast(dummy, C.c_void_p)
    for kw, want in ((dict(bases=False), _lib.ERR_INVALID_ARG), (dict(profile=False), _lib.ERR_INVALID_ARG),
                     (dict(n=0), _lib.ERR_EMPTY_SEQ), (dict(base=4), _lib.ERR_INVALID_BASE),
                     (dict(n=65536), _lib.ERR_SEQ_TOO_LONG)):
        keep, args = _args(**kw)
        assert entry(handle, *args) == want, kw
    for cons, pos in ((b"...(....", 3), (b".....)..", 5), (b"..|.....", 2), (b"((....).", 0)):
        keep, args = _args(cons=cons)
        assert entry(handle, *args) == _lib.ERR_INVALID_ARG, cons
        assert b"position %d" % pos in L.rnamc_last_error(), cons


def test_pool_without_contexts_is_invalid(built):
    from rna_algos_amd import _lib
    dummy = C.create_string_buffer(1 << 16)
    keep, args = _args(cons=b"(......)")
    assert _lib.lib().rnamc_context_profile_batch_multi(C.cast(dummy, C.c_void_p), *args) == _lib.ERR_INVALID_ARG


def test_stats_block_keeps_its_size_and_the_accessor_checks_its_arguments(built):
    from rna_algos_amd import _lib
    L = _lib.lib()
    assert "launches_context" not in [f for f, _ in _lib.BatchStats._fields_]
    n, ms = C.c_uint64(1), C.c_double(1.0)
    assert L.rnamc_context_profile_stats(None, C.byref(n), C.byref(ms)) == _lib.ERR_INVALID_ARG


def test_cli_text_round_trip(built, tmp_path, monkeypatch):
    """CapR's text format on a stubbed profile: names, order, one blank line per record, every f32 back"""
    from rna_algos_amd.bin import context_profile as cli
    rng = np.random.default_rng(5)
    profs = [rng.random((6, n)).astype(np.float32) for n in (1, 7, 12)]
    profs[1][2, 3] = np.float32(1e-30)
    text = cli.format_profiles(profs)
    lines = text.split("\n")
    assert lines[0] == ">0" and [ln.split(" ")[0] for ln in lines[1:7]] == [
        "Bulge", "Exterior", "Hairpin", "Internal", "Multibranch", "Stem"] and lines[7] == "" and lines[8] == ">1"
    assert len(lines[10].split(" ")) == 1 + 7
    back = cli.parse_profiles(text)
    assert len(back) == 3 and all(np.array_equal(a, b) for a, b in zip(profs, back))
    # main(): the library entry stubbed, tables synthetic
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nGGGAAACCC\n>b\nACGU\n")
    seen = {}

    def stub(seqs, contra, short, tables, cons, span):
        seen["args"] = (len(seqs), contra, short, cons, span)
        return [np.full((6, len(s)), 0.125, np.float32) for s in seqs], np.zeros(len(seqs), np.float32)

    monkeypatch.setattr(cli, "context_profile_batch", stub)
    out = tmp_path / "profile.txt"
    assert cli.main(["-i", str(fa), "-o", str(out), "-c", "--synthetic-tables", "1", "--max-bp-span", "7"]) == 0
    assert seen["args"] == (2, True, False, None, 7)
    got = cli.parse_profiles(out.read_text())
    assert [g.shape for g in got] == [(6, 9), (6, 4)] and all((g == 0.125).all() for g in got)
