"""RNA-RNA duplex folding, host side: rnamc_duplex_score against the independent reference
(tests/duplex_ref.py), the reference's enumeration against its own recurrences, the argument checks
of rnamc_duplex_batch that precede any device work, the Python mirror's structure strings and the
CLI's parsing and output format."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import duplex_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rnamc_duplex_batch", "rnamc_duplex_batch_multi")

# small strand pairs: mixed bases, a GU-rich pair, single bases, all-canonical runs
SMALL = [("GGAUC", "GAUCC"), ("GUGU", "UGUG"), ("G", "C"), ("ACGUACG", "CGUACGU"), ("GGGGGG", "CCCCC"),
         ("A", "UUUUUUUU"), ("GCGCAUAU", "U")]


def _tables(params):
    from rna_algos_amd.utils import FoldScoreSets
    return {"synthetic": params, "zero": FoldScoreSets.new(0.0)}


def test_declared_bound_and_exported(built):
    from rna_algos_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rnamc.h")).read(), flags=re.S)
    L = _lib.lib()
    for name, arity in (("rnamc_duplex_batch", 17), ("rnamc_duplex_batch_multi", 17), ("rnamc_duplex_score", 10)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == arity
    assert "#define RNAMC_ABI_VERSION 3u" in hdr and L.rnamc_abi_version() == 3


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("tab", ["synthetic", "zero"])
def test_score_of_every_duplex_matches_the_reference(params, tab, contra):
    """rnamc_duplex_score of EVERY duplex of the small pairs against the oracle-built score: both are
    f64 sums of the same f32 loop scores -> 1e-9 relative"""
    from rna_algos_amd.duplex import duplex_score
    P = _tables(params)[tab]
    checked = 0
    for sa, sb in SMALL:
        a, b = R.encode(sa), R.encode(sb)
        sc = R.Scores(P, a, b, contra)
        en = R.Enumeration(sc)
        for chain, w in zip(en.chains, en.weights):
            got = duplex_score(a, b, list(chain), contra, P)
            assert abs(got - w) <= 1e-9 * max(1.0, abs(w)), (sa, sb, chain, got, w)
            assert abs(sc.chain_score(list(chain)) - w) <= 1e-12 * max(1.0, abs(w))
            checked += 1
    assert checked > 500


@pytest.mark.parametrize("contra", [False, True])
@pytest.mark.parametrize("tab", ["synthetic", "zero"])
def test_reference_enumeration_agrees_with_its_recurrences(params, tab, contra):
    P = _tables(params)[tab]
    for sa, sb in SMALL + [("AAAA", "CCC")]:
        sc = R.Scores(P, R.encode(sa), R.encode(sb), contra)
        en, rc = R.Enumeration(sc), R.Recurrences(sc)
        if en.count == 0:
            assert rc.log_z == -np.inf and rc.best == -np.inf and not rc.P.any()
            continue
        assert abs(en.log_z - rc.log_z) <= 1e-12 * max(1.0, abs(en.log_z))
        assert abs(en.best - rc.best) <= 1e-12 * max(1.0, abs(en.best))
        assert np.max(np.abs(en.P - rc.P)) <= 1e-12
        assert np.max(np.abs(en.pa - rc.pa)) <= 1e-12 and np.max(np.abs(en.pb - rc.pb)) <= 1e-12
        if tab == "zero":
            assert round(np.exp(en.log_z)) == en.count
            assert len(en.pick) == 1  # every duplex weighs 1: the tie rule names the first single pair


def test_zero_tables_count_and_loop_limit(built):
    """GG x C*36 under zero tables: one pair (2 * 36), or two pairs (0, j1), (1, j2) with
    b = j1 - j2 - 1 <= 30"""
    from rna_algos_amd.utils import FoldScoreSets
    sc = R.Scores(FoldScoreSets.new(0.0), R.encode("GG"), R.encode("C" * 36), False)
    want = 2 * 36 + sum(1 for j1 in range(36) for j2 in range(j1) if j1 - j2 - 1 <= 30)
    assert round(np.exp(R.Recurrences(sc).log_z)) == want


def test_score_outside_the_model_and_malformed_chains(params):
    from rna_algos_amd import _lib
    from rna_algos_amd.duplex import duplex_score
    a, b = R.encode("GGAUC"), R.encode("GAUCC")
    for contra in (False, True):
        assert duplex_score(a, b, [(0, 0)], contra, params) == -np.inf      # G-G: not canonical
        assert duplex_score(a, b, [(0, 4), (1, 0)], contra, params) == -np.inf  # second pair G-G
        assert np.isfinite(duplex_score(a, b, [(0, 4), (1, 3)], contra, params))
        la, lb = R.encode("GG"), R.encode("C" * 36)
        assert np.isfinite(duplex_score(la, lb, [(0, 31), (1, 0)], contra, params))   # b = 30
        assert duplex_score(la, lb, [(0, 32), (1, 0)], contra, params) == -np.inf     # b = 31
        for chain in ([], [(0, 4), (0, 3)], [(0, 3), (1, 3)], [(1, 3), (0, 4)], [(5, 0)], [(0, 5)]):
            with pytest.raises(_lib.RnamcError) as e:
                duplex_score(a, b, chain, contra, params)
            assert e.value.status == _lib.ERR_INVALID_ARG, chain
    with pytest.raises(_lib.RnamcError) as e:
        duplex_score(np.array([0, 4], np.uint8), b, [(0, 0)], False, params)
    assert e.value.status == _lib.ERR_INVALID_BASE
    with pytest.raises(_lib.RnamcError) as e:
        duplex_score(np.zeros(0, np.uint8), b, [(0, 0)], False, params)
    assert e.value.status == _lib.ERR_EMPTY_SEQ


def _args(n_a=5, n_b=4, base=1, bases=True, offsets=True, pair=(0, 1), pair_ptrs=True, probs_off=True,
          bound_off=True, struct_off=True):
    """arguments of rnamc_duplex_batch after the handle for ONE pair of two records"""
    seq = np.full(n_a + n_b, base, np.uint8)
    offs = np.array([0, n_a, n_a + n_b], np.uint64)
    pa, pb = np.array([pair[0]], np.uint32), np.array([pair[1]], np.uint32)
    cells, nt = max(n_a * n_b, 1), max(n_a + n_b, 1)
    probs, bound, logz = np.zeros(cells, np.float32), np.zeros(nt, np.float32), np.zeros(1, np.float32)
    structs, best = np.zeros(nt, np.uint8), np.zeros(1, np.float32)
    zero = np.zeros(2, np.uint64)
    keep = (seq, offs, pa, pb, probs, bound, logz, structs, best, zero)
    args = (2, seq.ctypes.data if bases else None, offs.ctypes.data if offsets else None, 1,
            pa.ctypes.data if pair_ptrs else None, pb.ctypes.data if pair_ptrs else None, 0,
            probs.ctypes.data, zero.ctypes.data if probs_off else None,
            bound.ctypes.data, bound.ctypes.data, zero.ctypes.data if bound_off else None,
            logz.ctypes.data, structs.ctypes.data, zero.ctypes.data if struct_off else None, best.ctypes.data)
    return keep, args


@pytest.mark.parametrize("name", NAMES)
def test_argument_checks_precede_the_handle(built, name):
    """NULL pointers, an output without its offsets, a pair index past the records, an empty strand and
    a bad base are refused before the context or pool is looked at: the handle is a block of zeros"""
    from rna_algos_amd import _lib
    L = _lib.lib()
    entry = getattr(L, name)
    dummy = C.create_string_buffer(1 << 16)
    handle = C.cast(dummy, C.c_void_p)
    for kw, want in ((dict(bases=False), _lib.ERR_INVALID_ARG), (dict(offsets=False), _lib.ERR_INVALID_ARG),
                     (dict(pair_ptrs=False), _lib.ERR_INVALID_ARG), (dict(probs_off=False), _lib.ERR_INVALID_ARG),
                     (dict(bound_off=False), _lib.ERR_INVALID_ARG), (dict(struct_off=False), _lib.ERR_INVALID_ARG),
                     (dict(pair=(0, 2)), _lib.ERR_INVALID_ARG), (dict(pair=(7, 1)), _lib.ERR_INVALID_ARG),
                     (dict(n_b=0), _lib.ERR_EMPTY_SEQ), (dict(n_a=0), _lib.ERR_EMPTY_SEQ),
                     (dict(base=4), _lib.ERR_INVALID_BASE)):
        keep, args = _args(**kw)
        assert entry(handle, *args) == want, kw
    keep, args = _args()
    assert entry(None, *args) == _lib.ERR_INVALID_ARG


def test_pool_without_contexts_is_invalid_and_no_pairs_is_ok(built):
    from rna_algos_amd import _lib
    L = _lib.lib()
    dummy = C.create_string_buffer(1 << 16)
    handle = C.cast(dummy, C.c_void_p)
    keep, args = _args()
    assert L.rnamc_duplex_batch_multi(handle, *args) == _lib.ERR_INVALID_ARG
    args = list(args)
    args[3] = 0  # n_pairs == 0: nothing to do, the context is never touched
    assert L.rnamc_duplex_batch(handle, *args) == _lib.OK


def test_structure_strings_round_trip(built):
    from rna_algos_amd.duplex import DuplexFold, pairs_structure, structure_pairs
    assert structure_pairs("((..(&)..))") == [(0, 4), (1, 3), (4, 0)]
    assert pairs_structure(5, 5, [(0, 4), (1, 3), (4, 0)]) == "((..(&)..))"
    assert structure_pairs("...&..") == []
    f = DuplexFold(3, 2, -np.inf, None, None, None, "...&..", -np.inf)
    assert f.pairs() == []
    with pytest.raises(ValueError):
        structure_pairs("((&)")


def test_cli_arguments_and_output_format(built, tmp_path, monkeypatch):
    """the CLI with a stubbed fold: every query against every target, queries outermost, one
    tab-separated line per pair that parse_line reads back; --probs writes one matrix per pair"""
    from rna_algos_amd.bin import duplex_fold as cli
    from rna_algos_amd.duplex import DuplexFold, pairs_structure
    args = cli.parse_args(["-q", "q.fa", "-t", "t.fa", "-o", "o.tsv"])
    assert (args.query_file_path, args.target_file_path, args.output_file_path) == ("q.fa", "t.fa", "o.tsv")
    assert not args.uses_contra_model and args.probs is None and args.synthetic_tables is None
    args = cli.parse_args(["-q", "q", "-t", "t", "-o", "o", "-c", "--probs", "d", "--synthetic-tables", "3"])
    assert args.uses_contra_model and args.probs == "d" and args.synthetic_tables == 3
    with pytest.raises(SystemExit):
        cli.parse_args(["-q", "q.fa", "-o", "o.tsv"])

    q, t = tmp_path / "q.fa", tmp_path / "t.fa"
    q.write_text(">q1\nGGAUC\n>q2\nAAA\n")
    t.write_text(">t1\nGAUCC\n>t2\nCCC\n>t3\nUU\n")
    seen = {}

    def stub(seqs, pairs, contra, tables, want_probs=True, want_best=True, ctx=None):
        seen.update(pairs=list(pairs), contra=contra, want_probs=want_probs, want_best=want_best,
                    lens=[len(s) for s in seqs])
        out = []
        for x, (a, b) in enumerate(pairs):
            na, nb = len(seqs[a]), len(seqs[b])
            chain = [(0, nb - 1)] if x % 2 == 0 else []
            out.append(DuplexFold(na, nb, 1.5 + x if chain else -np.inf,
                                  np.full((na, nb), 0.25, np.float32) if want_probs else None, None, None,
                                  pairs_structure(na, nb, chain), 0.125 * x if chain else -np.inf))
        return out

    monkeypatch.setattr(cli, "duplex_fold_batch", stub)
    out, pdir = tmp_path / "o.tsv", tmp_path / "p"
    assert cli.main(["-q", str(q), "-t", str(t), "-o", str(out), "-c", "--probs", str(pdir),
                     "--synthetic-tables", "1"]) == 0
    assert seen["pairs"] == [(0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4)]
    assert seen["contra"] and seen["want_probs"] and seen["want_best"] and seen["lens"] == [5, 3, 5, 3, 2]
    lines = out.read_text().splitlines()
    assert len(lines) == 6 and all(len(ln.split("\t")) == 7 for ln in lines)
    rows = [cli.parse_line(ln) for ln in lines]
    assert [(r[0], r[1]) for r in rows] == [("q1", "t1"), ("q1", "t2"), ("q1", "t3"), ("q2", "t1"), ("q2", "t2"),
                                            ("q2", "t3")]
    assert rows[0] == ("q1", "t1", 1.5, 0.0, 0, 4, "(....&....)")
    assert rows[1] == ("q1", "t2", -np.inf, -np.inf, -1, -1, ".....&...")
    assert rows[2][2:6] == (3.5, 0.25, 0, 1)
    assert sorted(os.listdir(pdir)) == ["0_0.npy", "0_1.npy", "0_2.npy", "1_0.npy", "1_1.npy", "1_2.npy"]
    assert np.load(pdir / "1_2.npy").shape == (3, 2)
    # without --probs no matrix is asked for
    assert cli.main(["-q", str(q), "-t", str(t), "-o", str(out), "--synthetic-tables", "1"]) == 0
    assert not seen["want_probs"] and not seen["contra"]
