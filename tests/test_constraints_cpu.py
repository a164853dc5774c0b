"""CPU: hard constraints (include/rnamc.h).  The constraint parser and its errors, the pair
predicate (pair_allowed, rnamc_scoring.h; on the host through rnamc_constraint_check) exhaustively
against a plain restatement of the rules that tests crossing directly, is_compatible on random
structures, the argument checks of the constrained entries (before any device use) and the CLI
flags."""
import random

import numpy as np
import pytest

from rna_algos_amd import _lib
from rna_algos_amd import mccaskill_algo as M

MIN_SPAN = 5  # RNAMC_MIN_SPAN_HAIRPIN_CLOSE


def parse(c):
    """constraint string -> (bracket partner per position or None, list of constraint pairs)"""
    partner, stack, pairs = [None] * len(c), [], []
    for p, ch in enumerate(c):
        if ch == "(":
            stack.append(p)
        elif ch == ")":
            a = stack.pop()
            partner[a], partner[p] = p, a
            pairs.append((a, p))
    assert not stack
    return partner, pairs


def allowed(c, span, i, j):
    """The rules of include/rnamc.h, restated: crossing tested pair by pair (no enc)."""
    partner, pairs = parse(c)
    if span and j - i + 1 > span:
        return False
    if c[i] == "x" or c[j] == "x":
        return False
    if partner[i] is not None or partner[j] is not None:
        return partner[i] == j
    if c[i] == ">" or c[j] == "<":
        return False
    for a, b in pairs:
        if i < a < j < b or a < i < b < j:
            return False
    return True


def random_structure(rng, n, density=0.5):
    """a random nested dot-bracket string (pairs of any span)"""
    db, stack = [], []
    for p in range(n):
        r = rng.random()
        if stack and r < density * 0.5:
            stack.pop()
            db.append(")")
        elif r < density and p < n - 1:
            stack.append(p)
            db.append("(")
        else:
            db.append(".")
    while stack:  # openers never closed become dots
        db[stack.pop()] = "."
    return "".join(db)


def random_constraint(rng, n):
    """nested constraint pairs (adjacent and short ones included), x < > on some of the rest"""
    c = list(random_structure(rng, n, rng.choice([0.05, 0.15, 0.3])))
    for p in range(n):
        if c[p] == "." and rng.random() < 0.3:
            c[p] = rng.choice("x<>")
    return "".join(c)


def test_parser_errors(built):
    for bad, pos in [("((...)", 0), ("(...))", 5), (")(", 0), ("..|..", 2), ("..X..", 2),
                     ("..A..", 2), ("...{", 3), ("(.(.)", 0), (".)", 1)]:
        with pytest.raises(_lib.RnamcError) as e:
            M.check_constraint(bad)
        assert e.value.status == _lib.ERR_INVALID_ARG
        assert f"position {pos}" in str(e.value), (bad, str(e.value))
    with pytest.raises(_lib.RnamcError) as e:  # length differs from the sequence
        M.check_constraint("....", n=5)
    assert e.value.status == _lib.ERR_INVALID_ARG
    # valid: nesting, every character, constraint pairs of any span
    for ok in ["((..))", "(.(x).)<>", "()", "x" * 7, "<<..>>", "(<)..(>)", "."]:
        M.check_constraint(ok)


def test_entry_rejects_bad_records_before_device(built):
    """the constrained context entries validate the whole batch first: a bad record fails the call
    (record and position in rnamc_last_error) before the context is used (a dummy handle here, as in
    test_mfe_cpu; the pool entry, which needs real contexts, is covered in test_gpu_constraints)"""
    L = _lib.lib()
    bases = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], np.uint8)
    offsets = np.array([0, 4, 10], np.uint64)
    dummy = np.zeros(64, np.uint8)
    out_off = np.array([0, 10, 31], np.uint64)
    bpp = np.zeros(31, np.float32)
    rows = np.zeros(100, np.uint8)
    lz = np.zeros(2, np.float32)
    calls = {
        "bpp": lambda cons: L.rnamc_bpp_batch_constrained(dummy.ctypes.data, 2, bases.ctypes.data, offsets.ctypes.data,
                                                          cons, 0, 0, 0, bpp.ctypes.data, out_off.ctypes.data, None),
        "sample": lambda cons: L.rnamc_sample_batch_constrained(dummy.ctypes.data, 2, bases.ctypes.data,
                                                                offsets.ctypes.data, cons, 0, 0, 0, 3, 1,
                                                                rows.ctypes.data, None, None),
        "mfe": lambda cons: L.rnamc_mfe_batch_constrained(dummy.ctypes.data, 2, bases.ctypes.data, offsets.ctypes.data,
                                                          cons, 0, 0, 0, rows.ctypes.data, None, None),
        "logz": lambda cons: L.rnamc_log_partition_batch(dummy.ctypes.data, 2, bases.ctypes.data, offsets.ctypes.data,
                                                         cons, 0, 0, 0, lz.ctypes.data),
    }
    for cons, want in [(b"....(.(...", "record 1, position 2"), (b"..|.......", "record 0, position 2"),
                       (b"....)....(", "record 1, position 0")]:
        for name, call in calls.items():
            # a message of another kind first, so that the one read below is this call's own
            assert L.rnamc_constraint_check(b"|", 1, 0, None, None) == _lib.ERR_INVALID_ARG
            assert "record" not in L.rnamc_last_error().decode()
            assert call(cons) == _lib.ERR_INVALID_ARG, (name, cons)
            assert want in L.rnamc_last_error().decode(), (name, L.rnamc_last_error())


def test_entry_record_errors_and_check_order(built):
    """the five host-buffer entries share one record check and keep their own order of checks, all before
    the context is used (a dummy handle, as above): decreasing offsets, an empty record, a record above
    the length limit (decided from the offsets alone: its bases are all invalid here) and a base of 4;
    rnamc_mfe_batch_constrained tests a null `structs` before the constraints,
    rnamc_sample_batch_constrained its n_samples == 0 and `structs` after them"""
    L = _lib.lib()
    dummy = np.zeros(64, np.uint8)
    gam = np.array([0.5, 2.0], np.float32)
    rows = np.zeros(2 * 65536, np.uint8)
    vals = np.zeros(8, np.float32)
    bpp = np.zeros(64, np.float32)
    out_off = np.array([0, 10, 31], np.uint64)

    def entries(n_seqs, bases, offsets, cons=None, structs=rows.ctypes.data, n_samples=3):
        b, o = bases.ctypes.data, offsets.ctypes.data
        return {
            "bpp": lambda: L.rnamc_bpp_batch_constrained(dummy.ctypes.data, n_seqs, b, o, cons, 0, 0, 0,
                                                         bpp.ctypes.data, out_off.ctypes.data, None),
            "sample": lambda: L.rnamc_sample_batch_constrained(dummy.ctypes.data, n_seqs, b, o, cons, 0, 0, 0,
                                                               n_samples, 1, structs, None, None),
            "mfe": lambda: L.rnamc_mfe_batch_constrained(dummy.ctypes.data, n_seqs, b, o, cons, 0, 0, 0, structs,
                                                         None, None),
            "logz": lambda: L.rnamc_log_partition_batch(dummy.ctypes.data, n_seqs, b, o, cons, 0, 0, 0,
                                                        vals.ctypes.data),
            "centroid": lambda: L.rnamc_centroid_fold_batch(dummy.ctypes.data, n_seqs, b, o, cons, 0, 0, 0,
                                                            gam.ctypes.data, 2, structs, None, None, None, None,
                                                            None),
        }

    good = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], np.uint8)
    base4 = good.copy()
    base4[7] = 4
    cases = [
        ("decreasing offsets", 2, good, np.array([0, 6, 4], np.uint64), _lib.ERR_INVALID_ARG),
        ("empty record", 2, good, np.array([0, 4, 4], np.uint64), _lib.ERR_EMPTY_SEQ),
        ("record of 65536", 1, np.full(65536, 4, np.uint8), np.array([0, 65536], np.uint64),
         _lib.ERR_SEQ_TOO_LONG),
        ("base of 4", 2, base4, np.array([0, 4, 10], np.uint64), _lib.ERR_INVALID_BASE),
    ]
    for what, n_seqs, bases, offsets, want in cases:
        for name, call in entries(n_seqs, bases, offsets).items():
            assert call() == want, (what, name)
    # a record error comes before a constraint error
    for name, call in entries(2, base4, np.array([0, 4, 10], np.uint64), cons=b"....(.(...").items():
        assert call() == _lib.ERR_INVALID_BASE, name

    offsets = np.array([0, 4, 10], np.uint64)
    bad_cons = b"....(.(..."

    def fresh_message():  # a message of another kind first, so that the one read afterwards is the call's own
        assert L.rnamc_constraint_check(b"|", 1, 0, None, None) == _lib.ERR_INVALID_ARG
        assert "record" not in L.rnamc_last_error().decode()

    fresh_message()
    assert entries(2, good, offsets, cons=bad_cons, structs=None)["mfe"]() == _lib.ERR_INVALID_ARG
    assert "record" not in L.rnamc_last_error().decode()  # (the null `structs`, not the constraint)
    fresh_message()
    assert entries(2, good, offsets, cons=bad_cons, n_samples=0)["sample"]() == _lib.ERR_INVALID_ARG
    assert "record 1, position 2" in L.rnamc_last_error().decode()
    fresh_message()
    assert entries(2, good, offsets, cons=bad_cons, structs=None)["sample"]() == _lib.ERR_INVALID_ARG
    assert "record 1, position 2" in L.rnamc_last_error().decode()


def test_python_length_mismatch(built):
    """a string whose length differs from its sequence fails before any device use"""
    seqs = [np.array([0, 1, 2, 3, 0], np.uint8)]
    with pytest.raises(_lib.RnamcError) as e:
        M._constraint_bytes(["...."], [5])
    assert e.value.status == _lib.ERR_INVALID_ARG and "record 0" in str(e.value)
    with pytest.raises(_lib.RnamcError):
        M._constraint_bytes([".....", "....."], [5])
    assert M._constraint_bytes(None, [5]) is None
    assert M._constraint_bytes([None, None], [5, 3]) is None
    assert M._constraint_bytes([None, "x.."], [2, 3]) == b"..x.."
    del seqs


def test_pair_predicate_exhaustive(built):
    """every (i, j) of ~200 random constraint strings (n <= 40) and spans: pair_allowed, reached
    through a one-pair structure, equals the restatement"""
    rng = random.Random(11)
    checked = 0
    for t in range(200):
        n = rng.randint(2, 40)
        c = random_constraint(rng, n)
        span = rng.choice([0, 0, rng.randint(1, n + 2), rng.randint(2, MIN_SPAN)])
        for i in range(n):
            for j in range(i + 1, n):
                db = "." * i + "(" + "." * (j - i - 1) + ")" + "." * (n - 1 - j)
                assert M.is_compatible(db, c, span) == allowed(c, span, i, j), (c, span, i, j)
                checked += 1
    assert checked > 50000


def test_is_compatible_random_structures(built):
    rng = random.Random(12)
    n_true = 0
    for t in range(600):
        n = rng.randint(1, 40)
        c = random_constraint(rng, n)
        span = rng.choice([0, 0, rng.randint(1, n + 2)])
        db = random_structure(rng, n, rng.choice([0.1, 0.3, 0.6]))
        pt = parse(db)[1]
        want = all(allowed(c, span, i, j) for i, j in pt)
        assert M.is_compatible(db, c, span) == want, (db, c, span)
        n_true += want
    assert 50 < n_true < 590  # both outcomes are exercised


def test_constraint_special_cases(built):
    # a constraint pair (any bases: canonical or not is the model's business) admits itself and
    # pairs inside or outside it; its ends pair with each other only
    assert M.is_compatible("(.....)", "(.....)")
    assert M.is_compatible(".(...).", "(.....)")
    assert not M.is_compatible("(....).", "(.....)")
    assert not M.is_compatible("((...))", ".(....)")
    # crossing: (0, 4) crosses the constraint pair (2, 6); (0, 5) encloses (3, 4) and does not
    assert not M.is_compatible("(...)...", "..(...).")
    assert M.is_compatible("(....)..", "...()...")
    # nesting: pairs inside and outside a constraint pair, none across
    assert M.is_compatible("(.(...).)..(...)", ".(.....)........")
    # < pairs downstream only, > upstream only
    assert M.is_compatible("(...)", "<...>")
    assert not M.is_compatible("(...)", ">....")
    assert not M.is_compatible("(...)", "....<")
    # max_bp_span below the minimum span: no pair of the model's space is admitted
    assert not M.is_compatible("(...)", ".....", MIN_SPAN - 1)
    assert M.is_compatible(".....", ".....", 1)
    # None = no string; an all-dot string equals no string
    assert M.is_compatible("((...))", None) and M.is_compatible("((...))", ".......")
    # malformed structure / length mismatch
    for db, c in [("(..", "..."), ("...", "...."), ("..a", "...")]:
        with pytest.raises(_lib.RnamcError):
            M.is_compatible(db, c)


def test_malformed_structure_messages(built):
    """rnamc_constraint_check names the structure's fault and its position (not a stale message)"""
    L = _lib.lib()
    out = np.zeros(1, np.int32)
    for db, want in [(b"..)..", "structure position 2"), (b"(....", "structure position 0"),
                     (b"..a..", "structure position 2"), (b"...", "structure position 3"),
                     (b"......", "longer than n = 5")]:
        assert L.rnamc_constraint_check(b"|", 1, 0, None, None) == _lib.ERR_INVALID_ARG  # another message
        rc = L.rnamc_constraint_check(b".....", 5, 0, db, out.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int)))
        assert rc == _lib.ERR_INVALID_ARG, db
        assert want in L.rnamc_last_error().decode(), (db, L.rnamc_last_error())
    with pytest.raises(_lib.RnamcError) as e:
        M.is_compatible("(..", "...")
    assert "structure position 0" in str(e.value)


def test_cli_arguments(tmp_path):
    from rna_algos_amd.bin import accessibility, mccaskill_algo, mfe_fold, sample_fold
    for mod, extra in ((mfe_fold, []), (sample_fold, ["-n", "3"]), (mccaskill_algo, [])):
        a = mod.parse_args(["-i", "in.fa", "-o", "out.txt"] + extra)
        assert a.constraints is None and a.max_bp_span == 0
        a = mod.parse_args(["-i", "in.fa", "-o", "out.txt", "--constraints", "c.fa", "--max-bp-span", "150"]
                           + extra)
        assert a.constraints == "c.fa" and a.max_bp_span == 150
        with pytest.raises(SystemExit):
            mod.parse_args(["-i", "x", "-o", "y", "--max-bp-span", "-1"] + extra)
    a = accessibility.parse_args(["-i", "in.fa", "-o", "out.txt", "-w", "20", "-c", "-s"])
    assert (a.window, a.uses_contra_model, a.allows_short_hairpins) == (20, True, True)
    with pytest.raises(SystemExit):
        accessibility.parse_args(["-i", "in.fa", "-o", "out.txt"])
    with pytest.raises(SystemExit):
        accessibility.parse_args(["-i", "in.fa", "-o", "out.txt", "-w", "0"])


def test_cli_constraint_file_mismatch(built, tmp_path):
    """a record count or length mismatch of the constraint file: exit status 2 before any device use"""
    from rna_algos_amd.bin import mccaskill_algo, mfe_fold, sample_fold
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nGGGAAACCC\n>b\nGGGGAAAACCCC\n")
    bad_count = tmp_path / "c1.fa"
    bad_count.write_text(">a\n(.......)\n")
    bad_len = tmp_path / "c2.fa"
    bad_len.write_text(">a\n(.......)\n>b\n((...))\n")
    bad_char = tmp_path / "c3.fa"
    bad_char.write_text(">a\n(...|...)\n>b\n............\n")
    out = tmp_path / "out.txt"
    for mod, extra in ((mfe_fold, []), (sample_fold, ["-n", "2"]), (mccaskill_algo, [])):
        for cf in (bad_count, bad_len, bad_char):
            rc = mod.main(["-i", str(fa), "-o", str(out), "--synthetic-tables", "1", "--constraints", str(cf)]
                          + extra)
            assert rc == 2, (mod.__name__, cf)
            assert not out.exists()


def test_read_fasta_raw(tmp_path):
    from rna_algos_amd.utils import read_fasta_raw
    f = tmp_path / "c.fa"
    f.write_text(">r0 comment\n((..\n..))\n\n>r1\nx<>.\n")
    assert read_fasta_raw(str(f)) == [("r0", "((....))"), ("r1", "x<>.")]
