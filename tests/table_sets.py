"""Table sets for the tests that replace the tables of a live context (test_gpu_tables.py), pinned on the
CPU by test_table_sets_cpu.py.  Each set is a copy of FoldScoreSets.synthetic(1) ("A") changed in ONE block,
so that a cache a context failed to drop is singled out and the re-upload of the parameter block cannot
mask it:

  B_hp   Turner hairpin_scores_init (+ 1.5) and coeff_hairpin_len_extrapolation (-1.75 -> -0.5): what the
         kernels read only through the derived hairpin initiation table;
  B_len  what the tree-order 2-loop length tables are built from: Turner bulge_scores_init and
         interior_scores_init (+ 1.0), ninio_coeff (-> -0.4); CONTRAfold bulge_scores_len,
         interior_scores_len, interior_scores_symmetric, interior_scores_asymmetric (+ 0.25) and
         interior_scores_explicit (+ 0.3), accumulated;
  B_lim  the hairpin limits (4, 12, 13) and a full special-hairpin list of 64 entries, lengths cycling
         through 5 6 7 8 9 16, one entry scoring -inf followed by an entry with the same bases and a finite
         score (the reference returns at the FIRST match, and a -inf there falls through to the general
         formula: the duplicate must never be used);
  B_all  FoldScoreSets.synthetic(2);
  ZERO   FoldScoreSets.new(0.0): every structure weighs 1, exp(ln Z) is the number of structures.
"""
import functools

import numpy as np

# shapes (records, bases) of the replacement tests: 200 bases is the least that reaches the banded and the
# lane-per-cell forms of the tree-order sweep; records as entry_families.records
SMALL, LARGE = (3, 24), (4, 200)
ZERO_LENGTHS = (6, 11, 17, 24, 40, 80, 120, 160)
SPECIAL_LENS = (5, 6, 7, 8, 9, 16)
MAX_SPECIAL, MAX_SPECIAL_LEN = 64, 16
NEG_INF_ENTRY = 12  # (length 5; entry 13 repeats its bases)
HAIRPIN_LIMITS = (4, 12, 13)
PAIRS = [(0, 3), (1, 2), (2, 1), (2, 3), (3, 0), (3, 2)]

# the fields each set may differ from A in (accumulate() rewrites the cumulative forms)
FIELDS = {
    "B_hp": ["turner.hairpin_scores_init", "turner.coeff_hairpin_len_extrapolation"],
    "B_len": ["turner.bulge_scores_init", "turner.interior_scores_init", "turner.ninio_coeff",
              "contra.bulge_scores_len", "contra.interior_scores_len", "contra.interior_scores_symmetric",
              "contra.interior_scores_asymmetric", "contra.interior_scores_explicit",
              "contra.bulge_scores_len_cumulative", "contra.interior_scores_len_cumulative",
              "contra.interior_scores_symmetric_cumulative", "contra.interior_scores_asymmetric_cumulative"],
}
# (contra, allows_short_hairpins) of the models a set changes
MODELS = {"B_hp": [(False, False)], "B_len": [(False, False), (True, False)], "B_lim": [(False, False)],
          "B_all": [(False, False), (True, False)]}


def copy_of(P):
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets(_buf=P._buf.copy())


def special_block(P):
    """byte range of special_hairpin_scores, _seqs, _lens, num_special_hairpins and the three limits"""
    off, cnt = P._fields["turner.special_hairpin_scores"]
    assert cnt == MAX_SPECIAL
    return off, off + 4 * cnt + MAX_SPECIAL * MAX_SPECIAL_LEN + MAX_SPECIAL + 4 + 12


def special_list(P):
    """the special hairpins of a block -> list of (base codes, f32 score), and the three limits"""
    off, end = special_block(P)
    buf = P._buf
    seq_off = off + 4 * MAX_SPECIAL
    len_off = seq_off + MAX_SPECIAL * MAX_SPECIAL_LEN
    num, lo, hi, ext = (int(x) for x in buf[len_off + MAX_SPECIAL:end].view(np.uint32))
    scores = buf[off:seq_off].view(np.float32)
    out = [(buf[seq_off + MAX_SPECIAL_LEN * x:seq_off + MAX_SPECIAL_LEN * x + int(buf[len_off + x])].copy(),
            np.float32(scores[x])) for x in range(num)]
    return out, (lo, hi, ext)


def differing_bytes(P, Q):
    return np.nonzero(P._buf != Q._buf)[0]


def allowed_bytes(P, name):
    """mask of the bytes set `name` may differ from A in"""
    ok = np.zeros(len(P._buf), dtype=bool)
    if name == "B_lim":
        a, b = special_block(P)
        ok[a:b] = True
    for f in FIELDS.get(name, []):
        off, cnt = P._fields[f]
        ok[off:off + 4 * cnt] = True
    return ok


@functools.lru_cache(None)
def A():
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(1)


@functools.lru_cache(None)
def B_hp():
    P = copy_of(A())
    P.turner("hairpin_scores_init")[:] += np.float32(1.5)
    P.turner("coeff_hairpin_len_extrapolation")[0] = -0.5
    return P


@functools.lru_cache(None)
def B_len():
    P = copy_of(A())
    P.turner("bulge_scores_init")[:] += np.float32(1.0)
    P.turner("interior_scores_init")[:] += np.float32(1.0)
    P.turner("ninio_coeff")[0] = -0.4
    for f in ("bulge_scores_len", "interior_scores_len", "interior_scores_symmetric", "interior_scores_asymmetric"):
        P.field("contra." + f)[:] += np.float32(0.25)
    P.field("contra.interior_scores_explicit")[:] += np.float32(0.3)
    P.accumulate()
    return P


def special_entries(seed=64):
    """-> (seqs u8[64, 16], lens u8[64], scores f32[64]) of B_lim's list: distinct sequences but for entry
    NEG_INF_ENTRY + 1, which repeats entry NEG_INF_ENTRY; first and last base a canonical pair; scores
    uniform in (-4, 3), -inf at NEG_INF_ENTRY"""
    rng = np.random.default_rng(seed)
    seqs = np.zeros((MAX_SPECIAL, MAX_SPECIAL_LEN), dtype=np.uint8)
    lens = np.zeros(MAX_SPECIAL, dtype=np.uint8)
    seen = set()
    for x in range(MAX_SPECIAL):
        if x == NEG_INF_ENTRY + 1:
            seqs[x], lens[x] = seqs[x - 1], lens[x - 1]
            continue
        n = SPECIAL_LENS[x % len(SPECIAL_LENS)]
        while True:
            s = rng.integers(0, 4, n).astype(np.uint8)
            s[0], s[-1] = PAIRS[int(rng.integers(0, len(PAIRS)))]
            if bytes(s) not in seen:
                break
        seen.add(bytes(s))
        seqs[x, :n], lens[x] = s, n
    scores = rng.uniform(-4.0, 3.0, MAX_SPECIAL).astype(np.float32)
    scores[NEG_INF_ENTRY] = -np.inf
    assert int(lens[NEG_INF_ENTRY]) == 5
    return seqs, lens, scores


@functools.lru_cache(None)
def B_lim():
    from rna_algos_amd import _lib
    P = copy_of(A())
    seqs, lens, scores = special_entries()
    _lib.check(_lib.lib().rnamc_params_set_special_hairpins(P.ptr, MAX_SPECIAL, seqs.ctypes.data, lens.ctypes.data,
                                                            scores.ctypes.data))
    _lib.check(_lib.lib().rnamc_params_set_hairpin_limits(P.ptr, *HAIRPIN_LIMITS))
    return P


@functools.lru_cache(None)
def B_all():
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(2)


@functools.lru_cache(None)
def ZERO():
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.new(0.0)


SETS = {"B_hp": B_hp, "B_len": B_len, "B_lim": B_lim, "B_all": B_all}

PLANTED_ENTRIES = 26  # the first entries of B_lim's list: every length at least four times, -inf and its duplicate


@functools.lru_cache(None)
def planted():
    """-> (record, [(entry index, i, j)]): the first PLANTED_ENTRIES special hairpins of B_lim, three random
    bases after each (as test_gpu_parity.py::test_special_hairpins_and_gc_rich); 250 - 300 nt"""
    entries, _ = special_list(B_lim())
    rng = np.random.default_rng(65)
    parts, where, at = [], [], 0
    for x in range(PLANTED_ENTRIES):
        s = entries[x][0]
        parts += [s, rng.integers(0, 4, 3).astype(np.uint8)]
        where.append((x, at, at + len(s) - 1))
        at += len(s) + 3
    seq = np.concatenate(parts)
    assert 250 <= len(seq) <= 300, len(seq)
    return seq, where


@functools.lru_cache(None)
def long_loops():
    """two strong stems around an unpaired run of 44: hairpin loops of 16 and 36 bases and, by slipping the
    G and C runs against each other, the lengths around them: every one past the limit of 12, so its initiation
    term is B_lim's extrapolation; the run's few U pair with the G runs and close loops in between"""
    G, C_, A_, U = [2], [1], [0], [3]
    run = (A_ * 10 + U + A_ * 10) * 2 + A_ * 2
    assert len(run) == 44
    return np.array(G * 7 + A_ * 16 + C_ * 7 + run + G * 7 + A_ * 36 + C_ * 7, dtype=np.uint8)


def zero_records():
    from rna_algos_amd.workloads import synthetic_seq
    return [synthetic_seq(n, seed=4100 + n) for n in ZERO_LENGTHS]


def general_hairpin(P, seq, i, j):
    """get_hairpin_score's general formula (src/utils.rs:166-196) for a loop no longer than
    max_hairpin_len_extrapolation, in f32 in the reference's order"""
    _, (lo, hi, _) = special_list(P)
    n = j - i - 1
    assert n <= hi
    bi, bj = int(seq[i]), int(seq[j])
    s = np.float32(P.turner("hairpin_scores_init")[n])
    if n != lo:
        s = np.float32(s + P.turner("terminal_mismatch_scores_hairpin")[bi, bj, int(seq[i + 1]), int(seq[j - 1])])
    augu = (bi, bj) in PAIRS and (bi, bj) not in ((1, 2), (2, 1))
    return np.float32(s + (P.turner("helix_augu_end_penalty")[0] if augu else np.float32(0)))
