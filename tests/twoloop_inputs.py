"""Inputs that make one two-loop slot (a, b) carry the result (test_twoloop_inputs_cpu.py,
test_gpu_twoloop_slots.py).  A helper module, not a conftest.

A two-loop (stack, bulge, interior loop) has a unpaired bases on the left and b on the right,
a + b <= RNAMC_MAX_2LOOP_LEN = 30: 496 slots per cell.  On random inputs a lone long interior loop
carries almost no weight, so a slot that reads a neighbour's length term or is lost at the ragged end
of a level moves no probability by anything near the suite's absolute bounds.  Here the record is

    fill(pl) G^mo fill(a) C^mi fill(h) G^mi fill(b) C^mo fill(pr)

with matched brackets on the mo outer and mi inner stem pairs and x on every other base: the inner
helix closes a hairpin of h bases, and the outer stem can form only around the two-loop (a, b)
between (i, j), its innermost pair, and (k, l), the outermost inner pair.

  family S  mo = 6, mi = 5, h = 4, four placements (pl, pr): the slot decides the structure
  family E  mo = 1, mi = 6, h = 4, no pads: the outer pair is (0, n - 1), every outside guard and the
            first and last rows sit on their boundary
  family N  S's shape with every fill base A and no constraint: the G-C pairs between the runs
            compete, the per-diagonal lists hold many cells
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O
from constraint_masks import allowed_matrix, pairs_of, sscore

A, C, G, U = 0, 1, 2, 3
MAX_2LOOP = 30  # RNAMC_MAX_2LOOP_LEN
SLOTS = [(a, b) for a in range(MAX_2LOOP + 1) for b in range(MAX_2LOOP + 1 - a)]
assert len(SLOTS) == 496
MODELS = [(False, False), (True, False), (True, True)]  # (contra, allows_short_hairpins)
PLACEMENTS = (0, 1, 2, 3)
S_SHAPE = dict(mo=6, mi=5, h=4)
E_SHAPE = dict(mo=1, mi=6, h=4)


def layout(a, b, mo, mi, h, pl, pr):
    """-> (n, (i, j, k, l), outer stem pairs, inner stem pairs), outermost pair first"""
    i = pl + mo - 1
    k = i + a + 1
    l = k + 2 * mi + h - 1
    j = l + b + 1
    n = j + mo + pr
    outer = [(i - t, j + t) for t in reversed(range(mo))]
    inner = [(k + t, l - t) for t in range(mi)]
    return n, (i, j, k, l), outer, inner


def record(a, b, mo, mi, h, pl, pr, plain=False):
    """-> (seq, constraint string, mask, (i, j, k, l)).  plain: every fill base A, no constraint
    (string and mask None) — family N."""
    assert 0 <= a and 0 <= b and a + b <= MAX_2LOOP and 2 * mi + h >= 14
    rng = np.random.default_rng(1000 * a + 10 * b)
    fill = (lambda m: [A] * m) if plain else (lambda m: list(rng.integers(0, 4, m)))
    pieces = [fill(pl), [G] * mo, fill(a), [C] * mi, fill(h), [G] * mi, fill(b), [C] * mo, fill(pr)]
    seq = np.array([x for p in pieces for x in p], dtype=np.uint8)
    n, ijkl, outer, inner = layout(a, b, mo, mi, h, pl, pr)
    assert len(seq) == n
    if plain:
        return seq, None, None, ijkl
    c = ["x"] * n
    for p, q in outer + inner:
        c[p], c[q] = "(", ")"
    cons = "".join(c)
    mask = np.ascontiguousarray(allowed_matrix(cons, 0), dtype=np.uint8)
    return seq, cons, mask, ijkl


def full_structure(a, b, mo, mi, h, pl, pr):
    """dot-bracket of both stems around the (a, b) loop"""
    n, _, outer, inner = layout(a, b, mo, mi, h, pl, pr)
    db = ["."] * n
    for p, q in outer + inner:
        db[p], db[q] = "(", ")"
    return "".join(db)


class Rec:
    """one record of a family with everything the tests read off it"""

    def __init__(self, family, a, b, pl, pr, shape, plain=False):
        self.family, self.a, self.b, self.pl, self.pr = family, a, b, pl, pr
        self.shape = dict(shape, pl=pl, pr=pr)
        self.seq, self.cons, self.mask, self.ijkl = record(a, b, plain=plain, **self.shape)
        self.n = len(self.seq)
        _, _, self.outer, self.inner = layout(a, b, **self.shape)
        self.full = full_structure(a, b, **self.shape)

    def __repr__(self):
        return f"{self.family}(a={self.a}, b={self.b}, pl={self.pl}, pr={self.pr}, n={self.n})"


def _numbered(recs):
    for x, r in enumerate(recs):
        r.idx = x  # position in its family: the index into exact(), reference(), optimum(), ...
    return recs


@functools.lru_cache(maxsize=None)
def family_s():
    return _numbered([Rec("S", a, b, pl, (pl + b) % 3, S_SHAPE) for a, b in SLOTS for pl in PLACEMENTS])


@functools.lru_cache(maxsize=None)
def family_e():
    return _numbered([Rec("E", a, b, 0, 0, E_SHAPE) for a, b in SLOTS])


@functools.lru_cache(maxsize=None)
def family_n():
    return _numbered([Rec("N", a, b, 0, 0, S_SHAPE, plain=True) for a, b in SLOTS])


class Neighbour:
    """an unconstrained record without a slot of its own"""
    family, a, b, pl, pr, cons, mask, outer, inner = "X", None, None, 0, 0, None, None, [], []

    def __init__(self, seq):
        self.seq, self.n, self.full = seq, len(seq), "." * len(seq)

    def __repr__(self):
        return f"X(n={self.n})"


@functools.lru_cache(maxsize=None)
def family_x():
    """The tree-order sweeps are banded, and with that the lane-per-cell batch form can be chosen at
    all, when the call's longest sequence has 3 x 64 + 2 = 194 bases (run_batch_tree): every record
    of the families is shorter than 67, so the calls that are to take those forms hold this
    neighbour as well."""
    return _numbered([Neighbour(O.splitmix_seq(200, 7200))])


FAMILIES = {"S": family_s, "E": family_e, "N": family_n, "X": family_x}


def index(n, i, j):
    """slot of pair (i, j) in the packed diagonal-major triangle"""
    d = j - i
    return d * n - d * (d - 1) // 2 + i


@functools.lru_cache(maxsize=None)
def tables():
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(1)  # the tables of the session's `params` fixture


WORKERS = 8


def pmap(fn, items):
    """the oracle calls release the GIL"""
    tables(), O.lib()  # (created here, once, before any worker asks for them)
    with ThreadPoolExecutor(WORKERS) as pool:
        return list(pool.map(fn, items))


def _frozen(pair):
    pair[0].setflags(write=False)
    return pair


# the oracle's answers, computed once per session, shared by the tests and never modified
@functools.lru_cache(maxsize=None)
def exact(family, contra, short):
    """[(packed f64 probabilities, ln Z)] of O.exact_bpp_masked per record of the family"""
    recs = FAMILIES[family]()
    p = tables().ptr
    return pmap(lambda r: _frozen(O.exact_bpp_masked(p, r.seq, contra, short, r.mask)), recs)


@functools.lru_cache(maxsize=None)
def reference(family, contra, short):
    """[(packed f32 probabilities, ln Z f32)] of O.bpp_masked per record of the family"""
    recs = FAMILIES[family]()
    p = tables().ptr
    return pmap(lambda r: _frozen(O.bpp_masked(p, r.seq, contra, short, r.mask)), recs)


@functools.lru_cache(maxsize=None)
def optimum(family, contra, short):
    """[O.mfe_exact] per record of the family"""
    recs = FAMILIES[family]()
    p = tables().ptr
    return pmap(lambda r: O.mfe_exact(p, r.seq, contra, short, r.mask), recs)


@functools.lru_cache(maxsize=None)
def full_scores(family, contra, short):
    """[score of the full structure (both stems, the (a, b) loop)] per record"""
    recs = FAMILIES[family]()
    return [sscore(tables(), r.seq, r.full, contra, short) for r in recs]


def without(mask, n, pair):
    """the mask (None: everything allowed) with one pair removed"""
    m = np.ones((n, n), np.uint8) if mask is None else mask.copy()
    m[pair[0], pair[1]] = 0
    return m


@functools.lru_cache(maxsize=None)
def slot_use(family, contra, short):
    """P((i, j) and (k, l) both paired) per record — no base between them can pair, so together they
    close the two-loop (a, b).  The ensemble without the key (k, l) holds exactly the structures that
    lack the pair, so u = p_ij(M) - p_ij(M \\ {kl}) exp(ln Z_{M \\ kl} - ln Z_M)"""
    recs = FAMILIES[family]()
    full = exact(family, contra, short)
    p = tables().ptr

    def one(x):
        r = recs[x]
        i, j, k, l = r.ijkl
        xb, xz = full[x]
        wb, wz = O.exact_bpp_masked(p, r.seq, contra, short, without(r.mask, r.n, (k, l)))
        q = index(r.n, i, j)
        return max(float(xb[q]), 0.0) - max(float(wb[q]), 0.0) * float(np.exp(wz - xz))
    return pmap(one, range(len(recs)))


def tol(w, db):
    """the tolerance of tests/test_gpu_mfe.py on a score"""
    return 4 * (len(pairs_of(db)) + 1) * float(np.spacing(np.float32(max(1.0, abs(w)))))
