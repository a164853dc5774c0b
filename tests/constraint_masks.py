"""Pair masks of hard constraints for the masked CPU oracles (oracle/README.md), and the f64
enumeration of the constrained ensemble.  A helper module, not a conftest.

DESIGN.md section 11 defines every constraint rule as "removes pairs", so a constrained problem is
the unconstrained one with some sums_close keys absent.  allowed_matrix restates the rules of
include/rnamc.h directly (crossing tested pair by pair), independent of compile_constraint and
pair_allowed; O.bpp_masked / O.exact_bpp_masked / O.mfe_exact take its result as the mask.
"""
import ctypes as C
import functools
import math

import numpy as np

import oracle_lib as O
from test_constraints_cpu import parse
from test_mfe_cpu import nested_structures


def pairs_of(db):
    st, out = [], []
    for q, ch in enumerate(db):
        if ch == "(":
            st.append(q)
        elif ch == ")":
            out.append((st.pop(), q))
        else:
            assert ch == "."
    assert not st
    return out


def sscore(params, seq, db, contra, short):
    from rna_algos_amd import _lib
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    out = C.c_double()
    _lib.check(_lib.lib().rnamc_structure_score(params.ptr, seq.ctypes.data, len(seq), db.encode(),
                                                int(contra), int(short), C.byref(out)))
    return out.value


def tol(w, db):
    return 4 * (len(pairs_of(db)) + 1) * float(np.spacing(np.float32(max(1.0, abs(w)))))


def allowed_matrix(c, span):
    """allowed(c, span, i, j) for every i < j at once (the same rules, crossing pair by pair)"""
    n = len(c)
    _, pairs = parse(c)
    arr = np.array(list(c))
    ii, jj = np.indices((n, n))
    ok = jj > ii
    if span:
        ok &= jj - ii + 1 <= span
    ok[arr == "x", :] = False
    ok[:, arr == "x"] = False
    ok[arr == ">", :] = False
    ok[:, arr == "<"] = False
    for a, b in pairs:
        ok[[a, b], :] = False
        ok[:, [a, b]] = False
        ok[:a, a + 1:b] = False      # i < a < j < b
        ok[a + 1:b, b + 1:] = False  # a < i < b < j
    for a, b in pairs:
        ok[a, b] = not span or b - a + 1 <= span
    return ok


def mixed_constraint(n):
    """The "mixed" constraint for length n -> (string, span limit): a bracket pair at
    (n//8, n - n//8), a nested one at (n//3, n//3 + n//5), x on the 12 bases from n//5, < at
    n//2 + 30, > at n//2 + 60, span limit 2n//3.  Below n = 121 the pieces as written collide (the
    x run reaches n//3 below n = 90) or fall off the end (n//2 + 60 >= n): there the x run stops
    one base before the nested bracket and the < > offsets are n//8 and n//4."""
    c = ["."] * n
    lt, gt = (30, 60) if n // 2 + 60 < n else (n // 8, n // 4)
    marks = [(n // 8, "("), (n - n // 8, ")"), (n // 3, "("), (n // 3 + n // 5, ")"),
             (n // 2 + lt, "<"), (n // 2 + gt, ">")]
    marks += [(q, "x") for q in range(n // 5, min(n // 5 + 12, n // 3 - 1))]
    for q, ch in marks:
        assert 0 <= q < n and c[q] == ".", (n, q, ch)
        c[q] = ch
    return "".join(c), (2 * n) // 3


def mixed_case(n):
    """-> (sequence, constraint string, span limit, mask) of the mixed recipe at length n"""
    seq = O.splitmix_seq(n, 4400 + n)
    cons, span = mixed_constraint(n)
    return seq, cons, span, np.ascontiguousarray(allowed_matrix(cons, span), dtype=np.uint8)


def binds(constrained_packed, plain_packed):
    """the constrained key set holds between 15 % and 85 % of the plain one's pairs"""
    kc = int(np.sum(np.asarray(constrained_packed) >= -0.5))
    kp = int(np.sum(np.asarray(plain_packed) >= -0.5))
    return 0.15 * kp <= kc <= 0.85 * kp, kc, kp


# the oracle's answers for the mixed cases, computed once per session and shared by the GPU tests
@functools.lru_cache(maxsize=None)
def _params():
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(1)  # the tables of the session's `params` fixture


@functools.lru_cache(maxsize=None)
def reference(n, contra, short, constrained):
    """O.bpp_masked of the mixed case at length n (constrained) or of its sequence alone"""
    seq, _, _, mask = mixed_case(n)
    tables = _params()
    return O.bpp_masked(tables.ptr, seq, contra, short, mask if constrained else None)


@functools.lru_cache(maxsize=None)
def exact(n, contra, short, constrained):
    seq, _, _, mask = mixed_case(n)
    tables = _params()
    return O.exact_bpp_masked(tables.ptr, seq, contra, short, mask if constrained else None)


def warm(*calls):
    """fill the caches of several (function, n, contra, short, constrained) side by side: the oracle
    calls release the GIL, and at n = 640 one of them takes seconds"""
    from concurrent.futures import ThreadPoolExecutor
    calls = list(dict.fromkeys(calls))
    _params(), O.lib()  # (created here, once, before any worker asks for them)
    with ThreadPoolExecutor(len(calls)) as pool:
        for f in [pool.submit(fn, *args) for fn, *args in calls]:
            f.result()


def enumerate_constrained(params, seq, cons, span, contra, short):
    """(ln Z_c, {pair: p}, best score, best structures) over the nested structures of the model's
    space that satisfy the constraint, in f64"""
    from rna_algos_amd.mccaskill_algo import is_compatible
    ws, dbs = [], []
    for db in nested_structures(seq):
        if not is_compatible(db, cons, span):
            continue
        w = sscore(params, seq, db, contra, short)
        if w == -math.inf:
            continue
        ws.append(w)
        dbs.append(db)
    ws = np.array(ws, np.float64)
    m = ws.max()
    lz = m + math.log(np.exp(ws - m).sum())
    probs = {}
    for w, db in zip(ws, dbs):
        for p in pairs_of(db):
            probs[p] = probs.get(p, 0.0) + math.exp(w - lz)
    return lz, probs, m, ws, dbs
