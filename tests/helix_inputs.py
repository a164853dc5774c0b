"""Helix-rich inputs and tables for the tree-order tests (test_tree_helices_cpu.py,
test_gpu_tree_helices.py).  A helper module, not a conftest.

Why these inputs: the banded mid-field of the tree-order sweep (rnamc_tree_mx.h) exponentiates its
operand rows with one power-of-two scale per row and CHUNK of 32 consecutive k (the chunk grid is
absolute: k = 32 q .. 32 q + 31).  What a chunk can lose is set by the SPREAD of an operand row
inside it, max - min over the finite entries.  Along a run of G shared by two helices
(C^a G^64 C^b: the branch point k walks the run, one helix gains a stacked pair per step, the other
loses one) sums_1ormore_basepairs(i, k) rises and its partner falls by one stack score per k:
5.5 nats under strong_tables() — 170 nats over a chunk; random sequences stay below 70.
"""
import numpy as np

import oracle_lib as O

A, C, G, U = 0, 1, 2, 3
CHUNK = 32  # k per scale of the matrix-core mid-field (rnamc_tree_mx.h)
CANONICAL = [(A, U), (U, A), (C, G), (G, C), (G, U), (U, G)]
STRONG_STACK = 5.5  # nats: 3.4 kcal/mol at 37 C, a Turner-2004 GC-on-CG stack


def mild_tables():
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(1)


def strong_tables():
    """synthetic(1) with every canonical-on-canonical Turner stack at 5.5 nats (its own largest is
    4.83, GC on GC 4.27); the CONTRAfold block stays as it is"""
    p = mild_tables()
    stack = p.field("turner.stack_scores")
    for a, b in CANONICAL:
        for c, d in CANONICAL:
            stack[a][b][c][d] = STRONG_STACK
    return p


def run(base, count):
    return [base] * count


def seq(*pieces):
    out = []
    for p in pieces:
        out += p
    return np.array(out, dtype=np.uint8)


# extra C in front of the G-run of the split-run inputs: the run starts at k = 70 + a, its midpoint
# (where the two helices meet at equal length) is k = 102 + a.  (70 + a) mod 32 = 6, 11, 16, 22, 26, 0,
# 1, 2: spread over the chunk grid, and the midpoint 16 (a = 10), 0 (26), 1 (27), 2 (28) positions
# behind a chunk boundary.
SPLIT_A = (0, 5, 10, 16, 20, 26, 27, 28)


def split_run(a):
    """A^10 C^(60+a) G^64 C^60 U^10 A^3: two helices share the G-run inside a multiloop closed by A-U
    pairs"""
    return seq(run(A, 10), run(C, 60 + a), run(G, 64), run(C, 60), run(U, 10), run(A, 3))


def split_run_parts(a):
    """-> (first C of helix 1, first G, first C of helix 2, end of helix 2 (exclusive), closing pair)"""
    c1 = 10
    g = c1 + 60 + a
    c2 = g + 64
    end = c2 + 60
    return c1, g, c2, end, (9, end)


def bare_core(a):
    return seq(run(C, 60 + a), run(G, 64), run(C, 60))


def hairpins(stem, copies, tail):
    unit = run(G, stem) + run(A, 4) + run(C, stem) + run(A, tail)
    return seq(*([unit] * copies))


def helix_family():
    """-> list of (name, sequence); every member 192 <= n <= 450 (swept banded at band 64)"""
    fam = [(f"split_a{a}", split_run(a)) for a in SPLIT_A]
    fam += [(f"core_a{a}", bare_core(a)) for a in (10, 26)]
    fam += [("hairpins_40x5", hairpins(40, 5, 2)), ("hairpins_60x2", hairpins(60, 2, 0)),
            ("gc_120", seq(*([[G, C]] * 120)))]
    return fam


def controls():
    return [("splitmix_200", O.splitmix_seq(200, 7001)), ("splitmix_300", O.splitmix_seq(300, 7002))]


def family():
    return helix_family() + controls()


def chunk_spread(mat):
    """largest (max - min over finite entries) of a row or a column of `mat` (n x n, -inf = absent)
    within an aligned chunk of 32 k"""
    m = np.asarray(mat, dtype=np.float64)
    n = m.shape[0]
    pad = (-n) % CHUNK
    worst = 0.0
    for x in (m, m.T):
        fin = np.isfinite(x)
        hi = np.pad(np.where(fin, x, -np.inf), ((0, 0), (0, pad)), constant_values=-np.inf)
        lo = np.pad(np.where(fin, x, np.inf), ((0, 0), (0, pad)), constant_values=np.inf)
        hi = hi.reshape(n, -1, CHUNK).max(axis=2)
        lo = lo.reshape(n, -1, CHUNK).min(axis=2)
        ok = hi > -np.inf
        if ok.any():
            worst = max(worst, float((hi[ok] - lo[ok]).max()))
    return worst


def q1_spread(params, s, contra=False):
    return chunk_spread(O.fold_sums(params.ptr, s, contra)["sums_1ormore_basepairs"])


def dense(packed, n):
    """diagonal-major packed triangle -> n x n, absent pairs 0"""
    m = np.zeros((n, n), dtype=np.float64)
    p = np.asarray(packed, dtype=np.float64)
    off = 0
    for d in range(n):
        idx = np.arange(n - d)
        m[idx, idx + d] = np.maximum(p[off:off + n - d], 0.0)
        off += n - d
    return m


def split_run_pair_counts(packed, a):
    """expected number of pairs of helix 1 (C-block 1 with the G-run) and helix 2 (G-run with
    C-block 2), and the closing pair's probability"""
    c1, g, c2, end, (ci, cj) = split_run_parts(a)
    m = dense(packed, end + 13)
    return float(m[c1:g, g:c2].sum()), float(m[g:c2, c2:end].sum()), float(m[ci, cj])
