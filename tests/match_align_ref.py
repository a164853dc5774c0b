"""A numpy-f32 restatement of the pairwise-alignment stage (include/rnamc.h, "Pairwise alignment off
match-probability matrices"), written from that text and not from the C++.  A
helper module, not a test.

For a ProbMat P of n1 x n2 (border rows / columns: the pseudo bases), L1 = n1 - 2, L2 = n2 - 2:

    M[0][j] = M[i][0] = +0
    M[i][j] = max(M[i-1][j], M[i][j-1], (M[i-1][j-1] + g * P[i][j]) - 1)

all f32, the candidate one rounded multiply, one rounded add, one rounded subtract.  max is
order-free, so the matrix is filled by anti-diagonal here, one numpy expression per diagonal: every
numpy operation on float32 arrays rounds its result to f32 once, which is exactly "never fused".
"""
import numpy as np

F = np.float32


def fill(P, gamma):
    P = np.asarray(P, dtype=F)
    n1, n2 = P.shape
    l1, l2 = n1 - 2, n2 - 2
    M = np.zeros((l1 + 1, l2 + 1), dtype=F)
    g = F(gamma)
    for s in range(2, l1 + l2 + 1):
        i = np.arange(max(1, s - l2), min(l1, s - 1) + 1)
        j = s - i
        prod = g * P[i, j]              # one rounded multiply
        tot = M[i - 1, j - 1] + prod    # one rounded add
        cand = tot - F(1.0)             # one rounded subtract
        M[i, j] = np.maximum(np.maximum(M[i - 1, j], M[i, j - 1]), cand)
    return M


def traceback(M, n1):
    """skip-left, skip-right, match: exact float equality in that order -> (mate, n_matched)"""
    mate = np.full(n1, -1, dtype=np.int32)
    i, j = M.shape[0] - 1, M.shape[1] - 1
    count = 0
    while i > 0 and j > 0:
        if M[i, j] == M[i - 1, j]:
            i -= 1
        elif M[i, j] == M[i, j - 1]:
            j -= 1
        else:
            mate[i] = j
            count += 1
            i -= 1
            j -= 1
    return mate, count


def match_align(P, gamma):
    """-> (mate, n_matched, expect_accuracy)"""
    P = np.asarray(P, dtype=F)
    M = fill(P, gamma)
    mate, count = traceback(M, P.shape[0])
    return mate, count, M[-1, -1]


def listing(P, min_prob):
    """interior cells with p > 0 and p >= min_prob (f32), row-major -> (i, j, p)"""
    P = np.asarray(P, dtype=F)
    keep = np.zeros(P.shape, dtype=bool)
    inner = P[1:-1, 1:-1]
    keep[1:-1, 1:-1] = (inner > F(0)) & (inner >= F(min_prob))
    i, j = np.nonzero(keep)   # row-major: i ascending, then j ascending
    return i.astype(np.uint32), j.astype(np.uint32), P[i, j]


def marginals(P):
    """row_matched (n1) and col_matched (n2): the interior cells of the line ascending, one rounded
    f32 add each from +0; borders 0"""
    P = np.asarray(P, dtype=F)
    n1, n2 = P.shape
    rows = np.zeros(n1, dtype=F)
    cols = np.zeros(n2, dtype=F)
    for j in range(1, n2 - 1):
        rows[1:n1 - 1] = rows[1:n1 - 1] + P[1:n1 - 1, j]
    for i in range(1, n1 - 1):
        cols[1:n2 - 1] = cols[1:n2 - 1] + P[i, 1:n2 - 1]
    return rows, cols


def gapped_rows(mate, n2):
    """two gapped rows over the letter 'N': between two matches the unmatched bases of the first
    sequence come before those of the second"""
    n1 = len(mate)
    ra, rb = [], []
    pi = pj = 0
    stops = [(i, int(mate[i])) for i in range(1, n1 - 1) if mate[i] >= 0] + [(n1 - 1, n2 - 1)]
    for i, m in stops:
        ra.append("N" * (i - pi - 1) + "-" * (m - pj - 1))
        rb.append("-" * (i - pi - 1) + "N" * (m - pj - 1))
        if i < n1 - 1:
            ra.append("N")
            rb.append("N")
        pi, pj = i, m
    return "".join(ra), "".join(rb)


# ---- matrices the tests share

def random_probmat(rng, n1, n2, density=0.3):
    """a ProbMat with zero borders, a share of zero cells and values in (0, 1)"""
    P = np.zeros((n1, n2), dtype=F)
    if n1 > 2 and n2 > 2:
        inner = rng.random((n1 - 2, n2 - 2)).astype(F)
        inner[rng.random((n1 - 2, n2 - 2)) > density] = 0
        P[1:-1, 1:-1] = inner
    return P


def quantised_probmat(rng, n1, n2):
    """every cell a multiple of 1/4: with gammas 2 and 4 every candidate is exact and ties are
    everywhere, so the order of the equality tests decides the alignment"""
    P = np.zeros((n1, n2), dtype=F)
    if n1 > 2 and n2 > 2:
        P[1:-1, 1:-1] = rng.integers(0, 5, (n1 - 2, n2 - 2)).astype(F) / F(4)
    return P


def staircase(n1, n2, start=1, run=3, gap_a=1, gap_b=2):
    """p = 1 on a monotone path with gaps, 0 elsewhere -> (P, mate of the path).  Runs of `run` matches,
    then gap_a rows and gap_b columns skipped, from (start, 1) on."""
    P = np.zeros((n1, n2), dtype=F)
    mate = np.full(n1, -1, dtype=np.int32)
    i, j, k = start, 1, 0
    while i <= n1 - 2 and j <= n2 - 2:
        P[i, j] = 1
        mate[i] = j
        k += 1
        i += 1
        j += 1
        if k % run == 0:
            i += gap_a
            j += gap_b
    return P, mate
