"""The pair-HMM behind the Durbin path (rnamc_durbin_batch, oracle/durbin_oracle.c) in f64, written
from the model and not from the loops of either.  A helper module, not a test.

The model, read off src/durbin_algo.rs:79-242 of the reference:

  States      M, I and D over the real bases x = a[1:-1] and y = b[1:-1] (both sequences come with a
              pseudo base at each end, which nothing scores).  M consumes a base of each, I a base of
              `a`, D a base of `b`.  An alignment is a state sequence that consumes all of x and y.
  Emissions   match_scores[x_i][y_j] in M (first index: the base of `a`), insert_scores[base] in I
              and in D.
  Transitions start -> M  init_match_score       start -> I, D  init_insert_score
              M -> M      match2match_score      M -> I, M -> D, I -> M, D -> M  match2insert_score
              I -> I, D -> D  insert_extend_score
              I -> D and D -> I do not exist; every state goes to the end at 0, and so does the start
              (two empty sequences have one alignment of weight 1).  insert_switch_score is a field
              of AlignScores that no term reads.
  Result      the weight of an alignment is exp(sum of its scores); P[i][j] is the total weight of
              the alignments in which M consumes x_i with y_j over the total weight Z of all of them,
              at matrix coordinate (i + 1, j + 1); border rows and columns are 0.

Two statements of it.  `enumerate_alignments` walks every alignment and adds weights up in f64.
`forward_backward` is the textbook pair of recursions in the log domain (np.logaddexp, f64): f_k(i, j)
is the weight of all prefixes that consumed i bases of x and j of y and sit in state k, the emission of
k included; b_k(i, j) is the weight of everything that may follow, the emission of k EXCLUDED; then
P = f_M b_M / Z.  (The reference keeps the cell's own emission in its backward sums and adds the
transition out of the matched cell a second time when it joins the two; that factoring is not used
here.)  Both take `scores` as an AlignScores (or anything with its field names as attributes) and the
sequences WITH their pseudo bases, as oracle_lib.durbin does, and return (P, ln Z) with P of shape
(len(a), len(b)) in f64.  Where no alignment has a weight above 0, Z = 0 and the interior of P is NaN.
"""
import numpy as np

SCALARS = ("match2match_score", "match2insert_score", "insert_extend_score", "init_match_score",
           "init_insert_score")
NEG = -np.inf


class Model:
    """the scores in f64, named by what they are for"""

    def __init__(self, scores):
        for name in SCALARS:
            setattr(self, name, float(np.float64(getattr(scores, name))))
        self.insert = np.array(scores.insert_scores, dtype=np.float64).reshape(4)
        self.match = np.array(scores.match_scores, dtype=np.float64).reshape(4, 4)

    def transition(self, prev, state):
        """None where the model has no such transition"""
        if prev == "S":
            return self.init_match_score if state == "M" else self.init_insert_score
        if prev == "M" and state == "M":
            return self.match2match_score
        if prev == "M" or state == "M":
            return self.match2insert_score
        if prev == state:
            return self.insert_extend_score
        return None


def _real_bases(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    assert len(a) >= 2 and len(b) >= 2
    x, y = a[1:-1], b[1:-1]
    assert (len(x) == 0 or (x.min() >= 0 and x.max() < 4)) and (len(y) == 0 or (y.min() >= 0 and y.max() < 4))
    return x, y


def enumerate_alignments(scores, a, b):
    """every alignment, one after the other -> (P, ln Z).  Exponential in the lengths: up to 6 x 6."""
    mo = Model(scores)
    x, y = _real_bases(a, b)
    l1, l2 = len(x), len(y)
    weight = np.zeros((l1 + 2, l2 + 2), dtype=np.float64)
    total = [0.0]

    def walk(i, j, prev, w, matched):
        if i == l1 and j == l2:  # -> end, at 0
            total[0] += w
            for cell in matched:
                weight[cell] += w
            return
        for state in "MID":
            t = mo.transition(prev, state)
            if t is None:
                continue
            if state == "M" and i < l1 and j < l2:
                walk(i + 1, j + 1, "M", w * np.exp(t + mo.match[x[i], y[j]]), matched + [(i + 1, j + 1)])
            elif state == "I" and i < l1:
                walk(i + 1, j, "I", w * np.exp(t + mo.insert[x[i]]), matched)
            elif state == "D" and j < l2:
                walk(i, j + 1, "D", w * np.exp(t + mo.insert[y[j]]), matched)

    walk(0, 0, "S", 1.0, [])
    z = total[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        probs = weight / z
        probs[0] = probs[-1] = 0.0
        probs[:, 0] = probs[:, -1] = 0.0
        return probs, float(np.log(z))


def _lse(*terms):
    out = terms[0]
    for t in terms[1:]:
        out = np.logaddexp(out, t)
    return out


def forward_backward(scores, a, b):
    """forward and backward recursions in f64, one numpy expression per state and anti-diagonal
    -> (P, ln Z).  Index (i, j) of the sums: i bases of x and j of y are consumed."""
    mo = Model(scores)
    x, y = _real_bases(a, b)
    l1, l2 = len(x), len(y)
    shape = (l1 + 1, l2 + 1)
    t_mm, t_mi, t_ii = mo.match2match_score, mo.match2insert_score, mo.insert_extend_score
    s_m, s_i = mo.init_match_score, mo.init_insert_score
    em = np.full(shape, NEG)  # emissions of the state that ARRIVES at (i, j)
    em[1:, 1:] = mo.match[x[:, None], y[None, :]]
    ei = np.full(l1 + 1, NEG)
    ei[1:] = mo.insert[x]
    ed = np.full(l2 + 1, NEG)
    ed[1:] = mo.insert[y]
    start = np.full(shape, NEG)
    start[0, 0] = 0.0

    fm, fi, fd = np.full(shape, NEG), np.full(shape, NEG), np.full(shape, NEG)
    for s in range(1, l1 + l2 + 1):
        i = np.arange(max(0, s - l2), min(l1, s) + 1)
        j = s - i
        k = (i >= 1) & (j >= 1)
        p, q = i[k], j[k]
        fm[p, q] = em[p, q] + _lse(start[p - 1, q - 1] + s_m, fm[p - 1, q - 1] + t_mm,
                                   fi[p - 1, q - 1] + t_mi, fd[p - 1, q - 1] + t_mi)
        k = i >= 1
        p, q = i[k], j[k]
        fi[p, q] = ei[p] + _lse(start[p - 1, q] + s_i, fm[p - 1, q] + t_mi, fi[p - 1, q] + t_ii)
        k = j >= 1
        p, q = i[k], j[k]
        fd[p, q] = ed[q] + _lse(start[p, q - 1] + s_i, fm[p, q - 1] + t_mi, fd[p, q - 1] + t_ii)
    ln_z = float(_lse(start[l1, l2], fm[l1, l2], fi[l1, l2], fd[l1, l2]))

    # what may follow state k at (i, j): k's own emission is not part of it
    bm, bi, bd = np.full(shape, NEG), np.full(shape, NEG), np.full(shape, NEG)
    bm[l1, l2] = bi[l1, l2] = bd[l1, l2] = 0.0  # -> end
    for s in range(l1 + l2 - 1, 0, -1):
        i = np.arange(max(0, s - l2), min(l1, s) + 1)
        j = s - i
        to_m, to_i, to_d = np.full(len(i), NEG), np.full(len(i), NEG), np.full(len(i), NEG)
        k = (i < l1) & (j < l2)
        to_m[k] = em[i[k] + 1, j[k] + 1] + bm[i[k] + 1, j[k] + 1]
        k = i < l1
        to_i[k] = ei[i[k] + 1] + bi[i[k] + 1, j[k]]
        k = j < l2
        to_d[k] = ed[j[k] + 1] + bd[i[k], j[k] + 1]
        bm[i, j] = _lse(to_m + t_mm, to_i + t_mi, to_d + t_mi)
        bi[i, j] = _lse(to_m + t_mi, to_i + t_ii)
        bd[i, j] = _lse(to_m + t_mi, to_d + t_ii)

    probs = np.zeros((l1 + 2, l2 + 2), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        probs[1:-1, 1:-1] = np.exp(fm[1:, 1:] + bm[1:, 1:] - ln_z)
    return probs, ln_z
