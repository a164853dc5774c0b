"""Pairwise alignment off match-probability matrices that stay on the device (include/rnamc.h,
DESIGN.md section 20): thresholded sparse match probabilities, per-base marginals and gamma-centroid
(maximum expected accuracy) alignments of sequence pairs.

    match_align(probs, gamma)                      the estimator on the host (rnamc_match_align)
    match_align_mats(mats, gammas, ...)            the device stage over the caller's dense matrices
    pair_align_batch(seqs, pairs, align_scores)    the pair-HMM and the stage, pair after pair

Matrices are ProbMats: their border rows and columns belong to the pseudo bases, and every index
(`i`, `j`, `mate`) is a matrix coordinate, base k of a sequence at k + 1.
"""
import ctypes as C

import numpy as np

from . import _lib
from .durbin_algo import _default_context

_ALPHABET = "ACGU"


def match_align(probs, gamma):
    """-> (mate, n_matched, expect_accuracy) of one ProbMat: rnamc_match_align, no device."""
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    n1, n2 = probs.shape
    mate = np.empty(n1, dtype=np.int32)
    count, acc = C.c_uint32(0), C.c_float(0.0)
    _lib.check(_lib.lib().rnamc_match_align(probs.ctypes.data, n1, n2, C.c_float(gamma), mate.ctypes.data,
                                            C.byref(count), C.byref(acc)))
    return mate, int(count.value), np.float32(acc.value)


def mate_to_rows(mate, n2, a=None, b=None):
    """The two gapped rows of the alignment `mate` describes (n1 = len(mate), both with pseudo bases).
    Between two matches the unmatched bases of `a` come before those of `b`.  a, b: base codes WITH
    pseudo bases; None: every base is written 'N'."""
    n1 = len(mate)
    sa = "N" * n1 if a is None else "N" + "".join(_ALPHABET[x] for x in a[1:-1]) + "N"
    sb = "N" * n2 if b is None else "N" + "".join(_ALPHABET[x] for x in b[1:-1]) + "N"
    ra, rb = [], []
    pi, pj = 0, 0
    # (the two closing pseudo bases stand in as the last match: the tails come out the same way)
    for i, m in [(i, int(mate[i])) for i in range(1, n1 - 1) if mate[i] >= 0] + [(n1 - 1, n2 - 1)]:
        ra.extend(sa[pi + 1:i])
        rb.extend("-" * (i - pi - 1))
        ra.extend("-" * (m - pj - 1))
        rb.extend(sb[pj + 1:m])
        if i < n1 - 1:
            ra.append(sa[i])
            rb.append(sb[m])
        pi, pj = i, m
    return "".join(ra), "".join(rb)


def rows_to_mate(row_a, row_b):
    """The inverse of mate_to_rows: two gapped rows -> mate (with the two border rows, -1)."""
    assert len(row_a) == len(row_b)
    mate = [-1]
    j = 0
    for x, y in zip(row_a, row_b):
        if y != "-":
            j += 1
        if x != "-":
            mate.append(j if y != "-" else -1)
    mate.append(-1)
    return np.array(mate, dtype=np.int32)


class PairAlignment:
    """What the stage makes of one ProbMat: `.i .j .p` (views of the call's arrays, row-major),
    `.row_matched` / `.col_matched`, `.mate[g]`, `.n_matched[g]`, `.expect_accuracy[g]`,
    `.alignments[g] = (gapped_a, gapped_b, expect_accuracy)`, and `.probs` (the dense matrix) where
    the call asked for it."""

    def __init__(self, n1, n2, i, j, p, matched, mate, n_matched, accuracy, a=None, b=None, probs=None):
        self.n1, self.n2 = n1, n2
        self.i, self.j, self.p = i, j, p
        self.row_matched = None if matched is None else matched[:n1]
        self.col_matched = None if matched is None else matched[n1:]
        self.mate, self.n_matched, self.expect_accuracy = mate, n_matched, accuracy
        self.probs = probs
        self._a, self._b = a, b

    @property
    def alignments(self):
        return [mate_to_rows(self.mate[g], self.n2, self._a, self._b) + (self.expect_accuracy[g],)
                for g in range(len(self.mate))]

    def to_dict(self):
        return {(int(i), int(j)): np.float32(p) for i, j, p in zip(self.i, self.j, self.p)}


class _Outputs:
    """the arrays both entries fill, sized from the shapes of the matrices"""

    def __init__(self, shapes, gammas, min_prob, cap):
        self.shapes = shapes
        self.gammas = np.ascontiguousarray(gammas, dtype=np.float32).reshape(-1)
        self.ng = len(self.gammas)
        self.min_prob = float(min_prob)
        n = len(shapes)
        self.start = np.zeros(n, dtype=np.uint64)
        self.count = np.zeros(n, dtype=np.uint64)
        self.total = C.c_uint64(0)
        self.mate_off = np.zeros(n + 1, dtype=np.uint64)
        self.marg_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(np.array([self.ng * n1 for n1, _ in shapes], dtype=np.uint64), out=self.mate_off[1:])
        np.cumsum(np.array([n1 + n2 for n1, n2 in shapes], dtype=np.uint64), out=self.marg_off[1:])
        self.mate = np.empty(int(self.mate_off[-1]), dtype=np.int32)
        self.n_matched = np.zeros(n * self.ng, dtype=np.uint32)
        self.accuracy = np.zeros(n * self.ng, dtype=np.float32)
        self.matched = np.empty(int(self.marg_off[-1]), dtype=np.float32)
        self.alloc(cap)

    def alloc(self, cap):
        self.cap = int(cap)
        self.i = np.empty(self.cap, dtype=np.uint32)
        self.j = np.empty(self.cap, dtype=np.uint32)
        self.p = np.empty(self.cap, dtype=np.float32)

    def args(self):
        return [C.c_float(self.min_prob), self.gammas.ctypes.data if self.ng else None, self.ng,
                self.i.ctypes.data, self.j.ctypes.data, self.p.ctypes.data, self.cap, self.start.ctypes.data,
                self.count.ctypes.data, C.byref(self.total), self.mate.ctypes.data, self.mate_off.ctypes.data,
                self.n_matched.ctypes.data, self.accuracy.ctypes.data, self.matched.ctypes.data,
                self.marg_off.ctypes.data]

    def result(self, x, a=None, b=None, probs=None):
        n1, n2 = self.shapes[x]
        s, k, ng = int(self.start[x]), int(self.count[x]), self.ng
        mate = self.mate[int(self.mate_off[x]):int(self.mate_off[x + 1])].reshape(ng, n1)
        return PairAlignment(n1, n2, self.i[s:s + k], self.j[s:s + k], self.p[s:s + k],
                             self.matched[int(self.marg_off[x]):int(self.marg_off[x + 1])], mate,
                             self.n_matched[x * ng:(x + 1) * ng], self.accuracy[x * ng:(x + 1) * ng], a, b, probs)


def _call(entry, head, out, tail=()):
    """One call with the arrays as they are; when they are too small the call has set the total: a
    second call with room (the contract of rnamc_bpp_batch_sparse)."""
    rc = entry(*head, *out.args(), *tail)
    if rc == _lib.ERR_INVALID_ARG and out.total.value > out.cap:
        out.alloc(out.total.value)
        rc = entry(*head, *out.args(), *tail)
    _lib.check(rc)


def match_align_mats(mats, gammas, min_prob=0.0, ctx=None, cap=None):
    """mats: dense ProbMats (2-d float arrays, each at least 2 x 2).  -> list of PairAlignment, made on
    the device off one staged copy of every matrix."""
    if ctx is None:
        ctx = _default_context()
    mats = [np.ascontiguousarray(m, dtype=np.float32) for m in mats]
    shapes = [m.shape for m in mats]
    n1 = np.array([s[0] for s in shapes], dtype=np.uint32)
    n2 = np.array([s[1] for s in shapes], dtype=np.uint32)
    offs = np.zeros(len(mats) + 1, dtype=np.uint64)
    np.cumsum(np.array([m.size for m in mats], dtype=np.uint64), out=offs[1:])
    flat = np.concatenate([m.reshape(-1) for m in mats]) if mats else np.zeros(0, np.float32)
    out = _Outputs(shapes, gammas, min_prob, int(offs[-1]) // 4 + 64 if cap is None else cap)
    _call(_lib.lib().rnamc_match_align_mats,
          [ctx._h, len(mats), n1.ctypes.data, n2.ctypes.data, flat.ctypes.data, offs.ctypes.data], out)
    return [out.result(x) for x in range(len(mats))]


def pair_align_batch(seqs, pairs, align_scores, gammas=(1.0, 2.0, 4.0), min_prob=0.01, ctx=None, dense=False,
                     cap=None):
    """seqs: sequences WITH pseudo bases; pairs: list of (a, b) indices.  -> list of PairAlignment: the
    pair-HMM of durbin_algo_batch, then per pair the listed match probabilities (p > 0 and
    p >= min_prob), the marginals and one alignment per gamma.  No dense matrix reaches the host unless
    `dense` (then `.probs` holds what durbin_algo_batch returns)."""
    if ctx is None:
        ctx = _default_context()
    seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    bases = np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)
    pa = np.array([p[0] for p in pairs], dtype=np.uint32)
    pb = np.array([p[1] for p in pairs], dtype=np.uint32)
    shapes = [(int(lens[a]), int(lens[b])) for a, b in pairs]
    cells = sum(n1 * n2 for n1, n2 in shapes)
    out = _Outputs(shapes, gammas, min_prob, cells // 4 + 64 if cap is None else cap)
    tail, probs, out_offsets = [None, None], None, None
    if dense:
        out_offsets = np.zeros(len(pairs) + 1, dtype=np.uint64)
        np.cumsum(np.array([n1 * n2 for n1, n2 in shapes], dtype=np.uint64), out=out_offsets[1:])
        probs = np.empty(cells, dtype=np.float32)
        tail = [probs.ctypes.data, out_offsets.ctypes.data]
    _call(_lib.lib().rnamc_durbin_align_batch,
          [ctx._h, align_scores.ptr, len(seqs), bases.ctypes.data, offsets.ctypes.data, len(pairs),
           pa.ctypes.data, pb.ctypes.data], out, tail)
    res = []
    for x, (a, b) in enumerate(pairs):
        m = probs[int(out_offsets[x]):int(out_offsets[x + 1])].reshape(shapes[x]) if dense else None
        res.append(out.result(x, seqs[a], seqs[b], m))
    return res
