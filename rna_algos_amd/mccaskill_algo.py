"""Host-side mirror of the reference's `mccaskill_algo` module over the C ABI.

Reference interface (src/mccaskill_algo.rs:247-255):

    pub fn mccaskill_algo<T>(seq, uses_contra_model, allows_short_hairpins,
                             fold_score_sets) -> (SparseProbMat<T>, FoldScores<T>)

Same names, argument meaning and error behaviour (an empty sequence or a byte
outside ACGU raises where the reference panics).  All arithmetic runs in the HIP
kernels of librnamc.so; nothing here computes.
"""
import ctypes as C
import threading

import numpy as np

from . import _lib
from .utils import FoldScoreSets, MAX_SEQ_LEN


def bpp_len(n):
    return n * (n + 1) // 2


def bpp_index(n, i, j):
    """Slot of pair (i, j), i <= j, in the packed diagonal-major triangle."""
    d = j - i
    return d * n - d * (d - 1) // 2 + i


def _constraint_bytes(constraints, lens):
    """Per-record constraint strings (None entries = unconstrained) -> the concatenated bytes the
    constrained entries read (layout of the bases), or None when no record has one."""
    if constraints is None:
        return None
    constraints = list(constraints)
    if len(constraints) != len(lens):
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG,
                              f"{len(constraints)} constraints for {len(lens)} sequences")
    if all(c is None for c in constraints):
        return None
    parts = []
    for s, (c, n) in enumerate(zip(constraints, lens)):
        n = int(n)
        if c is None:
            c = b"." * n
        elif isinstance(c, str):
            c = c.encode("ascii", errors="replace")
        else:
            c = bytes(c)
        if len(c) != n:
            raise _lib.RnamcError(_lib.ERR_INVALID_ARG,
                                  f"constraint of record {s} has length {len(c)}, its sequence {n}")
        parts.append(c)
    return b"".join(parts)


def _span(max_bp_span):
    span = int(max_bp_span or 0)
    if span < 0 or span >= 2 ** 32:
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, f"max_bp_span {span} out of range")
    return span


def _pack(seqs):
    for s in seqs:
        if len(s) == 0:
            raise _lib.RnamcError(_lib.ERR_EMPTY_SEQ)
    lens = np.array([len(s) for s in seqs], dtype=np.uint64)
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    bases = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if seqs else \
        np.zeros(0, np.uint8)
    return lens, offsets, bases


def _centroid_fold_batch(entry, handle, seqs, centroid_thresholds, uses_contra_model,
                         allows_short_hairpins, constraints, max_bp_span, return_bpp):
    """rnamc_centroid_fold_batch / _multi on `handle` -> (folds, log partition f32[n_seqs]) or
    (folds, log partition, list of BppMatrix): folds[s][g] = (dot_bracket, expect_accuracy f32)."""
    lens, offsets, bases = _pack(seqs)
    cons = _constraint_bytes(constraints, lens)
    gammas = np.ascontiguousarray(centroid_thresholds, dtype=np.float32).reshape(-1)
    ng = len(gammas)
    rows = np.empty(max(int(offsets[-1]) * ng, 1), dtype=np.uint8)
    npairs = np.zeros(max(len(seqs) * ng, 1), dtype=np.uint32)
    acc = np.zeros(max(len(seqs) * ng, 1), dtype=np.float32)
    logz = np.empty(max(len(seqs), 1), dtype=np.float32)
    bpp = out_offsets = None
    if return_bpp:
        out_offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens * (lens + 1) // 2, out=out_offsets[1:])
        bpp = np.empty(max(int(out_offsets[-1]), 1), dtype=np.float32)
    _lib.check(entry(
        handle, len(seqs), bases.ctypes.data, offsets.ctypes.data, cons, _span(max_bp_span),
        int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), gammas.ctypes.data, ng,
        rows.ctypes.data, npairs.ctypes.data, acc.ctypes.data, logz.ctypes.data,
        bpp.ctypes.data if return_bpp else None, out_offsets.ctypes.data if return_bpp else None))
    folds = []
    for s in range(len(seqs)):
        n, base = int(lens[s]), int(offsets[s]) * ng
        block = bytes(rows[base:base + n * ng]).decode()
        folds.append([(block[g * n:(g + 1) * n], acc[s * ng + g]) for g in range(ng)])
    logz = logz[:len(seqs)]
    if not return_bpp:
        return folds, logz
    mats = [BppMatrix(int(lens[s]), bpp[int(out_offsets[s]):int(out_offsets[s + 1])])
            for s in range(len(seqs))]
    return folds, logz, mats


class BppMatrix:
    """One sequence's result: packed triangle of f32, absent pairs hold -1.0.
    `sparse()` gives the reference's SparseProbMat<T> as a dict {(i, j): p}."""

    def __init__(self, n, packed):
        self.n = int(n)
        self.packed = packed

    def __getitem__(self, ij):
        i, j = ij
        return float(self.packed[bpp_index(self.n, i, j)])

    def sparse(self):
        out = {}
        n = self.n
        off = 0
        for d in range(n):
            row = self.packed[off:off + n - d]
            for i in np.nonzero(row >= -0.5)[0]:
                out[(int(i), int(i) + d)] = float(row[i])
            off += n - d
        return out

    def dense(self):
        n = self.n
        m = np.full((n, n), -1.0, dtype=np.float32)
        off = 0
        for d in range(n):
            idx = np.arange(n - d)
            m[idx, idx + d] = self.packed[off:off + n - d]
            off += n - d
        return m


class SparseBpp:
    """One sequence's thresholded pair list (rnamc_bpp_batch_sparse): numpy views `i`, `j` (u32),
    `p` (f32) in packed-triangle order (span ascending, then i ascending), `paired_prob` (f32[n]:
    per base the probability of being paired, over ALL pairs whatever the threshold) and `n`."""

    def __init__(self, n, i, j, p, paired_prob):
        self.n = int(n)
        self.i, self.j, self.p = i, j, p
        self.paired_prob = paired_prob

    def __len__(self):
        return len(self.p)

    def to_dict(self):
        """{(i, j): p}: with min_prob 0 the reference's SparseProbMat<T>."""
        return {(int(a), int(b)): float(q) for a, b, q in zip(self.i, self.j, self.p)}

    def dense(self):
        """-> BppMatrix with absent and unlisted cells at -1."""
        n = self.n
        packed = np.full(bpp_len(n), -1.0, dtype=np.float32)
        i = self.i.astype(np.int64)
        d = self.j.astype(np.int64) - i
        packed[d * n - d * (d - 1) // 2 + i] = self.p
        return BppMatrix(n, packed)


# rnamc_bpp_batch_sparse, first call: list entries allotted per nucleotide (every base pairs with
# total probability <= 1, so a record lists at most n / min_prob pairs and in practice a few per
# base), capped at the cells that can pair at all, sum of bpp_len(n) - n.  A call that overflows is
# repeated ONCE with the exact total it reported.
SPARSE_PAIRS_PER_NT = 4
sparse_retries = 0  # calls repeated so far (diagnostics)


def _bpp_batch_sparse(entry, handle, seqs, uses_contra_model, allows_short_hairpins, min_prob,
                      constraints, max_bp_span):
    """rnamc_bpp_batch_sparse / _multi on `handle` -> (list of SparseBpp, log partition f32[n_seqs])."""
    lens, offsets, bases = _pack(seqs)
    cons = _constraint_bytes(constraints, lens)
    ns = len(seqs)
    start = np.zeros(max(ns, 1), dtype=np.uint64)
    count = np.zeros(max(ns, 1), dtype=np.uint64)
    paired = np.zeros(max(int(offsets[-1]), 1), dtype=np.float32)
    logz = np.empty(max(ns, 1), dtype=np.float32)
    total = C.c_uint64(0)
    most = int(np.sum(lens * (lens + 1) // 2 - lens))
    cap = max(min(int(SPARSE_PAIRS_PER_NT * int(offsets[-1])), most), 1)
    for attempt in range(2):
        pi = np.empty(cap, dtype=np.uint32)
        pj = np.empty(cap, dtype=np.uint32)
        pp = np.empty(cap, dtype=np.float32)
        status = entry(handle, ns, bases.ctypes.data, offsets.ctypes.data, cons, _span(max_bp_span),
                       int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), float(min_prob),
                       start.ctypes.data, count.ctypes.data, pi.ctypes.data, pj.ctypes.data,
                       pp.ctypes.data, cap, C.byref(total), paired.ctypes.data, logz.ctypes.data)
        if status == _lib.ERR_INVALID_ARG and attempt == 0 and total.value > cap:
            cap = int(total.value)  # too small: once more with the exact total
            global sparse_retries
            sparse_retries += 1
            continue
        _lib.check(status)
        break
    out = []
    for s in range(ns):
        a, b = int(start[s]), int(start[s]) + int(count[s])
        out.append(SparseBpp(int(lens[s]), pi[a:b], pj[a:b], pp[a:b],
                             paired[int(offsets[s]):int(offsets[s + 1])]))
    return out, logz[:ns]


# rows of a structural context profile (rnamc_context_profile_batch), CapR's order
CONTEXTS = ("bulge", "exterior", "hairpin", "internal", "multibranch", "stem")


def _context_profile_batch(entry, handle, seqs, uses_contra_model, allows_short_hairpins, constraints,
                           max_bp_span):
    """rnamc_context_profile_batch / _multi on `handle` -> (list of (6, n_s) f32 views, log partition
    f32[n_seqs])."""
    lens, offsets, bases = _pack(seqs)
    cons = _constraint_bytes(constraints, lens)
    ns = len(seqs)
    prof = np.zeros(max(6 * int(offsets[-1]), 1), dtype=np.float32)
    logz = np.empty(max(ns, 1), dtype=np.float32)
    _lib.check(entry(handle, ns, bases.ctypes.data, offsets.ctypes.data, cons, _span(max_bp_span),
                     int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), prof.ctypes.data,
                     logz.ctypes.data))
    out = [prof[6 * int(offsets[s]):6 * int(offsets[s + 1])].reshape(6, int(lens[s])) for s in range(ns)]
    return out, logz[:ns]


class WindowedBpp:
    """Result of windowed local folding (rnamc_bpp_windowed): `band` is an (N, B) f32 view,
    band[i, d] = the probability of pair (i, i + d) averaged over the windows that contain it (-1:
    no such pair); `paired_prob` f32[N]; `window_log_z` f32[n_windows]; `starts` u64[n_windows]."""

    def __init__(self, band, paired_prob, window_log_z, starts):
        self.band = band
        self.n, self.band_width = int(band.shape[0]), int(band.shape[1])
        self.paired_prob = paired_prob
        self.window_log_z = window_log_z
        self.starts = starts

    def pairs(self, min_prob=0.0):
        """(i, j, p) arrays of the present pairs with p >= min_prob, ordered by span, then i."""
        keep = (self.band > -0.5) & (self.band >= np.float32(min_prob))
        d, i = np.nonzero(keep.T)
        return i.astype(np.int64), (i + d).astype(np.int64), self.band[i, d]

    def to_dict(self, min_prob=0.0):
        """{(i, j): p} of `pairs(min_prob)`."""
        return {(int(a), int(b)): float(q) for a, b, q in zip(*self.pairs(min_prob))}


def window_plan(n, window, stride=1, max_bp_span=0):
    """rnamc_window_plan (host only, no device): the window starts (u64 array) and the band width of
    a windowed call -> (starts, band)."""
    head = (int(n), int(window), int(stride), _span(max_bp_span))
    if not (0 <= head[0] < 2 ** 64 and 0 <= head[1] < 2 ** 32 and 0 <= head[2] < 2 ** 32):
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, "window_plan: argument out of range")
    count, band = C.c_uint64(0), C.c_uint32(0)
    _lib.check(_lib.lib().rnamc_window_plan(*head, C.byref(count), C.byref(band), None, 0))
    starts = np.empty(max(count.value, 1), dtype=np.uint64)
    _lib.check(_lib.lib().rnamc_window_plan(*head, C.byref(count), C.byref(band), starts.ctypes.data,
                                            count.value))
    return starts[:count.value], int(band.value)


def _bpp_windowed(entry, handle, seq, window, uses_contra_model, allows_short_hairpins, stride, max_bp_span,
                  constraint):
    """rnamc_bpp_windowed / _multi on `handle` -> WindowedBpp"""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    n = int(seq.shape[0])
    starts, band = window_plan(n, window, stride, max_bp_span)
    cons = None
    if constraint is not None:
        cons = constraint.encode("ascii", errors="replace") if isinstance(constraint, str) else bytes(constraint)
        if len(cons) != n:
            raise _lib.RnamcError(_lib.ERR_INVALID_ARG, f"constraint has length {len(cons)}, the sequence {n}")
    out = np.empty((n, band), dtype=np.float32)
    paired = np.empty(n, dtype=np.float32)
    logz = np.empty(len(starts), dtype=np.float32)
    _lib.check(entry(handle, seq.ctypes.data, n, cons, int(window), int(stride), _span(max_bp_span),
                     int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), out.ctypes.data,
                     paired.ctypes.data, logz.ctypes.data))
    return WindowedBpp(out, paired, logz, starts)


class ColumnBpp(BppMatrix):
    """The averaged pair probabilities of an alignment over its COLUMNS: a BppMatrix (packed
    diagonal-major triangle, absent pairs at -1) whose indices are columns."""

    def to_dict(self, min_prob=0.0):
        """{(ci, cj): p} of the present column pairs with p >= min_prob."""
        return {(int(a), int(b)): float(q) for a, b, q in zip(*self.pairs(min_prob))}

    def pairs(self, min_prob=0.0):
        """(ci, cj, p) arrays of the present column pairs with p >= min_prob, ordered by span, then ci."""
        n = self.n
        keep = np.nonzero((self.packed > -0.5) & (self.packed >= np.float32(min_prob)))[0]
        keep = keep[keep >= n]  # (the main diagonal holds -1 anyway)
        # diagonal d starts at d n - d (d - 1) / 2: the diagonal of a packed index by searchsorted
        d_all = np.arange(n + 1, dtype=np.int64)
        starts = d_all * n - d_all * (d_all - 1) // 2
        d = np.searchsorted(starts, keep, side="right") - 1
        i = keep - starts[d]
        return i.astype(np.int64), (i + d).astype(np.int64), self.packed[keep]


class AlignmentBpp:
    """Result of alignment folding (rnamc_bpp_alignment): `bpp` a ColumnBpp over the alignment's columns
    (each pair's probability averaged over ALL rows), `col_paired` f32[n_cols], `folds` a list of
    (dot_bracket over the columns, expect_accuracy), one per gamma, `log_z` f32[n_rows] and `row_len`
    u32[n_rows] (bases of every row)."""

    def __init__(self, bpp, col_paired, folds, log_z, row_len):
        self.bpp = bpp
        self.n_cols = int(len(col_paired))
        self.col_paired = col_paired
        self.folds = folds
        self.log_z = log_z
        self.row_len = row_len

    def pairs(self, min_prob=0.0):
        """(ci, cj, p) arrays of the column pairs with averaged probability >= min_prob."""
        return self.bpp.pairs(min_prob)


def _align_rows_arg(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if rows.ndim != 2:
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, "alignment rows must be a 2-D array (n_rows, n_cols) of codes 0..4")
    if rows.shape[0] >= 2 ** 32 or rows.shape[1] >= 2 ** 32:
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, "alignment too large")
    return rows


def _bpp_alignment(entry, handle, rows, uses_contra_model, allows_short_hairpins, centroid_thresholds, max_bp_span,
                   return_bpp=True):
    """rnamc_bpp_alignment / _multi on `handle` -> AlignmentBpp (return_bpp False: .bpp is None)"""
    rows = _align_rows_arg(rows)
    n_rows, n_cols = int(rows.shape[0]), int(rows.shape[1])
    gammas = np.ascontiguousarray(centroid_thresholds, dtype=np.float32).reshape(-1)
    ng = len(gammas)
    bpp = np.empty(max(bpp_len(n_cols), 1), dtype=np.float32) if return_bpp else None
    paired = np.empty(max(n_cols, 1), dtype=np.float32)
    structs = np.empty(max(ng * n_cols, 1), dtype=np.uint8)
    npairs = np.zeros(max(ng, 1), dtype=np.uint32)
    acc = np.zeros(max(ng, 1), dtype=np.float32)
    logz = np.empty(max(n_rows, 1), dtype=np.float32)
    row_len = np.zeros(max(n_rows, 1), dtype=np.uint32)
    _lib.check(entry(handle, n_rows, n_cols, rows.ctypes.data if rows.size else None, _span(max_bp_span),
                     int(bool(uses_contra_model)), int(bool(allows_short_hairpins)),
                     gammas.ctypes.data if ng else None, ng, bpp.ctypes.data if return_bpp else None,
                     paired.ctypes.data, structs.ctypes.data if ng else None, npairs.ctypes.data if ng else None,
                     acc.ctypes.data if ng else None, logz.ctypes.data, row_len.ctypes.data))
    block = bytes(structs[:ng * n_cols]).decode()
    folds = [(block[g * n_cols:(g + 1) * n_cols], acc[g]) for g in range(ng)]
    return AlignmentBpp(ColumnBpp(n_cols, bpp[:bpp_len(n_cols)]) if return_bpp else None, paired[:n_cols], folds,
                        logz[:n_rows], row_len[:n_rows])


class MutantScan:
    """Result of a point-mutation scan (rnamc_mutant_scan), one entry per mutant m = 3 * idx + rank:
    `pos` (u32) and `base` (u8 code) of the mutant, `log_z` (f32) and `wt_log_z` (float),
    `dist2_q` (int64: the squared Euclidean distance of the mutant's pair-probability matrix from the
    wild type's in units of 2^-44), `max_dp` (f32) with `max_pair` (M x 2 int64, -1 -1 where no pair
    moved), `paired_prob` (M x n f32) and `wt_paired_prob` (f32[n])."""
    DIST2_QUANTUM = float(2 ** 44)

    def __init__(self, pos, base, log_z, wt_log_z, dist2_q, max_dp, max_pair, paired_prob, wt_paired_prob):
        self.pos, self.base = pos, base
        self.log_z, self.wt_log_z = log_z, float(wt_log_z)
        self.dist2_q = dist2_q
        self.max_dp, self.max_pair = max_dp, max_pair
        self.paired_prob, self.wt_paired_prob = paired_prob, wt_paired_prob

    def __len__(self):
        return len(self.pos)

    @property
    def dist2(self):
        """float64: dist2_q / 2^44"""
        return self.dist2_q.astype(np.float64) / MutantScan.DIST2_QUANTUM

    @property
    def delta_log_z(self):
        """float64: ln Z of the mutant - ln Z of the wild type"""
        return self.log_z.astype(np.float64) - np.float64(self.wt_log_z)

    def profile_correlation(self):
        """SNPfold's score: Pearson r of every mutant's paired-probability profile with the wild
        type's, in float64; NaN where either profile is constant."""
        a = np.asarray(self.wt_paired_prob, dtype=np.float64)
        b = np.asarray(self.paired_prob, dtype=np.float64).reshape(len(self), len(a))
        da = a - a.mean() if len(a) else a
        db = b - b.mean(axis=1, keepdims=True) if len(a) else b
        den = np.sqrt(np.sum(da * da) * np.sum(db * db, axis=1))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den > 0, np.sum(db * da[None, :], axis=1) / den, np.nan)

    def top(self, k):
        """indices of the k mutants with the largest dist2, descending (ties: the earlier mutant)"""
        order = np.argsort(-self.dist2_q, kind="stable")
        return order[:max(int(k), 0)]


def _positions(positions):
    """None or a u32 array of positions (RnamcError for one outside u32)"""
    if positions is None:
        return None
    pos = np.asarray(positions, dtype=np.int64).reshape(-1)
    if pos.size and (pos.min() < 0 or pos.max() >= 2 ** 32):
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, "mutant positions must lie in 0 .. 2^32 - 1")
    if 3 * pos.size >= 2 ** 32:
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, "3 * n_positions must be below 2^32")
    return np.ascontiguousarray(pos.astype(np.uint32))


def mutant_plan(seq, positions=None):
    """rnamc_mutant_plan (host only, no device): the mutant list of a scan -> (pos u32[M], base u8[M])"""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    if seq.shape[0] > MAX_SEQ_LEN:
        raise _lib.RnamcError(_lib.ERR_SEQ_TOO_LONG)
    pos = _positions(positions)
    head = (seq.ctypes.data, int(seq.shape[0]), None if pos is None else pos.ctypes.data,
            0 if pos is None else len(pos))
    count = C.c_uint64(0)
    _lib.check(_lib.lib().rnamc_mutant_plan(*head, C.byref(count), None, None, 0))
    mp = np.empty(max(count.value, 1), dtype=np.uint32)
    mb = np.empty(max(count.value, 1), dtype=np.uint8)
    _lib.check(_lib.lib().rnamc_mutant_plan(*head, C.byref(count), mp.ctypes.data, mb.ctypes.data, count.value))
    return mp[:count.value], mb[:count.value]


def _mutant_scan(entry, handle, seq, uses_contra_model, allows_short_hairpins, positions, constraint, max_bp_span):
    """rnamc_mutant_scan / _multi on `handle` -> MutantScan"""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    n = int(seq.shape[0])
    mp, mb = mutant_plan(seq, positions)
    pos = _positions(positions)
    cons = None
    if constraint is not None:
        cons = constraint.encode("ascii", errors="replace") if isinstance(constraint, str) else bytes(constraint)
        if len(cons) != n:
            raise _lib.RnamcError(_lib.ERR_INVALID_ARG, f"constraint has length {len(cons)}, the sequence {n}")
    M = len(mp)
    logz = np.empty(max(M, 1), dtype=np.float32)
    q = np.empty(max(M, 1), dtype=np.int64)
    dp = np.empty(max(M, 1), dtype=np.float32)
    mi = np.empty(max(M, 1), dtype=np.uint32)
    mj = np.empty(max(M, 1), dtype=np.uint32)
    paired = np.empty((max(M, 1), n), dtype=np.float32)
    wt_logz = C.c_float(0)
    wt_paired = np.empty(n, dtype=np.float32)
    _lib.check(entry(handle, seq.ctypes.data, n, cons, _span(max_bp_span), int(bool(uses_contra_model)),
                     int(bool(allows_short_hairpins)), None if pos is None else pos.ctypes.data,
                     0 if pos is None else len(pos), logz.ctypes.data, q.ctypes.data, dp.ctypes.data,
                     mi.ctypes.data, mj.ctypes.data, paired.ctypes.data, C.byref(wt_logz), wt_paired.ctypes.data))
    pair = np.stack([mi[:M], mj[:M]], axis=1).astype(np.int64)
    pair[pair == 0xffffffff] = -1
    return MutantScan(mp, mb, logz[:M], np.float32(wt_logz.value), q[:M], dp[:M], pair, paired[:M], wt_paired)


# one rnamc_twoloop_score (include/rnamc.h)
TWOLOOP_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("k", "<u4"), ("l", "<u4"),
                          ("score", "<f4")])


def _sparse_scores(n, packed):
    out = {}
    x = 0
    for d in range(n):
        row = packed[x:x + n - d]
        for i in np.nonzero(~np.isnan(row))[0]:
            out[(int(i), int(i) + d)] = float(row[i])
        x += n - d
    return out


class FoldScores:
    """FoldScores<T> (src/mccaskill_algo.rs:13-19): hairpin_scores, twoloop_scores,
    multibranch_close_scores, accessible_scores keyed like the reference's hash maps.
    No in-crate caller reads them, so they are materialised on first access
    (rnamc_fold_scores: device sweep for the key sets, host scoring)."""

    def __init__(self, materialise=None):
        self._materialise = materialise
        self._maps = None

    def _get(self, x):
        if self._maps is None:
            if self._materialise is None:
                self._maps = ({}, {}, {}, {})
            else:
                n, hp, mb, ac, tl = self._materialise()
                two = {(int(e["i"]), int(e["j"]), int(e["k"]), int(e["l"])): float(e["score"])
                       for e in tl}
                self._maps = (_sparse_scores(n, hp), two, _sparse_scores(n, mb),
                              _sparse_scores(n, ac))
        return self._maps[x]

    hairpin_scores = property(lambda self: self._get(0))
    twoloop_scores = property(lambda self: self._get(1))
    multibranch_close_scores = property(lambda self: self._get(2))
    accessible_scores = property(lambda self: self._get(3))


class FoldSums:
    """Mirror of `FoldSums<T>` (src/mccaskill_algo.rs:3-11), the value of the reference's first
    stage `get_fold_sums` / `get_fold_sums_contra` (282, 380).  The five dense members are n x n
    f32 arrays with the reference's initial values where it writes nothing (sums_external 0,
    the others -inf); `sums_close` and `sums_accessible`, hash maps in the reference, are
    {(i, j): value} dicts of the finite entries (built on first use; the dense form with -inf =
    absent is `dense["sums_close"]`)."""
    FIELDS = ("sums_external", "sums_rightmost_basepairs_external",
              "sums_rightmost_basepairs_multibranch", "sums_close", "sums_accessible",
              "sums_multibranch", "sums_1ormore_basepairs")
    SPARSE = ("sums_close", "sums_accessible")

    def __init__(self, n, dense):
        self.n = n
        self.dense = dense
        self._sparse = {}

    def __getattr__(self, name):
        if name in FoldSums.SPARSE:
            if name not in self._sparse:
                m = self.dense[name]
                ii, jj = np.nonzero(np.isfinite(m))
                self._sparse[name] = {(int(i), int(j)): float(m[i, j]) for i, j in zip(ii, jj)}
            return self._sparse[name]
        if name in FoldSums.FIELDS:
            return self.dense[name]
        raise AttributeError(name)


class Context:
    """Owns one rnamc_ctx (tables + workspace on one GPU)."""

    def __init__(self, fold_score_sets, device=-1, workspace_bytes=0):
        self._h = C.c_void_p()
        self._owned = True
        self._key = fold_score_sets.content_key()
        _lib.check(_lib.lib().rnamc_ctx_create(fold_score_sets.ptr, device, workspace_bytes,
                                               C.byref(self._h)))

    @classmethod
    def of_pool(cls, pool, idx=0):
        """Context `idx` of a Pool as a Context (owned by the pool: close() leaves it alone).
        A borrowed context syncs through its pool: it keeps no key of its own, and its sync_params is
        the pool's, so every context of the pool and the pool's key change together."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(_lib.lib().rnamc_pool_ctx(pool._h, idx))
        if not self._h:
            raise IndexError(idx)
        self._owned = False
        self._pool = pool  # keeps the owner alive; holds the key of the tables on the device
        return self

    def sync_params(self, fold_score_sets):
        """Upload the tables again if their contents differ from the ones on the device (a context
        borrowed from a Pool: on every context of that pool)."""
        pool = getattr(self, "_pool", None)
        if pool is not None:
            pool.sync_params(fold_score_sets)
            return
        key = fold_score_sets.content_key()
        if key != self._key:
            _lib.check(_lib.lib().rnamc_ctx_set_params(self._h, fold_score_sets.ptr))
            self._key = key

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if getattr(self, "_owned", True):
                try:
                    _lib.lib().rnamc_ctx_destroy(self._h)
                except Exception:  # interpreter shutdown: the binding module is already torn down
                    pass
            self._h = C.c_void_p()

    __del__ = close

    def set(self, name, value):
        _lib.check(_lib.lib().rnamc_ctx_set(self._h, name.encode(), int(value)))

    def stats(self):
        st = _lib.BatchStats()
        _lib.check(_lib.lib().rnamc_ctx_stats(self._h, C.byref(st), C.sizeof(st), None))
        out = {k: getattr(st, k) for k, _ in st._fields_}
        # (rnamc_context_profile_stats: beside the block, whose size is part of the ABI)
        launches, ms = C.c_uint64(0), C.c_double(0.0)
        _lib.check(_lib.lib().rnamc_context_profile_stats(self._h, C.byref(launches), C.byref(ms)))
        out["launches_context"], out["ms_context"] = launches.value, ms.value
        return out

    def bpp_batch(self, seqs, uses_contra_model, allows_short_hairpins, constraints=None,
                  max_bp_span=0):
        """seqs: list of np.uint8 code arrays -> (list of BppMatrix, log partition f32[]).
        constraints: None, or one constraint string (". x ( ) < >", None = unconstrained) per
        sequence; max_bp_span: longest admitted pair span j - i + 1, 0 = no limit
        (include/rnamc.h, hard constraints)."""
        lens, offsets, bases = _pack(seqs)
        cons = _constraint_bytes(constraints, lens)
        out_offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens * (lens + 1) // 2, out=out_offsets[1:])
        bpp = np.empty(int(out_offsets[-1]), dtype=np.float32)
        logz = np.empty(len(seqs), dtype=np.float32)
        _lib.check(_lib.lib().rnamc_bpp_batch_constrained(
            self._h, len(seqs), bases.ctypes.data, offsets.ctypes.data, cons, _span(max_bp_span),
            int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), bpp.ctypes.data,
            out_offsets.ctypes.data, logz.ctypes.data))
        mats = [BppMatrix(int(lens[s]), bpp[int(out_offsets[s]):int(out_offsets[s + 1])])
                for s in range(len(seqs))]
        return mats, logz

    def bpp_batch_into(self, bases, offsets, uses_contra_model, allows_short_hairpins, bpp,
                       out_offsets, log_partition=None):
        """rnamc_bpp_batch on caller-owned host buffers (numpy arrays): H2D + kernels + D2H."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        assert bpp.dtype == np.float32 and bpp.flags.c_contiguous
        _lib.check(_lib.lib().rnamc_bpp_batch(
            self._h, len(offsets) - 1, bases.ctypes.data, offsets.ctypes.data,
            int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), bpp.ctypes.data,
            out_offsets.ctypes.data,
            log_partition.ctypes.data if log_partition is not None else None))

    def bpp_batch_device(self, n_seqs, d_bases_ptr, offsets, uses_contra_model,
                         allows_short_hairpins, d_bpp_ptr, out_offsets, d_logz_ptr, stream_ptr):
        """Everything already in HBM; enqueues on `stream_ptr` and returns."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        _lib.check(_lib.lib().rnamc_bpp_batch_device(
            self._h, n_seqs, d_bases_ptr, offsets.ctypes.data, int(bool(uses_contra_model)),
            int(bool(allows_short_hairpins)), d_bpp_ptr, out_offsets.ctypes.data, d_logz_ptr,
            stream_ptr))

    def fold_scores_packed(self, seq, uses_contra_model, allows_short_hairpins):
        """-> (n, hairpin, multibranch_close, accessible packed triangles with NaN = key
        absent, twoloop entries as a TWOLOOP_DTYPE array)."""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        n = len(seq)
        if n == 0:
            raise _lib.RnamcError(_lib.ERR_EMPTY_SEQ)
        hp, mb, ac = (np.empty(bpp_len(n), dtype=np.float32) for _ in range(3))
        count = C.c_uint64(0)
        args = (self._h, seq.ctypes.data, n, int(bool(uses_contra_model)),
                int(bool(allows_short_hairpins)), hp.ctypes.data, mb.ctypes.data, ac.ctypes.data)
        _lib.check(_lib.lib().rnamc_fold_scores(*args, None, 0, C.byref(count)))
        tl = np.empty(count.value, dtype=TWOLOOP_DTYPE)
        _lib.check(_lib.lib().rnamc_fold_scores(*args, tl.ctypes.data, count.value,
                                                C.byref(count)))
        return n, hp, mb, ac, tl

    def fold_sums(self, seq, uses_contra_model, allows_short_hairpins):
        """FoldSums of one sequence (rnamc_fold_sums: the inside sweep alone, reference order)
        -> FoldSums"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        n = int(seq.shape[0])
        if n == 0:
            raise _lib.RnamcError(_lib.ERR_EMPTY_SEQ)
        mats = [np.empty((n, n), dtype=np.float32) for _ in FoldSums.FIELDS]
        _lib.check(_lib.lib().rnamc_fold_sums(self._h, seq.ctypes.data, n, int(uses_contra_model),
                                             int(allows_short_hairpins), *[m.ctypes.data for m in mats]))
        return FoldSums(n, dict(zip(FoldSums.FIELDS, mats)))

    def sample_batch(self, seqs, n_samples, uses_contra_model, allows_short_hairpins, seed=0,
                     constraints=None, max_bp_span=0):
        """Boltzmann sampling (rnamc_sample_batch): n_samples structures per sequence drawn with
        probability exp(score) / Z off the reference-order inside sweep -> (list of
        (n_samples, n_s) uint8 arrays of b'(', b')', b'.', log-weights f32[n_seqs, n_samples],
        log partition f32[n_seqs]).  constraints, max_bp_span: as bpp_batch (then Z is Z_c)."""
        n_samples = int(n_samples)
        lens, offsets, bases = _pack(seqs)
        cons = _constraint_bytes(constraints, lens)
        rows = np.empty(int(offsets[-1]) * n_samples, dtype=np.uint8)
        weights = np.empty((len(seqs), n_samples), dtype=np.float32)
        logz = np.empty(len(seqs), dtype=np.float32)
        _lib.check(_lib.lib().rnamc_sample_batch_constrained(
            self._h, len(seqs), bases.ctypes.data, offsets.ctypes.data, cons, _span(max_bp_span),
            int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), n_samples,
            int(seed) & (2**64 - 1),
            rows.ctypes.data if rows.size else None, weights.ctypes.data if weights.size else None,
            logz.ctypes.data if logz.size else None))
        out = [rows[int(offsets[s]) * n_samples:int(offsets[s + 1]) * n_samples].reshape(
            n_samples, int(lens[s])) for s in range(len(seqs))]
        return out, weights, logz

    def mfe_batch(self, seqs, uses_contra_model, allows_short_hairpins, constraints=None,
                  max_bp_span=0):
        """Maximum-score structure of every sequence (rnamc_mfe_batch: MFE under Turner, the
        Viterbi parse under CONTRAfold) -> (list of dot-bracket str, scores f32[n_seqs] = the sum
        of each structure's loop scores, dp_scores f32[n_seqs] = the max-plus sweep's value).
        constraints, max_bp_span: as bpp_batch."""
        lens, offsets, bases = _pack(seqs)
        cons = _constraint_bytes(constraints, lens)
        rows = np.empty(max(int(offsets[-1]), 1), dtype=np.uint8)
        scores = np.empty(len(seqs), dtype=np.float32)
        dp = np.empty(len(seqs), dtype=np.float32)
        _lib.check(_lib.lib().rnamc_mfe_batch_constrained(
            self._h, len(seqs), bases.ctypes.data, offsets.ctypes.data, cons, _span(max_bp_span),
            int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), rows.ctypes.data,
            scores.ctypes.data if scores.size else None, dp.ctypes.data if dp.size else None))
        out = [bytes(rows[int(offsets[s]):int(offsets[s + 1])]).decode() for s in range(len(seqs))]
        return out, scores, dp

    def log_partition_batch(self, seqs, uses_contra_model, allows_short_hairpins, constraints=None,
                            max_bp_span=0):
        """ln Z (ln Z_c under constraints, as bpp_batch) of every sequence: the reference-order
        inside sweep alone (rnamc_log_partition_batch) -> f32[n_seqs], equal bit for bit to
        bpp_batch's log partition in summation_mode 0."""
        lens, offsets, bases = _pack(seqs)
        cons = _constraint_bytes(constraints, lens)
        logz = np.empty(max(len(seqs), 1), dtype=np.float32)
        _lib.check(_lib.lib().rnamc_log_partition_batch(
            self._h, len(seqs), bases.ctypes.data, offsets.ctypes.data, cons, _span(max_bp_span),
            int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), logz.ctypes.data))
        return logz[:len(seqs)]

    def centroid_fold_batch(self, seqs, centroid_thresholds, uses_contra_model, allows_short_hairpins,
                            constraints=None, max_bp_span=0, return_bpp=False):
        """mccaskill_algo + centroid_fold of every sequence for every threshold on the device
        (rnamc_centroid_fold_batch) -> (folds, log partition f32[n_seqs]) with folds[s][g] =
        (dot_bracket, expect_accuracy), plus the list of BppMatrix when return_bpp is set.
        constraints, max_bp_span: as bpp_batch."""
        return _centroid_fold_batch(_lib.lib().rnamc_centroid_fold_batch, self._h, list(seqs),
                                    centroid_thresholds, uses_contra_model, allows_short_hairpins,
                                    constraints, max_bp_span, return_bpp)

    def bpp_batch_sparse(self, seqs, uses_contra_model, allows_short_hairpins, min_prob,
                         constraints=None, max_bp_span=0):
        """Pair probabilities >= min_prob of every sequence, compacted on the device
        (rnamc_bpp_batch_sparse) -> (list of SparseBpp, log partition f32[n_seqs]).
        constraints, max_bp_span: as bpp_batch."""
        return _bpp_batch_sparse(_lib.lib().rnamc_bpp_batch_sparse, self._h, list(seqs), uses_contra_model,
                                 allows_short_hairpins, min_prob, constraints, max_bp_span)

    def context_profile_batch(self, seqs, uses_contra_model, allows_short_hairpins, constraints=None,
                              max_bp_span=0):
        """Structural context profiles (rnamc_context_profile_batch): per base the probabilities of
        CONTEXTS -> (list of (6, n_s) f32 arrays, log partition f32[n_seqs]).
        constraints, max_bp_span: as bpp_batch."""
        return _context_profile_batch(_lib.lib().rnamc_context_profile_batch, self._h, list(seqs),
                                      uses_contra_model, allows_short_hairpins, constraints, max_bp_span)

    def bpp_windowed(self, seq, window, uses_contra_model, allows_short_hairpins, stride=1, max_bp_span=0,
                     constraint=None):
        """Windowed local folding of one (long) sequence (rnamc_bpp_windowed): every window of
        `window` bases folded with the span limit, each pair's probability averaged over the windows
        that contain it -> WindowedBpp.  constraint: None or one string over ". x < >"."""
        return _bpp_windowed(_lib.lib().rnamc_bpp_windowed, self._h, seq, window, uses_contra_model,
                             allows_short_hairpins, stride, max_bp_span, constraint)

    def bpp_alignment(self, rows, uses_contra_model, allows_short_hairpins, centroid_thresholds=(), max_bp_span=0,
                      return_bpp=True):
        """Alignment folding (rnamc_bpp_alignment): `rows` a u8 array (n_rows, n_cols) of codes 0..3 and
        4 for a gap (utils.read_align); every row folded without its gaps, the pair probabilities
        averaged per column pair over all rows on the device, one consensus fold per gamma
        -> AlignmentBpp."""
        return _bpp_alignment(_lib.lib().rnamc_bpp_alignment, self._h, rows, uses_contra_model,
                              allows_short_hairpins, centroid_thresholds, max_bp_span, return_bpp)

    def mutant_scan(self, seq, uses_contra_model, allows_short_hairpins, positions=None, constraint=None,
                    max_bp_span=0):
        """Point-mutation scan of one sequence (rnamc_mutant_scan): every single-base mutant of
        `positions` (None: all) folded and compared with the wild type on the device -> MutantScan.
        constraint: None or the wild type's string over ". x ( ) < >", applied to every mutant."""
        return _mutant_scan(_lib.lib().rnamc_mutant_scan, self._h, seq, uses_contra_model, allows_short_hairpins,
                            positions, constraint, max_bp_span)

    def debug_fetch(self, seq_idx, which, n):
        out = np.empty((n, n), dtype=np.float32)
        _lib.check(_lib.lib().rnamc_debug_fetch(self._h, seq_idx, which, out.ctypes.data))
        return out

    def debug_fetch_tree(self, seq_idx, slot):
        """rnamc_debug_fetch_tree -> (raw workspace matrix `slot` of the last tree-order call as f32[rows, ld]
        — whole rows only, the padding behind them dropped —, ld)"""
        ld, floats = C.c_uint32(), C.c_uint64()
        _lib.check(_lib.lib().rnamc_debug_fetch_tree(self._h, seq_idx, slot, None, 0, C.byref(ld), C.byref(floats)))
        out = np.empty(floats.value, dtype=np.float32)
        _lib.check(_lib.lib().rnamc_debug_fetch_tree(self._h, seq_idx, slot, out.ctypes.data, out.size, None, None))
        rows = out.size // ld.value
        return out[:rows * ld.value].reshape(rows, ld.value), ld.value


class Pool:
    """Owns one rnamc_pool: a device context per listed GPU (devices=None: every visible one);
    `bpp_batch` shards a batch over them inside librnamc (rnamc_bpp_batch_multi), one host
    thread per device, results written straight into the host triangles.  The pool holds the key of
    the tables its contexts were last given; a context borrowed with Context.of_pool syncs through
    its pool, never on its own."""

    def __init__(self, fold_score_sets, devices=None, workspace_bytes=0):
        self._h = C.c_void_p()
        self._key = fold_score_sets.content_key()
        if devices is None:
            arr, n = None, 0
        else:
            arr = (C.c_int * len(devices))(*devices)
            n = len(devices)
        _lib.check(_lib.lib().rnamc_pool_create(fold_score_sets.ptr, arr, n, workspace_bytes,
                                                C.byref(self._h)))

    def __len__(self):
        return int(_lib.lib().rnamc_pool_size(self._h))

    def sync_params(self, fold_score_sets):
        """Upload the tables to every context of the pool if their contents differ from the ones there."""
        key = fold_score_sets.content_key()
        if key != self._key:
            _lib.check(_lib.lib().rnamc_pool_set_params(self._h, fold_score_sets.ptr))
            self._key = key

    def set(self, name, value):
        _lib.check(_lib.lib().rnamc_pool_set(self._h, name.encode(), int(value)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            try:
                _lib.lib().rnamc_pool_destroy(self._h)
            except Exception:
                pass
            self._h = C.c_void_p()

    __del__ = close

    def bpp_batch(self, seqs, uses_contra_model, allows_short_hairpins, constraints=None,
                  max_bp_span=0):
        """As Context.bpp_batch, sharded over the pool's contexts (rnamc_bpp_batch_multi)."""
        lens, offsets, bases = _pack(seqs)
        cons = _constraint_bytes(constraints, lens)
        out_offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        np.cumsum(lens * (lens + 1) // 2, out=out_offsets[1:])
        bpp = np.empty(int(out_offsets[-1]), dtype=np.float32)
        logz = np.empty(len(seqs), dtype=np.float32)
        _lib.check(_lib.lib().rnamc_bpp_batch_multi_constrained(
            self._h, len(seqs), bases.ctypes.data, offsets.ctypes.data, cons, _span(max_bp_span),
            int(bool(uses_contra_model)), int(bool(allows_short_hairpins)), bpp.ctypes.data,
            out_offsets.ctypes.data, logz.ctypes.data))
        mats = [BppMatrix(int(lens[s]), bpp[int(out_offsets[s]):int(out_offsets[s + 1])])
                for s in range(len(seqs))]
        return mats, logz

    def centroid_fold_batch(self, seqs, centroid_thresholds, uses_contra_model, allows_short_hairpins,
                            constraints=None, max_bp_span=0, return_bpp=False):
        """As Context.centroid_fold_batch, sharded over the pool's contexts
        (rnamc_centroid_fold_batch_multi)."""
        return _centroid_fold_batch(_lib.lib().rnamc_centroid_fold_batch_multi, self._h, list(seqs),
                                    centroid_thresholds, uses_contra_model, allows_short_hairpins,
                                    constraints, max_bp_span, return_bpp)


    def bpp_batch_sparse(self, seqs, uses_contra_model, allows_short_hairpins, min_prob,
                         constraints=None, max_bp_span=0):
        """As Context.bpp_batch_sparse, sharded over the pool's contexts
        (rnamc_bpp_batch_sparse_multi)."""
        return _bpp_batch_sparse(_lib.lib().rnamc_bpp_batch_sparse_multi, self._h, list(seqs),
                                 uses_contra_model, allows_short_hairpins, min_prob, constraints, max_bp_span)

    def context_profile_batch(self, seqs, uses_contra_model, allows_short_hairpins, constraints=None,
                              max_bp_span=0):
        """As Context.context_profile_batch, sharded over the pool's contexts
        (rnamc_context_profile_batch_multi): the same bits."""
        return _context_profile_batch(_lib.lib().rnamc_context_profile_batch_multi, self._h, list(seqs),
                                      uses_contra_model, allows_short_hairpins, constraints, max_bp_span)

    def bpp_windowed(self, seq, window, uses_contra_model, allows_short_hairpins, stride=1, max_bp_span=0,
                     constraint=None):
        """As Context.bpp_windowed, the window list sharded over the pool's contexts
        (rnamc_bpp_windowed_multi): the same bits."""
        return _bpp_windowed(_lib.lib().rnamc_bpp_windowed_multi, self._h, seq, window, uses_contra_model,
                             allows_short_hairpins, stride, max_bp_span, constraint)


    def bpp_alignment(self, rows, uses_contra_model, allows_short_hairpins, centroid_thresholds=(), max_bp_span=0,
                      return_bpp=True):
        """As Context.bpp_alignment, the rows sharded over the pool's contexts
        (rnamc_bpp_alignment_multi): the same bits."""
        return _bpp_alignment(_lib.lib().rnamc_bpp_alignment_multi, self._h, rows, uses_contra_model,
                              allows_short_hairpins, centroid_thresholds, max_bp_span, return_bpp)

    def mutant_scan(self, seq, uses_contra_model, allows_short_hairpins, positions=None, constraint=None,
                    max_bp_span=0):
        """As Context.mutant_scan, the mutant list sharded over the pool's contexts
        (rnamc_mutant_scan_multi): the same bits in summation mode 0."""
        return _mutant_scan(_lib.lib().rnamc_mutant_scan_multi, self._h, seq, uses_contra_model,
                            allows_short_hairpins, positions, constraint, max_bp_span)


def shard_plan(lengths, n_shards):
    """rnamc_shard_plan: shard index of every sequence (host only, no device needed)."""
    lens = np.asarray(lengths, dtype=np.uint64)
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    out = np.zeros(len(lens), dtype=np.uint32)
    _lib.check(_lib.lib().rnamc_shard_plan(len(lens), offsets.ctypes.data, int(n_shards),
                                           out.ctypes.data))
    return out


# ONE pool per process for the module-level functions (workspaces and staging buffers are reused
# across calls); the single-sequence functions use ITS first context, so a process never holds two
# contexts on one device.  Which devices: RNAMC_DEVICES="0,2" lists them; under a one-process-per-GPU
# launch (LOCAL_RANK set: torchrun, bench.py) the rank's own device only — a rank that saw every
# device would open streams, tables and a workspace on all of them and shard its batch across its
# peers' GPUs; otherwise every visible device, as the reference's binary takes every core
# (src/bin/mccaskill_algo.rs:44-48).  The reference reads `&FoldScoreSets` on every call, and the
# set is mutable: the tables are re-uploaded whenever their CONTENT differs from what the contexts
# hold — never keyed by object identity, nothing is kept alive per set.
_ctx = None
_pool = None
_ctx_lock = threading.RLock()


def default_devices():
    """None = every visible device (resolved by rnamc_pool_create), else the list to use."""
    import os
    if os.environ.get("RNAMC_DEVICES"):
        return [int(x) for x in os.environ["RNAMC_DEVICES"].split(",") if x.strip() != ""]
    if os.environ.get("LOCAL_RANK") is not None:
        return [int(os.environ["LOCAL_RANK"])]
    return None


def _pool_for(fold_score_sets):
    global _pool
    with _ctx_lock:
        if _pool is None:
            _pool = Pool(fold_score_sets, default_devices())
        else:
            _pool.sync_params(fold_score_sets)
        return _pool


def _context_for(fold_score_sets):
    global _ctx
    with _ctx_lock:
        pool = _pool_for(fold_score_sets)  # (uploads changed tables to every context, this one included)
        if _ctx is None:
            _ctx = Context.of_pool(pool, 0)
        return _ctx


def mccaskill_algo_packed(seq, uses_contra_model, allows_short_hairpins, fold_score_sets):
    seq = np.asarray(seq, dtype=np.uint8)
    if seq.shape[0] > MAX_SEQ_LEN:
        raise _lib.RnamcError(_lib.ERR_SEQ_TOO_LONG)
    with _ctx_lock:  # tables of the shared context stay the caller's until the call returns
        mats, logz = _context_for(fold_score_sets).bpp_batch([seq], uses_contra_model,
                                                             allows_short_hairpins)
    return mats[0], float(logz[0])


def mccaskill_algo(seq, uses_contra_model, allows_short_hairpins, fold_score_sets):
    """(SparseProbMat, FoldScores) like the reference (src/mccaskill_algo.rs:247-280)."""
    mat, _ = mccaskill_algo_packed(seq, uses_contra_model, allows_short_hairpins, fold_score_sets)
    seq = np.array(seq, dtype=np.uint8)
    # the maps are filled on first access, with the tables as they were at call time
    frozen = FoldScoreSets(_buf=fold_score_sets._buf.copy())

    def materialise():
        with _ctx_lock:
            return _context_for(frozen).fold_scores_packed(seq, uses_contra_model,
                                                           allows_short_hairpins)
    return mat.sparse(), FoldScores(materialise)


def get_fold_sums(seq, fold_score_sets):
    """`get_fold_sums<T>(seq, &mut fold_scores) -> FoldSums<T>` (src/mccaskill_algo.rs:282-378,
    Turner) on the device.  The reference also fills `fold_scores` on the way; here that is
    `mccaskill_algo(...)[1]` / `Context.fold_scores_packed`."""
    with _ctx_lock:  # (as every function here: the tables stay the caller's until the call returns)
        return _context_for(fold_score_sets).fold_sums(seq, False, False)


def get_fold_sums_contra(seq, allows_short_hairpins, fold_score_sets):
    """`get_fold_sums_contra<T>(seq, &mut fold_scores, allows_short_hairpins, fold_score_sets)`
    (src/mccaskill_algo.rs:380-516) on the device."""
    with _ctx_lock:
        return _context_for(fold_score_sets).fold_sums(seq, True, allows_short_hairpins)


def mccaskill_algo_batch(seqs, uses_contra_model, allows_short_hairpins, fold_score_sets,
                         constraints=None, max_bp_span=0):
    """Whole FASTA at once, over the process's devices (`default_devices`: every visible GPU unless
    RNAMC_DEVICES / LOCAL_RANK say otherwise) — what src/bin/mccaskill_algo.rs:58-93 does on all
    cores with one pool task per record.  constraints (one string or None per sequence),
    max_bp_span: hard constraints, as Context.bpp_batch."""
    with _ctx_lock:
        return _pool_for(fold_score_sets).bpp_batch(list(seqs), uses_contra_model,
                                                    allows_short_hairpins, constraints, max_bp_span)


def mccaskill_algo_batch_sparse(seqs, uses_contra_model, allows_short_hairpins, fold_score_sets,
                                min_prob, constraints=None, max_bp_span=0):
    """mccaskill_algo_batch returning only the pairs with p >= min_prob (0: every key of the
    reference's SparseProbMat), compacted on the device: the dense triangles never reach the host
    -> (list of SparseBpp, log partition f32[n_seqs])."""
    with _ctx_lock:
        return _pool_for(fold_score_sets).bpp_batch_sparse(list(seqs), uses_contra_model,
                                                           allows_short_hairpins, min_prob, constraints,
                                                           max_bp_span)


def context_profile_batch(seqs, uses_contra_model, allows_short_hairpins, fold_score_sets, constraints=None,
                          max_bp_span=0):
    """Structural context profiles (CapR's profile) of every sequence over the process's devices:
    profiles[s] is a (6, n_s) f32 array whose rows are the probabilities that base u is unpaired in
    a bulge, the exterior loop, a hairpin, an internal loop or a multibranch loop, or is paired
    (CONTEXTS) -> (profiles, log partition f32[n_seqs]).  Always the reference's summation order."""
    with _ctx_lock:
        return _pool_for(fold_score_sets).context_profile_batch(list(seqs), uses_contra_model,
                                                                allows_short_hairpins, constraints, max_bp_span)


def context_profile(seq, uses_contra_model, allows_short_hairpins, fold_score_sets, constraint=None,
                    max_bp_span=0):
    """context_profile_batch of one record -> ((6, n) f32 array, log partition)."""
    prof, logz = context_profile_batch([seq], uses_contra_model, allows_short_hairpins, fold_score_sets,
                                       None if constraint is None else [constraint], max_bp_span)
    return prof[0], float(logz[0])


def mccaskill_algo_windowed(seq, window, uses_contra_model, allows_short_hairpins, fold_score_sets,
                            stride=1, max_bp_span=0, constraint=None):
    """Windowed local folding of one sequence of any length below 2^31 (RNAplfold / LocalFold): every
    window of `window` bases (starts 0, stride, 2 stride, ..., and one last window ending at the
    sequence's end) folded with max_bp_span, each pair's probability averaged over the windows that
    contain it, over the process's devices -> WindowedBpp.  The windows' triangles stay on the
    device; the result is the (N, band) array."""
    with _ctx_lock:
        return _pool_for(fold_score_sets).bpp_windowed(seq, window, uses_contra_model, allows_short_hairpins,
                                                       stride, max_bp_span, constraint)


def mutant_scan(seq, uses_contra_model, allows_short_hairpins, fold_score_sets, positions=None, constraint=None,
                max_bp_span=0):
    """Point-mutation scan of one sequence (riboSNitch / SNPfold / RNAsnp / RNAmute): every
    single-base mutant of `positions` (None: every base) folded over the process's devices and its
    pair probabilities compared with the wild type's on the device -> MutantScan.  No triangle
    reaches the host."""
    with _ctx_lock:
        return _pool_for(fold_score_sets).mutant_scan(seq, uses_contra_model, allows_short_hairpins, positions,
                                                      constraint, max_bp_span)


def alignment_fold(rows, uses_contra_model, allows_short_hairpins, fold_score_sets, centroid_thresholds=(),
                   max_bp_span=0):
    """Alignment folding (CentroidAlifold / PETfold / RNAalifold -p): every row of the alignment `rows`
    (u8 (n_rows, n_cols), codes 0..3 and 4 for a gap: utils.read_align) folded without its gaps over
    the process's devices, the pair probabilities mapped onto columns and averaged over all rows on the
    device, and the gamma-centroid fold of the averaged matrix for every gamma -> AlignmentBpp.  The
    rows' triangles stay on the device; the result is one triangle over the columns."""
    with _ctx_lock:
        return _pool_for(fold_score_sets).bpp_alignment(rows, uses_contra_model, allows_short_hairpins,
                                                        centroid_thresholds, max_bp_span)


def structure_score(seq, dot_bracket, uses_contra_model, allows_short_hairpins, fold_score_sets):
    """Log Boltzmann weight of one structure (rnamc_structure_score, host only): the sum of its
    loop scores; -inf for a structure outside the model's space.  exp(score - ln Z) is its
    probability."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    db = dot_bracket.encode() if isinstance(dot_bracket, str) else bytes(dot_bracket)
    out = C.c_double()
    _lib.check(_lib.lib().rnamc_structure_score(fold_score_sets.ptr, seq.ctypes.data,
                                                int(seq.shape[0]), db, int(bool(uses_contra_model)),
                                                int(bool(allows_short_hairpins)), C.byref(out)))
    return out.value


def sample_structures_batch(seqs, n_samples, uses_contra_model, allows_short_hairpins,
                            fold_score_sets, seed=0, constraints=None, max_bp_span=0):
    """Boltzmann samples of every sequence on the process's shared context -> (per sequence a
    list of n_samples (dot_bracket, log_weight), log partition f32[n_seqs]).  Sample t of
    sequence s depends on (tables, sequence, constraint, flags, seed, s, t) only.  constraints
    (one string or None per sequence), max_bp_span: hard constraints, as Context.bpp_batch."""
    seqs = [np.asarray(s, dtype=np.uint8) for s in seqs]
    for s in seqs:
        if s.shape[0] > MAX_SEQ_LEN:
            raise _lib.RnamcError(_lib.ERR_SEQ_TOO_LONG)
    with _ctx_lock:
        rows, weights, logz = _context_for(fold_score_sets).sample_batch(
            seqs, n_samples, uses_contra_model, allows_short_hairpins, seed, constraints, max_bp_span)
    out = [[(bytes(r).decode(), float(w)) for r, w in zip(m, ws)] for m, ws in zip(rows, weights)]
    return out, logz


def sample_structures(seq, n_samples, uses_contra_model, allows_short_hairpins, fold_score_sets,
                      seed=0, constraints=None, max_bp_span=0):
    """n_samples structures of one sequence drawn with probability exp(score) / Z -> (list of
    (dot_bracket, log_weight), ln Z).  constraints: one constraint string (or None)."""
    out, logz = sample_structures_batch([seq], n_samples, uses_contra_model, allows_short_hairpins,
                                        fold_score_sets, seed,
                                        None if constraints is None else [constraints], max_bp_span)
    return out[0], float(logz[0])


def mfe_fold_batch(seqs, uses_contra_model, allows_short_hairpins, fold_score_sets,
                   constraints=None, max_bp_span=0):
    """Maximum-score structure of every sequence on the process's shared context -> (list of
    (dot_bracket, score)); score is the f32 sum of the structure's loop scores (compare
    structure_score).  Ties go to the first maximal candidate in the grammar's order.
    constraints (one string or None per sequence), max_bp_span: as Context.bpp_batch."""
    seqs = [np.asarray(s, dtype=np.uint8) for s in seqs]
    for s in seqs:
        if s.shape[0] > MAX_SEQ_LEN:
            raise _lib.RnamcError(_lib.ERR_SEQ_TOO_LONG)
    with _ctx_lock:
        dbs, scores, _ = _context_for(fold_score_sets).mfe_batch(
            seqs, uses_contra_model, allows_short_hairpins, constraints, max_bp_span)
    return [(db, float(w)) for db, w in zip(dbs, scores)]


def mfe_fold(seq, uses_contra_model, allows_short_hairpins, fold_score_sets, constraints=None,
             max_bp_span=0):
    """Maximum-score (MFE / Viterbi) structure of one sequence -> (dot_bracket, score).
    constraints: one constraint string (or None)."""
    return mfe_fold_batch([seq], uses_contra_model, allows_short_hairpins, fold_score_sets,
                          None if constraints is None else [constraints], max_bp_span)[0]


# ---- hard constraints (include/rnamc.h) ----

def log_partition_batch(seqs, uses_contra_model, allows_short_hairpins, fold_score_sets,
                        constraints=None, max_bp_span=0):
    """ln Z (ln Z_c under the constraints) of every sequence: the inside sweep alone, reference
    order, on the process's shared context -> f32[n_seqs]."""
    seqs = [np.asarray(s, dtype=np.uint8) for s in seqs]
    for s in seqs:
        if s.shape[0] > MAX_SEQ_LEN:
            raise _lib.RnamcError(_lib.ERR_SEQ_TOO_LONG)
    with _ctx_lock:
        return _context_for(fold_score_sets).log_partition_batch(
            seqs, uses_contra_model, allows_short_hairpins, constraints, max_bp_span)


def constraint_probability(seq, constraint, uses_contra_model, allows_short_hairpins,
                           fold_score_sets, max_bp_span=0):
    """P(c) = Z_c / Z: the probability that a structure of the ensemble satisfies the constraint
    string `constraint` (None: no string) and the span limit.  exp(ln Z_c - ln Z) from one
    two-record batch of the inside-only entry (two calls when a span limit applies: it holds for
    a whole call).  Values that f32 rounding puts above 1 are clipped."""
    seq = np.asarray(seq, dtype=np.uint8)
    n = int(seq.shape[0])
    span = _span(max_bp_span)
    if span == 0 or span >= n:
        lz = log_partition_batch([seq, seq], uses_contra_model, allows_short_hairpins,
                                 fold_score_sets, [None, constraint])
        lz0, lzc = float(lz[0]), float(lz[1])
    else:
        lz0 = float(log_partition_batch([seq], uses_contra_model, allows_short_hairpins,
                                        fold_score_sets)[0])
        lzc = float(log_partition_batch([seq], uses_contra_model, allows_short_hairpins,
                                        fold_score_sets, [constraint], span)[0])
    return min(1.0, float(np.exp(np.float64(lzc) - np.float64(lz0))))


def unpaired_probability(seq, regions, uses_contra_model, allows_short_hairpins, fold_score_sets):
    """For each inclusive region (a, b) the probability that every base a..b is unpaired (its
    accessibility) -> f64[len(regions)].  One batch: the unconstrained record and one record per
    region with 'x' over it.  Values that f32 rounding puts above 1 are clipped."""
    seq = np.asarray(seq, dtype=np.uint8)
    n = int(seq.shape[0])
    cons = [None]
    for a, b in regions:
        a, b = int(a), int(b)
        if not 0 <= a <= b < n:
            raise _lib.RnamcError(_lib.ERR_INVALID_ARG, f"region ({a}, {b}) outside 0 .. {n - 1}")
        cons.append("." * a + "x" * (b - a + 1) + "." * (n - 1 - b))
    lz = log_partition_batch([seq] * len(cons), uses_contra_model, allows_short_hairpins,
                             fold_score_sets, cons).astype(np.float64)
    return np.minimum(1.0, np.exp(lz[1:] - lz[0]))


def check_constraint(constraint, n=None, max_bp_span=0):
    """Raise RnamcError (ERR_INVALID_ARG, with the position) unless `constraint` is a valid
    constraint string (of length n when n is given)."""
    c = constraint.encode("ascii", errors="replace") if isinstance(constraint, str) else bytes(constraint)
    if n is not None and len(c) != int(n):
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, f"constraint has length {len(c)}, sequence {n}")
    if b"\0" in c:
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, f"constraint position {c.index(0)}: NUL byte")
    if len(c) == 0:
        raise _lib.RnamcError(_lib.ERR_EMPTY_SEQ)
    _lib.check(_lib.lib().rnamc_constraint_check(c, len(c), _span(max_bp_span), None, None))


def is_compatible(dot_bracket, constraint, max_bp_span=0):
    """Does the structure `dot_bracket` satisfy the constraint string (None: none) and the span
    limit?  (rnamc_constraint_check, host only; the model's own pair rules are not checked.)"""
    db = dot_bracket.encode() if isinstance(dot_bracket, str) else bytes(dot_bracket)
    if constraint is None:
        constraint = b"." * len(db)
    c = constraint.encode("ascii", errors="replace") if isinstance(constraint, str) else bytes(constraint)
    if len(c) != len(db):
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG,
                              f"constraint has length {len(c)}, structure {len(db)}")
    if len(db) == 0:
        raise _lib.RnamcError(_lib.ERR_EMPTY_SEQ)
    out = C.c_int(0)
    _lib.check(_lib.lib().rnamc_constraint_check(c, len(c), _span(max_bp_span), db, C.byref(out)))
    return bool(out.value)
