"""RNA-RNA duplex folding (the RNAduplex / RNAhybrid / RNAplex question): where a short RNA binds a
long one, and how strongly.  For every pair of strands (A, B) the partition function over all
duplexes -- chains of intermolecular canonical pairs joined by stacks, bulges and interior loops of
at most 30 unpaired bases, no intramolecular pairs --, the probability of every pair (i, j), the
per-base bound probabilities and the best duplex, all on the GPU (rnamc_duplex_batch; the model is
stated in include/rnamc.h and DESIGN.md section 19).  No initiation term is added."""
import ctypes as C

import numpy as np

from . import _lib
from . import mccaskill_algo as _M


class DuplexFold:
    """One pair of strands.  log_z: ln Z (-inf without a canonical intermolecular pair); probs: (nA, nB)
    f32 or None; bound_a / bound_b: per-base probabilities of being paired with the other strand;
    structure: A's bases as '(' / '.', '&', B's bases as ')' / '.' (None without want_best);
    best_score: the log weight of that duplex (f32, the max-plus sweep's value)."""

    def __init__(self, n_a, n_b, log_z, probs, bound_a, bound_b, structure, best_score):
        self.n_a, self.n_b = n_a, n_b
        self.log_z = log_z
        self.probs = probs
        self.bound_a, self.bound_b = bound_a, bound_b
        self.structure = structure
        self.best_score = best_score

    def pairs(self):
        """the best duplex as [(i, j), ...], outer end first: i ascending in A, j descending in B"""
        if self.structure is None:
            return None
        return structure_pairs(self.structure)

    def __repr__(self):
        return f"DuplexFold({self.n_a}x{self.n_b}, log_z={self.log_z:.6g}, structure={self.structure!r})"


def structure_pairs(structure):
    """'((..(&)..))' -> [(0, 4), (1, 3), (4, 0)]"""
    a, _, b = structure.partition("&")
    opens = [x for x, ch in enumerate(a) if ch == "("]
    closes = [x for x, ch in enumerate(b) if ch == ")"]
    if len(opens) != len(closes):
        raise ValueError(f"unbalanced duplex structure {structure!r}")
    return list(zip(opens, reversed(closes)))


def pairs_structure(n_a, n_b, chain):
    """structure_pairs backwards"""
    a, b = ["."] * n_a, ["."] * n_b
    for i, j in chain:
        a[i], b[j] = "(", ")"
    return "".join(a) + "&" + "".join(b)


def _duplex_batch(entry, handle, seqs, pairs, uses_contra_model, want_probs=True, want_best=True,
                  want_bound=True):
    """rnamc_duplex_batch / _multi on `handle` -> list of DuplexFold, one per pair"""
    seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
    lens, offsets, bases = _M._pack(seqs)
    pa = np.ascontiguousarray([p[0] for p in pairs], dtype=np.uint32)
    pb = np.ascontiguousarray([p[1] for p in pairs], dtype=np.uint32)
    n_pairs = len(pairs)
    if n_pairs and (int(pa.max()) >= len(seqs) or int(pb.max()) >= len(seqs)):
        raise _lib.RnamcError(_lib.ERR_INVALID_ARG, "a pair names a sequence past the end")
    na = lens[pa].astype(np.uint64) if n_pairs else np.zeros(0, np.uint64)
    nb = lens[pb].astype(np.uint64) if n_pairs else np.zeros(0, np.uint64)
    out_off = np.zeros(n_pairs + 1, dtype=np.uint64)
    np.cumsum(na * nb, out=out_off[1:])
    base_off = np.zeros(n_pairs + 1, dtype=np.uint64)
    np.cumsum(na + nb, out=base_off[1:])
    probs = np.empty(int(out_off[-1]), np.float32) if want_probs else None
    bound = np.empty(int(base_off[-1]), np.float32) if want_bound else None
    structs = np.empty(int(base_off[-1]), np.uint8) if want_best else None
    best = np.empty(n_pairs, np.float32) if want_best else None
    logz = np.empty(n_pairs, np.float32)

    def ptr(x):
        return None if x is None else x.ctypes.data

    _lib.check(entry(handle, len(seqs), bases.ctypes.data, offsets.ctypes.data, n_pairs, pa.ctypes.data,
                     pb.ctypes.data, int(bool(uses_contra_model)), ptr(probs), out_off.ctypes.data,
                     ptr(bound), ptr(bound), base_off.ctypes.data, logz.ctypes.data, ptr(structs),
                     base_off.ctypes.data, ptr(best)))
    res = []
    for p in range(n_pairs):
        a, b = int(na[p]), int(nb[p])
        o, q = int(out_off[p]), int(base_off[p])
        structure = None
        if want_best:
            row = structs[q:q + a + b].tobytes().decode("ascii")
            structure = row[:a] + "&" + row[a:]
        res.append(DuplexFold(
            a, b, float(logz[p]),
            probs[o:o + a * b].reshape(a, b) if want_probs else None,
            bound[q:q + a] if want_bound else None, bound[q + a:q + a + b] if want_bound else None,
            structure, float(best[p]) if want_best else None))
    return res


def _entry_of(ctx, tables):
    """(entry, handle) of a Context, a Pool or -- None -- the process's pool (every visible device)"""
    L = _lib.lib()
    if ctx is None:
        return L.rnamc_duplex_batch_multi, _M._pool_for(tables)._h
    ctx.sync_params(tables)
    if isinstance(ctx, _M.Pool):
        return L.rnamc_duplex_batch_multi, ctx._h
    return L.rnamc_duplex_batch, ctx._h


def duplex_fold_batch(seqs, pairs, uses_contra_model, tables, want_probs=True, want_best=True, ctx=None):
    """Every pair (a, b) of `pairs` (indices into `seqs`, base codes 0..3) folded as a duplex of
    A = seqs[a] and B = seqs[b] -> list of DuplexFold.  want_probs=False keeps every nA x nB matrix
    on the device; want_best=False skips the max-plus sweep.  ctx: a Context or a Pool; None = the
    process's devices."""
    with _M._ctx_lock:
        entry, handle = _entry_of(ctx, tables)
        return _duplex_batch(entry, handle, list(seqs), list(pairs), uses_contra_model, want_probs, want_best)


def duplex_fold(a, b, uses_contra_model, tables, want_probs=True, want_best=True, ctx=None):
    """duplex_fold_batch of one pair -> DuplexFold"""
    return duplex_fold_batch([a, b], [(0, 1)], uses_contra_model, tables, want_probs, want_best, ctx)[0]


class DuplexScan:
    """One query against many targets: folds[t] is the DuplexFold of (query, target t)."""

    def __init__(self, folds):
        self.folds = folds
        self.log_z = np.array([f.log_z for f in folds], dtype=np.float32)

    def top(self, k):
        """the k targets with the largest ln Z, best first (ties: the earlier target)
        -> [(target index, DuplexFold), ...]"""
        order = np.argsort(-self.log_z.astype(np.float64), kind="stable")[:k]
        return [(int(t), self.folds[int(t)]) for t in order]

    def __len__(self):
        return len(self.folds)


def duplex_scan(query, targets, uses_contra_model, tables, want_probs=False, want_best=True, ctx=None):
    """`query` (strand A) against every target (strand B) -> DuplexScan.  By default no nA x nB matrix
    leaves the device: ln Z, the bound probabilities and the best duplex per target do."""
    targets = list(targets)
    seqs = [query] + targets
    pairs = [(0, t + 1) for t in range(len(targets))]
    return DuplexScan(duplex_fold_batch(seqs, pairs, uses_contra_model, tables, want_probs, want_best, ctx))


def duplex_score(a, b, chain, uses_contra_model, tables):
    """Log weight of one duplex (rnamc_duplex_score, host only): `chain` is [(i, j), ...], outer end
    first, or a structure string.  -inf for a chain outside the model (a non-canonical pair, a loop of
    more than 30); exp(score - ln Z) is the duplex's probability."""
    if isinstance(chain, str):
        chain = structure_pairs(chain)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    ci = np.ascontiguousarray([p[0] for p in chain], dtype=np.uint32)
    cj = np.ascontiguousarray([p[1] for p in chain], dtype=np.uint32)
    out = C.c_double()
    _lib.check(_lib.lib().rnamc_duplex_score(tables.ptr, a.ctypes.data, a.shape[0], b.ctypes.data, b.shape[0],
                                             len(chain), ci.ctypes.data, cj.ctypes.data,
                                             int(bool(uses_contra_model)), C.byref(out)))
    return out.value
