"""An independent f64 reference of the duplex model (include/rnamc.h; test
helper, host only).  It never calls the library's scorer: every loop score comes from the CPU
oracle's cell_scores on S' = A + three filler bases + B (2-loops, outer end) and R' = B + three filler
bases + A (inner end; minus basepair_scores under CONTRAfold).  The filler lifts every intermolecular
pair over the oracle's Turner span check; no 2-loop or end score of a duplex reads it.

On top of the scores: the exhaustive enumeration of every duplex (small strands), and the direct f64
evaluation of the inside / outside / max-plus recurrences (any size)."""
import numpy as np

import oracle_lib as O

NEG = -np.inf
MAX_LOOP = O.MAX_2LOOP_LEN
SLOTS = [(a, b) for a in range(MAX_LOOP + 1) for b in range(MAX_LOOP + 1 - a)]  # (a, b) ascending
SLOT_OF = {ab: x for x, ab in enumerate(SLOTS)}
DA = np.array([a + 1 for a, _ in SLOTS])
DB = np.array([b + 1 for _, b in SLOTS])
FILLER = np.zeros(3, dtype=np.uint8)


_SLOT_INDEX = {}


def _slot_index(L):
    """positions in SLOTS of the oracle's 2-loop list of a closing pair whose span admits a + b <= L"""
    if L not in _SLOT_INDEX:
        _SLOT_INDEX[L] = np.array([SLOT_OF[(a, b)] for a in range(L + 1) for b in range(L + 1 - a)], dtype=np.int64)
    return _SLOT_INDEX[L]


def canonical(x, y):
    return (x + y == 3) or (x + y == 5)


class Scores:
    """outer / inner: (nA, nB) f64, -inf where (A[i], B[j]) is not canonical; T[i, j, slot]: the score
    of the 2-loop closed by (i, j) enclosing (i + 1 + a, j - 1 - b), -inf where that pair does not
    exist or is not canonical"""

    def __init__(self, params, a, b, contra):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        b = np.ascontiguousarray(b, dtype=np.uint8)
        self.a, self.b, self.contra = a, b, contra
        na, nb = len(a), len(b)
        self.na, self.nb = na, nb
        s1 = np.concatenate([a, FILLER, b])
        r1 = np.concatenate([b, FILLER, a])
        bp = params.field("contra.basepair_scores").reshape(4, 4) if contra else None
        self.outer = np.full((na, nb), NEG)
        self.inner = np.full((na, nb), NEG)
        self.T = np.full((na, nb, len(SLOTS)), NEG)
        for i in range(na):
            for j in range(nb):
                if not canonical(int(a[i]), int(b[j])):
                    continue
                jj = na + 3 + j
                _, _, acc, tl = O.cell_scores(params.ptr, s1, contra, False, i, jj)
                self.outer[i, j] = float(acc)
                idx = _slot_index(min(MAX_LOOP, jj - i - 3))  # the oracle's list -> SLOTS
                ok = (i + DA[idx] < na) & (j - DB[idx] >= 0) & ~np.isnan(tl)
                self.T[i, j, idx[ok]] = tl[ok].astype(np.float64)
                _, _, acc_r, _ = O.cell_scores(params.ptr, r1, contra, False, j, nb + 3 + i)
                self.inner[i, j] = float(acc_r) - (float(bp[int(b[j]), int(a[i])]) if contra else 0.0)

    def chain_score(self, chain):
        """f64 log weight of [(i, j), ...] (outer end first); -inf outside the model"""
        w = self.outer[chain[0]]
        for (i, j), (k, l) in zip(chain, chain[1:]):
            x, y = k - i - 1, j - l - 1
            if x < 0 or y < 0 or x + y > MAX_LOOP:
                return NEG
            w = w + self.T[i, j, SLOT_OF[(x, y)]]
        return float(w + self.inner[chain[-1]])


def lse(x):
    x = np.asarray(x, dtype=np.float64)
    m = np.max(x) if x.size else NEG
    if not m > NEG:
        return NEG
    return float(m + np.log(np.sum(np.exp(x - m))))


def tie_key(chain):
    """the order in which the traceback meets the duplexes: start pair by (i, j); at a cell the inner end
    before any enclosed pair, those by (a, b)"""
    key = [(chain[0][0], chain[0][1], 0)]
    for (i, j), (k, l) in zip(chain, chain[1:]):
        key.append((1, k - i - 1, j - l - 1))
    key.append((0, 0, 0))
    return key


class Enumeration:
    """every duplex of the pair: ln Z, P, pa, pb, the maximum and its maximisers, all f64"""

    def __init__(self, sc):
        self.chains, self.weights = [], []
        na, nb = sc.na, sc.nb

        succ = {}  # cell -> its enclosed pairs [(k, l, score), ...] in (a, b) order

        def extend(chain, w):
            i, j = chain[-1]
            self.chains.append(tuple(chain))
            self.weights.append(w + sc.inner[i, j])
            if (i, j) not in succ:
                xs = np.nonzero(sc.T[i, j] > NEG)[0]
                succ[(i, j)] = [(i + int(DA[x]), j - int(DB[x]), float(sc.T[i, j, x])) for x in xs]
            for k, l, t in succ[(i, j)]:
                chain.append((k, l))
                extend(chain, w + t)
                chain.pop()

        for i in range(na):
            for j in range(nb):
                if sc.outer[i, j] > NEG:
                    extend([(i, j)], sc.outer[i, j])
        self.count = len(self.chains)
        w = np.array(self.weights, dtype=np.float64)
        self.log_z = lse(w)
        self.P = np.zeros((na, nb))
        for chain, x in zip(self.chains, w):
            p = np.exp(x - self.log_z)
            for i, j in chain:
                self.P[i, j] += p
        self.pa, self.pb = self.P.sum(axis=1), self.P.sum(axis=0)
        self.best = float(w.max()) if self.count else NEG
        order = np.argsort(-w, kind="stable")
        tied = [self.chains[x] for x in order if w[x] >= self.best - 1e-9 * (1.0 + abs(self.best))]
        self.maximisers = set(tied)
        self.pick = min(tied, key=tie_key) if tied else None
        # how far below the maximum the best duplex outside the tied set lies (inf: there is none)
        rest = [w[x] for x in order if self.chains[x] not in self.maximisers]
        self.margin = float(self.best - max(rest)) if rest else np.inf


class Recurrences:
    """the model's recurrences evaluated directly in f64: F, G, ln Z, P, pa, pb, max-plus F and best"""

    def __init__(self, sc):
        na, nb = sc.na, sc.nb
        F = np.full((na, nb), NEG)
        Mx = np.full((na, nb), NEG)
        for i in range(na - 1, -1, -1):
            for j in range(nb):
                if not sc.inner[i, j] > NEG:
                    continue
                ks, ls = i + DA, j - DB
                ok = (ks < na) & (ls >= 0)
                t = sc.T[i, j, ok]
                F[i, j] = lse(np.concatenate([[sc.inner[i, j]], t + F[ks[ok], ls[ok]]]))
                Mx[i, j] = np.max(np.concatenate([[sc.inner[i, j]], t + Mx[ks[ok], ls[ok]]]))
        G = np.full((na, nb), NEG)
        slot = np.arange(len(SLOTS))
        for k in range(na):
            for l in range(nb - 1, -1, -1):
                if not sc.outer[k, l] > NEG:
                    continue
                iss, jss = k - DA, l + DB
                ok = (iss >= 0) & (jss < nb)
                t = sc.T[iss[ok], jss[ok], slot[ok]]
                G[k, l] = lse(np.concatenate([[sc.outer[k, l]], t + G[iss[ok], jss[ok]]]))
        self.F, self.G, self.Mx = F, G, Mx
        self.log_z = lse((sc.outer + F).ravel())
        with np.errstate(invalid="ignore"):
            self.P = np.where((F > NEG) & (G > NEG), np.exp(F + G - self.log_z), 0.0) if self.log_z > NEG \
                else np.zeros((na, nb))
        self.pa, self.pb = self.P.sum(axis=1), self.P.sum(axis=0)
        self.best = float(np.max(sc.outer + Mx)) if na * nb else NEG


def encode(s):
    return np.array(["ACGU".index(ch) for ch in s], dtype=np.uint8)
