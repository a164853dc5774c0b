"""Replay of the Boltzmann sampler's decisions on the CPU (numpy only, no GPU).  A helper module, not
a conftest.

The grammar of rnamc_walk.h is unambiguous, so a dot-bracket row determines every decision that
produced it: `decisions` walks the same stack machine off the row alone, `Replay.terms` restates the
candidate terms of a cell (Grammar::term) over the CPU oracle's fold sums, and `Replay.audit` judges
one decision against the public contract of include/rnamc.h:

  RNG       Philox4x32-10, key = seed, counter = (decision index, t, s, 0), u = (word 0 >> 8) 2^-24
  order     candidates in the order of DESIGN.md section 9
  pick      the first candidate whose inclusive prefix of exp(term - max) exceeds u * total

The kernel forms the prefixes in f32 (wave scans carried across steps of 64 candidates); the audit
forms them in f64 and allows EPS * total on either side of the exact interval.

EPS = 2^-17, derived, not tuned.  As fractions of the total, the kernel's prefix and target differ
from the exact ones by at most
  - the adds on the way to a prefix: 6 levels of the 64-lane scan and, at the audited lengths (n <=
    700, 11 steps), 11 adds of the running sum, each rounding by <= 2^-24 of a partial sum that is
    itself <= the total: 17 * 2^-24;
  - the device expf, <= 2 ulp of every weight: 2 * 2^-24;
  - the rounding of v - mx before the exp: |v - mx| < 17 wherever a weight exceeds e^-17 = 4e-8 of
    the largest, so the difference is off by <= 2^-24 * 17 and the weight by that fraction of itself:
    17 * 2^-24 (the lighter candidates weigh less than 4e-8 of the total each, roundings included);
  - one rounding of u * run: 2^-24.
The sum is 37 * 2^-24, about 2^-18.8; EPS leaves a little over 3 x.  It is not widened: a decision
outside it is a defect of the kernel or of this replay.

`Replay.sample` is the reference sampler: the same machine driven forwards by the same Philox, in
f64.  Its mutants (MUTANTS) are the defects the audit has to reject.
"""
import numpy as np

import oracle_lib as O

X, E, C, M, O_, R = range(6)
NAMES = "XECMOR"
EPS = 2.0 ** -17
MAX_2LOOP_LEN = O.MAX_2LOOP_LEN
_MASK32 = 0xFFFFFFFF
_U64 = np.uint64
OPEN, CLOSE, DOT = ord("("), ord(")"), ord(".")


# ------------------------------------------------------------------------------------- Philox

def philox4x32_10(seed, c0, c1, c2, c3, rounds=10):
    """Philox4x32 (Salmon et al., SC'11): key = the two 32-bit halves of `seed` (low word first),
    counter words c0..c3 (ints or arrays, broadcast) -> four uint32 arrays"""
    k0, k1 = int(seed) & _MASK32, (int(seed) >> 32) & _MASK32
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    m32, sh = _U64(_MASK32), _U64(32)
    for _ in range(rounds):
        p0 = _U64(0xD2511F53) * c0
        p1 = _U64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ _U64(k0), p1 & m32, (p0 >> sh) ^ c3 ^ _U64(k1), p0 & m32
        k0 = (k0 + 0x9E3779B9) & _MASK32
        k1 = (k1 + 0xBB67AE85) & _MASK32
    return tuple(np.asarray(c).astype(np.uint32) for c in (c0, c1, c2, c3))


class Rng:
    """The sampler's uniforms.  The keyword arguments are the defects of MUTANTS; the defaults are
    the contract."""

    def __init__(self, seed, rounds=10, word=0, swap_dec_t=False, drop_high=False):
        self.seed = int(seed) & (2 ** 64 - 1)
        if drop_high:
            self.seed &= _MASK32
        self.rounds, self.word, self.swap = rounds, word, swap_dec_t

    def u(self, dec, t, s):
        """u of decision(s) `dec` of sample t of batch index s -> float64 (exact f32 values)"""
        a, b = (t, dec) if self.swap else (dec, t)
        w = philox4x32_10(self.seed, a, b, s, 0, self.rounds)[self.word]
        return (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


# ---------------------------------------------------------------------------- the stack machine

def count(typ, i, j):
    """candidates of a cell (Grammar::count)"""
    if typ == X:
        return j + 1
    if typ in (E, R):
        return j - i
    if typ == C:
        if j - i < 3:
            return 2
        L = min(MAX_2LOOP_LEN, j - i - 3)
        return 2 + (L + 1) * (L + 2) // 2
    if typ == M:
        return j - i - 1
    return j - i + 1


_SLOTS = {}


def twoloop_slots(i, j):
    """(a, b) of the 2-loop candidates of C(i, j), j - i >= 3, in order (a ascending, then b ascending)
    -> int array [count, 2]"""
    L = min(MAX_2LOOP_LEN, j - i - 3)
    if L not in _SLOTS:
        _SLOTS[L] = np.array([(a, b) for a in range(L + 1) for b in range(L + 1 - a)])
    return _SLOTS[L]


def twoloop_ab(i, j, y):
    """candidate y (1 .. cnt - 2) of C(i, j) -> (a, b)"""
    a, b = twoloop_slots(i, j)[y - 1]
    return int(a), int(b)


def twoloop_index(i, j, a, b):
    L = min(MAX_2LOOP_LEN, j - i - 3)
    return 1 + a * (2 * L + 3 - a) // 2 + b


def walk(n, pick, o_before_r=False, skip_hairpin_dec=False):
    """The machine of walk_structure: cells pop off a stack that starts with X(n - 1); pick(dec,
    type, i, j, cnt) names the candidate taken (None ends the walk).  Push order: X then E; C alone;
    O then R (R pops first).  Yields (dec, type, i, j, cnt, candidate).  The two flags are defects."""
    stack = [(X, 0, n - 1)]
    dec = 0
    while stack:
        typ, i, j = stack.pop()
        cnt = count(typ, i, j)
        y = pick(dec, typ, i, j, cnt)
        yield dec, typ, i, j, cnt, y
        if y is None:
            return
        if not (skip_hairpin_dec and typ == C and y == 0):
            dec += 1
        if typ == X:
            if y > 0:
                k = y - 1
                if k >= 1:
                    stack.append((X, 0, k - 1))
                stack.append((E, k, j))
        elif typ in (E, R):
            stack.append((C, i, i + 1 + y))
        elif typ == C:
            if y == cnt - 1:
                stack.append((M, i + 1, j - 1))
            elif y > 0:
                a, b = twoloop_ab(i, j, y)
                stack.append((C, i + 1 + a, j - 1 - b))
        elif typ == M:
            k = i + 1 + y
            if o_before_r:
                stack.append((R, k, j))
                stack.append((O_, i, k - 1))
            else:
                stack.append((O_, i, k - 1))
                stack.append((R, k, j))
        else:
            if y == j - i:
                stack.append((M, i, j))
            else:
                stack.append((R, i + y, j))


class NotInGrammar(ValueError):
    pass


def partners(row):
    row = np.frombuffer(bytes(row), dtype=np.uint8)
    n = len(row)
    pt = np.full(n, -1, dtype=np.int64)
    st = []
    for q in range(n):
        ch = row[q]
        if ch == OPEN:
            st.append(q)
        elif ch == CLOSE:
            if not st:
                raise NotInGrammar("unbalanced row")
            p = st.pop()
            pt[p], pt[q] = q, p
        elif ch != DOT:
            raise NotInGrammar(f"byte {ch} in a row")
    if st:
        raise NotInGrammar("unbalanced row")
    return pt


def decisions(row, seq=None, model=None):
    """Every decision of the walk that wrote `row`, from the dot-bracket alone -> list of (decision
    index, type, i, j, cnt, candidate).  The candidate of a cell is read off the structure: X the left
    end of the rightmost exterior pair (or none), E and R the partner of k, C hairpin / one inner pair
    / multiloop, M the left end of the rightmost branch, O one branch or more.  `seq`, if given,
    checks that every pair is canonical; the model changes no decision."""
    pt = partners(row)
    n = len(pt)
    if seq is not None:
        s = np.asarray(seq)
        for p in np.nonzero(pt > np.arange(n))[0]:
            if int(s[p]) + int(s[pt[p]]) not in (3, 5):
                raise NotInGrammar(f"pair ({p}, {pt[p]}) is not canonical")
    paired = pt >= 0
    idx = np.arange(n)
    prv = np.maximum.accumulate(np.where(paired, idx, -1))                   # last paired <= q
    nxt = np.append(np.minimum.accumulate(np.where(paired, idx, n)[::-1])[::-1], [n, n])  # first >= q

    def pick(dec, typ, i, j, cnt):
        if typ == X:
            l = int(prv[j])
            if l < 0:
                return 0
            k = int(pt[l])
            if not k < l:
                raise NotInGrammar(f"X({j}): {l} opens")
            return k + 1
        if typ in (E, R):
            l = int(pt[i])
            if not i < l <= j:
                raise NotInGrammar(f"{NAMES[typ]}({i},{j}): partner {l}")
            return l - i - 1
        if typ == C:
            k = int(nxt[i + 1])
            if k >= j:
                return 0
            l = int(pt[k])
            if not k < l < j:
                raise NotInGrammar(f"C({i},{j}): inner ({k},{l})")
            if int(nxt[l + 1]) >= j:
                a, b = k - i - 1, j - 1 - l
                if a + b > MAX_2LOOP_LEN:
                    raise NotInGrammar(f"C({i},{j}): one branch, {a} + {b} unpaired")
                return twoloop_index(i, j, a, b)
            return cnt - 1
        if typ == M:
            l = int(prv[j])
            k = int(pt[l]) if l > i else -1
            if not i < k < l:
                raise NotInGrammar(f"M({i},{j}): rightmost branch ({k},{l})")
            return k - i - 1
        k = int(nxt[i])
        if k > j:
            raise NotInGrammar(f"O({i},{j}): no branch")
        l = int(pt[k])
        if not k < l <= j:
            raise NotInGrammar(f"O({i},{j}): branch ({k},{l})")
        return k - i if int(nxt[l + 1]) > j else j - i

    return list(walk(n, pick))


def rebuild(n, decs):
    """the row that the decisions write (mark() of walk_structure)"""
    row = np.full(n, DOT, dtype=np.uint8)
    for _, typ, i, j, cnt, y in decs:
        if typ in (E, R):
            row[i], row[i + 1 + y] = OPEN, CLOSE
        elif typ == C and 0 < y < cnt - 1:
            a, b = twoloop_ab(i, j, y)
            row[i + 1 + a], row[j - 1 - b] = OPEN, CLOSE
    return row


# ------------------------------------------------------------------------------ terms and audit

class Replay:
    """One sequence under one model: the oracle's fold sums (with `mask`, the keys of a constrained
    call), the candidate terms of every cell, the audit and the reference sampler."""

    def __init__(self, params, seq, contra, short=False, mask=None):
        self.params, self.contra, self.short = params, bool(contra), bool(short)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.n = len(self.seq)
        fs = O.fold_sums_masked(params.ptr, self.seq, contra, short, mask)
        self.sums = fs
        self.z, self.zre, self.zrm = (fs["sums_external"], fs["sums_rightmost_basepairs_external"],
                                      fs["sums_rightmost_basepairs_multibranch"])
        self.qb, self.qa = fs["sums_close"], fs["sums_accessible"]
        self.qm, self.q1 = fs["sums_multibranch"], fs["sums_1ormore_basepairs"]
        f32 = np.float32
        self.ext_bp = f32(params.field("contra.external_score_basepair")[0])
        self.ext_un = f32(params.field("contra.external_score_unpair")[0])
        self.mb_bp = f32(params.field("contra.multibranch_score_basepair")[0])
        self.mb_un = f32(params.field("contra.multibranch_score_unpair")[0])
        self.cnb = f32(params.field("turner.coeff_num_branches")[0])
        self._scores, self._cells = {}, {}

    def cell_scores(self, i, j):
        key = (i, j)
        if key not in self._scores:
            self._scores[key] = O.cell_scores(self.params.ptr, self.seq, self.contra, self.short, i, j)
        return self._scores[key]

    def terms(self, typ, i, j):
        """the cnt terms of a cell in f32 with the kernel's association (Grammar::term)"""
        f32, ninf = np.float32, np.float32(-np.inf)
        with np.errstate(invalid="ignore"):
            if typ == X:
                out = np.empty(j + 1, dtype=f32)
                out[0] = self.ext_un * f32(j + 1) if self.contra else f32(0)
                if j >= 1:
                    zprev = np.concatenate([np.zeros(1, f32), self.z[0, 0:j - 1]]).astype(f32)
                    out[1:] = self.zre[0:j, j] + zprev  # zre + (x == 1 ? 0 : z)
                return out
            if typ in (E, R):
                l = np.arange(i + 1, j + 1)
                v = self.qa[i, l]
                if not self.contra:
                    return v.copy()
                bp, un = (self.ext_bp, self.ext_un) if typ == E else (self.mb_bp, self.mb_un)
                return (v + bp) + un * (j - l).astype(f32)  # (v + bp) + unpair * (j - l)
            if typ == C:
                hp, mb, _, tl = self.cell_scores(i, j)
                out = np.full(count(C, i, j), ninf, dtype=f32)
                if not np.isnan(hp):
                    out[0] = hp
                if j - i >= 2:
                    out[-1] = self.qm[i + 1, j - 1] + mb
                if len(tl):
                    ab = twoloop_slots(i, j)
                    v = self.qb[i + 1 + ab[:, 0], j - 1 - ab[:, 1]]
                    out[1:-1] = np.where(v > ninf, v + tl, ninf)
                return out
            if typ == M:
                k = np.arange(i + 1, j)
                if self.contra:
                    return self.q1[i, k - 1] + self.zrm[k, j]
                return self.q1[i, k - 1] + (self.zre[k, j] + self.cnb)  # q1 + (zre + C)
            out = np.empty(j - i + 1, dtype=f32)
            out[-1] = self.qm[i, j]
            k = np.arange(i, j)
            if self.contra:
                out[:-1] = self.zrm[k, j] + self.mb_un * (k - i).astype(f32)
                if j > i:
                    out[0] = self.zrm[i, j]
            else:
                out[:-1] = self.zre[k, j] + self.cnb
            return out

    def cell(self, typ, i, j):
        """-> (terms f32, weights exp(term - max) f64 with -inf -> 0, inclusive prefixes P f64)"""
        key = (typ, i, j)
        if key not in self._cells:
            t = self.terms(typ, i, j)
            assert len(t) == count(typ, i, j) and not np.isnan(t).any(), (key, t)
            t64 = t.astype(np.float64)
            mx = t64.max() if len(t64) else -np.inf
            if mx > -np.inf:
                w = np.where(t64 > -np.inf, np.exp(t64 - mx), 0.0)
            else:
                w = np.zeros(len(t64))
            self._cells[key] = (t, w, np.cumsum(w))
        return self._cells[key]

    def audit(self, decision, u, eps=EPS):
        """One decision against its uniform -> (passes, excess): with inclusive prefixes P and total
        T the pick c passes iff P[c-1] - eps T <= u T < P[c] + eps T; excess is the distance of u T
        from the exact interval [P[c-1], P[c]) as a fraction of T (0 inside)."""
        _, typ, i, j, cnt, c = decision
        _, w, P = self.cell(typ, i, j)
        if c is None or not 0 <= c < cnt or not w[c] > 0.0:
            return False, np.inf
        T = P[-1]
        lo, hi, x = (P[c - 1] if c else 0.0), P[c], u * T
        excess = max(lo - x, x - hi, 0.0) / T
        return bool(lo - eps * T <= x < hi + eps * T), float(excess)

    def local_score(self, decision):
        """the f32 local score that walk_structure adds at this decision, or None where it adds none"""
        f32 = np.float32
        _, typ, i, j, cnt, y = decision
        if typ == X:
            return self.ext_un * f32(j + 1) if (y == 0 and self.contra) else None
        if typ in (E, R):
            l = i + 1 + y
            sc = self.cell_scores(i, l)[2]
            if self.contra:
                bp, un = (self.ext_bp, self.ext_un) if typ == E else (self.mb_bp, self.mb_un)
                sc = f32(f32(sc + bp) + f32(un * f32(j - l)))
            return sc
        if typ == C:
            hp, mb, _, tl = self.cell_scores(i, j)
            return hp if y == 0 else (mb if y == cnt - 1 else tl[y - 1])
        if typ == M:
            return None if self.contra else self.cnb
        if y == j - i:
            return None
        if self.contra:
            return f32(self.mb_un * f32(y)) if y > 0 else None
        return self.cnb

    def log_weight(self, decs):
        """the walker's local scores summed in f32 in decision order"""
        lw = np.float32(0)
        for d in decs:
            sc = self.local_score(d)
            if sc is not None:
                lw = np.float32(lw + sc)
        return lw

    def audit_row(self, row, rng, s, t, tally=None):
        """Replay one sampled row -> (failures, f32 log-weight of the replay).  A failure is
        (decision, u, excess)."""
        decs = decisions(row, self.seq)
        assert len(decs) <= 4 * self.n + 16
        assert rebuild(self.n, decs).tobytes() == bytes(row)
        us = rng.u(np.arange(len(decs)), t, s)
        bad = []
        for d, u in zip(decs, us):
            ok, ex = self.audit(d, float(u))
            if not ok:
                bad.append((d, float(u), ex))
            if tally is not None:
                tally.add(d, ex)
        return bad, self.log_weight(decs)

    # ------------------------------------------------------------------ the reference sampler
    def sample(self, rng, s, t, mutant=None):
        """The machine driven forwards in f64 -> (row, f32 log-weight, decisions, complete).  With a
        mutant of MUTANTS the named defect; `complete` is False when a defective pick had no weight
        (the walk stops there, the decision is the last of the list)."""
        us = rng.u(np.arange(4 * self.n + 16), t, s)
        state = {"ok": True}

        def pick(dec, typ, i, j, cnt):
            _, w, P = self.cell(typ, i, j)
            T = P[-1] if len(P) else 0.0
            if not T > 0.0:
                state["ok"] = False
                return None
            x = us[dec] * T
            if mutant == "twoloop_l_ascending" and typ == C and cnt > 2:
                perm = np.array([0] + [twoloop_index(i, j, a, b)
                                       for a in range(min(MAX_2LOOP_LEN, j - i - 3) + 1)
                                       for b in range(min(MAX_2LOOP_LEN, j - i - 3) - a, -1, -1)] + [cnt - 1])
                c = int(perm[min(np.searchsorted(np.cumsum(w[perm]), x, side="right"), cnt - 1)])
            elif mutant == "exclusive_prefix":
                c = int(np.searchsorted(P, x, side="right")) + 1
                if c >= cnt:
                    c = int(np.nonzero(w > 0)[0][-1])
            elif mutant == "prefix_restarts_each_step":
                base = np.concatenate([[0.0], P])[(np.arange(cnt) // 64) * 64]
                hit = np.nonzero(P - base > x)[0]
                c = int(hit[0]) if len(hit) else int(np.nonzero(w > 0)[0][-1])
            else:
                c = int(np.searchsorted(P, x, side="right"))
            if not w[c] > 0.0:
                state["ok"] = False
                state["dead"] = c
            return c

        decs = []
        for d in walk(self.n, pick, o_before_r=(mutant == "o_before_r"),
                      skip_hairpin_dec=(mutant == "no_dec_on_hairpin")):
            decs.append(d)
            if not state["ok"]:
                break
        if not state["ok"]:
            return None, None, decs, False
        return rebuild(self.n, decs), self.log_weight(decs), decs, True


# the defects the audit must reject: name -> Rng keyword arguments (the rest act inside the machine)
MUTANTS = {
    "twoloop_l_ascending": {},
    "exclusive_prefix": {},
    "prefix_restarts_each_step": {},
    "o_before_r": {},
    "no_dec_on_hairpin": {},
    "dec_t_swapped": {"swap_dec_t": True},
    "s_within_sorted_group": {},
    "u_from_word_1": {"word": 1},
    "nine_rounds": {"rounds": 9},
    "seed_high_word_dropped": {"drop_high": True},
}


class Tally:
    """what a test audited: decisions by type and candidate count, C alternatives, the worst excess"""

    def __init__(self):
        self.decisions = 0
        self.wide = {t: 0 for t in (X, E, M, O_, R)}  # cnt > 512
        self.c_alt = {"hairpin": 0, "twoloop_a_b": 0, "multiloop": 0}
        self.cnts = set()
        self.excess = 0.0

    def add(self, d, excess):
        _, typ, i, j, cnt, y = d
        self.decisions += 1
        self.cnts.add(cnt)
        if np.isfinite(excess):
            self.excess = max(self.excess, excess)
        if typ == C:
            if y == 0:
                self.c_alt["hairpin"] += 1
            elif y == cnt - 1:
                self.c_alt["multiloop"] += 1
            elif min(twoloop_ab(i, j, y)) > 0:
                self.c_alt["twoloop_a_b"] += 1
        elif cnt > 512:
            self.wide[typ] += 1

    def wide_names(self):
        return {NAMES[t]: c for t, c in self.wide.items()}


# ------------------------------------------------------------------------------------- inputs

BOUNDARY_LENGTHS = (5, 64, 65, 512, 513, 700)  # X(n - 1) has n candidates: both sides of one step of
#                                                64 and of the 8 cached steps


def boundary_seq(n):
    return O.splitmix_seq(n, 5200 + n)


def wide_multiloop():
    """647 nt: G^12 A^3 [G^6 A^4 C^6] A^3 G^12 A^2 [26 x G^8 A^4 C^8 A^2] C^12 A^3 C^12.  Two strong
    helices around 572 bases of hairpin units (helix_inputs.hairpins): under the Turner tables nearly
    every sample closes both, so X(646) and E(0, 646) have more than 512 candidates, the outer
    multiloop picks its rightmost branch at the inner helix (R with 599 candidates), and the inner
    multiloop peels its branches off the right end one M / O pair at a time, the first of them over
    more than 512 candidates."""
    import helix_inputs as H
    small = H.run(H.G, 6) + H.run(H.A, 4) + H.run(H.C, 6)
    return H.seq(H.run(H.G, 12), H.run(H.A, 3), small, H.run(H.A, 3), H.run(H.G, 12), H.run(H.A, 2),
                 H.hairpins(8, 26, 2).tolist(), H.run(H.C, 12), H.run(H.A, 3), H.run(H.C, 12))
