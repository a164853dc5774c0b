"""An independent f64 restatement of the maximum-score recursion (test helper, host only).

It runs over the CPU oracle's loop-score maps (oracle_lib.fold_scores: hairpin, 2-loop,
multibranch-close and accessible scores of the pairs the inside grammar admits) and the rnamc_params
constants, in the (max, +) semiring, and returns the maximum and one argmax structure.  Every sum is
taken directly over its terms (no prefix forms), by anti-diagonal, numpy over the inner index."""
import numpy as np

import oracle_lib as O

NEG = -np.inf


def _tri(n, i, j):  # diag-major packed index of the oracle's maps
    d = j - i
    return d * n - d * (d - 1) // 2 + i


def mfe_ref(params, seq, contra, short):
    """-> (max score, dot-bracket of one structure attaining it)."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    n = int(seq.shape[0])
    hp, mb, ac, tl = O.fold_scores(params.ptr, seq, contra, short)
    f = params.field
    if contra:
        ebp, eun = float(f("contra.external_score_basepair")[0]), float(f("contra.external_score_unpair")[0])
        mbp, mun = float(f("contra.multibranch_score_basepair")[0]), float(f("contra.multibranch_score_unpair")[0])
    else:
        cnb = float(f("turner.coeff_num_branches")[0])
    loops = {}  # (i, j) -> list of (k, l, score)
    for e in tl:
        loops.setdefault((int(e["i"]), int(e["j"])), []).append((int(e["k"]), int(e["l"]), float(e["score"])))

    Cm = np.full((n, n), NEG)   # what the pair (i, j) closes
    QA = np.full((n, n), NEG)   # C + accessible
    ZE = np.full((n, n), NEG)   # rightmost pair of an exterior stretch [i, j]
    ZM = np.full((n, n), NEG)   # rightmost branch of a multiloop stretch [i, j]
    Q1 = np.full((n, n), NEG)   # >= 1 branch in [i, j]
    QM = np.full((n, n), NEG)   # >= 2 branches in [i, j]

    def close_terms(i, j):
        t = []
        h = hp[_tri(n, i, j)]
        if not np.isnan(h):
            t.append((float(h), ("h",)))
        for k, l, sc in loops.get((i, j), ()):
            t.append((Cm[k, l] + sc, ("t", k, l)))
        m = mb[_tri(n, i, j)]
        if not np.isnan(m) and j - i >= 2:
            t.append((QM[i + 1, j - 1] + float(m), ("m",)))
        return t

    def zr(i, j, bp, un):  # terms of ZE / ZM (i, j): the rightmost pair (i, l)
        l = np.arange(i + 1, j + 1)
        return QA[i, i + 1:j + 1] + (bp + un * (j - l) if contra else 0.0), l

    for d in range(n):
        for i in range(n - d):
            j = i + d
            a = _tri(n, i, j)
            if d >= 1 and not np.isnan(ac[a]):
                t = close_terms(i, j)
                if t:
                    Cm[i, j] = max(v for v, _ in t)
                    QA[i, j] = Cm[i, j] + float(ac[a])
            if d >= 1:
                v, _ = zr(i, j, ebp if contra else 0.0, eun if contra else 0.0)
                ZE[i, j] = v.max()
                v, _ = zr(i, j, mbp if contra else 0.0, mun if contra else 0.0)
                ZM[i, j] = v.max()
            if d >= 2:
                k = np.arange(i + 1, j)
                r = ZM[k, j] if contra else ZE[k, j] + cnb
                QM[i, j] = (Q1[i, k - 1] + r).max()
            k = np.arange(i, j)
            if d >= 1:
                u = (ZM[k, j] + mun * (k - i)) if contra else (ZE[k, j] + cnb)
                Q1[i, j] = max(u.max(), QM[i, j])
            else:
                Q1[i, j] = QM[i, j]
    # exterior: X(j) over the prefix [0, j]
    X = np.full(n + 1, NEG)  # X[j + 1] = best of [0, j]; X[0] = 0
    X[0] = 0.0
    for j in range(n):
        unp = eun * (j + 1) if contra else 0.0
        k = np.arange(0, j)
        best = unp
        if j >= 1:
            best = max(best, (ZE[k, j] + X[k]).max())
        X[j + 1] = best

    # traceback: first term equal to the cell's value
    db = ["."] * n
    stack = [("X", 0, n - 1)]
    while stack:
        kind, i, j = stack.pop()
        if kind == "X":
            if j < 0:
                continue
            if X[j + 1] == (eun * (j + 1) if contra else 0.0):
                continue
            for k in range(0, j):
                if ZE[k, j] + X[k] == X[j + 1]:
                    stack += [("X", 0, k - 1), ("E", k, j)]
                    break
            else:
                raise AssertionError("X traceback")
        elif kind in ("E", "R"):
            bp, un = (ebp, eun) if (contra and kind == "E") else ((mbp, mun) if contra else (0.0, 0.0))
            v, ls = zr(i, j, bp, un)
            target = ZE[i, j] if kind == "E" else (ZM[i, j] if contra else ZE[i, j])
            l = int(ls[np.flatnonzero(v == target)[0]])
            db[i], db[l] = "(", ")"
            stack.append(("C", i, l))
        elif kind == "C":
            for v, how in close_terms(i, j):
                if v == Cm[i, j]:
                    break
            if how[0] == "t":
                db[how[1]], db[how[2]] = "(", ")"
                stack.append(("C", how[1], how[2]))
            elif how[0] == "m":
                stack.append(("M", i + 1, j - 1))
        elif kind == "M":
            for k in range(i + 1, j):
                r = ZM[k, j] if contra else ZE[k, j] + cnb
                if Q1[i, k - 1] + r == QM[i, j]:
                    stack += [("O", i, k - 1), ("R", k, j)]
                    break
            else:
                raise AssertionError("M traceback")
        else:  # O
            if Q1[i, j] == QM[i, j]:
                stack.append(("M", i, j))
                continue
            for k in range(i, j):
                u = (ZM[k, j] + mun * (k - i)) if contra else (ZE[k, j] + cnb)
                if u == Q1[i, j]:
                    stack.append(("R", k, j))
                    break
            else:
                raise AssertionError("O traceback")
    return float(X[n]), "".join(db)
