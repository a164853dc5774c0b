"""CPU: the pair-mask entries of the oracle (rnamc_oracle_bpp_masked, rnamc_oracle_exact_bpp_masked)
and the max-plus compile (rnamc_oracle_mfe_exact), pinned before the GPU tests lean on them: a
neutral mask changes no byte; the masked exact and max-plus values against the f64 enumeration of
the constrained ensemble (host scorer only); the masked reference-order ln Z against the same
enumeration; the max-plus value against the independent restatement mfe_ref; the mixed recipe."""
import random

import numpy as np
import pytest

import oracle_lib as O
from constraint_masks import (allowed_matrix, binds, enumerate_constrained, mixed_case,
                              mixed_constraint, pairs_of)
from mfe_ref import mfe_ref
from test_constraints_cpu import allowed, random_constraint

MODELS = [(False, False), (True, False), (True, True)]  # (contra, allows_short_hairpins)


def tol(w, n_pairs):
    """tol() of test_gpu_mfe.py for a structure of n_pairs pairs"""
    return 4 * (n_pairs + 1) * float(np.spacing(np.float32(max(1.0, abs(w)))))


@pytest.mark.parametrize("contra,short", MODELS)
def test_neutral_mask_changes_no_byte(params, trnas, contra, short):
    seqs = [np.asarray(trnas[0][1], np.uint8)] + [O.splitmix_seq(n, 500 + n) for n in (1, 4, 5, 33, 120)]
    for seq in seqs:
        n = len(seq)
        ref, ref_z = O.bpp(params.ptr, seq, contra, short)
        ex, ex_z = O.exact_bpp(params.ptr, seq, contra, short)
        best = O.mfe_exact(params.ptr, seq, contra, short)
        _, _, ref_mats = O.bpp_dump(params.ptr, seq, contra, short)
        for mask in (None, np.ones((n, n), np.uint8)):
            b, z, mats = O.bpp_masked(params.ptr, seq, contra, short, mask, dump=True)
            assert b.tobytes() == ref.tobytes() and z.tobytes() == ref_z.tobytes()
            for got, want in zip(mats, ref_mats):
                assert got.tobytes() == want.tobytes()
            xb, xz = O.exact_bpp_masked(params.ptr, seq, contra, short, mask)
            assert xb.tobytes() == ex.tobytes() and xz == ex_z
            assert O.mfe_exact(params.ptr, seq, contra, short, mask) == best


def small_cases():
    rng = random.Random(5)
    out = []
    for k in range(8):
        n = 8 + (k * 5) % 15  # 8 .. 22, the lengths of test_exhaustive_small
        cons = random_constraint(rng, n)
        out.append((O.splitmix_seq(n, 8800 + k), cons, rng.choice([0, rng.randint(4, n)])))
    out.append((O.splitmix_seq(12, 8899), "(" + "." * 10 + ")", 0))  # a constraint pair at any bases
    return out


@pytest.mark.parametrize("contra,short", MODELS)
def test_masked_oracles_vs_enumeration(params, contra, short):
    worst_p = worst_z = worst_m = worst_r = 0.0
    for seq, cons, span in small_cases():
        n = len(seq)
        mask = allowed_matrix(cons, span)
        lz, probs, best, ws, dbs = enumerate_constrained(params, seq, cons, span, contra, short)
        xb, xz = O.exact_bpp_masked(params.ptr, seq, contra, short, mask)
        rb, rz = O.bpp_masked(params.ptr, seq, contra, short, mask)
        got = O.mfe_exact(params.ptr, seq, contra, short, mask)
        n_best = max(len(pairs_of(db)) for w, db in zip(ws, dbs) if w == best)
        idx = 0
        for d in range(n):
            for i in range(n - d):
                p, g = probs.get((i, i + d), 0.0), xb[idx]
                # equal key sets: a pair has a key exactly when a compatible structure holds it
                assert (g >= 0) == (p > 0), (cons, span, i, i + d, g, p)
                assert (rb[idx] >= 0) == (p > 0), (cons, span, i, i + d, rb[idx], p)
                if p > 0:
                    worst_p = max(worst_p, abs(g - p))
                    assert abs(g - p) <= 2e-6, (cons, span, i, i + d, g, p)
                idx += 1
        # tol() counts the f32 roundings of one structure's loop scores, which the enumeration adds
        # as the host scorer rounds them and the f64 oracles do not; ln Z, a weighted mean of such
        # errors, gets the bound of the structure with the most pairs among the best
        t = tol(best, n_best)
        worst_z, worst_m = max(worst_z, abs(xz - lz) / tol(lz, n_best)), max(worst_m, abs(got - best) / t)
        worst_r = max(worst_r, abs(float(rz) - lz))
        assert abs(xz - lz) <= tol(lz, n_best), (cons, span, xz, lz)
        assert abs(got - best) <= t, (cons, span, got, best)
        assert abs(float(rz) - lz) <= 2e-3, (cons, span, rz, lz)
    print(f"contra={contra} short={short}: masked exact max |dp| {worst_p:.2e}; |d ln Z| {worst_z:.3f} and "
          f"|d optimum| {worst_m:.3f} of tol(); reference order |d ln Z| {worst_r:.2e}")


@pytest.mark.parametrize("contra,short", MODELS)
def test_maxplus_vs_restatement(params, contra, short):
    worst = 0.0
    for n in (60, 100, 150):
        seq = O.splitmix_seq(n, 9100 + n)
        m, db = mfe_ref(params, seq, contra, short)
        got = O.mfe_exact(params.ptr, seq, contra, short)
        worst = max(worst, abs(got - m))
        assert abs(got - m) <= tol(m, len(pairs_of(db))), (n, got, m)
    print(f"contra={contra} short={short}: max |mfe_exact - mfe_ref| {worst:.2e}")


def test_mixed_recipe(params):
    """the recipe as written from n = 121, its adaptation below; the mask is the rule, pair by pair;
    the constraint binds"""
    c, span = mixed_constraint(400)
    want = ["."] * 400
    want[50], want[350], want[133], want[213], want[230], want[260] = "(", ")", "(", ")", "<", ">"
    want[80:92] = "x" * 12
    assert c == "".join(want) and span == 266
    for n in (65, 130, 257):
        seq, cons, span, mask = mixed_case(n)
        assert sorted(set(cons)) == sorted(set(".()x<>")) and span == 2 * n // 3
        for i in range(n):
            for j in range(n):
                assert bool(mask[i, j]) == (i < j and allowed(cons, span, i, j)), (n, i, j)
        plain, _ = O.bpp(params.ptr, seq, False, False)
        masked, _ = O.bpp_masked(params.ptr, seq, False, False, mask)
        ok, kc, kp = binds(masked, plain)
        assert ok, (n, kc, kp)
