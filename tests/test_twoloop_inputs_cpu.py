"""The conditions test_gpu_twoloop_slots.py rests on, stated with the CPU oracle alone, so that a
change of tables cannot turn the GPU tests vacuous (tests/twoloop_inputs.py has the inputs).

  * the masks come from constraint_masks.allowed_matrix and equal "the stem pairs and nothing else";
  * slot use u = P((i, j) and (k, l) both paired): at least 0.10 for every family S record in all
    three models, at least 0.01 for every family N record (measured with synthetic(1): S 0.505 Turner /
    0.415 CONTRAfold, N 0.0162 Turner / 0.149 CONTRAfold / 0.048 with short hairpins);
  * the best structure of every family S record is the full one, both stems around the (a, b) loop;
  * P(0, n - 1) of every family E record, a pure two-loop term, is at least 1e-6 (measured 2.2e-5 ..
    0.99 Turner, 3.2e-4 .. 0.85 CONTRAfold).
"""
import numpy as np
import pytest

import twoloop_inputs as T
from constraint_masks import pairs_of


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def test_slots_and_shapes():
    assert len(T.SLOTS) == 496 and len(set(T.SLOTS)) == 496 and (0, 0) in T.SLOTS and (0, 30) in T.SLOTS
    assert all(a + b <= T.MAX_2LOOP for a, b in T.SLOTS)
    assert len(T.family_s()) == 4 * 496 and len(T.family_e()) == 496 and len(T.family_n()) == 496
    assert max(r.n for r in T.family_s()) <= 66
    for a, b in ((0, 0), (3, 17), (30, 0)):
        four = [r for r in T.family_s() if (r.a, r.b) == (a, b)]
        assert [r.pl for r in four] == [0, 1, 2, 3] and all(r.pr == (r.pl + b) % 3 for r in four)
        assert sorted(r.ijkl[0] % 4 for r in four) == [0, 1, 2, 3]  # the row mod 4
    for r in T.family_e():
        assert (r.ijkl[0], r.ijkl[1]) == (0, r.n - 1)
    for r in T.family_n():
        assert r.cons is None and r.mask is None
        assert set(np.unique(r.seq)) <= {T.A, T.C, T.G}


@pytest.mark.parametrize("family", ["S", "E", "N"])
def test_layout_closes_exactly_the_slot(family):
    for r in {"S": T.family_s, "E": T.family_e, "N": T.family_n}[family]():
        i, j, k, l = r.ijkl
        mo, mi, h = r.shape["mo"], r.shape["mi"], r.shape["h"]
        assert (k - i - 1, j - l - 1) == (r.a, r.b), r
        assert l - k + 1 == 2 * mi + h >= 14
        assert r.outer[-1] == (i, j) and r.inner[0] == (k, l) and len(r.outer) == mo and len(r.inner) == mi
        assert r.outer[0] == (r.pl, r.n - 1 - r.pr)
        assert all((r.seq[p], r.seq[q]) == (T.G, T.C) for p, q in r.outer), r
        assert all((r.seq[p], r.seq[q]) == (T.C, T.G) for p, q in r.inner), r
        assert sorted(pairs_of(r.full)) == sorted(r.outer + r.inner)
        # the same draws whatever surrounds them: fill(pl), fill(a), fill(h), fill(b), fill(pr) in that order
        if family != "N":
            rng = np.random.default_rng(1000 * r.a + 10 * r.b)
            cuts = [(0, r.pl), (i + 1, r.a), (k + mi, h), (l + 1, r.b), (r.n - r.pr, r.pr)]
            for start, m in cuts:
                assert np.array_equal(r.seq[start:start + m], rng.integers(0, 4, m)), r


@pytest.mark.parametrize("family", ["S", "E"])
def test_mask_is_the_stem_pairs_only(family):
    for r in {"S": T.family_s, "E": T.family_e}[family]():
        want = np.zeros((r.n, r.n), np.uint8)
        for p, q in r.outer + r.inner:
            want[p, q] = 1
        assert np.array_equal(r.mask, want), r
        assert r.cons.count("(") == r.cons.count(")") == len(r.outer) + len(r.inner)
        assert set(r.cons) <= set("()x")


@pytest.mark.parametrize("contra,short", T.MODELS)
def test_slot_use_family_s(contra, short):
    recs = T.family_s()
    u = np.array(T.slot_use("S", contra, short))
    w = int(np.argmin(u))
    print(f"contra={contra} short={short}: family S slot use {u.min():.4f} ({recs[w]}) .. {u.max():.6f}")
    assert np.all(u >= 0.10), [recs[x] for x in np.flatnonzero(u < 0.10)][:10]
    # u is a joint probability: never above either pair's own
    for r, v, (xb, _) in zip(recs, u, T.exact("S", contra, short)):
        i, j, k, l = r.ijkl
        assert v <= min(xb[T.index(r.n, i, j)], xb[T.index(r.n, k, l)]) + 1e-12, r


@pytest.mark.parametrize("contra,short", T.MODELS)
def test_slot_use_family_n(contra, short):
    recs = T.family_n()
    u = np.array(T.slot_use("N", contra, short))
    w = int(np.argmin(u))
    print(f"contra={contra} short={short}: family N slot use {u.min():.4f} ({recs[w]}) .. {u.max():.6f}, "
          f"{int((u < 0.05).sum())} below 0.05")
    assert np.all(u >= 0.01), [recs[x] for x in np.flatnonzero(u < 0.01)][:10]


@pytest.mark.parametrize("contra,short", T.MODELS)
def test_optimum_is_the_full_structure(contra, short):
    recs = T.family_s()
    best = T.optimum("S", contra, short)
    full = T.full_scores("S", contra, short)
    bad = [(r, o, f) for r, o, f in zip(recs, best, full) if not abs(o - f) <= T.tol(o, r.full)]
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("contra,short", T.MODELS)
def test_family_e_outer_pair_is_visible(contra, short):
    recs = T.family_e()
    ex = T.exact("E", contra, short)
    p = np.array([xb[T.index(r.n, 0, r.n - 1)] for r, (xb, _) in zip(recs, ex)])
    lz = max(abs(z) for _, z in ex)
    print(f"contra={contra} short={short}: family E P(0, n - 1) {p.min():.3g} .. {p.max():.3g}, |ln Z| <= {lz:.2f}")
    assert np.all(p >= 1e-6), [recs[x] for x in np.flatnonzero(p < 1e-6)][:10]
    # under the pair sit the (a, b) loop, the loops (a + t, b + t) onto the inner stem's next pairs and
    # the bare hairpin: the slot itself carries most of it (measured: at least 0.65 Turner, 0.54
    # CONTRAfold), so a relative check of the pair sees the slot
    share = np.array(T.slot_use("E", contra, short)) / p
    assert np.all(share >= 0.5), [recs[x] for x in np.flatnonzero(share < 0.5)][:10]
