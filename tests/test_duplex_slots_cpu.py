"""The conditions test_gpu_duplex_slots.py rests on, stated with the f64 reference alone
(tests/duplex_ref.py over the CPU oracle's loop scores), so that a change of tables cannot turn the GPU
tests vacuous (tests/duplex_slots.py has the inputs).  For every record of families D and T and both
models, under the seeded synthetic tables:

  * the cells that can pair are exactly the G-C cells of the stems;
  * every designed pair has P >= 0.4;
  * the designed duplex, the twelve stem pairs around the (a, b) loop, is the optimum;
  * it leads the best duplex that lacks one of its pairs by at least 0.25 nats (family D and a fixed
    fifth of family T: the flanks of a family T record are further A's, which the model never reads);
  * its share exp(w - ln Z) of the ensemble is at least 0.3;
  * the closing and the enclosed cell of every family T placement sit on the lane the placement
    names, in the sweep it names.

P, ln Z, the optimum and the share come from tests/golden/duplex_slots_f64.npz; every tenth record
is evaluated again here and must agree to 1e-12.
"""
import numpy as np
import pytest

import duplex_ref as R
import duplex_slots as S

MODELS = [False, True]


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def test_families():
    recs, d, t = S.records(), S.family_d(), S.family_t()
    assert [(r.a, r.b) for r in d] == S.SLOTS and len(set(S.SLOTS)) == 496
    assert all(a + b <= R.MAX_LOOP for a, b in S.SLOTS)
    assert all(r.flanks == (0, 0, 0, 0) for r in d)
    slots = S.t_slots()
    edge = [s for s in S.SLOTS if 0 in s]
    rim = [s for s in S.SLOTS if sum(s) == R.MAX_LOOP]
    assert len(edge) == 61 and len(rim) == 31 and set(edge) <= set(slots) and set(rim) <= set(slots)
    assert len(slots) == len(set(slots)) == 90 + 58
    # eight placements a slot; a stack or a bulge has its two cells on neighbouring lanes, so two coincide
    for s in slots:
        mine = [r for r in t if (r.a, r.b) == s]
        assert len(mine) == 8 - (s[0] == 0) - (s[1] == 0), s
        assert len({r.flanks for r in mine}) == len(mine)
        assert {(r.lanes, r.cell, r.lane) for r in mine} <= {(x, y, z) for x in "AB" for y in ("closing", "enclosed")
                                                             for z in (0, 127)}
    assert [r.idx for r in recs] == list(range(len(recs))) and len(recs) == len(d) + len(t)
    assert max(max(r.na, r.nb) for r in recs) < S.NEIGHBOUR_LEN
    for by_col in (False, True):
        seqs, pairs = S.call(by_col)
        assert len(pairs) == len(recs) + 1
        na, nb = [len(seqs[p]) for p, _ in pairs], [len(seqs[q]) for _, q in pairs]
        assert (max(nb) < max(na)) == by_col  # the host's rule (rnamc_entries_duplex.cpp)
        assert all(np.array_equal(seqs[p], r.seq_a) and np.array_equal(seqs[q], r.seq_b)
                   for r, (p, q) in zip(recs, pairs))


def test_strands_and_designed_duplex():
    for r in S.records():
        s1, s2 = r.stems
        assert len(s1) == len(s2) == S.STEM and set(s1 + s2) <= set("GC")
        pl, pr, ql, qr = r.flanks
        assert r.sa == "A" * pl + s1 + "A" * r.a + s2 + "A" * pr
        assert r.sb == "A" * ql + S.rc(s2) + "A" * r.b + S.rc(s1) + "A" * qr
        assert "U" not in r.sa + r.sb
        assert len(r.chain) == 12 and r.chain[5] == r.closing and r.chain[6] == r.enclosed
        (i, j), (k, l) = r.closing, r.enclosed
        assert (k - i - 1, j - l - 1) == (r.a, r.b)
        for (p, q), (u, v) in zip(r.chain, r.chain[1:]):
            assert (u - p - 1, q - v - 1) in ((0, 0), (r.a, r.b))
        assert all({r.sa[p], r.sb[q]} == {"G", "C"} for p, q in r.chain)
        # the cells that can pair: a stem base of A with the complementary stem base of B, nothing else
        can = {(p, q) for p in range(r.na) for q in range(r.nb) if R.canonical(int(r.seq_a[p]), int(r.seq_b[q]))}
        want = {(p, q) for p in range(r.na) for q in range(r.nb)
                if r.sa[p] in "GC" and r.sb[q] in "GC" and r.sa[p] != r.sb[q]}
        assert can == want and set(r.chain) <= can
        assert all(r.sa[p] == "A" for p in range(r.na) if not any(p == c[0] for c in r.chain))
        assert all(r.sb[q] == "A" for q in range(r.nb) if not any(q == c[1] for c in r.chain))


def test_tile_edge_layout():
    """k_duplex_step runs a lane per position of B when it steps along A (by_col = 0) and a lane per
    position of A when it steps along B; a workgroup owns 128 consecutive lanes"""
    seen = set()
    for r in S.family_t():
        by_col = r.lanes == "A"
        cell = r.closing if r.cell == "closing" else r.enclosed
        v, n_lanes = S.lane_of(r, cell, by_col)
        assert v == (cell[0] if by_col else cell[1]) and n_lanes == (r.na if by_col else r.nb)
        assert v % S.BLOCK == r.lane and n_lanes >= S.BLOCK + 1
        # lane 127 of the first workgroup with a second one behind it, lane 0 of the second
        assert v == (S.BLOCK if r.lane == 0 else S.BLOCK - 1) and v + 1 < n_lanes
        seen.add((r.lanes, r.cell, r.lane))
    assert len(seen) == 8


@pytest.mark.parametrize("contra", MODELS)
def test_fixture_is_the_reference(contra):
    """every tenth record evaluated again: the fixture's values to 1e-12"""
    g = S.golden()
    live = S.live(contra)
    assert len(live) == len(S.records()[::10]) >= 160
    assert {S.records()[x].family for x in live} == {"D", "T"}
    for x, ref in live.items():
        for f in S.FIELDS:
            want = g[(f, contra)][x]
            assert np.all(np.abs(getattr(ref, f) - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), (S.records()[x], f)
        r = S.records()[x]
        cells = r.sa.count("G") * r.sb.count("C") + r.sa.count("C") * r.sb.count("G")
        assert ref.live.all() and len(ref.p) == cells  # every G-C cell of the stems has a finite F and G


@pytest.mark.parametrize("contra", MODELS)
def test_designed_pairs_and_share(contra):
    g, recs = S.golden(), S.records()
    p, share = g[("designed", contra)].min(axis=1), g[("share", contra)]
    for fam in "DT":
        sel = np.array([r.family == fam for r in recs])
        print(f"contra={contra} family {fam}: designed P {p[sel].min():.4f} .. {p[sel].max():.4f}, "
              f"share {share[sel].min():.4f} .. {share[sel].max():.4f}")
    assert p.shape == (len(recs),)
    assert np.all(p >= 0.4), [recs[x] for x in np.flatnonzero(p < 0.4)][:10]
    assert np.all(share >= 0.3), [recs[x] for x in np.flatnonzero(share < 0.3)][:10]
    # the designed duplex is the optimum: its score w = ln Z + ln share is the f64 maximum
    w = g[("log_z", contra)] + np.log(share)
    best = g[("best", contra)]
    assert np.all(np.abs(w - best) <= 1e-9 * np.maximum(1.0, np.abs(best)))


@pytest.mark.parametrize("contra", MODELS)
def test_margin(contra):
    g, recs = S.golden(), S.margin_records()
    assert len(recs) >= 496 + len(S.family_t()) // 5 and {r.lanes for r in recs} == {None, "A", "B"}
    res = S.margins(contra)
    m = np.array([x[0] for x in res])
    print(f"contra={contra}: margin {m.min():.4f} .. {m.max():.4f} nats over {len(recs)} records")
    assert np.all(m >= 0.25), [recs[x] for x in np.flatnonzero(m < 0.25)][:10]
    for r, (_, w, best) in zip(recs, res):
        # the graph form's optimum is the recurrences' and is the designed duplex
        assert abs(best - g[("best", contra)][r.idx]) <= 1e-12 * max(1.0, abs(best)), r
        assert abs(w - best) <= 1e-12 * max(1.0, abs(best)), r


@pytest.mark.parametrize("contra", MODELS)
def test_margin_graph_is_the_literal_form(contra):
    """ChainGraph against the literal procedure (outer, inner and T rows of a designed pair set to
    -inf, Recurrences evaluated again), every pair of six records"""
    t = S.family_t()
    for r in (S.family_d()[0], S.family_d()[17], S.family_d()[495], S.family_d()[250], t[3], t[-1]):
        sc = R.Scores(S.tables(), r.seq_a, r.seq_b, contra)
        graph = S.ChainGraph(sc)
        assert abs(graph.best() - R.Recurrences(sc).best) <= 1e-12
        for c in r.chain:
            assert abs(graph.best(c) - S.best_lacking(sc, c)) <= 1e-12, (r, c)
