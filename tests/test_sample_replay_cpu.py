"""The CPU side of the sampler's decision audit (tests/sample_replay.py): the Philox known answers,
the new oracle entries, `decisions` against the reference sampler's own walk, the reference
sampler's distribution against the brute-force ensemble, and the teeth: every defect of
sample_replay.MUTANTS is rejected by the audit that the GPU test applies to the kernel."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import sample_replay as SR
from test_gpu_sample import DIST_SEQS, pair_freq, sigma

MODELS = [(False, False), (True, False), (True, True)]
SEED = 0x9E3779B97F4A7C15  # high word set: the key's second word matters


@functools.lru_cache(maxsize=None)
def _tables():
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(1)  # the tables of the session's `params` fixture


@functools.lru_cache(maxsize=None)
def replay(key, contra, short):
    return SR.Replay(_tables(), INPUTS[key], contra, short)


INPUTS = {}


@pytest.fixture(scope="module")
def inputs(built, trnas):
    """one batch, in this order: DIST_SEQS (s = 0..7), two tRNAs (8, 9), the n = 700 input (10)"""
    for k, s in enumerate(DIST_SEQS):
        INPUTS[f"dist{k}"] = s
    INPUTS["trna0"], INPUTS["trna1"] = trnas[0][1], trnas[3][1]
    INPUTS["n700"] = SR.boundary_seq(700)
    return list(INPUTS)


def test_philox_known_answers():
    """the three published Philox4x32-10 vectors (Random123 kat_vectors): key words; counter -> output"""
    kat = [((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
            "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for (k0, k1), ctr, want in kat:
        got = SR.philox4x32_10(k0 | (k1 << 32), *ctr)
        assert " ".join(f"{int(w):08x}" for w in got) == want
    # arrays broadcast to the scalar answers, and u is word 0's top 24 bits
    w = SR.philox4x32_10(SEED, np.arange(5), 3, 2, 0)
    for d in range(5):
        assert [int(x[d]) for x in w] == [int(x) for x in SR.philox4x32_10(SEED, d, 3, 2, 0)]
    assert SR.Rng(SEED).u(np.arange(5), 3, 2).tolist() == [(int(x) >> 8) / 2 ** 24 for x in w[0]]


@pytest.mark.parametrize("contra,short", MODELS)
def test_cell_scores_match_fold_scores(params, trnas, contra, short):
    """rnamc_oracle_cell_scores bit for bit against the maps of O.fold_scores on two tRNAs: every
    key's hairpin, multibranch-close and accessible score, every 2-loop insert at its (a, b) slot in
    the reference's visiting order, and NaN exactly at the slots whose inner pair is not canonical"""
    from rna_algos_amd.mccaskill_algo import bpp_index
    for _, seq in (trnas[0], trnas[3]):
        n = len(seq)
        hp, mb, ac, tl = O.fold_scores(params.ptr, seq, contra, short)
        keys = [(i, j) for i in range(n) for j in range(i + 1, n) if not np.isnan(mb[bpp_index(n, i, j)])]
        assert len(keys) > 100
        inserts = {}
        for e in tl:
            inserts.setdefault((int(e["i"]), int(e["j"])), []).append(e)
        seen = 0
        for i, j in keys:
            x = bpp_index(n, i, j)
            h, m, a, two = O.cell_scores(params.ptr, seq, contra, short, i, j)
            assert np.array([h, m, a]).tobytes() == np.array([hp[x], mb[x], ac[x]]).tobytes(), (i, j)
            slots = O.twoloop_slots(i, j)
            assert len(two) == len(slots) == SR.count(SR.C, i, j) - 2
            order = []
            for e in inserts.get((i, j), []):
                q = slots.index((int(e["k"]) - i - 1, j - 1 - int(e["l"])))
                assert two[q].tobytes() == e["score"].tobytes(), (i, j, q)
                order.append(q)
            assert order == sorted(order)  # the list's order is the reference's visiting order
            seen += len(order)
            for q, (a_, b_) in enumerate(slots):
                canon = int(seq[i + 1 + a_]) + int(seq[j - 1 - b_]) in (3, 5)
                assert np.isnan(two[q]) == (not canon)
        assert seen == len(tl)


def test_fold_sums_masked(params):
    """no mask: the bytes of O.fold_sums; a mask: the sums that O.bpp_masked dumps"""
    import constraint_masks as CM
    seq, _, _, mask = CM.mixed_case(120)
    for contra, short in MODELS:
        plain = O.fold_sums(params.ptr, seq, contra, short)
        none = O.fold_sums_masked(params.ptr, seq, contra, short, None)
        ones = O.fold_sums_masked(params.ptr, seq, contra, short, np.ones((120, 120), np.uint8))
        got = O.fold_sums_masked(params.ptr, seq, contra, short, mask)
        _, _, mats = O.bpp_masked(params.ptr, seq, contra, short, mask, dump=True)
        for name in O.FOLD_SUMS_FIELDS:
            assert plain[name].tobytes() == none[name].tobytes() == ones[name].tobytes()
        for name, m in zip(("sums_close", "sums_accessible", "sums_external", "sums_1ormore_basepairs"), mats):
            assert got[name].tobytes() == m.tobytes()
        assert got["sums_close"].tobytes() != plain["sums_close"].tobytes()
        assert not np.isfinite(got["sums_close"][mask == 0]).any()


def _draw(r, rng, s, ts, mutant=None):
    return [r.sample(rng, s, t, mutant) for t in ts]


@pytest.mark.parametrize("contra,short", MODELS)
def test_decisions_invert_the_walk(inputs, contra, short):
    """`decisions` reads off the row exactly the decisions the reference sampler made, the row
    rebuilt from them is the row, and a walk has at most 4 n + 16 of them"""
    rng = SR.Rng(SEED)
    for s, key in enumerate(inputs):
        if key == "n700" and (contra, short) != MODELS[1]:
            continue  # (one model at this length: its fold sums take seconds)
        r = replay(key, contra, short)
        seen = set()
        for row, lw, decs, ok in _draw(r, rng, s, range(300 if key.startswith("dist") else 20)):
            assert ok
            if row.tobytes() in seen:
                continue
            seen.add(row.tobytes())
            got = SR.decisions(row, r.seq, (contra, short))
            assert got == decs
            assert len(decs) <= 4 * r.n + 16
            assert SR.rebuild(r.n, got).tobytes() == row.tobytes()
            assert [d[0] for d in got] == list(range(len(got)))
        assert len(seen) > 1


def test_decisions_reject_what_the_grammar_cannot_write():
    for db in ("(..", "..)", "(.a.)", "(" + "." * 16 + "(...)" + "." * 16 + ")"):
        with pytest.raises(SR.NotInGrammar):
            SR.decisions(db.encode())
    with pytest.raises(SR.NotInGrammar):
        SR.decisions(b"(...)", np.array([0, 0, 0, 0, 0], np.uint8))  # A-A


@pytest.mark.parametrize("contra,short", MODELS)
def test_reference_sampler_is_the_ensemble(inputs, params, contra, short):
    """pair frequencies of the reference sampler on DIST_SEQS against the brute-force ensemble
    under the rule of test_gpu_sample (5 sigma + 1e-3): the replay's grammar and terms are the
    ensemble's"""
    N = 3000
    rng = SR.Rng(11)
    for s, seq in enumerate(DIST_SEQS):
        r = replay(f"dist{s}", contra, short)
        rows = np.array([row for row, _, _, _ in _draw(r, rng, s, range(N))])
        _, bp, _ = O.bruteforce(params.ptr, seq, contra, short)
        f = pair_freq(rows)
        bound = 5 * sigma(bp, N) + 1e-3
        assert np.all(np.abs(f - bp) <= bound), f"max excess {np.max(np.abs(f - bp) - bound)}"


def _audit_all(inputs, contra, short, mutant):
    """run the (mutated) sampler over the batch and audit its rows as the GPU test audits the
    kernel's: against the contract's Philox and the caller's s -> rejected decisions per input"""
    true_rng = SR.Rng(SEED)
    rng = SR.Rng(SEED, **SR.MUTANTS[mutant]) if mutant else true_rng
    lens = [len(INPUTS[k]) for k in inputs]
    rank = np.empty(len(inputs), dtype=int)
    rank[np.argsort([-x for x in lens], kind="stable")] = np.arange(len(inputs))
    rejected = {}
    for s, key in enumerate(inputs):
        r = replay(key, contra, short)
        s_used = int(rank[s]) if mutant == "s_within_sorted_group" else s
        bad = 0
        for t, (row, lw, decs, ok) in enumerate(_draw(r, rng, s_used, range(5 if key == "n700" else 20), mutant)):
            if ok:
                fails, lw2 = r.audit_row(row, true_rng, s, t)
                if mutant != "o_before_r":  # (that one also adds the local scores in another order)
                    assert lw2.tobytes() == lw.tobytes()
                bad += len(fails)
            else:  # a defective pick of no weight: the decision it stopped at is the evidence
                us = true_rng.u(np.arange(len(decs)), t, s)
                bad += sum(not r.audit(d, float(u))[0] for d, u in zip(decs, us))
        rejected[key] = bad
    return rejected


@pytest.mark.parametrize("contra,short", MODELS)
def test_audit_accepts_the_reference_sampler(inputs, contra, short):
    assert sum(_audit_all(inputs, contra, short, None).values()) == 0


@pytest.mark.parametrize("mutant", list(SR.MUTANTS))
def test_teeth(inputs, mutant):
    """each defect, on the inputs on which the faithful sampler passes, is rejected"""
    contra, short = MODELS[1]
    rejected = _audit_all(inputs, contra, short, mutant)
    print(mutant, rejected)
    groups = {"dist": sum(v for k, v in rejected.items() if k.startswith("dist")),
              "trna": rejected["trna0"] + rejected["trna1"], "n700": rejected["n700"]}
    if mutant in ("prefix_restarts_each_step", "o_before_r"):
        # the longer inputs carry these two.  In a 16 .. 22-mer only a C cell of span >= 14 has more
        # than 64 candidates, and a pick past the 64th needs an interior loop of 10 and more unpaired
        # bases; and the order of O and R matters in a multiloop alone, which 20 samples of so short a
        # sequence need not hold
        del groups["dist"]
    assert all(v > 0 for v in groups.values()), groups
