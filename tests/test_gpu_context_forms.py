"""Structural context profiles (rnamc_context_profile_batch) past 257 bases and
under every launch form of the reference-order sweep (section 4d, tests/knob_table.py).

The entry is the one consumer of the MATRICES the outside sweep leaves in the workspace (M_Q1C, the
interleaved {M_PM, M_PM2}, M_Z, M_QB, M_MBC, the copy of M_QM taken between the sweeps).  The
knob-forms suite holds every form to the oracle's pair probabilities; here
  a. lone records of 513 and 600 bases and one ragged call are held to the f64 replay of the sums
     (tests/context_ref.py),
  b. the profile under every form equals the default-knob profile bit for bit, and the default-knob
     profile is held to the replay,
  c. the seven matrices themselves equal the oracle's under the same forms.

The bound on |device - f64 replay| of an input list is 4 x D(list), D = the largest |device_arith
replay - f64 replay| over rows 0 .. 4: a property of the reference alone, computed here from the two
replays; nothing measured on the device enters it.  The factor 4 covers the device's expf and numpy's
f32 exp differing by an ulp in opposite directions on the dominant terms, the ties of the
quantisation and the last rounding to f32.  D itself may not exceed 2e-7 (twice the largest value
measured on a CPU at n = 257 .. 600), so a broken model cannot loosen its own bound.  Every base of
every compared record counts."""
import concurrent.futures
import functools

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_knob_forms import (VARIANT_IDS, VARIANTS, context, dmin_outside, groups_of, is_latency_group,
                                 make_seqs, outside_forms, pairwise_rows, ragged_lens, wide_lens)

pytestmark = pytest.mark.gpu

variants = pytest.mark.parametrize("model", VARIANTS, ids=VARIANT_IDS)
D_MAX = 2e-7
RAGGED_CALL = (513, 300, 257, 256, 255, 65, 5, 1)
HELD_RAGGED = (10, 9, 6, 4)  # positions of the records of 330, 257, 129 and 65 bases in ragged_lens()
LONG23 = tuple(range(10, 33))  # the record of 330 bases and the 22 drawn from 245 .. 330
WIDE_FORMS = [dict(latency_mode=0, block_threads=b, order_inside=o) for b in (64, 256) for o in (0, 1, 2)]


@functools.lru_cache(None)
def _tables():
    from rna_algos_amd.utils import FoldScoreSets
    return FoldScoreSets.synthetic(1)


def lone(n):
    return O.splitmix_seq(n, 9000 + n)


@functools.lru_cache(None)
def ragged_seqs():
    assert [ragged_lens()[x] for x in HELD_RAGGED] == [330, 257, 129, 65]
    assert all(245 <= ragged_lens()[x] <= 330 for x in LONG23)
    return make_seqs(ragged_lens(), 11)


@functools.lru_cache(None)
def wide_seqs():
    return make_seqs(wide_lens(), 12)


@functools.lru_cache(None)
def held_wide():
    """the first record of the wide batch and its longest"""
    return (0, int(np.argmax(wide_lens())))


def _input_lists():
    return {"a": [lone(513), lone(600), lone(300)],
            "ragged": [ragged_seqs()[x] for x in HELD_RAGGED],
            "wide": [wide_seqs()[x] for x in held_wide()]}


def _threaded(fn, jobs):
    # (the oracle runs outside the interpreter lock; longest records first)
    with concurrent.futures.ThreadPoolExecutor(12) as pool:
        return list(pool.map(fn, jobs))


@functools.lru_cache(None)
def _all_replays():
    import context_ref as R
    jobs = [(name, x, m) for name, seqs in _input_lists().items() for x in range(len(seqs)) for m in VARIANTS]
    lists = _input_lists()
    jobs.sort(key=lambda j: -len(lists[j[0]][j[1]]))
    got = _threaded(lambda j: R.replay_both(lists[j[0]][j[1]], j[2][0], j[2][1], _tables()), jobs)
    return dict(zip(jobs, got))


def replays(name, model):
    """[(f64 replay, device_arith replay)] of the input list `name`, computed once for the module"""
    return [_all_replays()[(name, x, model)] for x in range(len(_input_lists()[name]))]


def model_error(name, model):
    """D of an input list; the device bound is four times it"""
    import context_ref as R
    D = R.model_error(replays(name, model))
    print("D(%s, %s) = %.3e" % (name, VARIANT_IDS[VARIANTS.index(model)], D))
    assert 0 < D <= D_MAX, (name, model, D)
    return D


def deviation(prof, replay):
    assert prof.shape == replay[0].shape and np.isfinite(prof).all() and (prof >= 0).all()
    return float(np.abs(prof[:5] - replay[0][:5]).max())


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
                                    for x, y in zip(a, b))


def first_difference(a, b):
    for s, (x, y) in enumerate(zip(a, b)):
        bad = np.argwhere(x.view(np.uint32) != y.view(np.uint32))
        if len(bad):
            r, u = bad[0]
            return f"record {s} (n = {x.shape[1]}): {len(bad)} values differ, first row {r} base {u}: {x[r, u]!r} != {y[r, u]!r}"
    return "equal"


# ---- a. lengths past 257 ---------------------------------------------------------------------------

@functools.lru_cache(None)
def lone_profiles(model):
    """{n: (profile, paired_prob of the sparse entry)}: every record of the ragged call alone, and n = 600"""
    out = {}
    with context(_tables()) as ctx:
        for n in RAGGED_CALL + (600,):
            prof, _ = ctx.context_profile_batch([lone(n)], *model)
            sp, _ = ctx.bpp_batch_sparse([lone(n)], *model, 0.0)
            out[n] = (prof[0].copy(), sp[0].paired_prob.copy())
    return out


@variants
@pytest.mark.parametrize("n", [513, 600])
def test_lone_record_matches_replay(built, model, n):
    """n = 513: two carries of the 256-wide scan of k_ctx_finish, three workgroups of k_ctx_mb2, nine
    strides of k_ctx_mb13; at default knobs the lone record takes the latency forms"""
    import context_ref as R
    bound = 4 * model_error("a", model)
    r = replays("a", model)[(513, 600).index(n)]
    prof, paired = lone_profiles(model)[n]
    err = deviation(prof, r)
    print(model, n, "max |device - replay| %.3e" % err, "by row", ["%.1e" % v for v in np.abs(prof[:5] - r[0][:5]).max(axis=1)],
          "bound %.3e" % bound, "row maxima", np.round(r[0].max(axis=1), 3))
    assert err <= bound
    assert np.array_equal(prof[R.STEM], paired)  # row 5: the sparse entry's paired_prob, bit for bit
    dev = float(np.abs(prof.astype(np.float64).sum(axis=0) - 1).max())
    own = float(np.abs(r[0].sum(axis=0) - 1).max())
    print(model, n, "|sum - 1| device %.2e replay %.2e" % (dev, own))
    assert dev <= own + 6 * bound


@variants
def test_ragged_call_equals_lone_calls_and_replay(built, model):
    """records of 513 .. 1 bases share every launch through grid.y, whole workgroups returning early: the
    lone-call bits, and the records of 513 and 300 bases held to the replay"""
    import context_ref as R
    bound = 4 * model_error("a", model)
    alone = lone_profiles(model)
    with context(_tables()) as ctx:
        prof, _ = ctx.context_profile_batch([lone(n) for n in RAGGED_CALL], *model)
        assert ctx.stats()["n_groups"] == 1
        sp, _ = ctx.bpp_batch_sparse([lone(n) for n in RAGGED_CALL], *model, 0.0)
    want = [alone[n][0] for n in RAGGED_CALL]
    assert same_bits(prof, want), first_difference(prof, want)
    assert all(np.array_equal(p[R.STEM], q.paired_prob) for p, q in zip(prof, sp))
    for n, r in ((513, replays("a", model)[0]), (300, replays("a", model)[2])):
        err = deviation(prof[RAGGED_CALL.index(n)], r)
        print(model, "ragged call, n =", n, "max |device - replay| %.3e" % err, "bound %.3e" % bound)
        assert err <= bound


@variants
def test_every_class_is_exercised_past_257(built, model):
    """not vacuous: every row of the replay reaches 0.05 somewhere on the inputs of case a"""
    tops = np.max([r.max(axis=1) for r, _ in replays("a", model)], axis=0)
    print(model, "row maxima", np.round(tops, 3))
    assert (tops >= 0.05).all(), tops


# ---- b. every form, bit for bit --------------------------------------------------------------------

@functools.lru_cache(None)
def default_ragged(model):
    with context(_tables()) as ctx:
        prof, logz = ctx.context_profile_batch(ragged_seqs(), *model)
        assert ctx.stats()["n_groups"] == 1
    return [p.copy() for p in prof], np.asarray(logz).copy()


def run_form(model, **knobs):
    """the ragged batch under the knobs: the default-knob bits; -> the statistics of the call"""
    want, want_z = default_ragged(model)
    with context(_tables(), **knobs) as ctx:
        prof, logz = ctx.context_profile_batch(ragged_seqs(), *model)
        st = ctx.stats()
    assert same_bits(prof, want), f"{knobs}: {first_difference(prof, want)}"
    assert np.array_equal(np.asarray(logz).view(np.uint32), want_z.view(np.uint32)), f"{knobs}: ln Z differs"
    assert st["launches_context"] > 0
    return st


@variants
def test_default_form_matches_replay(built, model):
    """the default-knob profiles of the records of 330, 257, 129 and 65 bases of the ragged batch against
    the replay: with it, the equalities below pin every form to the replay"""
    bound = 4 * model_error("ragged", model)
    prof, _ = default_ragged(model)
    for x, r in zip(HELD_RAGGED, replays("ragged", model)):
        err = deviation(prof[x], r)
        print(model, "ragged batch, n =", ragged_lens()[x], "max |device - replay| %.3e" % err, "bound %.3e" % bound)
        assert err <= bound


@pytest.mark.parametrize("row", range(len(pairwise_rows())))
def test_pairwise_rows(built, row):
    """every row of the pairwise cover of the reference-order knobs, the model round-robin as in
    tests/test_gpu_knob_forms.py"""
    knobs = pairwise_rows()[row]
    st = run_form(VARIANTS[row % 3], **knobs)
    assert st["n_groups"] == len(groups_of(ragged_lens(), max_seqs=knobs["group_max_seqs"]))


@variants
@pytest.mark.parametrize("knobs", [dict(latency_mode=0), dict(latency_mode=2), dict(fuse_inside=0),
                                   dict(block_threads=64)], ids=str)
def test_single_knobs(built, model, knobs):
    assert run_form(model, **knobs)["n_groups"] == 1


@variants
@pytest.mark.parametrize("min_cells,max_diag", [(2000, 90), (0, 37)])
def test_dual_max_diag_both_transitions(built, model, min_cells, max_diag):
    """case d of the knob forms: one kernel -> two kernels on two streams -> one kernel again within a
    sweep; the per-kernel accounting shows that the knobs took effect"""
    group = groups_of(ragged_lens())[0]
    forms = outside_forms(group, dmin_outside(*model), dual_min_cells=min_cells, dual_max_diag=max_diag)
    st = run_form(model, latency_mode=0, profile=2, dual_min_cells=min_cells, dual_max_diag=max_diag)
    assert st["n_groups"] == 1
    assert st["launches_outside_main"] == st["launches_outside_tail"] == sum(forms) > 0
    assert st["launches_outside_small"] == len(forms) - sum(forms) > 0


@variants
@pytest.mark.parametrize("lat_pairs", [0, 1])
def test_lat_split(built, model, lat_pairs):
    """case f: the un-merged two-stream schedule of the latency forms, filed as "tail" by the accounting"""
    st = run_form(model, latency_mode=2, group_max_seqs=5, lat_split=1, lat_pairs=lat_pairs, profile=2)
    assert st["n_groups"] == len(groups_of(ragged_lens(), max_seqs=5))
    assert st["launches_outside_tail"] == st["launches_outside_main"] > 0
    assert st["launches_outside_small"] > 0


@variants
def test_mixed_latency_and_batch_groups(built, model):
    """case e: one call whose groups fall on both sides of lat_max_cells"""
    groups = groups_of(ragged_lens(), max_seqs=5)
    kinds = [is_latency_group(g, model[0], 750) for g in groups]
    assert True in kinds and False in kinds
    st = run_form(model, latency_mode=1, group_max_seqs=5, lat_max_cells=750)
    assert st["n_groups"] == len(groups)


@variants
def test_wide_batch_forms(built, model):
    """420 records under latency_mode 0: the fused k_inside2 and the non-split k_inside forms of the low
    diagonals, block_threads 64 / 256 x order_inside 0 / 1 / 2, equal among themselves; two records held
    to the replay"""
    bound = 4 * model_error("wide", model)
    first = None
    for knobs in WIDE_FORMS:
        with context(_tables(), **knobs) as ctx:
            prof, logz = ctx.context_profile_batch(wide_seqs(), *model)
            assert ctx.stats()["n_groups"] == 1
        if first is None:
            first = ([p.copy() for p in prof], np.asarray(logz).copy())
            for x, r in zip(held_wide(), replays("wide", model)):
                err = deviation(prof[x], r)
                print(model, "wide batch, n =", wide_lens()[x], "max |device - replay| %.3e" % err, "bound %.3e" % bound)
                assert err <= bound
        else:
            assert same_bits(prof, first[0]), f"{knobs}: {first_difference(prof, first[0])}"
            assert np.array_equal(np.asarray(logz).view(np.uint32), first[1].view(np.uint32)), knobs


# ---- c. the matrices themselves, under the same rows ------------------------------------------------

MATRICES = ("sums_close", "sums_accessible", "sums_external", "sums_1ormore_basepairs", "multibranch_close",
            "probs_multibranch", "probs_multibranch2")


def fetched_records(max_seqs):
    """positions in LONG23 of the three longest records of the LAST group of a call of the 23 long
    records (the library sorts stably, longest first, and cuts as groups_of does)"""
    lens = [ragged_lens()[x] for x in LONG23]
    order = sorted(range(len(lens)), key=lambda x: -lens[x])
    last = groups_of(lens, max_seqs=max_seqs)[-1]
    return order[len(lens) - len(last):][:3]


@functools.lru_cache(None)
def _all_dumps():
    """the oracle's seven matrices of every record some row fetches, once per record and model"""
    jobs = sorted({(x, VARIANTS[row % 3]) for row, knobs in enumerate(pairwise_rows())
                   for x in fetched_records(knobs["group_max_seqs"])})
    got = _threaded(lambda j: O.bpp_dump(_tables().ptr, ragged_seqs()[LONG23[j[0]]], *j[1])[2], jobs)
    return dict(zip(jobs, got))


@pytest.mark.parametrize("row", range(len(pairwise_rows())))
def test_matrices_under_pairwise_rows(built, row):
    """what the outside sweep leaves behind, not only what bpp reads of it: after rnamc_bpp_batch under
    the row, matrices 0 .. 6 of the three longest records of the last group are the oracle's bits, NaN
    equal to NaN.  Tells a defect of the sweep from one of the context stage, and pins
    probs_multibranch / probs_multibranch2 under the forms."""
    model, knobs = VARIANTS[row % 3], pairwise_rows()[row]
    seqs = [ragged_seqs()[x] for x in LONG23]
    compared = 0
    with context(_tables(), **knobs) as ctx:
        ctx.bpp_batch(seqs, *model)
        assert ctx.stats()["n_groups"] == len(groups_of([len(s) for s in seqs], max_seqs=knobs["group_max_seqs"]))
        for x in fetched_records(knobs["group_max_seqs"]):
            n = len(seqs[x])
            iu = np.triu_indices(n)
            for w, name in enumerate(MATRICES):
                g, r = ctx.debug_fetch(x, w, n)[iu], _all_dumps()[(x, model)][w][iu]
                bad = ~((g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r)))
                if bad.any():
                    k = np.nonzero(bad)[0]
                    spans = iu[1][k] - iu[0][k]
                    kk = k[np.argmin(spans)] if w < 5 else k[np.argmax(spans)]
                    pytest.fail(f"row {row} {knobs}: {name} of record {x} (n = {n}): {bad.sum()} cells differ, e.g. "
                                f"({iu[0][kk]}, {iu[1][kk]}) device {g[kk]!r} oracle {r[kk]!r}")
                compared += 1
    print("row", row, "matrices compared", compared)
    assert compared >= 14
