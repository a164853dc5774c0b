"""Every duplex two-loop slot (a, b), a + b <= 30, in every form of the duplex sweeps
(rnamc_duplex_batch): k_duplex_step is compiled for {inside sum, outside sum,
max-plus} x {lines along A, lines along B}, each with its own tile indexing, pair roles and staged
base windows, and k_duplex_trace walks the slots once more.  On random strands a lone long interior
loop carries almost no weight; the strands of tests/duplex_slots.py make one slot carry the result
(families D and T: every slot, and the slots' cells on lanes 0 and 127 of a 128-lane workgroup), and
tests/test_duplex_slots_cpu.py holds the conditions that give the checks below their power.

One context, the seeded synthetic tables.  Per model and stepping direction ONE call folds every
record (the direction is the chunk's: a neighbour pair 1 x 200 or 200 x 1 sets it), every output
requested.  Against the f64 reference (tests/duplex_ref.py; the designed pairs' P, ln Z and the
optimum of every record from tests/golden/duplex_slots_f64.npz, every cell of every tenth record
evaluated here):

  * ln Z, P, pa, pb within the bounds of test_gpu_duplex.py, no NaN, P = 0 exactly where the
    reference is -inf;
  * the twelve designed pairs, and pa / pb at their bases, RELATIVE: |p / p_f64 - 1| <= 2 (2 m + 2) 2^-24
    with m = 12, 3.1e-6: one hardware exp2 and one log2 rounding per level of F, of G and of the final
    ratio, every sum along the designed chain being dominated by one term.  Derived, not measured.  A
    slot that read a neighbouring length entry (about 0.1 nat away) moves a designed P >= 0.4 by more
    than 1e-3 relative even at P = 0.99;
  * pa and pb of every base: the f64 sum of the returned row or column rounded once;
  * |d ln Z| within the bound, and, from the reference, that 0.05 nat in the slot's score would break
    it: the designed duplex holds at least 0.3 of the ensemble;
  * the max-plus value within its bound of the f64 optimum, the structure EXACTLY the designed duplex
    (it leads by 0.25 nat), duplex_score(structure) the returned value;
  * the two stepping directions: identical bits;
  * every subset of the outputs (every workspace layout): the bits of the all-outputs call.
"""
import contextlib
import io
from types import SimpleNamespace

import numpy as np
import pytest

import duplex_ref as R
import duplex_slots as S
from test_gpu_duplex import check_against, same, tol_p, tol_z

pytestmark = pytest.mark.gpu

M_PAIRS = 12
REL_BOUND = 2 * (2 * M_PAIRS + 2) * 2.0 ** -24
MODELS = [False, True]
DIRECTIONS = [False, True]  # by_col: the sweep steps along B


@pytest.fixture(scope="module")
def ctx(params):
    from rna_algos_amd.mccaskill_algo import Context
    c = Context(params, device=0)
    yield c
    c.close()


_FOLDS = {}


def folds(ctx, contra, by_col):
    """every record in ONE call, once per model and direction; the neighbour's fold is dropped"""
    if (contra, by_col) not in _FOLDS:
        from rna_algos_amd import _lib
        from rna_algos_amd.duplex import _duplex_batch
        seqs, pairs = S.call(by_col)
        res = _duplex_batch(_lib.lib().rnamc_duplex_batch, ctx._h, seqs, pairs, contra)
        assert (res[-1].n_a, res[-1].n_b) == ((S.NEIGHBOUR_LEN, 1) if by_col else (1, S.NEIGHBOUR_LEN))
        _FOLDS[(contra, by_col)] = res[:-1]
    return _FOLDS[(contra, by_col)]


def test_bound_is_derived():
    assert abs(REL_BOUND - 3.1e-6) < 5e-9 and REL_BOUND <= 1e-4


@pytest.mark.parametrize("by_col", DIRECTIONS, ids=["along_A", "along_B"])
@pytest.mark.parametrize("contra", MODELS, ids=["turner", "contra"])
def test_every_slot(params, ctx, contra, by_col):
    from rna_algos_amd.duplex import duplex_score
    recs, g = S.records(), S.golden()
    fs = folds(ctx, contra, by_col)
    assert len(fs) == len(recs)
    worst = {"D": 0.0, "T": 0.0}
    worst_z = worst_best = 0.0
    for r, f in zip(recs, fs):
        assert (f.n_a, f.n_b) == (r.na, r.nb)
        P = f.probs.astype(np.float64)
        assert not np.isnan(f.probs).any() and not np.isnan(f.bound_a).any() and not np.isnan(f.bound_b).any(), r
        # the reference is -inf wherever the two bases cannot pair
        code = r.seq_a[:, None].astype(int) + r.seq_b[None, :]
        assert not f.probs[(code != 3) & (code != 5)].any(), r
        # ln Z, and that an error of 0.05 nat in the slot's score (d ln Z >= share x 0.05) would break it
        log_z, share = g[("log_z", contra)][r.idx], g[("share", contra)][r.idx]
        assert abs(f.log_z - log_z) <= tol_z(log_z), r
        assert share * 0.05 > tol_z(log_z), r
        worst_z = max(worst_z, abs(f.log_z - log_z) / tol_z(log_z))
        # the designed pairs, relative
        want = g[("designed", contra)][r.idx]
        got = np.array([P[c] for c in r.chain])
        dev = float(np.max(np.abs(got / want - 1.0)))
        worst[r.family] = max(worst[r.family], dev / REL_BOUND)
        assert dev <= REL_BOUND, (r, dev, REL_BOUND)
        # pa, pb: the f64 sums of the returned matrix rounded once
        for bound, total in ((f.bound_a, P.sum(axis=1)), (f.bound_b, P.sum(axis=0))):
            assert np.all(np.abs(bound - total) <= 2.0 ** -24 * 1.000001 * total + 1e-45), r
        # the max-plus sweep and the traceback
        tb = (min(r.na, r.nb) + 1) * 2.0 ** -24 * g[("top", contra)][r.idx]
        best = g[("best", contra)][r.idx]
        assert abs(f.best_score - best) <= tb, r
        worst_best = max(worst_best, abs(f.best_score - best) / tb)
        assert f.pairs() == r.chain, (r, f.structure)
        assert abs(duplex_score(r.seq_a, r.seq_b, f.structure, contra, params) - f.best_score) <= tb, r
    label = f"contra={contra} by_col={by_col}"
    print(f"{label}: worst |p/p64 - 1| of a designed pair over the bound {REL_BOUND:.3g}: family D {worst['D']:.3f}, "
          f"family T {worst['T']:.3f}; worst |d ln Z| over its bound {worst_z:.3f}, |d best| {worst_best:.3f}")


@pytest.mark.parametrize("by_col", DIRECTIONS, ids=["along_A", "along_B"])
@pytest.mark.parametrize("contra", MODELS, ids=["turner", "contra"])
def test_every_cell_of_every_tenth_record(ctx, contra, by_col):
    recs = S.records()
    fs = folds(ctx, contra, by_col)
    worst = 0.0
    for x, ref in S.live(contra).items():
        r, f = recs[x], fs[x]
        dense = SimpleNamespace(log_z=ref.log_z, P=ref.dense(r), pa=ref.pa, pb=ref.pb)
        with contextlib.redirect_stdout(io.StringIO()):  # (check_against prints a line per record)
            check_against(f, dense, f"{r} contra={contra} by_col={by_col}")
        assert float(np.max(np.abs(f.probs - dense.P))) <= tol_p(r.na + r.nb)
        # 0 exactly where the reference is -inf
        dead = np.ones((r.na, r.nb), bool)
        dead[ref.ci[ref.live], ref.cj[ref.live]] = False
        assert not f.probs[dead].any(), r
        # pa and pb at the designed pairs' bases, relative
        ia, jb = [c[0] for c in r.chain], [c[1] for c in r.chain]
        dev = max(float(np.max(np.abs(f.bound_a[ia] / ref.pa[ia] - 1.0))),
                  float(np.max(np.abs(f.bound_b[jb] / ref.pb[jb] - 1.0))),
                  float(np.max(np.abs(f.probs[ia, jb] / ref.designed - 1.0))))
        worst = max(worst, dev / REL_BOUND)
        assert dev <= REL_BOUND, (r, dev, REL_BOUND)
    print(f"contra={contra} by_col={by_col}: worst relative deviation of pa, pb, P at the designed bases over the "
          f"bound: {worst:.3f}")


@pytest.mark.parametrize("contra", MODELS, ids=["turner", "contra"])
def test_direction_independence(ctx, contra):
    """a cell's terms are the same values in the same order whichever strand is stepped along"""
    along_a, along_b = folds(ctx, contra, False), folds(ctx, contra, True)
    bad = [r for r, x, y in zip(S.records(), along_a, along_b) if not same(x, y)]
    assert not bad, (len(bad), bad[:5])


SUBSET_SLOTS = [(0, 0), (1, 1), (1, 0), (3, 1), (2, 5), (5, 3), (7, 4), (9, 9)]
OUTPUTS = ("probs", "pa", "pb", "logz", "structs", "best")
SUBSETS = [("logz",), ("best",), ("structs", "best"), ("pa",), ("probs",), ("logz", "best"), ("pb", "structs")]


def raw_call(ctx, seqs, pairs, contra, want):
    """rnamc_duplex_batch through ctypes with exactly the outputs of `want`; what is not asked for is
    passed as NULL -> {name: array}; pa and pb share one array, as in the Python mirror"""
    from rna_algos_amd import _lib
    from rna_algos_amd import mccaskill_algo as M
    lens, offsets, bases = M._pack([np.ascontiguousarray(s, dtype=np.uint8) for s in seqs])
    pa = np.ascontiguousarray([p[0] for p in pairs], dtype=np.uint32)
    pb = np.ascontiguousarray([p[1] for p in pairs], dtype=np.uint32)
    na, nb = lens[pa].astype(np.uint64), lens[pb].astype(np.uint64)
    out_off = np.zeros(len(pairs) + 1, dtype=np.uint64)
    np.cumsum(na * nb, out=out_off[1:])
    base_off = np.zeros(len(pairs) + 1, dtype=np.uint64)
    np.cumsum(na + nb, out=base_off[1:])
    out = {"probs": np.full(int(out_off[-1]), np.nan, np.float32), "bound": np.full(int(base_off[-1]), np.nan, np.float32),
           "logz": np.full(len(pairs), np.nan, np.float32), "structs": np.full(int(base_off[-1]), 0xFF, np.uint8),
           "best": np.full(len(pairs), np.nan, np.float32)}

    def ptr(name, arr):
        return out[arr].ctypes.data if name in want else None

    _lib.check(_lib.lib().rnamc_duplex_batch(
        ctx._h, len(seqs), bases.ctypes.data, offsets.ctypes.data, len(pairs), pa.ctypes.data, pb.ctypes.data,
        int(contra), ptr("probs", "probs"), out_off.ctypes.data, ptr("pa", "bound"), ptr("pb", "bound"),
        base_off.ctypes.data, ptr("logz", "logz"), ptr("structs", "structs"), base_off.ctypes.data,
        ptr("best", "best")))
    is_a = np.zeros(int(base_off[-1]), bool)
    for p in range(len(pairs)):
        is_a[int(base_off[p]):int(base_off[p]) + int(na[p])] = True
    out["pa"], out["pb"] = out["bound"][is_a], out["bound"][~is_a]
    return out


@pytest.mark.parametrize("contra", MODELS, ids=["turner", "contra"])
def test_output_subsets(ctx, contra):
    """every n_mat of the workspace layout (1 .. 5 floats a cell) over pairs whose cell counts are odd
    and even mixed, so that the padding that keeps the f64 matrices on even floats is exercised: each
    call returns, for what it returns, the bits of the all-outputs call, and writes nothing else"""
    recs = [S.family_d()[R.SLOT_OF[s]] for s in SUBSET_SLOTS]
    assert [(r.a, r.b) for r in recs] == SUBSET_SLOTS
    cells = [r.na * r.nb for r in recs]
    assert sum(c % 2 for c in cells) == 4 and cells[0] % 2 == 0 and cells[1] % 2 == 1
    seqs = [s for r in recs for s in (r.seq_a, r.seq_b)]
    pairs = [(2 * x, 2 * x + 1) for x in range(len(recs))]
    full = raw_call(ctx, seqs, pairs, contra, OUTPUTS)
    assert not any(np.isnan(full[k]).any() for k in ("probs", "pa", "pb", "logz", "best"))
    assert set(full["structs"].tobytes()) <= set(b"().")
    # the all-outputs call is the big call's fold of the same records
    big = folds(ctx, contra, False)
    for x, r in enumerate(recs):
        assert np.float32(big[r.idx].log_z).tobytes() == full["logz"][x].tobytes()
        assert np.float32(big[r.idx].best_score).tobytes() == full["best"][x].tobytes()
    assert np.array_equal(np.concatenate([big[r.idx].probs.ravel() for r in recs]), full["probs"])
    n_mats = set()
    for want in SUBSETS:
        got = raw_call(ctx, seqs, pairs, contra, want)
        need_g = bool({"probs", "pa", "pb"} & set(want))
        n_mats.add((2 if need_g or "logz" in want else 0) + (2 if need_g else 0) + (1 if {"structs", "best"} & set(want) else 0))
        for k in OUTPUTS:
            if k in want:
                assert got[k].tobytes() == full[k].tobytes(), (want, k)
            elif k == "structs":
                assert (got[k] == 0xFF).all(), (want, k)
            else:
                assert np.isnan(got[k]).all(), (want, k)
    assert n_mats == {1, 2, 3, 4, 5}
