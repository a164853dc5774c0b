"""The context's device buffers across calls of growing and shrinking size: every entry family on ONE
context, first with 3 records of 24 nt, then with 12 records of 400 nt (4 800 bases: past the 4 096-byte
floor of every staged buffer, the bases included, so every buffer of the family is freed and allocated
again), then with the 24-nt records again (the grown buffers are kept).  Every result must equal, bit for
bit, the result of the same call on a freshly created context, and both contexts must close normally."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL, LARGE = (3, 24), (12, 400)


def records(shape):
    from rna_algos_amd.workloads import synthetic_seq
    count, n = shape
    return [synthetic_seq(n, seed=1700 + 31 * n + k) for k in range(count)]


def freeze(x):
    """a result of any entry as nested tuples of bytes"""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (np.floating, float)):
        return np.float64(x).tobytes()
    if isinstance(x, (np.integer, int, str, bytes, type(None))):
        return x
    if isinstance(x, dict):
        return tuple((k, freeze(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(freeze(v) for v in x)
    return freeze({k: v for k, v in vars(x).items() if not k.startswith("_")})


# a sequence whose windows / mutants are `count` records of n bases
def windowed(ctx, shape):
    count, n = shape
    return ctx.bpp_windowed(records((1, n + count - 1))[0], n, False, False, stride=1)


def mutants(ctx, shape):
    count, n = shape
    return ctx.mutant_scan(records((1, n))[0], False, False, positions=list(range(0, n, 3 * n // count)))


def durbin(ctx, shape):
    from rna_algos_amd.durbin_algo import AlignScores, durbin_algo_batch, with_pseudo_bases
    count, _ = shape
    scores = AlignScores.new(0.0)
    scores.transfer()
    seqs = [with_pseudo_bases(r) for r in records(shape)]
    return durbin_algo_batch(seqs, [(k, (k + 1) % count) for k in range(count)], scores, ctx)


# (name, honours summation_mode 1, call)
FAMILIES = [
    ("bpp_batch", True, lambda c, s: c.bpp_batch(records(s), False, False)),
    ("log_partition_batch", False, lambda c, s: c.log_partition_batch(records(s), False, False)),
    ("sample_batch", False, lambda c, s: c.sample_batch(records(s), 4, False, False, seed=7)),
    ("mfe_batch", False, lambda c, s: c.mfe_batch(records(s), False, False)),
    ("centroid_fold_batch", True, lambda c, s: c.centroid_fold_batch(records(s), [0.5, 2.0, 8.0], False, False)),
    ("bpp_batch_sparse", True, lambda c, s: c.bpp_batch_sparse(records(s), False, False, 0.01)),
    ("bpp_windowed", True, windowed),
    ("mutant_scan", True, mutants),
    ("durbin_batch", False, durbin),
]


@pytest.mark.parametrize("mode", [0, 1])
def test_results_do_not_depend_on_what_the_context_held_before(params, mode):
    from rna_algos_amd.mccaskill_algo import Context
    families = [f for f in FAMILIES if mode == 0 or f[1]]

    def fresh(call, shape):
        c = Context(params, device=0)
        c.set("summation_mode", mode)
        try:
            return freeze(call(c, shape))
        finally:
            c.close()
            assert not c._h

    want = {(name, shape): fresh(call, shape) for name, _, call in families for shape in (SMALL, LARGE)}
    assert all(want[name, SMALL] != want[name, LARGE] for name, _, _ in families)
    ctx = Context(params, device=0)
    ctx.set("summation_mode", mode)
    try:
        for shape in (SMALL, LARGE, SMALL):
            for name, _, call in families:
                assert freeze(call(ctx, shape)) == want[name, shape], (name, shape, mode)
    finally:
        ctx.close()
    assert not ctx._h
