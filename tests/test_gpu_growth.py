"""The context's device buffers across calls of growing and shrinking size: every entry family on ONE
context, first with 3 records of 24 nt, then with 12 records of 400 nt (4 800 bases: past the 4 096-byte
floor of every staged buffer, the bases included, so every buffer of the family is freed and allocated
again), then with the 24-nt records again (the grown buffers are kept).  Every result must equal, bit for
bit, the result of the same call on a freshly created context, and both contexts must close normally."""
import pytest

from entry_families import FAMILIES, freeze

pytestmark = pytest.mark.gpu

SMALL, LARGE = (3, 24), (12, 400)


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
