"""What the library enqueues is what the pure schedule says: the launch counts of a call on the card
against the lines of tests/golden/sweep_schedule.txt marked G, which tests/schedule_host_check.cpp
computes from rna_algos_amd/csrc/rnamc_schedule.h alone (tests/test_schedule_cpu.py holds the fixture
against that program, so it cannot go stale).  A case names one fixture line per lock-step group of
its call; lengths, model variant and knobs are read from the lines, nothing is compiled here.  Every
case takes a context of its own.  Results are not compared: the parity tests do that."""
import os

import pytest

from test_gpu_knob_forms import context, groups_of, make_seqs, ragged_lens

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"turner": (False, False), "contra": (True, False), "contra-short": (True, True)}
COUNTS = ("inside", "outside", "other", "main", "tail", "small")


def fixture_gpu_lines():
    """name -> (lengths, contra, short, opts, knobs, counts) of the lines marked G"""
    out = {}
    with open(os.path.join(ROOT, "tests", "golden", "sweep_schedule.txt")) as f:
        for ln in f:
            if not ln.startswith("G "):
                continue
            name, *fields = ln.split()[1:]
            kv = dict(x.split("=", 1) for x in fields)
            lens = []
            for run in kv["lens"].split(","):
                n, _, times = run.partition("x")
                lens += [int(n)] * int(times or 1)
            shape, model, opts, knobs = name.split("/")
            knobs = {} if knobs == "-" else {k: int(v) for k, v in (x.split("=") for x in knobs.split(","))}
            out[name] = (lens, *MODELS[model], opts, knobs, {k: int(kv[k]) for k in COUNTS})
    return out


# case -> (the call's lengths, knobs of the batch plan, the fixture line of every group in order)
CASES = {
    "defaults": ([120] * 6, {}, ["equal120/turner/full/-"]),
    "batch-forms": ([120] * 6, {}, ["equal120/turner/full/latency_mode=0"]),
    "latency-unmerged": ([120] * 6, {}, ["equal120/turner/full/latency_mode=2,lat_merge=0"]),
    "lat-split": ([120] * 6, {}, ["equal120/turner/full/lat_split=1"]),
    "dual-window": (ragged_lens(), {}, ["ragged41/turner/full/latency_mode=0,dual_min_cells=2000,dual_max_diag=90"]),
    "two-groups": ([120] * 3 + [90] * 3, {"group_max_seqs": 3}, ["equal120x3/contra/full/-", "equal90x3/contra/full/-"]),
    "contra-short": ([120] * 6, {}, ["equal120/contra-short/full/-"]),
    "max-plus": ([120] * 6, {}, ["equal120/turner/maxplus/-"]),
}


def test_every_marked_line_is_run():
    used = [name for _, _, names in CASES.values() for name in names]
    assert sorted(used) == sorted(fixture_gpu_lines())


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_counts(params, case):
    lens, plan_knobs, names = CASES[case]
    lines = fixture_gpu_lines()
    groups = groups_of(lens, max_seqs=plan_knobs.get("group_max_seqs", 8192))
    assert [lines[n][0] for n in names] == groups, "the fixture lines are not the groups of this call"
    _, contra, short, opts, knobs, _ = lines[names[0]]
    assert all(lines[n][1:5] == (contra, short, opts, knobs) for n in names)
    want = {k: sum(lines[n][5][k] for n in names) for k in COUNTS}
    seqs = make_seqs(lens, 20270)
    with context(params, profile=2, **plan_knobs, **knobs) as ctx:
        if opts == "maxplus":
            ctx.mfe_batch(seqs, contra, short)
            want["other"] += len(groups)  # (the entry's traceback, one launch per group)
        else:
            ctx.bpp_batch(seqs, contra, short)
        st = ctx.stats()
    assert st["n_groups"] == len(groups)
    got = {"inside": st["launches_inside"], "outside": st["launches_outside"], "other": st["launches_other"],
           "main": st["launches_outside_main"], "tail": st["launches_outside_tail"],
           "small": st["launches_outside_small"]}
    assert got == want
