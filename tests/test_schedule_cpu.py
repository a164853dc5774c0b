"""CPU suite: the launch schedule of the reference-order sweep (rna_algos_amd/csrc/rnamc_schedule.h),
driven by a stand-alone program (tests/schedule_host_check.cpp) built with the address and
undefined-behaviour sanitizers.  The program includes the schedule header only, opens no device and
is not loaded into Python.  Over its whole grid of group shapes, model variants, sweep options and
knob values its checking sink holds every launch's reads against the happens-before relation of the
steps (a failed rule is a FAIL line and a nonzero exit); the lines of the cases it marks F or G are
held against tests/golden/sweep_schedule.txt, recorded from the schedule as it stood inside run_batch
before it moved into the header.  A mismatch is read with `<program> --dump <case>`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sweep_schedule.txt")
HEADER = os.path.join(ROOT, "rna_algos_amd", "csrc", "rnamc_schedule.h")


def fixture_lines():
    with open(FIXTURE) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip()]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("schedule") / "schedule_host_check")
    # (the sanitizers' runtimes are linked statically: the program needs nothing from its environment)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "schedule_host_check.cpp")])
    return exe


@pytest.fixture(scope="module")
def grid(program):
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return run.returncode, run.stdout


def test_header_is_free_of_hip():
    """compiles as plain C++17 with no include path, and includes nothing of the project"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", HEADER])
    includes = [ln.split()[1] for ln in open(HEADER) if ln.startswith("#include")]
    assert sorted(includes) == ["<algorithm>", "<cstdint>"]


def test_every_grid_case_passes_the_checking_sink(grid):
    rc, out = grid
    fails = [ln for ln in out.splitlines() if ln.startswith("FAIL")]
    assert rc == 0 and not fails, "\n".join(fails[:40]) or out[-2000:]
    lines = out.splitlines()
    assert lines[-1] == "OK"
    cases = [ln for ln in lines if ln[:2] in ("G ", "F ", "- ")]
    assert lines[-2] == f"cases {len(cases)}" and len(cases) > 10000
    names = [ln.split(" ")[1] for ln in cases]
    assert len(set(names)) == len(names)


def test_fixture_matches(grid):
    """every fixture line is what the program prints today, and the program marks no case the fixture lacks"""
    _, out = grid
    marked = [ln for ln in out.splitlines() if ln[:2] in ("G ", "F ")]
    want = fixture_lines()
    got = {ln.split(" ")[1]: ln for ln in marked}
    moved = [f"- {ln}\n+ {got.get(ln.split(' ')[1], '(no such case)')}" for ln in want
             if got.get(ln.split(" ")[1]) != ln]
    assert not moved, "\n".join(moved[:20])
    assert len(marked) == len(want)


def test_fixture_covers_every_schedule_and_both_rings(program):
    """the fixture holds a max-plus sweep, both inside and both outside schedules with their forms, and
    traces in which either ring comes round to a slot again"""
    names = [ln.split(" ")[1] for ln in fixture_lines()]
    seen = set()
    for name in ("equal120/turner/maxplus/-", "equal120/turner/full/latency_mode=0", "equal120/turner/full/lat_split=1",
                 "equal120/turner/full/latency_mode=2,lat_merge=0", "equal120/contra-short/full/-",
                 "wide120/contra/full/latency_mode=0,dual_min_cells=0",
                 "ragged41/turner/full/latency_mode=0,dual_min_cells=2000,dual_max_diag=90"):
        assert name in names
        trace = subprocess.run([program, "--dump", name], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        seen |= {ln.split(" ")[0] + (" outside" if ln.startswith("pair_lat outside") else "") for ln in trace}
        seen |= {"wrap " + ring for ring in "AB" if sum(ln.startswith(f"record {ring}") for ln in trace) > 16}
        seen |= {what for what in ("head=1", "form=14", "class=1") if any(what in ln for ln in trace)}
        roles = [ln.split("roles=")[1][0] for ln in trace if "roles=" in ln]
        if "".join(roles).strip("7") and roles[0] == roles[-1] == "7":
            seen.add("one kernel, two, one again")
    assert {"mfe_inside", "inside", "inside2", "inside_zr2", "pair_tail", "inside_lat", "pair_lat", "outside",
            "outside_lat", "pair_lat outside", "record", "wait", "count", "wrap A", "wrap B", "head=1", "form=14",
            "class=1", "one kernel, two, one again"} <= seen
