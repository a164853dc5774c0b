"""tests/knob_table.py against the three places a knob must appear in: the name list of
rnamc_ctx_set (rna_algos_amd/csrc/rnamc_ctx.cpp), the GPU suite (tests/test_gpu_*.py) and the knob
paragraph of include/rnamc.h.  The only names rnamc_ctx_set may accept beyond the table are the ones
compiled under RNAMC_DEBUG_KNOBS, found by their #ifdef.  Also: the pairwise table of
tests/test_gpu_knob_forms.py covers every pair of values it promises."""
import glob
import itertools
import os
import re

import knob_table as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ctx_set_names():
    """-> (release names, names compiled under RNAMC_DEBUG_KNOBS only), from the source of rnamc_ctx_set"""
    text = open(os.path.join(ROOT, "rna_algos_amd", "csrc", "rnamc_ctx.cpp")).read()
    body = text[text.index("int rnamc_ctx_set(rnamc_ctx* c, const char* name"):]
    body = body[:body.index("\nint rnamc_ctx_last_stats")]
    release, debug = [], []
    stack = []  # one entry per open conditional: True while inside the RNAMC_DEBUG_KNOBS branch
    for line in body.splitlines():
        s = line.strip()
        if s.startswith("#if"):
            stack.append(bool(re.match(r"#\s*ifdef\s+RNAMC_DEBUG_KNOBS\b", s)))
        elif s.startswith("#else") or s.startswith("#elif"):
            stack[-1] = False
        elif s.startswith("#endif"):
            stack.pop()
        for name in re.findall(r'k == "([a-z0-9_]+)"', line):
            (debug if any(stack) else release).append(name)
    assert not stack
    return release, debug


def knob_paragraph():
    """the comment in front of rnamc_ctx_set's declaration, from "Knobs;" on"""
    text = open(os.path.join(ROOT, "include", "rnamc.h")).read()
    end = text.index("int rnamc_ctx_set(rnamc_ctx* ctx, const char* name, int64_t value);")
    return text[text.rindex("/* Knobs;", 0, end):end]


def test_every_knob_of_the_library_is_in_the_table():
    release, debug = ctx_set_names()
    assert len(release) >= 40 and sorted(debug) == sorted(set(debug)) and len(debug) >= 1
    missing = sorted(set(release) - set(K.KNOBS))
    assert not missing, f"knobs of rnamc_ctx_set without a row in tests/knob_table.py: {missing}"
    stale = sorted(set(K.KNOBS) - set(release))
    assert not stale, f"rows of tests/knob_table.py that rnamc_ctx_set does not accept: {stale}"
    assert not set(debug) & set(release), "a debug-only name is also accepted outside its #ifdef"
    for name, (default, mode, values) in K.KNOBS.items():
        assert mode in K.MODES, name
        assert isinstance(values, tuple), name


def test_every_knob_is_set_in_a_gpu_test():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    assert files
    text = "\n".join(open(f).read() for f in files)
    # set as ctx.set("name", ...), as a keyword of a run(..., name=...) helper or as a key of a knob dict
    unset = [name for name in K.KNOBS
             if not re.search(r'["\']%s["\']|\b%s\s*=' % (name, name), text)]
    assert not unset, f"knobs no tests/test_gpu_*.py sets: {unset}"


def test_every_knob_is_documented_in_the_header():
    para = knob_paragraph()
    undocumented = [name for name in K.KNOBS if f'"{name}"' not in para]
    assert not undocumented, f"knobs the knob paragraph of include/rnamc.h does not name: {undocumented}"


def uncovered_pairs(rows, domains):
    """pairs ((knob a, value), (knob b, value)) of `domains` that no row of `rows` holds together"""
    missing = []
    for a, b in itertools.combinations(sorted(domains), 2):
        seen = {(r[a], r[b]) for r in rows}
        missing += [((a, x), (b, y)) for x in domains[a] for y in domains[b] if (x, y) not in seen]
    return missing


def test_uncovered_pairs_helper():
    dom = {"a": (0, 1), "b": (0, 1, 2)}
    rows = [{"a": x, "b": y} for x in dom["a"] for y in dom["b"]]
    assert uncovered_pairs(rows, dom) == []
    assert uncovered_pairs(rows[:-1], dom) == [(("a", 1), ("b", 2))]


def test_pairwise_table_covers_every_pair():
    import test_gpu_knob_forms as F
    rows = F.pairwise_rows()
    assert len(rows) <= 24
    assert set(F.PAIRWISE_DOMAINS) == {
        "block_threads", "order_inside", "order_outside", "fuse_inside", "dual_outside", "dual_min_cells",
        "latency_mode", "lat_pairs", "lat_merge", "lat_split", "lat_zr_ahead", "lat_inside", "lat_e_waves",
        "group_max_seqs"}
    assert set(F.PAIRWISE_DOMAINS["dual_min_cells"]) == {0, 4096, K.KNOBS["dual_min_cells"][0]}
    assert set(F.PAIRWISE_DOMAINS["lat_e_waves"]) == {0, 64, 2048}
    assert set(F.PAIRWISE_DOMAINS["group_max_seqs"]) == {3, 17, 8192}
    for r in rows:
        assert set(r) == set(F.PAIRWISE_DOMAINS)
        assert all(r[k] in F.PAIRWISE_DOMAINS[k] for k in r)
    # every other knob of the table over the whole range rnamc_ctx_set admits
    assert F.PAIRWISE_DOMAINS["block_threads"] == (64, 128, 192, 256)
    assert F.PAIRWISE_DOMAINS["order_inside"] == (0, 1, 2) and F.PAIRWISE_DOMAINS["order_outside"] == (0, 1, 2, 3, 4)
    assert F.PAIRWISE_DOMAINS["latency_mode"] == (0, 1, 2) and F.PAIRWISE_DOMAINS["lat_inside"] == (0, 2)
    missing = uncovered_pairs(rows, F.PAIRWISE_DOMAINS)
    assert not missing, f"{len(missing)} pairs of values in no row, e.g. {missing[:4]}"
