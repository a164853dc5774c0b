"""CPU suite: the host-only pieces the pool entries share (rna_algos_amd/csrc/rnamc_shards.h), driven by
a stand-alone program (tests/shards_host_check.cpp) built with the address and undefined-behaviour
sanitizers: RecordShards for 1, 2, 3 and 8 shards of 0, 1, 2, 7 and 33 records against a direct
recomputation from the plan's assignment, run_shards' first-failure rule, check_constraints' message.
The program opens no device and is not loaded into Python; the plans it used are held against
rnamc_shard_plan here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shards_host_check(built, tmp_path):
    from rna_algos_amd.mccaskill_algo import shard_plan
    csrc = os.path.join(ROOT, "rna_algos_amd", "csrc")
    exe = os.path.join(str(tmp_path), "shards_host_check")
    # (rnamc_host.cpp reads HIP's headers for its host-device scoring code and calls nothing of HIP; the
    # sanitizers' runtimes are linked statically: the program needs nothing from its environment)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-pthread",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "shards_host_check.cpp"),
                           os.path.join(csrc, "rnamc_host.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK", run.stdout
    plans = [ln.split(" ") for ln in lines if ln.startswith("plan ")]
    assert len(plans) == 4 * 5 * 2
    for _, world, lens, shard_of in plans:
        lens = [] if lens == "-" else [int(x) for x in lens.split(",")]
        got = [] if shard_of == "-" else [int(x) for x in shard_of.split(",")]
        assert shard_plan(lens, int(world)).tolist() == got
