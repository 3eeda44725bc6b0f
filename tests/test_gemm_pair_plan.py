"""The paired GEMM launch on the CPU: tests/gemm_pair_probe.cpp, a stand-alone program built
against csrc/gemm_plan.h with the host compiler, checks the launcher's own workgroup -> (member,
job) map and its overlap rule.  It is built and run a second time with
-fsanitize=address,undefined (host code in its own executable; nothing is preloaded)."""
import os
import subprocess

import pytest

from gemm_plan_util import CSRC, ROOT, host_compiler

MEMBERS = 7  # the probe's table: unsplit (grouped, plain), split 3, split 7 (plain, grouped), tail split (grouped, plain)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or ROCm clang++)")
    exe = str(tmp_path_factory.mktemp("gemm_pair_probe") / "probe")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "gemm_pair_probe.cpp"), "-o", exe], check=True)

    def run(cmd):
        out = subprocess.run([exe, cmd], check=True, capture_output=True, text=True).stdout
        return [line.split() for line in out.splitlines()]
    return run


def test_pair_map_covers_both_members_once(probe):
    """Every workgroup id of [0, n0 + n1) maps to exactly one (member, job) and every job of both
    members is hit once: unsplit members, split 3 and split 7, a tail-split member at 256 CUs,
    plain and grouped raster, every ordered pair (so both member orders)."""
    rows = [[int(x) for x in r] for r in probe("map")]
    assert len(rows) == MEMBERS * MEMBERS
    assert {(r[0], r[1]) for r in rows} == {(i, j) for i in range(MEMBERS) for j in range(MEMBERS)}
    for i, j, n0, n1, ok, m_split, split in rows:
        assert n0 > 0 and n1 > 0
        assert ok == 1, f"members {i}, {j}: the pair map misses or repeats a job"
    by_first = {r[0]: r for r in rows}
    assert by_first[2][6] == 3 and by_first[3][6] == 7 and by_first[4][6] == 7  # the splits the table names
    for t in (5, 6):  # the tail-split members really are tail-split at 256 CUs
        assert by_first[t][5] > 0 and by_first[t][6] > 1


def test_overlap_rule(probe):
    got = {name: int(v) for name, v in probe("overlap")}
    assert got["dependent"] == 0  # member 1 reads member 0's C
    assert got["column_slices"] == 1  # disjoint column slices of one buffer
    assert got["column_slices_shared"] == 0
    assert got["workspace_over_rowsum"] == 0
    assert got["both_write_one_c"] == 0
