"""CPU check of the DropPath-skip liveness predicates of csrc/gemm_plan.h against brute force.

tests/drop_skip_probe.cpp compiles the header as the host sees it (the kernels compile the same
text), so these are the decisions the fp32 GEMM makes: a block tile runs over no K tile when
every row in it belongs to a dead group, and a 32-element K chunk is skipped when every k in it
does."""
import functools
import os
import subprocess
import tempfile

import pytest

from gemm_plan_util import CSRC, ROOT, host_compiler

GROUPS = (1, 5, 32, 300, 1200)


@functools.lru_cache(maxsize=None)
def _exe():
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or ROCm clang++)")
    tmp = tempfile.TemporaryDirectory(prefix="drop_skip_probe_")
    _exe.keep = tmp  # removed at interpreter exit
    exe = os.path.join(tmp.name, "probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "drop_skip_probe.cpp"), "-o", exe], check=True)
    return exe


def _probe(*args):
    out = subprocess.run([_exe(), *map(str, args)], check=True, capture_output=True, text=True).stdout
    return [int(c) for c in out.strip()]


def _extents(group):
    # not multiples of 32 or 128; whole groups and a ragged last group
    return sorted({4 * group + 3 if group >= 32 else 137, 3 * group + group // 2 + 1 if group >= 32 else 61,
                   4 * group if group >= 300 else 4 * group + 1})


def _patterns(n):
    """Masks over n groups: all live, all dead, first / last (dead alone and live alone), alternating."""
    pats = {"1" * n, "0" * n, "0" + "1" * (n - 1), "1" * (n - 1) + "0", "1" + "0" * (n - 1), "0" * (n - 1) + "1",
            ("10" * n)[:n], ("01" * n)[:n],
            ("s-" * n)[:n], ("0n" * n)[:n]}  # a scale and -0.0f; NaN counts as live
    return sorted(p for p in pats if len(p) == n)


def _dead(ch):
    return ch in "0-"


@pytest.mark.parametrize("group", GROUPS)
def test_rows_all_dead_matches_brute_force(group):
    for M in _extents(group):
        assert M % 128 != 0
        n = -(-M // group)
        for mask in _patterns(n):
            for tile in (128, 256):
                want = [int(all(_dead(mask[i // group]) for i in range(t0, min(t0 + tile, M))))
                        for t0 in range(0, M, tile)]
                assert _probe("rows", group, M, tile, mask) == want, (group, M, tile, mask)


@pytest.mark.parametrize("group", GROUPS)
def test_chunk_live_matches_brute_force(group):
    for K in _extents(group):
        n = -(-K // group)
        for mask in _patterns(n):
            want = [int(any(not _dead(mask[k // group]) for k in range(k0, min(k0 + 32, K)))) for k0 in range(0, K, 32)]
            assert _probe("chunks", group, K, mask) == want, (group, K, mask)


def test_extents_cover_partial_tiles_and_chunks():
    ks = [K for g in GROUPS for K in _extents(g)]
    assert any(K % 32 for K in ks) and any(K % 128 for K in ks)
    # 1200 tokens per sample against 128-row tiles and 32-element chunks: the flagship's stage-2 geometry
    assert 4800 in _extents(1200) and 4800 % 128 != 0
