"""CPU checks of the GEMM launch plan and variant tables (csrc/gemm_plan.h), read through
tests/gemm_plan_probe.cpp: the launcher's own arithmetic, built with the host compiler.

The families' central guarantee -- the autotuner's pick never changes a result bit -- rests
on every variant of every family cutting K at the same boundaries and splitting the same
rows; that, the tile cover and the workspace sizes are properties of plan_gemm alone."""
import pytest

from gemm_plan_util import GEMM_B16, GEMM_BF16, GEMM_F32, GEMM_F32E, probe, tail_plan_m_split

CUS = 256
COLS = ("mode", "v", "rows", "cols", "bk", "split", "ktile_per_split", "m_split", "tiles_m1", "tiles_m", "tiles_n",
        "nblocks", "slab_bytes", "rowsum_bytes", "deep")
SHAPES = [(700, 300, 1000), (520, 264, 999), (384, 192, 320)]
CASES = ([(M, N, K, 1, s) for (M, N, K) in SHAPES for s in (1, 4, 5)]
         + [(24, 40, 300000, 1, 512), (128, 128, 31, 1, 4), (64, 64, 64, 96, 1)])  # (M, N, K, batch, split_k)
NVARIANTS = {GEMM_F32: 13, GEMM_BF16: 5, GEMM_F32E: 5, GEMM_B16: 3}  # table lengths (fp32e shares the 16-bit table)


def plans(M, N, K, batch, split_k, cus=CUS, row_scale=0):
    return [dict(zip(COLS, r)) for r in probe("plan", M, N, K, batch, split_k, cus, row_scale)]


def test_tables_and_autotune_candidates():
    """Table lengths, and the candidates in the order the autotuner times them (ties go to the
    first): with operands that can / cannot be staged by DMA."""
    rows = probe("tables")
    got = {rows[i][0]: (rows[i][1], rows[i + 1], rows[i + 2]) for i in range(0, len(rows), 3)}
    assert got == {
        GEMM_F32: (13, [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], [0, 1, 3, 4, 5, 6, 7]),
        GEMM_BF16: (5, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]),
        GEMM_F32E: (5, [0, 1, 2], [0, 1, 2]),
        GEMM_B16: (3, [0, 1, 2], [0, 1, 2]),
    }


@pytest.mark.parametrize("case", CASES)
def test_plan_invariants(case):
    M, N, K, batch, split_k = case
    ps = plans(*case)
    # every mode and every variant legal for it (fp32e: not the bf16-image variants)
    assert [(p["mode"], p["v"]) for p in ps] == (
        [(GEMM_F32, v) for v in range(13)] + [(GEMM_BF16, v) for v in range(5)]
        + [(GEMM_F32E, v) for v in range(3)] + [(GEMM_B16, v) for v in range(3)])
    first = ps[0]
    for p in ps:
        # the precondition of bit-identity: the same K boundaries and the same split rows
        assert (p["split"], p["m_split"], p["ktile_per_split"] * p["bk"]) == \
            (first["split"], first["m_split"], first["ktile_per_split"] * first["bk"]), p
        assert p["tiles_m1"] * p["rows"] == p["m_split"], p
        # the tiles cover M and N and the last tile is not empty
        assert (p["tiles_m"] - 1) * p["rows"] < M - p["m_split"] <= p["tiles_m"] * p["rows"], p
        assert (p["tiles_n"] - 1) * p["cols"] < N <= p["tiles_n"] * p["cols"], p
        kps = p["ktile_per_split"] * p["bk"]
        assert (p["split"] - 1) * kps < K <= p["split"] * kps, p
        assert p["nblocks"] == p["tiles_m1"] * p["tiles_n"] + p["tiles_m"] * p["tiles_n"] * batch * p["split"], p
        # mdemi_gemm_workspace_size plans variant 0 of the fp32 family for all of them
        assert (p["slab_bytes"], p["rowsum_bytes"], p["deep"]) == \
            (first["slab_bytes"], first["rowsum_bytes"], first["deep"]), p
        assert p["deep"] == (split_k == 512), p
    assert 1 <= first["split"] <= max(split_k, 4)
    if case == (128, 128, 31, 1, 4):
        assert first["split"] == 1  # one 32-element K chunk: nothing to split
    if first["split"] > 1:
        assert first["slab_bytes"] >= first["split"] * batch * (M - first["m_split"]) * N * 4
    else:
        assert first["slab_bytes"] == 0


def test_deep_combine_leaves_row_scale_to_the_epilogue():
    """split_k = 33 over the 33 chunks of K = 1056 with a plain store takes the deep column-sum
    combine; the same descriptor with a row_scale must not, because column sums apply no scale:
    it keeps the slabs and the ordinary combine, and asks for no column-sum scratch."""
    plain, scaled = plans(24, 40, 1056, 1, 33), plans(24, 40, 1056, 1, 33, row_scale=1)
    assert len(plain) == len(scaled) > 0
    for p, s in zip(plain, scaled):
        assert p["split"] == s["split"] == 33 and p["deep"] == 1 and s["deep"] == 0, (p, s)
        assert {k: v for k, v in p.items() if k != "deep"} == {k: v for k, v in s.items() if k != "deep"}


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_tail_plan_matches_python_statement(cus):
    """tail_plan (C++) against tail_plan_m_split, the Python statement test_gemm_tail_split uses
    to find the split rows on the device it runs on."""
    for M, N, K in SHAPES + [(24, 40, 300000), (128, 128, 31), (64, 64, 64), (9600, 3072, 768)]:
        (m_split, split), = probe("tail", M, N, K, cus)
        assert m_split == tail_plan_m_split(M, N, K, cus), (M, N, K, cus)
        assert (split >= 2) == (m_split > 0) and (m_split > 0 or split == 1)
        # plan_gemm adopts it: the same rows, the same pieces
        p = plans(M, N, K, 1, 1, cus)[0]
        assert (p["m_split"], p["split"]) == (m_split, split)


def test_tail_plan_engages_for_the_profiled_shape():
    """9600x3072x768 on 256 CUs: 1800 tiles = 2 rounds of 768 + 264, which the last 11 tile rows
    hold; rows are cut at (75 - 11) // 2 * 256 = 8192, and 768 // 264 = 2 K pieces fit."""
    assert probe("tail", 9600, 3072, 768, 256) == [[8192, 2]]


def test_set_variant_bounds_follow_the_tables():
    """Each mdemi_gemm_set_variant* hook accepts -1 and every index of its family's table and
    rejects -2 and the table length, without touching the GPU."""
    from mdemi import _lib
    lib = _lib.load()
    n = {row[0]: row[1] for row in probe("tables")[::3]}
    assert n == NVARIANTS
    hooks = [(lambda v: lib.mdemi_gemm_set_variant(v, 8), n[GEMM_F32]),
             (lib.mdemi_gemm_set_variant_m16, n[GEMM_BF16]),
             (lib.mdemi_gemm_set_variant_b16, n[GEMM_B16])]
    for hook, length in hooks:
        try:
            for v in range(-1, length):
                assert hook(v) == 0, v
            for v in (-2, length):
                assert hook(v) < 0, v
                assert b"set_variant" in lib.mdemi_last_error()
        finally:
            assert hook(-1) == 0
