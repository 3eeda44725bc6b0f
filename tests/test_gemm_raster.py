"""The GEMM workgroup -> job map (csrc/gemm_plan.h: xcd_lin, tile_of, job_of -- the text the
kernels compile, run on the host by tests/gemm_plan_probe.cpp) checked for being a bijection:
every (batch entry, K piece, row tile, column tile) job is computed by exactly one workgroup
for any grid the launcher builds (plan_gemm: n1 whole-K tiles + tiles_m * tiles_n * batch *
split split jobs), and every tile of one K piece sits on one XCD (workgroup id mod 8) except
where the XCD ranges cut the job list."""
import itertools

import pytest

from gemm_plan_util import probe


def jobs_of(tiles_m1, tiles_m, tiles_n, batch, split, group_m):
    """(b, sidx, tm, tn) of every workgroup id, in launch order."""
    return [tuple(r) for r in probe("jobs", tiles_m1, tiles_m, tiles_n, batch, split, group_m)]


SHAPES = [  # (tiles_m1, tiles_m, tiles_n, batch, split)
    (0, 75, 24, 1, 1), (0, 2, 18, 1, 64), (0, 3, 5, 1, 7), (64, 11, 24, 1, 4),
    (0, 1, 1, 96, 1), (0, 2, 3, 40, 1), (0, 9, 2, 3, 5), (0, 13, 7, 1, 1),
]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("group_m", [0, 8])
def test_job_map_is_a_bijection(shape, group_m):
    tiles_m1, tiles_m, tiles_n, batch, split = shape
    nblocks = tiles_m1 * tiles_n + tiles_m * tiles_n * batch * split
    jobs = jobs_of(tiles_m1, tiles_m, tiles_n, batch, split, group_m)
    expect = {(0, 0, tm, tn) for tm, tn in itertools.product(range(tiles_m1), range(tiles_n))}
    expect |= {(b, s, tiles_m1 + tm, tn) for b, s, tm, tn in
               itertools.product(range(batch), range(split), range(tiles_m), range(tiles_n))}
    assert len(set(jobs)) == nblocks and set(jobs) == expect


def test_split_pieces_stay_on_one_xcd():
    # wgrad-like: 2 x 18 tiles, 64 K pieces -> each XCD owns 8 whole pieces
    tiles_m, tiles_n, split = 2, 18, 64
    xcd_of = {}
    jobs = jobs_of(0, tiles_m, tiles_n, 1, split, 8)
    assert len(jobs) == tiles_m * tiles_n * split
    for bid, (_, s, _, _) in enumerate(jobs):
        xcd_of.setdefault(s, set()).add(bid % 8)
    assert all(len(x) == 1 for x in xcd_of.values())
