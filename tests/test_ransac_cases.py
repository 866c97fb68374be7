"""The shared yardstick's own test (no GPU): tests/ransac_cases.py restates the sampling of csrc/ransac_common.h for both
solvers, so it is checked here for either sample size, with the mutation its users must catch.  Also the host view of the
shared workspace: the byte counts of the three entries are the sums of their 16-byte aligned parts, whatever the order."""
import numpy as np
import pytest

import e_solver_cases as ec
import h_solver_cases as hc
import hl_solver_cases as hl
import ransac_cases as rc


@pytest.mark.parametrize("n,K", [(4, 4), (4, 5), (4, 17), (4, hc.TILE + 1), (5, 5), (5, 6), (5, 17), (5, ec.TILE + 1)])
def test_samples_are_distinct_and_in_range_and_the_skip_mutation_is_caught(n, K):
    cases, seed = (hc, hc.SEED) if n == 4 else (ec, ec.SEED)
    s = cases.samples(seed, 1, 300, K)
    assert np.array_equal(s, rc.samples(n, seed, 1, 300, K)) and s.shape == (300, n)
    assert s.min() >= 0 and s.max() < K
    assert all(len(set(row)) == n for row in s.tolist())
    if K > n:
        assert len({tuple(r) for r in s.tolist()}) > 1
    mutated = rc.samples(n, seed, 1, 300, K, off_by_one=True)
    assert (mutated != s).any()
    assert any(len(set(row)) < n for row in mutated.tolist()) or mutated.max() >= K       # a repeated or out-of-range index


def _al16(x):
    return (x + 15) & ~15


def _core(B, M, nblk):
    return sum(_al16(x) for x in (4 * B, 4 * B * M, 16 * B * M, 8 * B * nblk, 48 * B, 48 * B, 16 * B, B * M))


@pytest.mark.parametrize("B,M,T", [(1, 1, 1), (2, 40, 10), (3, 257, 257), (1, 2048, 256), (32, 2048, 3000), (5, 1, 517)])
def test_workspace_sizes_are_the_sums_of_their_aligned_parts(B, M, T):
    from glue_factory_amd import lib
    L = lib.load()
    assert L.gf_h_ws_bytes(B, M, T) == _core(B, M, (T + hc.HYPS - 1) // hc.HYPS)
    extra = _al16(4 * 9 * ec.MAXSOL * B * T) + _al16(4 * B * T)
    assert L.gf_e_ws_bytes(B, M, T) == _core(B, M, (T * ec.MAXSOL + ec.HYPS - 1) // ec.HYPS) + extra


@pytest.mark.parametrize("B,M,Ln,T", [(1, 1, 0, 1), (1, 0, 1, 1), (2, 40, 7, 10), (3, 257, 257, 257)])
def test_point_and_line_workspace_size_is_the_core_the_line_part_and_the_block_models(B, M, Ln, T):
    from glue_factory_amd import lib
    nblk = (T + hl.HYPS - 1) // hl.HYPS
    lines = sum(_al16(x) for x in (4 * B, 4 * B * Ln, 2 * 16 * B * Ln, 16 * B * Ln, B * Ln))
    assert lib.load().gf_hl_ws_bytes(B, M, Ln, T) == _core(B, M, nblk) + lines + _al16(4 * 12 * B * nblk)
