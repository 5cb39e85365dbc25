"""Host-side pieces of the D-sharded mask-trained dp_gp_lvm (pure NumPy, no GPU): the split of the columns by cost
(weighted_shard_bounds) against a brute-force search, its agreement with shard_bounds at equal costs, and the per-share column
batches of a mask, whose union must be the batch of the whole mask — shares without any observed column included."""
import itertools

import numpy as np
import pytest

from dp_gp_lvm_amd.models.dp_gp_lvm import shard_bounds, weighted_shard_bounds
from dp_gp_lvm_amd.utils import missing


def all_bounds(costs, world, align):
    return [weighted_shard_bounds(costs, r, world, align) for r in range(world)]


def brute_force_optimum(costs, world, align):
    """The smallest largest share over ALL contiguous aligned splits into `world` shares (empty ones allowed)."""
    d = len(costs)
    marks = sorted(set(list(range(0, d, align)) + [d]))
    best = np.inf
    for cuts in itertools.combinations_with_replacement(marks, world - 1):
        edges = (0,) + cuts + (d,)
        best = min(best, max(costs[a:b].sum() for a, b in zip(edges[:-1], edges[1:])))
    return best


@pytest.mark.parametrize('align', [1, 2, 3])
@pytest.mark.parametrize('world', range(1, 9))
def test_weighted_split_is_a_contiguous_aligned_cover_with_the_optimal_largest_share(world, align):
    rng = np.random.default_rng(100 * world + align)
    for trial in range(12):
        d = int(rng.integers(1, 13)) if trial < 9 else int(rng.integers(13, 200))
        costs = rng.integers(0, 50, d).astype(np.float64) if trial % 2 else rng.random(d) * 10.0
        if trial % 4 == 3:
            costs[rng.random(d) < 0.4] = 0.0                        # (columns that cost nothing)
        b = all_bounds(costs, world, align)
        assert b[0][0] == 0 and b[-1][1] == d
        for (lo, hi), (lo2, _) in zip(b[:-1], b[1:]):
            assert hi == lo2
        for lo, hi in b:
            assert 0 <= lo <= hi <= d and (lo % align == 0 or lo == d) and (hi % align == 0 or hi == d)
        if world <= -(-d // align):                                  # (a fortiori while world <= D / align)
            assert all(hi > lo for lo, hi in b), (costs, b)
        largest = max(costs[lo:hi].sum() for lo, hi in b)
        if d <= 12:
            want = brute_force_optimum(costs, world, align)
            assert largest <= want * (1.0 + 1e-12) + 1e-12, (costs, world, align, b, largest, want)
        assert b == all_bounds(costs.copy(), world, align)          # deterministic: every rank computes the same bounds


@pytest.mark.parametrize('world', range(1, 9))
def test_equal_costs_reproduce_shard_bounds(world):
    for d in range(world, 41):
        for cost in (1, 7):
            got = all_bounds(np.full(d, cost), world, 1)
            assert got == [shard_bounds(d, r, world) for r in range(world)], (d, world, got)


def test_the_mask_cost_places_empty_columns():
    """The model's cost, observed rows + 1: a block of never-observed columns still gets spread, and the heavy columns are not
    all on one rank."""
    obs = np.zeros((20, 8), dtype=bool)
    obs[:, 4:] = True
    costs = obs.sum(axis=0) + 1
    b = all_bounds(costs, 4, 1)
    assert all(hi > lo for lo, hi in b) and b != [shard_bounds(8, r, 4) for r in range(4)]
    assert max(costs[lo:hi].sum() for lo, hi in b) == 25                     # (4 empty + 1 full | 1 | 1 | 1 full column)


@pytest.mark.parametrize('world', [1, 2, 3, 5, 7])
def test_union_of_the_local_batches_is_the_global_batch(world):
    rng = np.random.default_rng(world)
    obs = rng.random((9, 11)) >= 0.4
    obs[:, :4] = False                                               # (a run of never-observed columns: whole shares with none)
    obs[:, 8] = False
    whole = missing.observed_columns(obs)
    assert np.array_equal(whole, np.flatnonzero(obs.any(axis=0)))
    for bounds in ([shard_bounds(11, r, world) for r in range(world)], all_bounds(obs.sum(axis=0) + 1, world, 1)):
        parts = [missing.observed_columns(obs, lo, hi) for lo, hi in bounds]
        for (lo, hi), p in zip(bounds, parts):
            assert np.array_equal(p, missing.observed_columns(obs[:, lo:hi]))      # counted from lo
            assert p.size == 0 or (p.min() >= 0 and p.max() < hi - lo)
        assert np.array_equal(np.concatenate([p + lo for (lo, _), p in zip(bounds, parts)]), whole)
    if world >= 3:
        lo, hi = shard_bounds(11, 0, world)
        assert missing.observed_columns(obs, lo, hi).size == 0         # rank 0 owns no observed column
