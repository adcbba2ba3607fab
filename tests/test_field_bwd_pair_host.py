"""Host restatement of the tile walk of the pair form of the fused field backward (csrc/mlp.hip: pair_walk and the trip loops of
field_pair_color_kernel / field_pair_sdf_kernel).  No GPU: the one property that can hang a machine -- every wave of a workgroup
meeting the same number of workgroup barriers -- and the one that decides the sums -- every tile accumulated exactly once -- are
checked on the loop bounds alone."""
import numpy as np

CUS = 256                       # MI355X; the launch takes min(ceil(n_tiles / 4), CUs) workgroups, every grid up to CUs is walked here
BARRIERS_PER_TRIP = {"color": 4, "sdf": 2}


def pair_walk(block, pair, grid, n_tiles):
    """pair_walk() of csrc/mlp.hip -> (chunk, n_chunks, trips)"""
    n_chunks = 4 * grid
    first = 4 * block
    trips = (n_tiles - first + n_chunks - 1) // n_chunks if first < n_tiles else 0
    return first + pair, n_chunks, trips


def walk_of_workgroup(block, grid, n_tiles):
    """-> per pair: (barrier trips made, tiles accumulated, tiles loaded): the loop body of the kernels, index arithmetic only"""
    out = []
    for pair in range(4):
        chunk, n_chunks, trips = pair_walk(block, pair, grid, n_tiles)
        made, accumulated, loaded = 0, [], []
        for trip in range(trips):
            want = chunk + trip * n_chunks
            active = want < n_tiles
            tile = want if active else n_tiles - 1
            loaded.append(tile)
            if active:
                accumulated.append(tile)
            made += 1                                   # the trip's barriers: under no condition
        out.append((made, accumulated, loaded))
    return out


def test_every_wave_of_a_workgroup_meets_the_same_barriers_and_every_tile_is_accumulated_once():
    """n_tiles 0 .. 4 CUs 2 + 9 (not only the multiples of 4 the host side produces) x every grid 1 .. CUs, vectorised over
    n_tiles, workgroups and pairs.  The trip count is a function of the workgroup alone (equal barriers for its eight waves by
    construction of `trips`); what has to hold is that it is enough for each pair's own tiles, with at most one idle trip, and
    that the pairs' own tiles add up to the call.  A tile t belongs to chunk t % n_chunks on trip t / n_chunks, so "enough trips
    for every pair" IS "every tile accumulated, and once"; the written-out form of that is the next test's."""
    n = np.arange(0, 4 * CUS * 2 + 10, dtype=np.int32)[:, None]          # [N, 1]
    for grid in range(1, CUS + 1):
        n_chunks = 4 * grid
        first = 4 * np.arange(grid, dtype=np.int32)[None, :]             # [1, grid]
        trips = np.where(first < n, (n - first + n_chunks - 1) // n_chunks, 0)                       # [N, grid]
        for pair in range(4):
            chunk = first + pair
            own = np.where(chunk < n, (n - chunk + n_chunks - 1) // n_chunks, 0)                      # tiles the pair has to walk
            idle = trips - own
            assert idle.min() >= 0 and idle.max() <= 1, (grid, pair)
            total = own.sum(axis=1) if pair == 0 else total + own.sum(axis=1)
        assert (total == n[:, 0]).all(), grid


def test_the_scalar_restatement_agrees_on_the_unequal_trip_cases():
    """The loop written out wave by wave, at the sizes of the GPU tests: a workgroup whose pairs have unequal tile counts still makes
    the same number of trips in each wave of it, for both launches' barrier counts."""
    cases = [(1, 1), (1, 4), (2, 5), (2, 6), (CUS, 4 * CUS + 1), (CUS, 4 * CUS + 2), (CUS, 8 * CUS + 4), (CUS, 8 * CUS + 9)]
    cases += [(grid, n_tiles) for grid in (1, 2, 3, 7) for n_tiles in range(0, 8 * grid + 10)]
    for grid, n_tiles in cases:
        every = []
        for block in range(grid):
            walks = walk_of_workgroup(block, grid, n_tiles)
            for launch, per_trip in BARRIERS_PER_TRIP.items():
                assert len({made * per_trip for made, _, _ in walks}) == 1, (launch, grid, n_tiles, block)
            for made, accumulated, loaded in walks:
                assert all(0 <= t < n_tiles for t in loaded)
                every += accumulated
        assert sorted(every) == list(range(n_tiles)), (grid, n_tiles)
