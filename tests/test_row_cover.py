"""The row-cover checks of tests/helpers.py on synthetic outputs, without a GPU.  A persistent loop whose workgroups take groups g,
g + grid, g + 2 grid, ... of 64 rows can go wrong in ways that a comparison on inputs tiled with a period dividing the stride, or on rows
sampled at a stride, cannot see.  Each fault below is built so that such a comparison passes, and the cover check must reject it."""
import numpy as np
import pytest

from helpers import DistinctRows, check_cover, free_q_mask, group_cover

GRID = 8  # workgroups of the simulated loop: a stride of 512 rows
B = 4 * GRID * 64 + 37  # four full iterations and a ragged fifth
PERIOD = 256  # a tile period that divides the stride, as the full-size parity tests have


@pytest.fixture(scope="module")
def humanoid():
    from mecano_amd import random_tools as rt
    return rt.nextHumanoid(np.random.default_rng(43))


def kernel(x):
    """A row-wise stand-in for a HIP kernel: any function of the row's input alone."""
    m = np.cos(np.arange(x.shape[1] * 5, dtype=np.float64).reshape(x.shape[1], 5))
    return np.sin(x @ m) + x[:, :5] ** 2


def outputs(x, fault=None):
    """The kernel's [B + 1, 5] output buffer (a NaN guard row behind the batch) with one of the faults in."""
    n = len(x)
    out = np.full((n + 1, 5), np.nan)
    out[:n] = kernel(x)
    if fault == "iteration_shift":  # iteration k >= 1 computes the rows of iteration k - 1
        out[GRID * 64:n] = kernel(x[: n - GRID * 64])
    elif fault == "group_shift":  # one group's rows from the group before it
        g = 13
        out[g * 64:(g + 1) * 64] = kernel(x[(g - 1) * 64:g * 64])
    elif fault == "ragged_tail":  # the last, partial group never written
        out[n // 64 * 64:n] = np.nan
    elif fault == "guard":  # one row too many
        out[n] = kernel(x[:1])[0]
    return out


def tiled_inputs(sys_):
    base = DistinctRows(sys_, PERIOD, 7)
    return base.q[np.arange(B) % PERIOD]


def distinct_inputs(sys_):
    return DistinctRows(sys_, PERIOD, 7).rows(np.arange(B))[0]


def tile_check(out, x_base):
    """What the full-size tests checked on tiled inputs: first tile equals the last full one, and a strided sample against the base
    (test_config4_at_full_size_on_one_gpu takes every 512th row; a prime stride here, so that no sampled row lands in the tail)."""
    n_tiles = B // PERIOD
    assert np.array_equal(out[:PERIOD], out[(n_tiles - 1) * PERIOD:n_tiles * PERIOD])
    idx = np.arange(0, B, 509)
    assert np.allclose(out[idx], kernel(x_base[idx % PERIOD]), rtol=0, atol=1e-12)


def stride_check(out, x):
    """What the other big-batch checks did: rows at a stride of 499 and the last row."""
    idx = np.unique(np.concatenate([np.arange(0, B, 499), [B - 1]]))
    assert np.allclose(out[idx], kernel(x[idx]), rtol=0, atol=1e-12)


def cover_check(out, x, grid=None):
    idx = group_cover(B, grid)
    check_cover(out[:B], out[B:], idx, kernel(x[idx]), 1e-12, absolute=True, record=False, every_row=False)


def test_group_cover_touches_every_group_and_the_edges():
    for n in (1, 37, 64, 65, 127, 128, 4096, 4133, 262144 + 37):
        idx = group_cover(n)
        assert idx.min() >= 0 and idx.max() < n and np.array_equal(idx, np.unique(idx))
        assert np.array_equal(np.unique(idx // 64), np.arange((n + 63) // 64))  # one row of every group
        assert set(range(min(64, n))) <= set(idx.tolist())  # the first group
        if n >= 64:
            lf = n // 64 - 1
            assert set(range(lf * 64, lf * 64 + 64)) <= set(idx.tolist())  # the last full group
        assert set(range(n // 64 * 64, n)) <= set(idx.tolist())  # the ragged one
        assert n - 1 in idx
        lanes = idx[idx // 64 == 5] % 64 if n > 6 * 64 else None
        assert lanes is None or (37 * 5 + 11) % 64 in lanes
    # the lanes rotate: a lane-confined fault (one of 64 lanes) is seen in a quarter of the groups or more, not in none
    idx = group_cover(65536)
    assert len(np.unique(idx % 64)) == 64
    # with a grid: every row of the first group of each iteration
    idx = group_cover(B, GRID)
    for k in range(0, (B + 63) // 64, GRID):
        assert set(range(k * 64, min(B, k * 64 + 64))) <= set(idx.tolist())


def test_distinct_rows_reproduce_the_device_construction_bit_for_bit(humanoid):
    torch = pytest.importorskip("torch")
    d = DistinctRows(humanoid, 100, 3)
    mask = free_q_mask(humanoid)
    assert (~mask).sum() == 4  # the floating base's quaternion
    n = 1000
    idx = np.array([0, 99, 100, 101, 517, 999])
    for tdt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        full = d.device(torch, n, tdt, device="cpu")
        host = d.rows(idx, ndt)
        for t, h in zip(full, host):
            assert np.array_equal(t.numpy()[idx].astype(np.float64), h)
        q = full[0].numpy()
        assert np.array_equal(q[100:, ~mask], q[:n - 100, ~mask])  # quaternions: the base's, unchanged
        for t in full:  # every row a different state
            assert len(np.unique(t.numpy(), axis=0)) == n


@pytest.mark.parametrize("fault", ["iteration_shift", "group_shift", "ragged_tail", "guard"])
def test_cover_rejects_what_tiles_and_strides_let_through(humanoid, fault):
    x_tiled, x = tiled_inputs(humanoid), distinct_inputs(humanoid)
    # the checker is not blind to the right answer ...
    cover_check(outputs(x), x, GRID)
    # ... the old checks pass the fault ...
    out_tiled = outputs(x_tiled, fault)
    tile_check(out_tiled[:B], x_tiled[:PERIOD])
    if fault in ("group_shift", "guard"):
        stride_check(outputs(x, fault)[:B], x)
    # ... and the cover on distinct rows does not, with or without the loop's grid
    for grid in (None, GRID):
        with pytest.raises(AssertionError):
            cover_check(outputs(x, fault), x, grid)
