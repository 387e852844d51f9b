"""CPU tier: the ground the column driver's limit tests (test_gpu_column_limits.py) stand on, checked where no GPU
is: the tile counts of the tall grids against a mirror of tile_count, which grids the rules send to which driver, the
starts, the branches of column_order_default the graded volume reaches, the damage, and the oracle's boxes."""
import numpy as np
import pytest

import column_cases as C


def test_constants_are_the_ones_the_grids_were_chosen_for():
    """A change of the tile shape or of COL_MAX_NK that moves a grid off its edge fails here instead of turning the
    GPU tests vacuous."""
    assert C.column_constants() == (8, 8, 32, 32)


@pytest.mark.parametrize("shape,nk,column,in_place", C.TALL_GRIDS, ids=[C.grid_id(g[0]) for g in C.TALL_GRIDS])
def test_tall_grids_sit_on_the_edges_of_the_column_rule(shape, nk, column, in_place):
    tx, ty, tz, max_nk = C.column_constants()
    assert C.tiles(shape) == (C.tile_count(shape[0], tx), C.tile_count(shape[1], ty), nk)
    assert C.column_eligible(shape) == column == (nk <= max_nk)
    assert C.in_place_eligible(shape) == in_place
    assert (tz * (max_nk - 1) < shape[2] <= tz * max_nk) == (nk == max_nk)
    st = C.tall_starts(shape)
    assert st.shape == (5, 3) and (st >= 0).all() and (st < np.array(shape)).all()
    assert len({tuple(s) for s in st}) == 5
    assert tuple(st[0]) == (0, 0, 0) and tuple(st[1]) == tuple(n - 1 for n in shape)
    assert st[2][2] == tz * (nk - 1) and C.tile_of(shape, st[2])[2] == nk - 1           # first cell of the top tile
    assert st[3][2] == tz * (nk - 1) - 1 and C.tile_of(shape, st[3])[2] == nk - 2       # last cell of the tile below
    assert C.tile_of(shape, st[4])[2] in (nk // 2 - 1, nk // 2)


def test_the_edges_are_all_there():
    by_nk = {}
    for shape, nk, column, in_place in C.TALL_GRIDS:
        by_nk.setdefault(nk, []).append((shape, column, in_place))
    assert sorted(by_nk) == [31, 32, 33]
    assert [g[2] for g in by_nk[32]] == [True, False] and all(g[1] for g in by_nk[32])
    assert by_nk[32][0][0][0] % 8 and by_nk[32][1][0][2] % 32 == 8      # ragged x in place; 8 live cells in the top tile
    assert not any(g[1] for g in by_nk[33])
    assert [g[0][2] % 32 for g in by_nk[33]] == [1, 0]                   # one cell too tall; whole rows, too tall
    assert C.NK32_GRIDS == [(9, 8, 1024), (17, 3, 1000)]


@pytest.mark.parametrize("shape", [g[0] for g in C.TALL_GRIDS], ids=C.grid_id)
def test_graded_volume_reaches_every_branch_of_the_default_order(shape):
    v = C.velocity(shape, "graded")
    assert v.dtype == np.float32 and (v > 0.14).all() and (v < 0.43).all()
    got = C.default_orders(shape, v, C.tall_starts(shape))
    assert got[0] == (111, "slow end") and got[1] == (111, "fast end") and got[4] == (115, "middle"), got
    assert {g[1] for g in got} == {"slow end", "fast end", "middle"}
    r = C.velocity(shape, "random")
    assert r.dtype == np.float32 and (r >= 0.1).all() and (r <= 0.5).all() and not np.array_equal(r, v)


def test_order_default_mirror():
    assert C.order_default((9, 8, 64), 0.10, 0.1, 0.5) == (111, "fast end")
    assert C.order_default((9, 8, 64), 0.49, 0.1, 0.5) == (111, "slow end")
    assert C.order_default((90, 8, 64), 0.49, 0.1, 0.5) == (115, "middle")          # wider than deep
    assert C.order_default((9, 8, 64), 0.30, 0.1, 0.5) == (115, "middle")
    assert C.order_default((9, 8, 64), 0.30, 0.3, 0.3) == (115, "middle")           # a flat line


@pytest.mark.parametrize("shape", C.MANY_GRIDS, ids=C.grid_id)
def test_many_starts(shape):
    st = C.many_starts(shape)
    assert st.shape == (C.MANY, 3) and C.MANY > 64 and (st >= 0).all() and (st < np.array(shape)).all()
    assert tuple(st[0]) == (0, 0, 0) and tuple(st[64]) == tuple(n - 1 for n in shape)
    assert C.tile_of(shape, st[0]) != C.tile_of(shape, st[64])
    assert (st[4] == st[5]).all()
    assert C.column_eligible(shape)
    assert C.in_place_eligible(shape) == (shape == (9, 8, 64))
    assert C.tiles((9, 8, 64)) == (2, 1, 2) and C.tiles((17, 16, 97)) == (3, 2, 4)


def test_other_grids():
    assert C.in_place_eligible(C.ANY_ADDRESS_GRID)
    assert (C.ANY_ADDRESS_STARTS < np.array(C.ANY_ADDRESS_GRID)).all()
    cells = int(np.prod(C.ANY_ADDRESS_GRID))
    for off in C.ANY_ADDRESS_OFFSETS:       # (the allocator's alignment is at least 64 bytes; GUARD floats keep it)
        for s in range(len(C.ANY_ADDRESS_STARTS)):
            assert ((C.GUARD + off + s * cells) * 4 % 64 == 0) == (off == 16)
    for shape in C.HANDOVER_CANDIDATES:
        assert C.in_place_eligible(shape)
        st = C.handover_starts(shape)
        assert st.shape == (2, 3) and (st >= 0).all() and (st < np.array(shape)).all()


def test_damage_only_raises():
    rng = np.random.default_rng(3)
    for shape, start in (((9, 8, 1024), (4, 4, 992)), ((3, 10, 1025), (0, 0, 0)), ((20, 37, 96), (19, 0, 95)), ((8, 8, 32), (1, 2, 3))):
        box = rng.uniform(1.0, 2.0, size=shape).astype(np.float32)
        box[start] = 0
        for fn in (C.damage, C.damage_heavy):
            d = fn(box, start)
            assert d.dtype == np.float32 and d[start] == 0 and (d >= box).all() and np.isinf(d).any()
            assert ((d > box) & np.isfinite(d)).any()
        assert np.isinf(C.damage_heavy(box, start)).sum() > np.isinf(C.damage(box, start)).sum()
        top = 32 * (C.tiles(shape)[2] - 1)
        if top:
            dz = np.nonzero(np.isinf(C.damage(box, start)).any(axis=(0, 1)))[0]
            assert dz.min() < top <= dz.max()


def test_oracle_boxes_are_finite_with_zero_at_the_start(oracle):
    """Every tall grid, both volumes: oracle_boxes asserts it for each box."""
    offs = C.six_offsets()
    assert offs.shape == (7, 3) and {tuple(o) for o in offs[:-1]} == {(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)}
    for shape, _nk, _c, _i in C.TALL_GRIDS:
        for kind in C.VELOCITIES:
            boxes = C.oracle_boxes(oracle, C.velocity(shape, kind), offs, C.tall_starts(shape))
            assert len(boxes) == 5 and all(b.shape == shape and b.dtype == np.float32 for b in boxes)
