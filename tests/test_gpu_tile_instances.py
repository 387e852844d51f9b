"""GPU tier (-m gpu): every kernel ttsweep_tile.hip can launch for a small star - tile_six_kernel and
tile_sweep_kernel<NE, EXACT>, NE in {6, 18, 26} -, with every halo R in {1, 2} and every z-face depth FZ in 1..4, on
grids of several tiles per axis with ragged last tiles, every cell of every box against the CPU oracle, bit for bit.

The other TILE tests reach four of the seven instances (the six kernel, <26, false>, <18, true>, <26, true>), R = 1
only with FZ = 1, and leave a start on a tile edge to chance.  Here the stars of tile_cases.py are solved from starts
in the grid's corners, on both sides of a tile corner and inside the z halo of the tile below and the tile above -
where the EXACT instances' start_at decides whether a reverse-only entry is dead although the start lies in another
tile -, three starts to a launch.  Grid C's last z tile has 2 cells, fewer than the faces of the FZ 3 and 4 stars are
deep; B's has exactly 4.

Every test asserts the kernel it ran on (kernel_variant, fallbacks; the six star runs the hyperplane launches under
OPT_ASYNC = 0, every other star by rule).  Fresh device solves start from boxes full of -7.0, a value no solve
produces.  A solve's return value and its per-start outcome are asserted as include/ttsweep.h defines them: 1 exactly
where a travel time improved - half26 from the origin reaches no cell, so its fresh box is already at rest.  The
stars, grids, starts and damage are pinned without a GPU by test_tile_cases_cpu.py."""
import numpy as np
import pytest

import tile_cases as T
from conftest import assert_bit_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

CELL, TILE = 1, 3
POISON = -7.0


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


class Case:
    """A star on a grid: the volume, the starts and the oracle's boxes for them (computed once, never written to)."""

    def __init__(self, P, oracle, name, grid):
        self.name, self.grid, self.star, self.shape = name, grid, T.STARS[name], T.GRIDS[grid]
        self.what = f"{name} on {grid} {T.grid_id(self.shape)}"
        self.v = T.velocity(self.shape)
        self.fs = P.inputs.make_fs(self.star.offs)
        self.starts = T.starts_of(grid)
        self.want = T.oracle_boxes(oracle, self.v, self.star, self.starts)
        for box in self.want:
            box.setflags(write=False)
        pull = P.build_pull_star(self.fs, self.star.starstart, self.star.starstop)
        assert T.tile_instance(pull) == self.star.instance and (T.tile_R(pull), T.tile_fz(pull)) == (self.star.R, self.star.FZ)


@pytest.fixture(scope="module")
def cases(P, oracle):
    cache = {}

    def get(name, grid):
        if (name, grid) not in cache:
            cache[name, grid] = Case(P, oracle, name, grid)
        return cache[name, grid]

    return get


def solver(P, case, kernel=TILE):
    sol = P.TravelTimeSolver(case.shape, case.fs, case.star.starstart, case.star.starstop)
    sol.set_option(P.OPT_KERNEL, kernel)
    if kernel == TILE and case.star.instance == T.SIX:
        sol.set_option(P.OPT_ASYNC, 0)      # the six kernel: a launch per hyperplane instead of the column pipelines
    sol.set_velocity(case.v)
    return sol


def poisoned(n, shape):
    import torch
    return torch.full((n,) + tuple(shape), POISON, dtype=torch.float32, device="cuda:0")


def on_device(boxes):
    import torch
    return torch.from_numpy(np.stack(boxes)).to("cuda:0")


def assert_ran_on_tile(st, what):
    assert st["kernel_variant"] == TILE and st["fallbacks"] == 0, (what, st)
    assert st["launches"] > 1, (what, st)       # hyperplane launches, not the one-launch column driver


def assert_boxes(got, want, starts, what):
    got = got.cpu().numpy()
    for s in range(len(want)):
        assert_bit_equal(got[s], want[s], f"{what}, start {tuple(starts[s])}")


@pytest.mark.parametrize("name,grid", T.cases(), ids=[f"{n}-{g}" for n, g in T.cases()])
def test_every_instance_and_halo_geometry_vs_oracle(P, cases, name, grid):
    """Three starts to a solve, one context: fresh boxes, the converged boxes again (0, no bit moves), damaged boxes
    (a block back at INFINITY across the first z-tile boundary, a slab raised) restored with init = 0."""
    case = cases(name, grid)
    with solver(P, case) as sol:
        for batch in T.batches(grid):
            starts, want = case.starts[batch], case.want[batch]
            n = len(starts)
            what = f"{case.what}, starts {[tuple(s) for s in starts]}"
            improved = [T.improves(f, w) for f, w in zip(T.fresh_boxes(case.shape, starts), want)]
            assert improved == [int(not (name == "half26" and tuple(s) == (0, 0, 0))) for s in starts], what
            tt = poisoned(n, case.shape)
            assert sol.solve_device(starts, tt, init=True) == max(improved), what
            assert_ran_on_tile(sol.stats(), f"{what} fresh")
            assert sol.changed(n) == improved, what
            assert_boxes(tt, want, starts, f"{what} fresh")
            # the converged boxes again: nothing to do, no bit moves
            assert sol.solve_device(starts, tt, init=False) == 0, what
            st = sol.stats()
            assert st["kernel_variant"] == TILE and st["fallbacks"] == 0, (what, st)
            assert sol.changed(n) == [0] * n, what
            assert_boxes(tt, want, starts, f"{what} second solve")
            # damaged boxes: tile state and z faces are rebuilt from the boxes' own values
            damaged = [T.damage(want[s], starts[s]) for s in range(n)]
            hurt = [T.improves(d, w) for d, w in zip(damaged, want)]
            assert hurt == improved, what       # (a box with nothing reached has nothing to damage)
            dmg = on_device(damaged)
            assert sol.solve_device(starts, dmg, init=False) == max(hurt), what
            assert_ran_on_tile(sol.stats(), f"{what} damaged")
            assert sol.changed(n) == hurt, what
            assert_boxes(dmg, want, starts, f"{what} after damage")


@pytest.mark.parametrize("name", list(T.STARS))
def test_cell_kernel_agrees_with_tile_on_A(P, cases, name):
    """The per-cell kernel, an independent implementation (one hop per pass, no tiles, no faces), over the same star
    range, volume and starts: the oracle's bits, hence TILE's."""
    case = cases(name, "A")
    n = len(case.starts)
    with solver(P, case, kernel=CELL) as sol:
        tt = poisoned(n, case.shape)
        assert sol.solve_device(case.starts, tt, init=True) == 1, case.what
        st = sol.stats()
        assert st["kernel_variant"] == CELL and st["fallbacks"] == 0, (case.what, st)
        assert sol.changed(n) == [T.improves(f, w) for f, w in zip(T.fresh_boxes(case.shape, case.starts), case.want)]
        assert_boxes(tt, case.want, case.starts, f"{case.what} (CELL)")
