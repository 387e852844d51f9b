"""GPU tier (-m gpu): the TILE kernel's column driver (ttsweep_column.hip, solve_column in ttsweep_driver.cpp) at the
edges of the interior its other tests stay in, every cell of every box against the CPU oracle, bit for bit.

  A  columns of 31, 32 and 33 tiles: COL_MAX_NK = 32 is the bits of a mask word, and 33 tiles must run as hyperplane
     launches by rule
  B  more than 64 starts (the work counters key a lane on s & 63), and one context used for 1, 70, 2 and 70 starts
  C  caller arrays at any float address (kernels 3, 1 and 2): the drivers' pack, unpack and direct-store kernels
  D  the hand-over to the hyperplane launches after the one launch has run into its wall-clock limit
  E  the sweep-cap error with the caller's arrays half relaxed, and the solve that resumes from them

Every test asserts the driver it ran on (kernel_variant, launches, fallbacks): a later change of a selection rule
cannot move one onto another path while it stays green.  Fresh device solves start from boxes full of -7.0, a value
no solve produces.  The grids, starts, volumes and damage come from column_cases.py (pinned without a GPU by
test_column_cases_cpu.py)."""
import numpy as np
import pytest

import column_cases as C
import strip_cases as S
from conftest import assert_bit_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

CELL, STRIP, TILE = 1, 2, 3
POISON = -7.0


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


@pytest.fixture(scope="module")
def six(P):
    offs = P.inputs.read_triples(P.inputs.star_path("six"))
    assert np.array_equal(offs, C.six_offsets())
    return offs, P.inputs.make_fs(offs)


class Case:
    """A grid, a velocity volume, starts and the oracle's boxes for them."""

    def __init__(self, oracle, shape, v, offs, fs, starts):
        self.shape, self.v, self.offs, self.fs = tuple(shape), v, offs, fs
        self.starts = np.asarray(starts, dtype=np.int32).reshape(-1, 3)
        self.want = C.oracle_boxes(oracle, v, offs, self.starts)


@pytest.fixture(scope="module")
def cases(oracle, six):
    """Oracle boxes, computed once per (grid, volume) of the module and never written to."""
    cache = {}

    def get(shape, kind, starts_of):
        key = (tuple(shape), kind, starts_of.__name__)
        if key not in cache:
            cache[key] = Case(oracle, shape, C.velocity(shape, kind), six[0], six[1], starts_of(shape))
        return cache[key]

    return get


def solver(P, case, options=None, kernel=TILE):
    sol = P.TravelTimeSolver(case.shape, case.fs)
    sol.set_option(P.OPT_KERNEL, kernel)
    for key, value in (options or {}).items():
        sol.set_option(getattr(P, key), value)
    sol.set_velocity(case.v)
    return sol


def poisoned(n, shape):
    import torch
    return torch.full((n,) + tuple(shape), POISON, dtype=torch.float32, device="cuda:0")


def on_device(boxes):
    import torch
    return torch.from_numpy(np.stack(boxes)).to("cuda:0")


def assert_ran_on(st, driver, what=""):
    """columns: ONE launch of column pipelines; hyperplanes: a launch per tile hyperplane, by rule; hand-over: the
    one launch gave up and the hyperplane launches finished the solve."""
    assert st["kernel_variant"] == TILE, (what, st)
    if driver == "columns":
        assert st["launches"] == 1 and st["fallbacks"] == 0, (what, st)
    elif driver == "hyperplanes":
        assert st["launches"] > 1 and st["fallbacks"] == 0, (what, st)
    else:
        assert driver == "hand-over"
        assert st["launches"] > 1 and st["fallbacks"] == 1, (what, st)


def assert_boxes(got, want, starts, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    for s in range(len(want)):
        assert_bit_equal(got[s], want[s], f"{what}, start {tuple(starts[s])}")


def four_steps(P, case, driver, options=None, what=""):
    """Fresh on the device, the converged boxes again, damaged boxes, host boxes: one context."""
    n = len(case.starts)
    with solver(P, case, options) as sol:
        tt = poisoned(n, case.shape)
        assert sol.solve_device(case.starts, tt, init=True) == 1, what
        assert_ran_on(sol.stats(), driver, f"{what} fresh")
        assert sol.changed(n) == [1] * n, what
        assert_boxes(tt, case.want, case.starts, f"{what} fresh")
        # the converged boxes again: nothing to do, no bit moves
        assert sol.solve_device(case.starts, tt, init=False) == 0, what
        st = sol.stats()
        assert st["kernel_variant"] == TILE and st["fallbacks"] == 0 and (st["launches"] == 1) == (driver == "columns"), (what, st)
        assert sol.changed(n) == [0] * n, what
        assert_boxes(tt, case.want, case.starts, f"{what} second solve")
        # damaged boxes: every tile is due from the boxes' own values (the mask ~0u where a column has 32 tiles)
        dmg = on_device([C.damage(case.want[s], case.starts[s]) for s in range(n)])
        assert sol.solve_device(case.starts, dmg, init=False) == 1, what
        assert_ran_on(sol.stats(), driver, f"{what} damaged")
        assert sol.changed(n) == [1] * n, what
        assert_boxes(dmg, case.want, case.starts, f"{what} after damage")
        # host boxes: staged by the library, solved as boxes that arrive with values
        boxes = C.fresh_boxes(case.shape, case.starts)
        assert sol.solve(case.starts, boxes) == 1, what
        assert_ran_on(sol.stats(), driver, f"{what} host boxes")
        assert_boxes(boxes, case.want, case.starts, f"{what} host boxes")


# ---------------------------------------------------------------------------
# A: tall columns
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", C.VELOCITIES)
@pytest.mark.parametrize("shape,nk,column,in_place", C.TALL_GRIDS, ids=[C.grid_id(g[0]) for g in C.TALL_GRIDS])
def test_columns_of_31_32_and_33_tiles(P, cases, shape, nk, column, in_place, kind):
    """The default order on both volumes.  31 and 32 tiles: one launch, in the caller's arrays where their rows are
    whole tiles, in the padded volumes where the top tile has 8 live cells; 33 tiles: hyperplane launches by rule,
    not as a fallback.  Starts in both corners, on both sides of the top tile's lower face and mid-column."""
    assert C.tiles(shape)[2] == nk and C.column_eligible(shape) == column and C.in_place_eligible(shape) == in_place
    case = cases(shape, kind, C.tall_starts)
    if kind == "graded":
        assert {o[1] for o in C.default_orders(shape, case.v, case.starts)} == {"slow end", "fast end", "middle"}
    four_steps(P, case, "columns" if column else "hyperplanes", what=f"{C.grid_id(shape)} {kind}")


NK32_OPTIONS = [
    ({"OPT_TILE_ORDER": 0}, "columns"), ({"OPT_TILE_ORDER": 115}, "columns"), ({"OPT_TILE_ORDER": 429}, "columns"),
    ({"OPT_TILE_IN_PLACE": 0}, "columns"), ({"OPT_QUEUES": 1}, "columns"),
    ({"OPT_ASYNC": 0}, "hyperplanes"),      # the hyperplane driver's own tallest case
]


@pytest.mark.parametrize("options,driver", NK32_OPTIONS, ids=["-".join(f"{k[4:]}={v}" for k, v in o.items()) for o, _ in NK32_OPTIONS])
@pytest.mark.parametrize("shape", C.NK32_GRIDS, ids=C.grid_id)
def test_columns_of_32_tiles_under_every_option(P, cases, shape, options, driver):
    """Sweep orders that flip z (col_flip shifts by 32 - NK = 0), the padded volumes forced, one claim sequence, and
    a launch per hyperplane: the same bits."""
    four_steps(P, cases(shape, "random", C.tall_starts), driver, options, what=f"{C.grid_id(shape)} {options}")


# ---------------------------------------------------------------------------
# B: many starts, one context
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", C.MANY_GRIDS, ids=C.grid_id)
def test_70_starts_after_1_and_2_on_one_context(P, cases, shape):
    """Batches of 1, 70 and 2 starts fresh, then the 70 from damaged boxes: the resident grid, the work counters and
    the per-start state are sized from the batch and regrown on demand; starts 0 and 64 share a lane of the work
    counters and lie in different tiles."""
    case = cases(shape, "random", C.many_starts)
    assert len(case.starts) == 70 and C.tile_of(shape, case.starts[0]) != C.tile_of(shape, case.starts[64])
    with solver(P, case) as sol:
        for index in (slice(0, 1), slice(0, 70), slice(63, 65)):
            starts, want = case.starts[index], case.want[index]
            n = len(starts)
            tt = poisoned(n, shape)
            assert sol.solve_device(starts, tt, init=True) == 1, n
            assert_ran_on(sol.stats(), "columns", f"{n} starts fresh")
            assert sol.changed(n) == [1] * n
            assert_boxes(tt, want, starts, f"{n} starts fresh")
        dmg = on_device([C.damage(case.want[s], case.starts[s]) for s in range(70)])
        assert sol.solve_device(case.starts, dmg, init=False) == 1
        assert_ran_on(sol.stats(), "columns", "70 starts damaged")
        assert sol.changed(70) == [1] * 70
        assert_boxes(dmg, case.want, case.starts, "70 starts after damage")


# ---------------------------------------------------------------------------
# C: caller arrays at any float address
# ---------------------------------------------------------------------------

class Guarded:
    """n boxes inside one flat device buffer, `offset` floats behind GUARD poisoned floats and in front of GUARD more:
    offset 1, 8, 16 puts the first box 4, 32, 64 bytes past the allocator's alignment."""

    def __init__(self, n, shape, offset):
        import torch
        self.cells = int(np.prod(shape))
        self.lo = C.GUARD + offset
        self.hi = self.lo + n * self.cells
        self.buf = torch.full((self.hi + C.GUARD,), POISON, dtype=torch.float32, device="cuda:0")
        assert self.buf.data_ptr() % 64 == 0
        self.tt = self.buf[self.lo:self.hi].view((n,) + tuple(shape))
        assert self.tt.is_contiguous() and self.tt.data_ptr() == self.buf.data_ptr() + 4 * self.lo

    def fill(self, boxes):
        self.tt.copy_(on_device(boxes))

    def assert_guards(self, what):
        front, back = self.buf[:self.lo].cpu().numpy(), self.buf[self.hi:].cpu().numpy()
        assert (front == np.float32(POISON)).all() and (back == np.float32(POISON)).all(), \
            f"{what}: {int((front != np.float32(POISON)).sum())} guard floats in front of the boxes and " \
            f"{int((back != np.float32(POISON)).sum())} behind them were written"


@pytest.fixture(scope="module")
def any_address_tile(oracle, six):
    shape = C.ANY_ADDRESS_GRID
    return Case(oracle, shape, C.velocity(shape), six[0], six[1], C.ANY_ADDRESS_STARTS)


@pytest.fixture(scope="module")
def any_address_five(P, oracle):
    """The direct-store suite's grid with lanes along z (two lane tiles, the second with 3 live lanes), 5-FS star."""
    shape = (65, 66, 67)
    L = S.StripLayout(shape)
    assert L.bax == 2 and L.btiles == 2 and L.last_tile_lanes == 3
    offs = P.inputs.read_triples(P.inputs.star_path("5"))
    return Case(oracle, shape, S.velocity(shape), offs, P.inputs.make_fs(offs), [(32, 33, 65), (0, 0, 0)])


def any_address(P, case, kernel, options, offset, check_stats):
    n = len(case.starts)
    what = f"kernel {kernel} {options}, boxes {4 * offset} bytes past the alignment"
    with solver(P, case, options, kernel) as sol:
        g = Guarded(n, case.shape, offset)
        assert (g.tt.data_ptr() % 64 == 0) == (offset == 16)
        assert sol.solve_device(case.starts, g.tt, init=True) == 1, what
        check_stats(sol.stats(), f"{what} fresh")
        assert sol.changed(n) == [1] * n, what
        g.assert_guards(f"{what} fresh")
        assert_boxes(g.tt, case.want, case.starts, f"{what} fresh")
        g.fill([C.damage(case.want[s], case.starts[s]) for s in range(n)])
        assert sol.solve_device(case.starts, g.tt, init=False) == 1, what
        check_stats(sol.stats(), f"{what} damaged")
        assert sol.changed(n) == [1] * n, what
        g.assert_guards(f"{what} damaged")
        assert_boxes(g.tt, case.want, case.starts, f"{what} after damage")


@pytest.mark.parametrize("offset", C.ANY_ADDRESS_OFFSETS)
def test_column_driver_with_boxes_at_any_float_address(P, any_address_tile, offset):
    """The ABI promises no alignment beyond float: boxes that are not 64-byte aligned are relaxed in the padded
    volumes (column_in_place), the aligned ones where they lie - the same bits, and not a float outside the boxes."""
    any_address(P, any_address_tile, TILE, {}, offset, lambda st, what: assert_ran_on(st, "columns", what))


def _cell(st, what):
    assert st["kernel_variant"] == CELL and st["fallbacks"] == 0, (what, st)


def _strip_one_launch(st, what):
    assert st["kernel_variant"] == STRIP and st["launches"] == 1 and st["fallbacks"] == 0, (what, st)


def _strip_passes(st, what):
    assert st["kernel_variant"] == STRIP and st["launches"] > 1 and st["fallbacks"] == 0, (what, st)


@pytest.mark.parametrize("offset", C.ANY_ADDRESS_OFFSETS)
@pytest.mark.parametrize("kernel,options,check_stats", [(CELL, {}, _cell), (STRIP, {"OPT_ASYNC": 1}, _strip_one_launch),
                                                        (STRIP, {"OPT_ASYNC": 0}, _strip_passes)],
                         ids=["cell", "strip-one-launch", "strip-passes"])
def test_cell_and_strip_with_boxes_at_any_float_address(P, any_address_five, kernel, options, check_stats, offset):
    """The pack and unpack kernels (16-byte accesses where both sides allow them), the batched initialisation and the
    one-launch solve's stores into the caller's boxes, with boxes 4, 32 and 64 bytes past the alignment."""
    any_address(P, any_address_five, kernel, options, offset, check_stats)


# ---------------------------------------------------------------------------
# D: the hand-over
# ---------------------------------------------------------------------------

HANDOVER_GRID = C.HANDOVER_CANDIDATES[0]


@pytest.fixture(scope="module")
def handover(oracle, six):
    shape = HANDOVER_GRID
    return Case(oracle, shape, C.velocity(shape), six[0], six[1], C.handover_starts(shape))


def _handed_over(P, sol, case, solve, want_changed, what):
    """`solve` under a limit of 1 ms: finished by the hyperplane launches, the oracle's boxes, no error left."""
    sol.set_option(P.OPT_ASYNC_TIMEOUT_MILLI, 1)
    assert solve() == 1, what
    assert_ran_on(sol.stats(), "hand-over", what)
    assert sol.changed(len(case.starts)) == want_changed, what
    assert P._lib.last_error() == "", what
    sol.set_option(P.OPT_ASYNC_TIMEOUT_MILLI, 0)


def _long_enough(sol, solve, what):
    """The same solve without the limit first: a grid whose launch is over in less than twice the limit says so here
    instead of failing on `fallbacks`."""
    assert solve() == 1, what
    st = sol.stats()
    print(f"{what}: {st['solve_ms']:.3f} ms in one launch without the limit")
    assert_ran_on(st, "columns", f"{what}, no limit")
    assert st["solve_ms"] >= 2.0, f"{what}: the unlimited one-launch solve took {st['solve_ms']:.3f} ms - the grid is too small for a 1 ms limit"


def _after_the_handover(P, sol, case, what):
    """The same context, no limit: fresh boxes in one launch, and the converged boxes again."""
    n = len(case.starts)
    tt = poisoned(n, case.shape)
    assert sol.solve_device(case.starts, tt, init=True) == 1, what
    assert_ran_on(sol.stats(), "columns", f"{what}, afterwards")
    assert_boxes(tt, case.want, case.starts, f"{what}, afterwards")
    assert sol.solve_device(case.starts, tt, init=False) == 0, what
    assert sol.changed(n) == [0] * n, what
    assert_boxes(tt, case.want, case.starts, f"{what}, afterwards, second solve")


@pytest.mark.parametrize("in_place", [1, 0], ids=["in-place", "padded"])
def test_fresh_solve_that_gives_up_is_finished_by_the_hyperplane_launches(P, handover, in_place):
    """OPT_ASYNC_TIMEOUT_MILLI = 1: the launch drains with the boxes somewhere on their way (in the caller's arrays,
    which are then packed, or in the padded volumes), tile state and z faces are rebuilt from the boxes and the
    hyperplane launches finish the solve.

    The grid is the first of column_cases.HANDOVER_CANDIDATES whose unlimited one-launch solve of these two starts
    reads solve_ms >= 5 (five times the limit) in each of five runs.  72 x 64 x 256 on an MI355X, 62 sweeps: in
    place 6.82, 6.84, 6.83, 6.82, 6.84 ms in five fresh contexts (7.29, 6.82, 6.79, 6.80, 6.80, 6.83 in one);
    padded 6.12, 6.09, 6.11, 6.10, 6.10 ms (6.11, 6.07, 6.05, 6.06, 6.06, 6.09 in one).  (96 x 96 x 256: 8.2 / 7.3 ms,
    128 x 128 x 256: 8.2 / 7.4 ms.)  A second machine read 5.98 ms in place and 5.35 ms padded in this test's own
    unlimited solve.  The oracle needs 2.3 s for the two boxes."""
    case, n = handover, len(handover.starts)
    what = f"{C.grid_id(case.shape)} in place {in_place}"
    with solver(P, case, {"OPT_TILE_IN_PLACE": in_place}) as sol:
        tt = poisoned(n, case.shape)
        _long_enough(sol, lambda: sol.solve_device(case.starts, tt, init=True), what)
        tt = poisoned(n, case.shape)
        _handed_over(P, sol, case, lambda: sol.solve_device(case.starts, tt, init=True), [1] * n, what)
        assert_boxes(tt, case.want, case.starts, what)
        _after_the_handover(P, sol, case, what)


def test_solve_from_boxes_that_gives_up_is_finished_by_the_hyperplane_launches(P, handover):
    """In place, from boxes with values: box 0 heavily damaged, box 1 converged - `changed` names box 0 alone; then
    host boxes, box 0 fresh and box 1 converged."""
    case, n = handover, len(handover.starts)
    what = f"{C.grid_id(case.shape)} from boxes"
    with solver(P, case) as sol:
        boxes = [C.damage_heavy(case.want[0], case.starts[0]), case.want[1]]
        tt = on_device(boxes)
        _long_enough(sol, lambda: sol.solve_device(case.starts, tt, init=False), what)
        assert sol.changed(n) == [1, 0]
        tt = on_device(boxes)
        _handed_over(P, sol, case, lambda: sol.solve_device(case.starts, tt, init=False), [1, 0], what)
        assert_boxes(tt, case.want, case.starts, what)
        host = [C.fresh_boxes(case.shape, case.starts[:1])[0], case.want[1].copy()]
        _handed_over(P, sol, case, lambda: sol.solve(case.starts, host), [1, 0], f"{what} (host)")
        assert_boxes(host, case.want, case.starts, f"{what} (host)")
        _after_the_handover(P, sol, case, what)


# ---------------------------------------------------------------------------
# E: the cap error in place
# ---------------------------------------------------------------------------

def test_sweep_cap_error_in_place_leaves_boxes_a_solve_resumes_from(P, any_address_tile):
    """TTSWEEP_OPT_MAX_SWEEPS = 2 with device boxes relaxed where they lie: "did not converge", and the caller's own
    arrays hold a half-relaxed state - every value the length of a real path, so a solve with init = 0 and a higher
    cap reaches the oracle's fixed point from it."""
    case, n = any_address_tile, len(any_address_tile.starts)
    assert C.in_place_eligible(case.shape)
    with solver(P, case) as sol:
        sol.set_option(P.OPT_MAX_SWEEPS, 2)
        tt = poisoned(n, case.shape)
        assert tt.data_ptr() % 64 == 0 and (4 * int(np.prod(case.shape))) % 64 == 0
        with pytest.raises(P.TTSweepError, match="did not converge"):
            sol.solve_device(case.starts, tt, init=True)
        half = tt.cpu().numpy()
        for s in range(n):      # a state between the fresh box and the fixed point: nothing below it, no poison left
            assert (half[s] >= case.want[s]).all() and half[s][tuple(case.starts[s])] == 0, s
            assert np.isfinite(half[s]).sum() > 1, s
        short = [int(not np.array_equal(half[s], case.want[s])) for s in range(n)]
        sol.set_option(P.OPT_MAX_SWEEPS, 100000)
        assert sol.solve_device(case.starts, tt, init=False) == 1
        assert_ran_on(sol.stats(), "columns", "after the cap error")
        assert sol.changed(n) == short
        assert_boxes(tt, case.want, case.starts, "resumed after the cap error")
        assert sol.solve_device(case.starts, tt, init=False) == 0
