"""GPU tier (-m gpu): the STRIP kernel (kernel 2, sweep_units_kernel) on stars of every plane reach ra in 0..7 and
every lane reach rb in 1..7, on a grid whose units have neighbours on every axis - every cell of every box against
the CPU oracle, bit for bit, INFINITY cells included.

From ra, rb and the fixed strip halo the kernel and its planners derive the staged planes (2 ra + np), the slab rows
(tb + 2 rb), the units an improved plane is told to (push_improved: Alo, Ahi, the plane bit; the rounding for
two-plane units depends on the parity of ra), the zone bits of a lane (lane < rb, lane >= 64 - rb) and the per-plane
item lists split over 4 or 8 waves.  The other STRIP tests run stars with ra = rb (1, 4 or 7), mostly where units have
no neighbour on some axis.  The stars of strip_star_cases.py have ra = 0, ra != rb in both orders, staged planes
without items (holes in plane_mask, the own plane among them), planes with one item for four or eight waves and planes
with items for all eight; the grid is strip_cases.MAIN_SHAPE (two lane tiles, the second with 3 live lanes; five
strips, the last with 2 live cells; 65 planes) and, for every third case, the same extents with the user's axes
assigned otherwise.  Starts: the centre, the first lane of the ragged lane tile, and the (0, 0, 0) corner where its
box is worth it - all of a case's starts in one solve.  test_strip_star_cases_cpu.py pins all of this without a GPU.

What the cases see that a reach-7-everywhere star does not (scratch builds with one changed value each, pass drivers):
a low lane zone one lane narrow (lane < rb - 1) fails flat_b and ra7_rb1 - with rb = 1 the zone is lane 0 alone, with a
wider zone another lane of it nearly always improves in the same turn - and ra in place of rb in the high lane zone
fails every case with ra < rb; the damaged-box resume of the schedule tests (reach 7 on every axis) and the seeded
random grids of test_gpu_parity.py pass both."""
import numpy as np
import pytest

import strip_cases as S
import strip_star_cases as C
from conftest import assert_bit_equal
from strip_cases import damage_to_infinity

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

CELL, STRIP = 1, 2
ONE_PLANE, TWO_PLANE = 1 << 20, 0           # OPT_PAIR_MIN_STARTS: never pair planes / always

# (id, one launch per solve?, options)
DRIVERS = [
    ("one-launch-one-plane", 1, {"OPT_PAIR_MIN_STARTS": ONE_PLANE}),
    ("one-launch-two-plane", 1, {"OPT_PAIR_MIN_STARTS": TWO_PLANE}),
    ("passes-one-plane", 0, {"OPT_PAIR_MIN_STARTS": ONE_PLANE}),
    ("passes-two-plane", 0, {"OPT_PAIR_MIN_STARTS": TWO_PLANE}),
    ("one-launch-waves8", 1, {"OPT_ASYNC_WAVES": 8, "OPT_PAIR_MIN_STARTS": ONE_PLANE}),    # the latency instance
    ("one-launch-handoff3", 1, {"OPT_ASYNC_HANDOFF": 3}),
]
RESUME_DRIVERS = [DRIVERS[0], DRIVERS[3]]


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


class Solved:
    """A case on a grid: the volume, the star, the starts and the oracle's boxes (computed once, never written to)."""

    def __init__(self, P, oracle, name, grid):
        self.case, self.shape = C.CASES[name], C.GRIDS[grid]
        self.what = f"{name} on {grid}"
        self.layout = S.StripLayout(self.shape)
        self.v = S.velocity(self.shape)
        self.fs = self.case.fs(P.inputs.make_fs, self.shape)
        self.starts = C.starts_of(self.case, self.shape)
        self.want = C.oracle_boxes(oracle, self.case, self.shape, self.starts)
        for st, box in zip(self.starts, self.want):
            box.setflags(write=False)
            assert box[tuple(st)] == 0 and np.isfinite(box).sum() > 1, self.what
            assert self.case.exempt or C.meets_start_condition(self.case, box, self.shape), self.what
        dp = C.device_pull(P.build_pull_star(self.fs), self.shape)
        assert C.reach(dp)[:2] == (self.case.ra, self.case.rb), self.what
        self.improved = [C.improves(f, w) for f, w in zip(S.fresh_boxes(self.shape, self.starts), self.want)]
        assert self.improved == [1] * len(self.starts), self.what
        self.damaged = None

    def damaged_boxes(self, oracle):
        """The converged boxes damaged to INFINITY across a lane-tile boundary, across a strip boundary and in the
        last plane (the flat cases: in the start's plane as well), and what the oracle makes of them."""
        if self.damaged is None:
            boxes = []
            for st, w in zip(self.starts, self.want):
                b = damage_to_infinity(self, w.copy(), st)
                if self.case.ra == 0:
                    b = C.damage_in_the_start_plane(self.layout, b, st)
                boxes.append(b)
            want = C.oracle_boxes(oracle, self.case, self.shape, self.starts, tts=boxes)
            self.damaged = boxes, want
        return self.damaged


@pytest.fixture(scope="module")
def solved(P, oracle):
    C.check_grids()
    cache = {}

    def get(name, grid):
        if (name, grid) not in cache:
            cache[name, grid] = Solved(P, oracle, name, grid)
        return cache[name, grid]

    return get


def strip_solver(P, g, one_launch, options, kernel=STRIP):
    sol = P.TravelTimeSolver(g.shape, g.fs)
    S.set_options(P, sol, one_launch, options, kernel=kernel)
    sol.set_velocity(g.v)
    return sol


@pytest.mark.parametrize("driver,one_launch,options", DRIVERS, ids=[d[0] for d in DRIVERS])
@pytest.mark.parametrize("name,grid", C.matrix(), ids=[f"{n}-{g}" for n, g in C.matrix()])
def test_star_vs_oracle(P, solved, name, grid, driver, one_launch, options):
    """Fresh boxes of all starts of the case in one solve: the asked driver ran on the STRIP kernel and never gave up;
    every box is the oracle's bit for bit; the device validator finds no open edge in one box and the oracle's count
    of INFINITY cells; a fresh context solves the converged boxes again, reports no change and moves no bit."""
    import torch
    g = solved(name, grid)
    what = f"{g.what}, {driver}"
    n = len(g.starts)
    tt = torch.empty((n,) + g.shape, dtype=torch.float32, device="cuda:0")
    with strip_solver(P, g, one_launch, options) as sol:
        assert sol.solve_device(g.starts, tt, init=True) == 1, what
        st = sol.stats()
        assert st["kernel_variant"] == STRIP, what
        assert st["fallbacks"] == 0, what
        assert (st["launches"] == 1) == bool(one_launch), (what, st["launches"])
        assert sol.changed(n) == g.improved, what
        host = tt.cpu().numpy()
        for s in range(n):
            assert_bit_equal(host[s], g.want[s], f"{what}: start {tuple(g.starts[s])}")
        k = len(driver) % n
        assert sol.validate_device(g.starts[k], tt[k]) == (0, int(np.isinf(g.want[k]).sum()), 0), what
    again = tt.clone()
    with strip_solver(P, g, one_launch, options) as sol:     # (a fresh context: nothing is remembered)
        assert sol.solve_device(g.starts, again, init=False) == 0, what
        st = sol.stats()
        assert st["kernel_variant"] == STRIP and st["fallbacks"] == 0, (what, st)
        assert sol.changed(n) == [0] * n, what
    assert torch.equal(again.view(torch.int32), tt.view(torch.int32)), f"{what}: the second solve stored something"


@pytest.mark.parametrize("driver,one_launch,options", RESUME_DRIVERS, ids=[d[0] for d in RESUME_DRIVERS])
@pytest.mark.parametrize("name", list(C.CASES))
def test_resume_from_damaged_boxes(P, oracle, solved, name, driver, one_launch, options):
    """init = 0 from the damaged boxes: the oracle's result from the same boxes (a one-directional star need not
    restore every cell: INFINITY is a result), and 1 exactly for the starts whose box had something to restore."""
    import torch
    g = solved(name, "main")
    what = f"{g.what}, {driver}, damaged"
    boxes, want = g.damaged_boxes(oracle)
    n = len(boxes)
    for s in range(n):
        assert np.isinf(boxes[s]).sum() > np.isinf(g.want[s]).sum() or g.case.exempt, what
        assert (want[s] <= boxes[s]).all() and (want[s] >= g.want[s]).all(), what
    hurt = [C.improves(b, w) for b, w in zip(boxes, want)]
    assert max(hurt) == 1 or g.case.exempt, what
    tt = torch.from_numpy(np.stack(boxes)).to("cuda:0")
    with strip_solver(P, g, one_launch, options) as sol:
        assert sol.solve_device(g.starts, tt, init=False) == max(hurt), what
        st = sol.stats()
        assert st["kernel_variant"] == STRIP and st["fallbacks"] == 0, (what, st)
        assert sol.changed(n) == hurt, what
    got = tt.cpu().numpy()
    for s in range(n):
        assert_bit_equal(got[s], want[s], f"{what}: start {tuple(g.starts[s])}")


@pytest.mark.parametrize("name", C.CELL_CASES)
def test_cell_kernel_agrees(P, solved, name):
    """The per-cell kernel, an independent implementation (no units, no staged planes, no items): the same boxes."""
    import torch
    g = solved(name, "main")
    n = len(g.starts)
    tt = torch.empty((n,) + g.shape, dtype=torch.float32, device="cuda:0")
    with strip_solver(P, g, None, {}, kernel=CELL) as sol:
        assert sol.solve_device(g.starts, tt, init=True) == 1, g.what
        st = sol.stats()
        assert st["kernel_variant"] == CELL and st["fallbacks"] == 0, (g.what, st)
    host = tt.cpu().numpy()
    for s in range(n):
        assert_bit_equal(host[s], g.want[s], f"{g.what} (CELL): start {tuple(g.starts[s])}")
