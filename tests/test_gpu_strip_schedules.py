"""GPU tier (-m gpu): the STRIP kernel's schedule contract - every TTSWEEP_OPT_GATE_*, OPT_ASYNC*,
OPT_DEFER_MARGIN_MILLI, OPT_PAIR_MIN_STARTS and OPT_QUEUES decides WHEN a unit is relaxed and never changes a bit of
the result - on grids whose units have neighbours on every axis.

Main grid 65 x 66 x 67: two lane tiles (the second with 3 live lanes), five strips (the last with 2 live cells), 65
planes (the last two-plane unit owns one): 650 one-plane or 330 two-plane units per start.  Second grid 40 x 33 x 70:
another axis permutation, one lane tile of 40 lanes, five strips.  Star: random, reach 7 on every axis, asymmetric
(dead-edge cells exist).  Every comparison is bit equality over every cell of every box with the CPU oracle."""
import numpy as np
import pytest

import strip_cases as S
from conftest import assert_bit_equal
from strip_cases import SCHEDULES, damage_to_infinity, schedule_id

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

STRIP = 2


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


class Grid:
    def __init__(self, P, oracle, shape, starts):
        self.shape = shape
        self.layout = S.StripLayout(shape)
        self.v = S.velocity(shape)
        self.offs = S.star_offsets()
        self.fs = P.inputs.make_fs(self.offs)
        self.starts = starts
        self.want = S.oracle_boxes(oracle, self.v, self.offs, starts)
        for s, box in enumerate(self.want):
            assert np.isfinite(box).all() and box[tuple(starts[s])] == 0, f"oracle box {s}"


@pytest.fixture(scope="module")
def geometry(P):
    """The conditions every test of this module stands on: the layouts (host mirror of make_layout_strip) and the
    star (reach 7, forward-only and reverse-only pull entries in the library's own pull star)."""
    main, second = S.check_layouts()
    offs = S.star_offsets()
    S.check_star(offs)
    flags = [e[3] for e in P.build_pull_star(P.inputs.make_fs(offs))]
    assert flags.count(1) > 0 and flags.count(2) > 0, "no forward-only / reverse-only pull entries"
    S.check_schedule_groups()
    return main, second


@pytest.fixture(scope="module")
def main(P, oracle, geometry):
    return Grid(P, oracle, S.MAIN_SHAPE, S.main_starts())


@pytest.fixture(scope="module")
def second(P, oracle, geometry):
    return Grid(P, oracle, S.SECOND_SHAPE, S.second_starts())


def solve_and_check(P, grid, index, one_launch, options, what, want=None, fs=None, validate=True):
    """The assertions of the schedule matrix: fresh boxes of grid.starts[index], solved by the STRIP kernel under
    (one_launch, options) - the solve improves, runs the asked driver and never gives up; every box is `want` bit
    for bit; the device validator finds no open edge in one box; a fresh context with the same options solves the
    converged boxes again, reports no change and leaves every bit alone."""
    import torch
    dev = torch.device("cuda:0")
    starts = grid.starts[index]
    want = [grid.want[i] for i in np.arange(len(grid.starts))[index]] if want is None else want
    fs = grid.fs if fs is None else fs
    n = len(starts)
    tt = torch.empty((n,) + grid.shape, dtype=torch.float32, device=dev)
    with P.TravelTimeSolver(grid.shape, fs) as sol:
        S.set_options(P, sol, one_launch, options, kernel=STRIP)
        sol.set_velocity(grid.v)
        assert sol.solve_device(starts, tt, init=True) == 1, what
        st = sol.stats()
        assert st["kernel_variant"] == STRIP, what
        assert st["fallbacks"] == 0, what
        assert (st["launches"] == 1) == bool(one_launch), (what, st["launches"])
        assert sol.changed(n) == [1] * n, what
        host = tt.cpu().numpy()
        for s in range(n):
            assert_bit_equal(host[s], want[s], f"{what}: start {tuple(starts[s])}")
        if validate:
            k = len(options) % n
            assert sol.validate_device(starts[k], tt[k]) == (0, 0, 0), what
    again = tt.clone()
    with P.TravelTimeSolver(grid.shape, fs) as sol:           # (a fresh context: nothing is remembered)
        S.set_options(P, sol, one_launch, options, kernel=STRIP)
        sol.set_velocity(grid.v)
        assert sol.solve_device(starts, again, init=False) == 0, what
        assert sol.stats()["fallbacks"] == 0, what
        assert sol.changed(n) == [0] * n, what
    assert torch.equal(again.view(torch.int32), tt.view(torch.int32)), f"{what}: the second solve stored something"


def test_grids_and_star_are_what_the_tests_need(geometry, main, second):
    """At least 2 lane tiles and 2 strips with ragged remainders and an odd plane count on the main grid (650 / 330
    units per start), strips but one lane tile on the second; 11 starts of which one lies in the 3-lane tile, one
    in the 2-cell strip, one on the last plane and one is a duplicate."""
    m, s = geometry
    st = main.starts
    assert len(st) == 11 and len(second.starts) == 4
    assert st[3][m.bax] >= (m.btiles - 1) * m.TB and st[4][m.cax] >= (m.cstrips - 1) * m.K
    assert st[5][m.aax] == m.planes - 1 and (st[6] == st[3]).all()
    assert tuple(st[0]) == (32, 33, 33) and tuple(st[1]) == (0, 0, 0) and tuple(st[2]) == (64, 65, 66)
    assert len(S.SCHEDULES) == sum(len(r) for r in S.SCHEDULE_GROUPS.values())


SCHEDULE_IDS = [schedule_id(a, o) for a, o in SCHEDULES]


@pytest.mark.parametrize("nstart", [3, 11])
@pytest.mark.parametrize("one_launch,options", SCHEDULES, ids=SCHEDULE_IDS)
def test_schedule_matrix_on_the_main_grid(P, main, one_launch, options, nstart):
    """Every entry of SCHEDULES with 3 starts (fewer than queues) and 11 (more, dealt unevenly)."""
    solve_and_check(P, main, slice(0, nstart), one_launch, options, f"{nstart} starts {one_launch} {options}")


@pytest.mark.parametrize("one_launch,options", SCHEDULES[::5], ids=SCHEDULE_IDS[::5])
def test_schedule_matrix_on_the_second_grid(P, second, one_launch, options):
    """Every fifth entry on the other axis permutation (one lane tile, five strips), 4 starts."""
    solve_and_check(P, second, slice(0, 4), one_launch, options, f"second grid {one_launch} {options}")


@pytest.mark.parametrize("one_launch", [1, 0], ids=["one-launch", "passes"])
@pytest.mark.parametrize("speed,r0", [(0, 0), (500, 1000), (2000, 3000), (9000, 30000), (250, 0), (100000, 100000)])
def test_gate_on_the_main_grid(P, main, speed, r0, one_launch):
    """The distance gate on shells of units instead of a line: off, crawling from radius 0, far ahead, under both
    drivers, 8 starts (as many as queues)."""
    solve_and_check(P, main, slice(0, 8), one_launch, {"OPT_GATE_SPEED_MILLI": speed, "OPT_GATE_R0_MILLI": r0},
                    f"gate {speed}/{r0} driver {one_launch}")


@pytest.mark.parametrize("one_launch", [1, 0], ids=["one-launch", "passes"])
@pytest.mark.parametrize("pair", [0, 1 << 20], ids=["two-plane", "one-plane"])
@pytest.mark.parametrize("nstart", [3, 8, 11])
@pytest.mark.parametrize("queues", [1, 3, 8])
def test_queues_starts_and_unit_size(P, main, queues, nstart, pair, one_launch):
    """Fewer starts than queues, as many, more (dealt unevenly; with one queue all 11 share one ring, within its
    limit of 32), units of one and of two planes, both drivers."""
    solve_and_check(P, main, slice(0, nstart), one_launch, {"OPT_QUEUES": queues, "OPT_PAIR_MIN_STARTS": pair},
                    f"{queues} queues {nstart} starts pair {pair} driver {one_launch}")


# ---------------------------------------------------------------------------
# resume from a damaged box
# ---------------------------------------------------------------------------

DRIVERS = [pytest.param(1, 1 << 20, id="one-launch-one-plane"), pytest.param(1, 0, id="one-launch-two-plane"),
           pytest.param(0, 1 << 20, id="passes-one-plane"), pytest.param(0, 0, id="passes-two-plane")]


def far_cell(shape, start):
    return tuple(0 if 2 * s >= n else n - 1 for s, n in zip(start, shape))


@pytest.fixture(scope="module")
def seeded(main, oracle):
    """Converged boxes of the first 3 starts with one cell, far from the start, lowered to half its value (a seed),
    and what the oracle makes of the same boxes."""
    boxes = []
    for s in range(3):
        b = main.want[s].copy()
        far = far_cell(main.shape, main.starts[s])
        assert b[far] > 0
        b[far] = np.float32(0.5) * b[far]
        boxes.append(b)
    want = S.oracle_boxes(oracle, main.v, main.offs, main.starts[:3], tts=boxes)
    for s in range(3):
        assert (want[s] <= boxes[s]).all() and (want[s] < main.want[s]).sum() > 1, "the seed improves its neighbours"
    return boxes, want


def resume(P, grid, one_launch, pair, boxes):
    import torch
    tt = torch.from_numpy(np.stack(boxes)).to("cuda:0")
    with P.TravelTimeSolver(grid.shape, grid.fs) as sol:
        S.set_options(P, sol, one_launch, {"OPT_PAIR_MIN_STARTS": pair}, kernel=STRIP)
        sol.set_velocity(grid.v)
        rc = sol.solve_device(grid.starts[:len(boxes)], tt, init=False)
        st = sol.stats()
        assert st["kernel_variant"] == STRIP and st["fallbacks"] == 0
        return rc, sol.changed(len(boxes)), tt.cpu().numpy()


@pytest.mark.parametrize("one_launch,pair", DRIVERS)
def test_resume_from_boxes_damaged_to_infinity(P, main, one_launch, pair):
    boxes = [damage_to_infinity(main, main.want[s].copy(), main.starts[s]) for s in range(3)]
    for s in range(3):
        assert np.isinf(boxes[s]).sum() > 65 * 66 * 3
    rc, changed, got = resume(P, main, one_launch, pair, boxes)
    assert rc == 1 and changed == [1, 1, 1]
    for s in range(3):
        assert_bit_equal(got[s], main.want[s], f"start {tuple(main.starts[s])} after damage")


@pytest.mark.parametrize("one_launch,pair", DRIVERS)
def test_resume_from_boxes_with_a_seed(P, main, seeded, one_launch, pair):
    boxes, want = seeded
    rc, changed, got = resume(P, main, one_launch, pair, [b.copy() for b in boxes])
    assert rc == 1 and changed == [1, 1, 1]
    for s in range(3):
        assert_bit_equal(got[s], want[s], f"start {tuple(main.starts[s])} with a seed at {far_cell(main.shape, main.starts[s])}")


@pytest.mark.parametrize("one_launch,pair", DRIVERS)
def test_resume_leaves_a_converged_box_among_damaged_ones_alone(P, main, one_launch, pair):
    boxes = [damage_to_infinity(main, main.want[0].copy(), main.starts[0]), main.want[1].copy(),
             damage_to_infinity(main, main.want[2].copy(), main.starts[2])]
    rc, changed, got = resume(P, main, one_launch, pair, boxes)
    assert rc == 1 and changed == [1, 0, 1]
    for s in range(3):
        assert_bit_equal(got[s], main.want[s], f"start {tuple(main.starts[s])}")


# ---------------------------------------------------------------------------
# one context, solves in a row
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def faster(main, oracle):
    """The oracle's boxes of the first 8 starts in the velocities v * 1.7."""
    v = (main.v * np.float32(1.7)).astype(np.float32)
    return v, S.oracle_boxes(oracle, v, main.offs, main.starts[:8])


@pytest.mark.parametrize("options", [{}, {"OPT_ASYNC_HANDOFF": 3, "OPT_ASYNC_WAVES": 8}], ids=["defaults", "handoff3-waves8"])
def test_solves_in_a_row_in_one_context(P, main, faster, options):
    """11 starts, 3 other starts, another velocity volume with 8 starts, the first volume again with 1 start (the
    latency instance by the default rule): nothing of a solve (rings, flags, deferred bits, padding cells) reaches
    the next one."""
    import torch
    v2, want2 = faster
    steps = [(main.v, slice(0, 11), main.want), (None, slice(3, 6), main.want[3:6]), (v2, slice(0, 8), want2),
             (main.v, slice(0, 1), main.want[:1])]
    with P.TravelTimeSolver(main.shape, main.fs) as sol:
        S.set_options(P, sol, None, options)
        for step, (v, index, want) in enumerate(steps):
            if v is not None:
                sol.set_velocity(v)
            starts = main.starts[index]
            tt = torch.empty((len(starts),) + main.shape, dtype=torch.float32, device="cuda:0")
            assert sol.solve_device(starts, tt, init=True) == 1, step
            st = sol.stats()
            assert st["kernel_variant"] == STRIP and st["launches"] == 1 and st["fallbacks"] == 0, (step, st)
            got = tt.cpu().numpy()
            for s in range(len(starts)):
                assert_bit_equal(got[s], want[s], f"solve {step} of the row, start {tuple(starts[s])}")


# ---------------------------------------------------------------------------
# the workload's star
# ---------------------------------------------------------------------------

SPREAD = [0, 5, 19, 22, 24, 25, 26, 27, 28, 33]


@pytest.fixture(scope="module")
def cell_boxes_818(P, main, oracle):
    """818-FS on the main grid, 3 starts, by the CELL kernel (an independent implementation); its box of the centre
    start is the oracle's."""
    import torch
    offs = P.inputs.read_triples(P.inputs.star_path("818"))
    fs = P.inputs.make_fs(offs)
    tt = torch.empty((3,) + main.shape, dtype=torch.float32, device="cuda:0")
    with P.TravelTimeSolver(main.shape, fs) as sol:
        sol.set_option(P.OPT_KERNEL, 1)
        sol.set_velocity(main.v)
        assert sol.solve_device(main.starts[:3], tt, init=True) == 1
        assert sol.stats()["kernel_variant"] == 1
    boxes = list(tt.cpu().numpy())
    want, _, _ = oracle.converge(main.v, oracle.make_star(offs), main.starts[0], order=1)
    assert_bit_equal(boxes[0], want, "CELL kernel, 818-FS, centre start")
    return fs, boxes


def test_the_spread_covers_every_group_and_the_eight_wave_entries():
    picked = set(SPREAD)
    assert len(picked) == 10
    for name, rng in S.SCHEDULE_GROUPS.items():
        assert picked & set(rng), name
    assert {i for i, (_, o) in enumerate(SCHEDULES) if o.get("OPT_ASYNC_WAVES") == 8} <= picked


@pytest.mark.parametrize("entry", SPREAD, ids=[SCHEDULE_IDS[i] for i in SPREAD])
def test_workload_star_on_the_main_grid(P, main, cell_boxes_818, entry):
    """818-FS (the flagship star: symmetric, reach 7) on the main grid under ten schedules, against the CELL kernel."""
    fs, want = cell_boxes_818
    one_launch, options = SCHEDULES[entry]
    solve_and_check(P, main, slice(0, 3), one_launch, options, f"818-FS {one_launch} {options}", want=want, fs=fs)
