"""GPU tier (-m gpu): where the lanes of the STRIP kernel run along z, the one-launch solve stores every improved cell
into the caller's box as well as into its padded volume, and the copy back after the solve is left out.  Whatever
reaches the caller's boxes that way - or, where the copy still runs (other layouts, a fallback), through it - is the
CPU oracle's fixed point, bit for bit, in every cell of every box.

Grids: 65 x 66 x 51 with the 818-offset star (the headline's axis roles: the lanes run along z, the caller's stride-1
axis; one lane tile of 51 lanes, five strips with a ragged last one, 65 planes); 65 x 66 x 67 (no axis fits a wave:
the lanes run along z in two lane tiles, the second with 3 live lanes) and 40 x 70 x 90 (the lanes run along x: this
layout keeps the copy back) with the 5-FS star."""
import numpy as np
import pytest

import strip_cases as S
from conftest import assert_bit_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

STRIP = 2
INF = np.float32(np.inf)
SEED = 733

HEAD_SHAPE = (65, 66, 51)
X_SHAPE = (40, 70, 90)
TILED_SHAPE = (65, 66, 67)


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


def head_starts():
    """The centre, both extreme corners, one on the last plane, four seeded ones.  Batches: [:1], [:3], all 8."""
    L = S.StripLayout(HEAD_SHAPE)
    rng = np.random.default_rng(SEED)
    fixed = [(32, 33, 25), (0, 0, 0), (64, 65, 50), L.block(L.planes - 1, 7, 30)]
    rnd = np.stack([rng.integers(0, n, size=4) for n in HEAD_SHAPE], axis=1)
    return np.array(fixed + [tuple(r) for r in rnd], dtype=np.int32)


class Grid:
    def __init__(self, P, oracle, shape, star, starts):
        self.shape = shape
        self.layout = S.StripLayout(shape)
        self.v = S.velocity(shape)
        self.offs = P.inputs.read_triples(P.inputs.star_path(star))
        self.fs = P.inputs.make_fs(self.offs)
        self.starts = np.asarray(starts, dtype=np.int32)
        self.want = S.oracle_boxes(oracle, self.v, self.offs, self.starts)
        for s, box in enumerate(self.want):
            assert np.isfinite(box).all() and box[tuple(self.starts[s])] == 0, f"oracle box {s}"


@pytest.fixture(scope="module")
def head(P, oracle):
    L = S.StripLayout(HEAD_SHAPE)
    assert (L.aax, L.bax, L.cax) == (0, 2, 1), "the lanes run along z, the strips along y, the planes along x"
    assert (L.btiles, L.last_tile_lanes, L.cstrips, L.last_strip_cells, L.planes) == (1, 51, 5, 2, 65)
    g = Grid(P, oracle, HEAD_SHAPE, "818", head_starts())
    assert g.starts[3][L.aax] == L.planes - 1
    return g


@pytest.fixture(scope="module")
def lanes_along_x(P, oracle):
    L = S.StripLayout(X_SHAPE)
    assert (L.aax, L.bax, L.cax) == (1, 0, 2) and L.btiles == 1 and L.last_tile_lanes == 40
    return Grid(P, oracle, X_SHAPE, "5", [(20, 35, 45), (39, 69, 89)])


@pytest.fixture(scope="module")
def lanes_tiled(P, oracle):
    L = S.StripLayout(TILED_SHAPE)
    assert L.bax == 2 and L.btiles == 2 and L.last_tile_lanes == 3, "lanes along z, two lane tiles, the second with 3 live lanes"
    return Grid(P, oracle, TILED_SHAPE, "5", [(32, 33, 65), (0, 0, 0)])


def one_launch(P, grid, options=None):
    sol = P.TravelTimeSolver(grid.shape, grid.fs)
    S.set_options(P, sol, 1, options or {}, kernel=STRIP)
    sol.set_velocity(grid.v)
    return sol


def poisoned(n, shape):
    """Device boxes full of a value no solve produces: a cell the solve leaves out shows."""
    import torch
    return torch.full((n,) + tuple(shape), -7.0, dtype=torch.float32, device="cuda:0")


def check_fresh(P, grid, index, options=None, fallbacks=False):
    starts = grid.starts[index]
    n = len(starts)
    tt = poisoned(n, grid.shape)
    with one_launch(P, grid, options) as sol:
        assert sol.solve_device(starts, tt, init=True) == 1
        st = sol.stats()
        assert st["kernel_variant"] == STRIP
        if fallbacks:
            assert st["fallbacks"] > 0 and st["launches"] > 1, st
        else:
            assert st["fallbacks"] == 0 and st["launches"] == 1, st
        assert sol.changed(n) == [1] * n
    got = tt.cpu().numpy()
    for s in range(n):
        assert_bit_equal(got[s], grid.want[np.arange(len(grid.starts))[index][s]], f"start {tuple(starts[s])}")
    return got


@pytest.mark.parametrize("nstart", [1, 3, 8])
def test_lanes_along_the_callers_stride_1_axis(P, head, nstart):
    """1 and 3 starts: units of one plane (1: the eight-wave instance by the default rule); 8 starts with units of
    two planes forced as on the headline workload, and with the default rule."""
    check_fresh(P, head, slice(0, nstart))
    if nstart == 8:
        check_fresh(P, head, slice(0, nstart), {"OPT_PAIR_MIN_STARTS": 0})
    if nstart == 3:
        check_fresh(P, head, slice(0, nstart), {"OPT_PAIR_MIN_STARTS": 0, "OPT_ASYNC_WAVES": 4})


@pytest.mark.parametrize("pair", [0, 1 << 20], ids=["two-plane", "one-plane"])
def test_lanes_along_x(P, lanes_along_x, pair):
    """The lanes of a store would lie a whole (y, z) plane of the caller's box apart: the layout keeps the copy back
    (csrc/strip_rules.h), and the caller's boxes are exact all the same."""
    check_fresh(P, lanes_along_x, slice(0, 2), {"OPT_PAIR_MIN_STARTS": pair})


@pytest.mark.parametrize("pair", [0, 1 << 20], ids=["two-plane", "one-plane"])
def test_lanes_tiled(P, lanes_tiled, pair):
    """Two lane tiles: the second one's lanes from 3 on own no cell of the caller's box."""
    check_fresh(P, lanes_tiled, slice(0, 2), {"OPT_PAIR_MIN_STARTS": pair})


def damaged(box, start, seed):
    """A seeded 5 % of the cells raised to INFINITY, none lowered; the start keeps its 0."""
    out = box.copy()
    hit = np.random.default_rng(seed).random(box.shape) < 0.05
    out[hit] = INF
    out[tuple(start)] = 0
    assert (out >= box).all() and np.isinf(out).sum() > 0.04 * box.size
    return out


def test_boxes_with_values_and_two_solves_in_a_row(P, head):
    """init=False from damaged boxes (the fixed point above a state that lies nowhere below it is the same one), then
    - same context - other starts, damaged elsewhere: the second solve neither inherits the first one's boxes nor its
    'in step' verdict."""
    import torch
    with one_launch(P, head) as sol:
        for step, index in enumerate([slice(0, 3), slice(3, 8)]):
            starts = head.starts[index]
            want = head.want[index]
            boxes = [damaged(want[s], starts[s], SEED + 10 * step + s) for s in range(len(starts))]
            tt = torch.from_numpy(np.stack(boxes)).to("cuda:0")
            assert sol.solve_device(starts, tt, init=False) == 1, step
            st = sol.stats()
            assert st["kernel_variant"] == STRIP and st["launches"] == 1 and st["fallbacks"] == 0, (step, st)
            got = tt.cpu().numpy()
            for s in range(len(starts)):
                assert_bit_equal(got[s], want[s], f"solve {step}, start {tuple(starts[s])}")
        # ... and a solve of fresh boxes behind them
        tt = poisoned(2, head.shape)
        assert sol.solve_device(head.starts[:2], tt, init=True) == 1
        got = tt.cpu().numpy()
        for s in range(2):
            assert_bit_equal(got[s], head.want[s], f"fresh boxes after the row, start {tuple(head.starts[s])}")


def test_converged_boxes_come_back_untouched(P, head):
    """Nothing improves, so nothing is stored: whatever the caller's boxes hold afterwards is what they held."""
    import torch
    tt = torch.from_numpy(np.stack(head.want[:3])).to("cuda:0")
    with one_launch(P, head) as sol:
        assert sol.solve_device(head.starts[:3], tt, init=False) == 0
        st = sol.stats()
        assert st["launches"] == 1 and st["fallbacks"] == 0, st
        assert sol.changed(3) == [0, 0, 0]
    got = tt.cpu().numpy()
    for s in range(3):
        assert_bit_equal(got[s], head.want[s], f"start {tuple(head.starts[s])}")


def test_fallback_copies_the_volumes_back(P, head):
    """A wall-clock limit of 1 ms: the one launch gives up with the boxes on their way, the pass driver - which stores
    into the padded volumes only - finishes them, and the copy back runs."""
    check_fresh(P, head, slice(0, 8), {"OPT_ASYNC_TIMEOUT_MILLI": 1, "OPT_PAIR_MIN_STARTS": 0}, fallbacks=True)


def dead_edge_cells(P, grid, start):
    """The cells of `start` with an edge the reference never relaxes (csrc/ttsweep_plan.cpp, fill_special_box): the
    start itself when the pull star has a forward-only entry, start - e for every reverse-only entry e."""
    cells = []
    for di, dj, dk, flags, _h in P.build_pull_star(grid.fs):
        c = tuple(int(x) for x in start) if flags == 1 else (start[0] - di, start[1] - dj, start[2] - dk) if flags == 2 else None
        if c is not None and all(0 <= c[d] < grid.shape[d] for d in range(3)):
            cells.append(tuple(int(x) for x in c))
    return cells


@pytest.fixture(scope="module")
def asymmetric(P, oracle):
    """The headline's axis roles with the random asymmetric star of the schedule tests (57 forward-only and 57
    reverse-only pull entries): a dead-edge box of thousands of cells around every start."""
    g = Grid.__new__(Grid)
    g.shape, g.layout, g.v = HEAD_SHAPE, S.StripLayout(HEAD_SHAPE), S.velocity(HEAD_SHAPE)
    g.offs = S.star_offsets()
    S.check_star(g.offs)
    g.fs = P.inputs.make_fs(g.offs)
    g.starts = head_starts()[:4]
    g.want = S.oracle_boxes(oracle, g.v, g.offs, g.starts)
    return g


@pytest.mark.parametrize("special", [1, 32], ids=["special-1", "special-32"])
@pytest.mark.parametrize("nstart", [1, 4])
def test_large_dead_edge_boxes(P, asymmetric, nstart, special):
    """Entries for one start's dead-edge cells overlap in time when the box is large and they come often (after every
    unit / every 32 units): the caller's box must not keep a value that the padded volume has since improved."""
    cells = dead_edge_cells(P, asymmetric, asymmetric.starts[0])
    lo, hi = np.min(cells, axis=0), np.max(cells, axis=0)
    assert np.prod(hi - lo + 1) > 1000, (lo, hi)
    for rep in range(3):
        check_fresh(P, asymmetric, slice(0, nstart), {"OPT_ASYNC_SPECIAL": special})


def test_dead_edge_cells(P, head):
    """The centre start owns two dead-edge cells (itself and the far end of the star's last offset): the wave that
    relaxes them stores into the caller's box too."""
    cells = dead_edge_cells(P, head, head.starts[0])
    assert len(set(cells)) >= 2, cells
    got = check_fresh(P, head, slice(0, 1), {"OPT_ASYNC_SPECIAL": 1, "OPT_ASYNC_WAVES": 4})
    for c in cells:
        assert got[0][c].view(np.uint32) == head.want[0][c].view(np.uint32), c
    far = [c for c in cells if c != tuple(head.starts[0])]
    assert all(np.isfinite(head.want[0][c]) and head.want[0][c] > 0 for c in far)
