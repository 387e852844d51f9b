"""GPU tier (-m gpu) of windowed, strided event location (include/ttsweep.h, "locate window"):
ttsweep_locate_window_device through TravelTimeSolver.locate_window and the two-stage locate_refine, bit for bit
(through u64, no tolerances) against TravelTimeSolver.locate and the numpy restatement
tests/locate_window_reference.py."""
import numpy as np
import pytest

from conftest import Golden
import locate_cases as Cs
import locate_window_reference as W

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
TILE = 4096                 # LOC_WC * LOC_BLOCK: candidates of one block of locate_window_search_kernel


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


def dev():
    import torch
    return torch.device("cuda:0")


def u64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def star818(P):
    return P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))


def synthetic_events(rng, tt, E, drop=0.15, noise=0.01):
    """Picks T_k[cell] + t0 + noise at random cells that every box reaches, a share of them dropped (weight 0)."""
    K = tt.shape[0]
    flat = tt.reshape(K, -1)
    ok = np.flatnonzero(np.all(np.isfinite(flat), axis=0))
    cells = ok[rng.integers(0, len(ok), E)] if len(ok) else rng.integers(0, flat.shape[1], E)
    t0 = rng.uniform(-5, 5, E)
    T = flat[:, cells].T.astype(np.float64)
    picks = np.where(np.isfinite(T), T, 0.0) + t0[:, None] + noise * rng.standard_normal((E, K))
    w = rng.uniform(0.5, 2.0, (E, K))
    w[rng.random((E, K)) < drop] = 0.0
    w[np.arange(E), rng.integers(0, K, E)] = 1.0      # at least one pick per event
    return picks, w, cells


def outputs(res):
    return res.cell.cpu().numpy(), res.misfit.cpu().numpy(), res.t0.cpu().numpy()


def same(got, want, what=""):
    """(cell, misfit, t0) equal on the bits; the NaN of t0 is the quiet NaN 0x7ff8000000000000 on both sides"""
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(u64(got[1]), u64(want[1])), what
    assert np.array_equal(u64(got[2]), u64(want[2])), what


def check_window(sol, tt, picks, w=None, lo=None, hi=None, stride=1, what=""):
    """locate_window on the device == the restatement; returns the device outputs as numpy"""
    import torch
    tt = np.ascontiguousarray(tt, dtype=F32)
    res = sol.locate_window(torch.from_numpy(tt).to(dev()), picks, w, lo, hi, stride)
    assert res.cell.dtype == torch.int32 and res.cell.device == dev() and res.volumes is None
    got = outputs(res)
    same(got, W.locate_window(tt, picks, w, lo, hi, stride), what)
    shape = tt.shape[1:]
    xyz = res.xyz.numpy()
    assert np.array_equal(xyz[got[0] >= 0], np.argwhere(np.ones(shape, bool))[got[0][got[0] >= 0]]), what
    assert np.all(xyz[got[0] < 0] == -1)
    return got


def golden_stations():
    out = []
    for name in ("g24", "g9"):
        g = Golden(name)
        out.append((name, np.stack([tt for _, _, _, _, tt, _ in g.cases()])))
    return out


# ---- the whole grid with stride 1 is locate ----
@pytest.mark.parametrize("case", golden_stations(), ids=lambda c: c[0])
def test_whole_grid_equals_locate_on_golden_boxes(P, case):
    import torch
    name, tt = case
    rng = np.random.default_rng(len(name) + tt.shape[0])
    picks, w, _ = synthetic_events(rng, tt, 40)
    n = np.array(tt.shape[1:])
    with P.TravelTimeSolver(tt.shape[1:], star818(P)) as sol:
        tdev = torch.from_numpy(np.ascontiguousarray(tt, dtype=F32)).to(dev())
        want = outputs(sol.locate(tdev, picks, w))
        same(outputs(sol.locate_window(tdev, picks, w)), want, name)
        same(outputs(sol.locate_window(tdev, picks, w, lo=[0, 0, 0], hi=n - 1, stride=[1, 1, 1])), want, name)
        same(outputs(sol.locate_window(tdev, picks[:5], None)), outputs(sol.locate(tdev, picks[:5], None)), name)


@pytest.mark.parametrize("K", [8, 9, 24, 33])
def test_whole_grid_equals_locate_at_the_register_widths(P, K):
    """a full register instance, one over, the 24 of the bench and the from-memory instance, on 4097 cells"""
    import torch
    c = Cs.k_edge_case(K, 4097)
    with P.TravelTimeSolver(c["shape"], star818(P)) as sol:
        tdev = torch.from_numpy(c["tt"]).to(dev())
        for picks, w in ((c["picks"], c["weights"]), (c["none"]["picks"], None)):
            got = outputs(sol.locate_window(tdev, picks, w))
            same(got, outputs(sol.locate(tdev, picks, w)), f"K={K}")
            same(got, W.locate_window(c["tt"], picks, w), f"K={K} restatement")


# ---- windows ----
def range_box(seed, K=4, shape=Cs.RANGE_SHAPE, inf_share=0.05):
    rng = np.random.default_rng(seed)
    tt = rng.uniform(0, 9, (K,) + tuple(shape)).astype(F32)
    tt[rng.random(tt.shape) < inf_share] = INF
    return rng, tt


def seeded_windows(rng, shape, E):
    lo = np.stack([rng.integers(0, n, E) for n in shape], 1)
    hi = np.stack([rng.integers(lo[:, a], shape[a]) for a in range(3)], 1)
    return lo, hi


@pytest.mark.parametrize("stride", [(1, 1, 1), (2, 3, 4), (9, 9, 13)], ids=str)
def test_distinct_windows(P, stride):
    """19 events on 5 x 7 x 11, every window different: a single cell, a fixed-depth plane, a single column, the
    whole grid and 15 seeded ones; (9, 9, 13) exceeds every extent: one candidate per axis"""
    shape = Cs.RANGE_SHAPE
    rng, tt = range_box(19)
    E = 19
    picks, w, _ = synthetic_events(rng, tt, E, noise=0.5)
    lo, hi = seeded_windows(rng, shape, E)
    lo[0], hi[0] = (3, 4, 5), (3, 4, 5)                     # a single cell
    lo[1], hi[1] = (0, 0, 6), (4, 6, 6)                     # a fixed depth
    lo[2], hi[2] = (2, 5, 0), (2, 5, 10)                    # a single column
    lo[3], hi[3] = (0, 0, 0), (4, 6, 10)                    # the whole grid
    assert len({tuple(lo[e]) + tuple(hi[e]) for e in range(E)}) == E
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        cell, _, _ = check_window(sol, tt, picks, w, lo, hi, stride, str(stride))
    c = np.array(np.unravel_index(cell[cell >= 0], shape)).T
    assert np.all((c - lo[cell >= 0]) % np.array(stride) == 0) and np.all(c <= hi[cell >= 0])
    if stride == (9, 9, 13):
        ok = cell >= 0
        assert np.array_equal(cell[ok], np.ravel_multi_index(tuple(lo[ok].T), shape))


def test_group_edges(P):
    """runs of 1, 7, 8, 9 and 17 consecutive events with one window, next to each other"""
    shape = Cs.RANGE_SHAPE
    rng, tt = range_box(42)
    runs = (1, 7, 8, 9, 17)
    E = sum(runs)
    picks, w, _ = synthetic_events(rng, tt, E, noise=0.5)
    rlo, rhi = seeded_windows(rng, shape, len(runs))
    rlo[2], rhi[2] = (0, 0, 0), (4, 6, 10)
    assert len({tuple(rlo[r]) + tuple(rhi[r]) for r in range(len(runs))}) == len(runs)
    lo, hi = np.repeat(rlo, runs, axis=0), np.repeat(rhi, runs, axis=0)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        check_window(sol, tt, picks, w, lo, hi, 1)
        check_window(sol, tt, picks, w, lo, hi, (2, 1, 3), "strided")


TILE_EDGE_SHAPE = (17, 257, 241)
TILE_EDGE_WINDOWS = {1: (1, 1, 1), 255: (3, 5, 17), 256: (4, 8, 8), 257: (1, 257, 1), TILE - 1: (5, 9, 91),
                     TILE: (16, 16, 16), TILE + 1: (17, 1, 241), 8676: (3, 12, 241)}


def test_tile_edges(P):
    """candidate counts of 1, 255, 256, 257, 4095, 4096 (the tile), 4097 and 8676 (three tiles) per window, inside
    17 x 257 x 241; two events per window (one group), the minimum of the second planted at the last candidate"""
    import torch
    shape = TILE_EDGE_SHAPE
    rng = np.random.default_rng(4096)
    tt = rng.uniform(1, 9, (2,) + shape).astype(F32)
    tt[rng.random(tt.shape) < 0.01] = INF
    los, his = [], []
    for count, e in TILE_EDGE_WINDOWS.items():
        assert count == int(np.prod(e))
        lo = np.array([rng.integers(0, shape[a] - e[a] + 1) for a in range(3)])
        los += [lo, lo]
        his += [lo + np.array(e) - 1] * 2
    lo, hi = np.array(los), np.array(his)
    E = len(lo)
    picks = rng.uniform(0, 9, (E, 2))
    for e in range(1, E, 2):                        # J = +0 at the window's last candidate
        tt[:, hi[e][0], hi[e][1], hi[e][2]] = (3.0, 4.0)
        picks[e] = (5.0, 6.0)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        cell, mis, _ = check_window(sol, tt, picks, None, lo, hi, 1)
    assert np.array_equal(cell[1::2], np.ravel_multi_index(tuple(hi[1::2].T), shape)) and np.all(mis[1::2] == 0)


def test_ties_go_to_the_lo_corner_and_stay_on_the_lattice(P):
    shape = (9, 8, 7)
    tt = np.ones((2,) + shape, F32)
    picks = np.array([[3.0, 3.0]] * 3)
    lo = np.array([[1, 2, 1], [0, 0, 0], [8, 7, 6]])
    hi = np.array([[7, 7, 5], [8, 7, 6], [8, 7, 6]])
    corner = np.ravel_multi_index(tuple(lo.T), shape)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        cell, mis, _ = check_window(sol, tt, picks, None, lo, hi, 1)
        assert np.array_equal(cell, corner) and np.all(mis == 0)
        cell, _, _ = check_window(sol, tt, picks, None, lo, hi, 2)
        assert np.array_equal(cell, corner)
        tt[1] = 2.0                             # J > 0, the same at every cell ...
        tt[1, 2::2, 1::2, 2::2] = 1.0           # ... but J = 0 at cells off the lattice of event 0 (x odd, y, z even)
        cell, mis, _ = check_window(sol, tt, picks[:1], None, lo[:1], hi[:1], 2)
        assert cell[0] == corner[0] and mis[0] > 0
        cell, mis, _ = check_window(sol, tt, picks[:1], None, lo[:1], hi[:1], 1)
        assert cell[0] != corner[0] and mis[0] == 0


def test_infinity(P):
    import torch
    shape = (6, 7, 8)
    rng = np.random.default_rng(8)
    tt = rng.uniform(0, 9, (3,) + shape).astype(F32)
    tt[1, :3] = INF                             # x < 3 is not reached by station 1
    picks, w, _ = synthetic_events(rng, tt, 4, drop=0.0)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        inside = check_window(sol, tt, picks, w, [0, 1, 2], [2, 5, 6], 1, "wholly inside")
        assert np.all(inside[0] == -1) and np.all(inside[1] == np.inf)
        none = sol.locate(torch.from_numpy(np.full((3,) + shape, INF)).to(dev()), picks, w)
        assert np.all(none.cell.cpu().numpy() == -1)
        assert np.array_equal(u64(inside[2]), u64(none.t0.cpu().numpy())), "the NaN bits of locate"
        partly = check_window(sol, tt, picks, w, [1, 1, 2], [4, 5, 6], (1, 2, 1), "partly inside")
        assert np.all(partly[0] >= 3 * 7 * 8) and np.all(np.isfinite(partly[1]))
        w0 = w.copy()
        w0[:, 1] = 0.0                          # the station with the INF region has no pick: ignored
        tt[1] = INF
        free = check_window(sol, tt, picks, w0, [0, 1, 2], [2, 5, 6], 1, "zero weight")
        assert np.all(free[0] >= 0) and np.all(free[0] < 3 * 7 * 8)


def test_batch_independence(P):
    import torch
    shape = Cs.RANGE_SHAPE
    rng, tt = range_box(7)
    E = 21
    picks, w, _ = synthetic_events(rng, tt, E, noise=0.5)
    lo, hi = seeded_windows(rng, shape, E)
    lo[4:14], hi[4:14] = lo[4], hi[4]           # a run of ten shares a window: groups of 8 and 2
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        tdev = torch.from_numpy(tt).to(dev())
        for stride in (1, (2, 1, 3)):
            every = outputs(sol.locate_window(tdev, picks, w, lo, hi, stride))
            same(outputs(sol.locate_window(tdev, picks, w, lo, hi, stride)), every, "call to call")
            r = slice(None, None, -1)
            rev = outputs(sol.locate_window(tdev, picks[r].copy(), w[r].copy(), lo[r], hi[r], stride))
            same(tuple(a[r] for a in rev), every, "reversed")
            for e in range(E):
                one = outputs(sol.locate_window(tdev, picks[e:e + 1], w[e:e + 1], lo[e:e + 1], hi[e:e + 1], stride))
                same(one, tuple(a[e:e + 1] for a in every), f"event {e} alone")


def test_refusals_leave_the_outputs(P):
    import torch
    rng = np.random.default_rng(1)
    shape = (6, 5, 4)
    tt = torch.from_numpy(rng.uniform(0, 5, (3,) + shape).astype(F32)).to(dev())
    good = rng.uniform(0, 5, (4, 3))
    ones = np.ones((4, 3))
    LO, HI = np.zeros((4, 3), np.int32), np.tile(np.array(shape, np.int32) - 1, (4, 1))

    def arr(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.int32)

    def edit(a, e, axis, v):
        b = a.copy()
        b[e, axis] = v
        return b

    with P.TravelTimeSolver(shape, star818(P)) as sol:
        tp = sol._box_pointers(tt, 3)
        cases = ((good, ones, edit(LO, 2, 1, 5), edit(HI, 2, 1, 3), [1, 1, 1], "event 2"),  # lo > hi
                 (good, ones, LO, edit(HI, 3, 0, 6), [1, 1, 1], "event 3"),                    # hi >= n
                 (good, ones, edit(LO, 1, 2, -1), HI, [1, 1, 1], "event 1"),                   # lo < 0
                 (good, ones, LO, HI, [1, 0, 1], "stride"),
                 (good, ones, LO, None, [1, 1, 1], "lo and hi"),
                 (good, ones, None, HI, [1, 1, 1], "lo and hi"),
                 (np.where(np.eye(4, 3) > 0, np.nan, good), ones, LO, HI, [1, 1, 1], "pick"),
                 (good, np.where(np.eye(4, 3) > 0, -1.0, 1.0), LO, HI, [1, 1, 1], "weight"),
                 (good, np.array([[1.0] * 3, [0.0] * 3, [1.0] * 3, [1.0] * 3]), LO, HI, [1, 1, 1], "no weight"))
        for picks, w, lo, hi, stride, msg in cases:
            pd, wd = torch.from_numpy(picks).to(dev()), torch.from_numpy(w).to(dev())
            cell = torch.full((4,), 77, dtype=torch.int32, device=dev())
            mis = torch.full((4,), 3.5, dtype=torch.float64, device=dev())
            t0 = torch.full((4,), -2.5, dtype=torch.float64, device=dev())
            lo, hi, st = arr(lo), arr(hi), arr(stride)
            rc = sol._L.ttsweep_locate_window_device(
                sol._ctx, 3, tp, 4, pd.data_ptr(), wd.data_ptr(), None if lo is None else lo.ctypes.data,
                None if hi is None else hi.ctypes.data, st.ctypes.data, cell.data_ptr(), mis.data_ptr(), t0.data_ptr())
            assert rc < 0 and msg in P._lib.last_error(), msg
            assert torch.all(cell == 77) and torch.all(mis == 3.5) and torch.all(t0 == -2.5), msg
            with pytest.raises(P.TTSweepError):
                sol.locate_window(tt, pd, wd, lo, hi, stride)
        with pytest.raises(P.TTSweepError):
            sol.locate_window(tt, good, None, LO[:3], HI[:3])           # [E, 3] with the wrong E
        with pytest.raises(P.TTSweepError):
            sol.locate_window(tt, good, None, LO.astype(float), HI)     # float windows
        # a correct call works afterwards
        same(outputs(sol.locate_window(tt, good, ones, LO, HI, [1, 1, 1])), outputs(sol.locate(tt, good, ones)))


def test_boxes_and_solve_state_are_left_alone(P):
    import torch
    shape = (30, 26, 14)
    v = P.inputs.velocity_model(*shape, seed=21)
    rng = np.random.default_rng(5)
    stations = np.stack([rng.integers(0, shape[0], 6), rng.integers(0, shape[1], 6), np.zeros(6, int)], 1)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        sol.set_velocity(v)
        tt = torch.empty((6,) + shape, dtype=torch.float32, device=dev())
        assert sol.solve_device(stations, tt, init=True) == 1
        before = tt.clone()
        tth = tt.cpu().numpy()
        picks, w, _ = synthetic_events(rng, tth, 30)
        same(outputs(sol.locate_window(tt, picks, w, [2, 3, 1], [20, 25, 9], (2, 2, 1))),
             W.locate_window(tth, picks, w, [2, 3, 1], [20, 25, 9], (2, 2, 1)))
        fine = sol.locate_refine(tt, picks, w, stride=3)
        same(outputs(fine), W.refine(tth, picks, w, stride=3)[:3])
        assert torch.equal(tt.view(torch.int32), before.view(torch.int32))
        assert sol.solve_device(stations, tt, init=False) == 0          # still answered as a confirming pass


# ---- locate_refine ----
def check_refine(sol, tdev, tth, picks, w, stride, radius=None, what=""):
    res = sol.locate_refine(tdev, picks, w, stride=stride, radius=radius)
    rc, rm, rt, cc, cm = W.refine(tth, picks, w, stride=stride, radius=radius)
    same(outputs(res), (rc, rm, rt), what)
    assert np.array_equal(res.coarse_cell.cpu().numpy(), cc), what
    assert np.array_equal(u64(res.coarse_misfit.cpu().numpy()), u64(cm)), what
    return res


@pytest.mark.parametrize("stride", [2, (2, 3, 4)], ids=str)
def test_refine_on_golden_boxes(P, stride):
    import torch
    name, tt = golden_stations()[0]
    tth = np.ascontiguousarray(tt, dtype=F32)
    rng = np.random.default_rng(77)
    picks, w, _ = synthetic_events(rng, tth, 40, drop=0.15)
    with P.TravelTimeSolver(tth.shape[1:], star818(P)) as sol:
        tdev = torch.from_numpy(tth).to(dev())
        res = check_refine(sol, tdev, tth, picks, w, stride, what=name)
        check_refine(sol, tdev, tth, picks[:9], w[:9], stride, radius=1, what=name + " radius 1")
        full = sol.locate(tdev, picks, w)
    mis, cm, fm = (u64(a.cpu().numpy()) for a in (res.misfit, res.coarse_misfit, full.misfit))
    assert np.all(mis <= cm) and np.all(mis >= fm)      # J >= +0: the order of the bits is the order of the values
    print(f"refined cells equal to locate's: {np.mean(outputs(res)[0] == full.cell.cpu().numpy()):.3f}")


def test_refine_falls_back_to_the_whole_grid(P):
    """event 0: every lattice node inadmissible but an off-lattice cell is not: stage 2 is the whole grid, exact"""
    import torch
    shape = (9, 8, 7)
    rng = np.random.default_rng(3)
    tt = rng.uniform(0, 9, (3,) + shape).astype(F32)
    tt[0, ::2, ::2, ::2] = INF
    picks, w, _ = synthetic_events(rng, tt, 3, drop=0.0)
    w[1:, 0] = 0.0                              # events 1 and 2 do not use station 0: they have lattice nodes
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        tdev = torch.from_numpy(tt).to(dev())
        res = check_refine(sol, tdev, tt, picks, w, 2)
        full = outputs(sol.locate(tdev, picks[:1], w[:1]))
    cell, cc = res.cell.cpu().numpy(), res.coarse_cell.cpu().numpy()
    assert cc[0] == -1 and np.isinf(res.coarse_misfit.cpu().numpy()[0]) and np.all(cc[1:] >= 0)
    assert cell[0] == full[0][0] >= 0 and u64(res.misfit.cpu().numpy()[:1]) == u64(full[1])
    assert np.any(np.array(np.unravel_index(cell[0], shape)) % 2 == 1)


# ---- full size ----
@pytest.fixture(scope="module")
def bench_stations(P):
    """241 x 241 x 51, the 24 start-24 boxes solved on the device as stations: (solver, boxes on the device, on the host)"""
    import torch
    shape = (241, 241, 51)
    starts = P.inputs.read_triples(P.inputs.starts_path("24"))
    v = P.inputs.velocity_model(*shape, seed=20160507)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        sol.set_velocity(v)
        tt = torch.empty((len(starts),) + shape, dtype=torch.float32, device=dev())
        assert sol.solve_device(starts, tt, init=True) == 1
        yield sol, tt, tt.cpu().numpy()


def test_full_size_whole_grid_equals_locate(P, bench_stations):
    import torch
    sol, tt, tth = bench_stations
    rng = np.random.default_rng(64)
    picks, w, _ = synthetic_events(rng, tth, 64, noise=0.05)
    pd, wd = torch.from_numpy(picks).to(dev()), torch.from_numpy(w).to(dev())
    same(outputs(sol.locate_window(tt, pd, wd)), outputs(sol.locate(tt, pd, wd)))


def test_full_size_refine(P, bench_stations):
    """256 events through locate_refine(stride=4) against the restatement's refine(): stage 1 is 48 373 lattice nodes"""
    import torch
    sol, tt, tth = bench_stations
    rng = np.random.default_rng(256)
    picks, w, _ = synthetic_events(rng, tth, 256, noise=0.05)
    pd, wd = torch.from_numpy(picks).to(dev()), torch.from_numpy(w).to(dev())
    res = check_refine(sol, tt, tth, picks, w, 4)
    full = sol.locate(tt, pd, wd)
    mis, cm, fm = (u64(a.cpu().numpy()) for a in (res.misfit, res.coarse_misfit, full.misfit))
    assert np.all(mis <= cm) and np.all(mis >= fm)
    print(f"refined cells equal to locate's: {np.mean(outputs(res)[0] == full.cell.cpu().numpy()):.4f} of 256")
