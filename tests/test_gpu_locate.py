"""GPU tier (-m gpu) of event location (include/ttsweep.h, "locate"): ttsweep_locate_device through
TravelTimeSolver.locate, bit for bit against the numpy restatement tests/locate_reference.py (cell, misfit bits, t0
bits, volume bits) on recorded, solved and hand-made boxes; independent of the batch, deterministic, refusing bad
picks and weights without touching an output, leaving the boxes and the solve's state alone, and feeding
frechet_operator."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, Golden
import locate_cases as Cs
import locate_reference as L

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


def dev():
    import torch
    return torch.device("cuda:0")


def u64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


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


def star818(P):
    return P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))


def check_locate(P, tt, picks, weights=None, vol_events=(), ref_events=None, what="", sol=None):
    """locate on the device == the restatement (every event, or ref_events), bit for bit; returns the result.  sol: a
    solver of the boxes' shape to use (one is made when None)."""
    import torch
    tt = np.ascontiguousarray(tt, dtype=F32)
    shape = tt.shape[1:]
    if sol is None:
        with P.TravelTimeSolver(shape, star818(P)) as own:
            return check_locate(P, tt, picks, weights, vol_events, ref_events, what, own)
    tdev = torch.from_numpy(tt).to(dev())
    res = sol.locate(tdev, picks, weights, misfit_events=list(vol_events) or None)
    assert res.cell.dtype == torch.int32 and res.cell.device == dev() and res.misfit.dtype == torch.float64
    cell, mis, t0 = res.cell.cpu().numpy(), res.misfit.cpu().numpy(), res.t0.cpu().numpy()
    idx = np.arange(len(picks)) if ref_events is None else np.asarray(ref_events)
    w = None if weights is None else np.asarray(weights)[idx]
    with np.errstate(all="ignore"):          # the float-range cases overflow on purpose
        rc, rm, rt, rv = L.locate(tt, np.asarray(picks)[idx], w,
                                  volumes=[i for i, e in enumerate(idx) if e in vol_events])
    assert np.array_equal(cell[idx], rc), what
    assert np.array_equal(u64(mis[idx]), u64(rm)), what
    nan = np.isnan(rt)
    assert np.array_equal(np.isnan(t0[idx]), nan), what
    assert np.array_equal(u64(t0[idx][~nan]), u64(rt[~nan])), what
    xyz = res.xyz.numpy()
    assert np.array_equal(xyz[cell >= 0], np.argwhere(np.ones(shape, bool))[cell[cell >= 0]]), what
    assert np.all(xyz[cell < 0] == -1)
    if vol_events:
        vols = res.volumes.cpu().numpy()
        for v, e in enumerate(vol_events):
            i = int(np.flatnonzero(idx == e)[0])
            assert np.array_equal(u64(vols[v]), u64(rv[i])), (what, e)
    return res


def golden_stations():
    out = []
    for name in ("g24", "g9"):
        g = Golden(name)
        boxes = [tt for _, _, _, _, tt, _ in g.cases()]
        out.append((name, np.stack(boxes)))
    return out


@pytest.mark.parametrize("case", golden_stations(), ids=lambda c: c[0])
def test_golden_boxes_as_stations(P, case):
    name, tt = case
    rng = np.random.default_rng(len(name) + tt.shape[0])
    picks, w, _ = synthetic_events(rng, tt, 40)
    check_locate(P, tt, picks, w, vol_events=(0, 3), what=name)
    check_locate(P, tt, picks[:5], None, what=name + " unweighted")


FR = np.load(os.path.join(GOLDEN, "float_range.npz"))
FR_META = json.loads(bytes(FR["meta"]).decode())


@pytest.mark.parametrize("key", sorted(FR_META))
def test_float_range_boxes_as_stations(P, key):
    tt = FR[f"tt_{key}"]
    rng = np.random.default_rng(sum(map(ord, key)))
    picks, w, _ = synthetic_events(rng, tt, 16, noise=1.0)
    check_locate(P, tt, picks, w, vol_events=(1,), what=key)


def test_seeded_boxes_solved_on_the_device(P):
    import torch
    shape = (30, 26, 14)
    v = P.inputs.velocity_model(*shape, seed=21)
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))
    rng = np.random.default_rng(5)
    stations = np.stack([rng.integers(0, shape[0], 12), rng.integers(0, shape[1], 12), np.zeros(12, int)], 1)
    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((12,) + shape, dtype=torch.float32, device=dev())
        assert sol.solve_device(stations, tt, init=True) == 1
        tth = tt.cpu().numpy()
    picks, w, _ = synthetic_events(rng, tth, 100)
    check_locate(P, tth, picks, w, vol_events=(0, 50, 99))


def test_ties_go_to_the_smallest_index(P):
    tt = np.zeros((3, 9, 8, 7), F32)
    tt[0] = 1.0
    tt[1] = 2.0
    tt[2, :, :, 3:] = 5.0               # J = 0 at every cell with z < 3 and at no other
    picks = np.array([[1.0, 2.0, 0.0], [3.0, 4.0, 2.0]])
    res = check_locate(P, tt, picks, vol_events=(0,))
    assert res.cell.cpu().numpy()[0] == 0
    tt[:, 0, 0, 0] = INF                # now the smallest is cell 1
    res = check_locate(P, tt, picks)
    assert res.cell.cpu().numpy()[0] == 1


def test_single_pick_gives_the_smallest_admissible_cell(P):
    rng = np.random.default_rng(2)
    tt = rng.uniform(0, 9, (4, 10, 9, 5)).astype(F32)
    tt[2].reshape(-1)[:17] = INF
    w = np.zeros((3, 4))
    w[:, 2] = 1.0
    res = check_locate(P, tt, rng.uniform(0, 9, (3, 4)), w)
    assert np.all(res.cell.cpu().numpy() == 17) and np.all(res.misfit.cpu().numpy() == 0)


def test_zero_weight_stations_with_all_inf_boxes(P):
    rng = np.random.default_rng(4)
    tt = rng.uniform(0, 9, (5, 11, 7, 6)).astype(F32)
    tt[1] = INF
    tt[3] = INF
    picks, w, _ = synthetic_events(rng, tt[[0, 2, 4]], 20)
    P5 = np.zeros((20, 5))
    W5 = np.zeros((20, 5))
    P5[:, [0, 2, 4]], W5[:, [0, 2, 4]] = picks, w
    P5[:, [1, 3]] = 1e30                # finite, never read: weight 0
    res = check_locate(P, tt, P5, W5, vol_events=(7,))
    assert np.all(res.cell.cpu().numpy() >= 0)


def test_boxes_partly_at_infinity_and_no_admissible_cell(P):
    rng = np.random.default_rng(6)
    tt = rng.uniform(0, 9, (6, 13, 9, 7)).astype(F32)
    tt[rng.random(tt.shape) < 0.3] = INF
    picks, w, _ = synthetic_events(rng, tt, 30)
    check_locate(P, tt, picks, w, vol_events=(2,))
    tt2 = np.full((2, 5, 4, 3), INF)
    tt2[0, 0, 0, 0] = 1.0
    tt2[1, 1, 1, 1] = 1.0               # no cell is reached by both
    res = check_locate(P, tt2, np.array([[1.0, 1.0], [2.0, 3.0]]), vol_events=(0,))
    assert np.all(res.cell.cpu().numpy() == -1) and np.all(np.isinf(res.misfit.cpu().numpy()))
    assert np.all(np.isnan(res.t0.cpu().numpy()))
    assert np.all(np.isinf(res.volumes.cpu().numpy()))


@pytest.mark.parametrize("K", [33, 200])
def test_many_stations_read_the_boxes_on_use(P, K):
    rng = np.random.default_rng(K)
    tt = rng.uniform(0, 20, (K, 12, 10, 9)).astype(F32)
    tt[rng.random(tt.shape) < 0.01] = INF
    picks, w, _ = synthetic_events(rng, tt, 20, noise=0.5)
    check_locate(P, tt, picks, w, vol_events=(0, 19))


def bench_stations(P):
    import torch
    shape = (241, 241, 51)
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))
    starts = P.inputs.read_triples(P.inputs.starts_path("24"))
    v = P.inputs.velocity_model(*shape, seed=20160507)
    sol = P.TravelTimeSolver(shape, fs)
    sol.set_velocity(v)
    tt = torch.empty((len(starts),) + shape, dtype=torch.float32, device=dev())
    assert sol.solve_device(starts, tt, init=True) == 1
    return sol, starts, tt


def test_full_size_events_batch_independence_and_state(P):
    """241x241x51, the 24 start-24 boxes as stations, 4097 seeded events (15 % of picks dropped): a sample of
    events against the restatement; the same bits alone, in a batch of 7 and in the batch of 4097; two calls
    identical; boxes and the solve's state unchanged."""
    import torch
    sol, starts, tt = bench_stations(P)
    with sol:
        changed = sol.changed(len(starts))
        before = tt.clone()
        tth = tt.cpu().numpy()
        rng = np.random.default_rng(4096)
        picks, w, _ = synthetic_events(rng, tth, 4097, noise=0.05)
        pd, wd = torch.from_numpy(picks).to(dev()), torch.from_numpy(w).to(dev())
        a = sol.locate(tt, pd, wd)
        b = sol.locate(tt, pd, wd)
        for f in ("cell", "misfit", "t0"):
            assert torch.equal(getattr(a, f).view(torch.int32 if f == "cell" else torch.int64),
                               getattr(b, f).view(torch.int32 if f == "cell" else torch.int64)), f
        sample = [0, 1, 6, 2048, 4095, 4096]
        cell, mis, t0 = a.cell.cpu().numpy(), a.misfit.cpu().numpy(), a.t0.cpu().numpy()
        rc, rm, rt, _ = L.locate(tth, picks[sample], w[sample])
        assert np.array_equal(cell[sample], rc)
        assert np.array_equal(u64(mis[sample]), u64(rm)) and np.array_equal(u64(t0[sample]), u64(rt))
        for lo, hi in ((6, 7), (2044, 2051), (0, 7)):
            s = sol.locate(tt, pd[lo:hi], wd[lo:hi])
            assert np.array_equal(s.cell.cpu().numpy(), cell[lo:hi])
            assert np.array_equal(u64(s.misfit.cpu().numpy()), u64(mis[lo:hi]))
            assert np.array_equal(u64(s.t0.cpu().numpy()), u64(t0[lo:hi]))
        J, _ = L.misfit(tth, picks[6], w[6])
        vol = sol.locate(tt, pd[6:7], wd[6:7], misfit_events=[0]).volumes
        assert np.array_equal(u64(vol.cpu().numpy()[0]), u64(J))
        assert torch.equal(tt.view(torch.int32), before.view(torch.int32))
        assert sol.changed(len(starts)) == changed
        assert sol.solve_device(starts, tt, init=False) == 0          # still answered as a confirming pass


def test_noise_free_events_are_recovered(P):
    rng = np.random.default_rng(9)
    tt = golden_stations()[0][1]
    picks, w, cells = synthetic_events(rng, tt, 60, drop=0.1, noise=0.0)
    res = check_locate(P, tt, picks, w)
    rc, _, _, _ = L.locate(tt, picks, w)
    found = res.cell.cpu().numpy()
    assert np.array_equal(found[rc == cells], cells[rc == cells])
    assert np.mean(rc == cells) > 0.5


def test_bad_picks_and_weights_are_refused_and_leave_the_outputs(P):
    import torch
    rng = np.random.default_rng(1)
    tt = torch.from_numpy(rng.uniform(0, 5, (3, 6, 5, 4)).astype(F32)).to(dev())
    good = rng.uniform(0, 5, (4, 3))
    with P.TravelTimeSolver((6, 5, 4), star818(P)) as sol:
        tp = sol._box_pointers(tt, 3)
        for picks, w, msg in ((np.where(np.eye(4, 3) > 0, np.nan, good), None, "pick"),
                              (np.where(np.eye(4, 3) > 0, np.inf, good), None, "pick"),
                              (good, np.where(np.eye(4, 3) > 0, -1.0, 1.0), "weight"),
                              (good, np.where(np.eye(4, 3) > 0, np.inf, 1.0), "weight"),
                              (good, np.where(np.eye(4, 3) > 0, np.nan, 1.0), "weight"),
                              (good, np.array([[1.0] * 3, [0.0] * 3, [1.0] * 3, [1.0] * 3]), "no weight")):
            pd = torch.from_numpy(picks).to(dev())
            wd = None if w is None else torch.from_numpy(w).to(dev())
            cell = torch.full((4,), 77, dtype=torch.int32, device=dev())
            mis = torch.full((4,), 3.5, dtype=torch.float64, device=dev())
            t0 = torch.full((4,), -2.5, dtype=torch.float64, device=dev())
            vol = torch.full((1, 6, 5, 4), 9.0, dtype=torch.float64, device=dev())
            ev = (C.c_int * 1)(0)
            rc = sol._L.ttsweep_locate_device(sol._ctx, 3, tp, 4, pd.data_ptr(), None if wd is None else wd.data_ptr(),
                                              cell.data_ptr(), mis.data_ptr(), t0.data_ptr(), 1, ev,
                                              sol._box_pointers(vol, 1))
            assert rc < 0 and msg in P._lib.last_error()
            assert torch.all(cell == 77) and torch.all(mis == 3.5) and torch.all(t0 == -2.5) and torch.all(vol == 9.0)
            with pytest.raises(P.TTSweepError):
                sol.locate(tt, pd, wd)
        with pytest.raises(P.TTSweepError):
            sol.locate(tt, good[:, :2])                 # [E, K] with the wrong K
        with pytest.raises(P.TTSweepError):
            sol.locate(tt, good.astype(np.float32))     # float32 picks
        with pytest.raises(P.TTSweepError):
            sol.locate(tt, good, misfit_events=[4])


def test_located_cells_feed_the_frechet_operator(P):
    """Passive tomography: locate, then frechet_operator(stations, tt, located cells): t_recv is T_k at the cells."""
    import torch
    shape = (24, 22, 12)
    v = P.inputs.velocity_model(*shape, seed=8)
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))
    rng = np.random.default_rng(8)
    stations = np.stack([rng.integers(0, shape[0], 8), rng.integers(0, shape[1], 8), np.zeros(8, int)], 1)
    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((8,) + shape, dtype=torch.float32, device=dev())
        assert sol.solve_device(stations, tt, init=True) == 1
        picks, w, _ = synthetic_events(rng, tt.cpu().numpy(), 30)
        loc = sol.locate(tt, picks, w)
        xyz = loc.xyz.numpy()
        assert np.all(xyz >= 0)
        op = sol.frechet_operator(stations, tt, xyz)
        want = tt.reshape(8, -1)[:, loc.cell.to(torch.int64)].reshape(-1).cpu()
        assert torch.equal(op.t_recv.view(torch.int32), want.view(torch.int32))


# ---- the cases of locate_cases.py (their claims are checked by the CPU tier, tests/test_locate_cpu.py) ----
def outputs(res):
    return res.cell.cpu().numpy(), res.misfit.cpu().numpy(), res.t0.cpu().numpy()


def assert_periodic(cell, mis, t0, period, what):
    """every output equals the output of its row: event e against event e % period"""
    first = np.arange(len(cell)) % period
    assert np.array_equal(cell, cell[first]), what
    assert np.array_equal(u64(mis), u64(mis[first])) and np.array_equal(u64(t0), u64(t0[first])), what


@pytest.mark.parametrize("variant", ["unit", "weighted"])
def test_second_and_third_batches_on_a_grid_of_many_tiles(P, variant):
    """17 x 59 x 4095 (1003 tiles, the last partial), K = 2, 2 * 16727 + 5 events that repeat 97 distinct rows: three
    batches of ttsweep_locate_device, each ending in a partial event block (the formula of Cs.batches mirrors
    LOC_PARTIALS and LOC_ET).  The distinct rows against the restatement bit for bit, every event against its row,
    the events around each batch edge again as calls of their own, the planted ties at their smallest index, one
    misfit volume of the last batch."""
    import torch
    E, period = Cs.BIG_E, Cs.BIG_P
    ntiles, eb, starts = Cs.batches(Cs.BIG_SHAPE, E)
    assert len(starts) >= 3 and eb % Cs.ET != 0 and ntiles > 3 * 256 and starts[-1] + eb > E
    tt = np.array(Cs.big_box())
    rows_p, rows_w = Cs.big_rows(variant)
    picks, w = Cs.periodic(rows_p, E), Cs.periodic(rows_w, E)
    ref = Cs.big_reference(variant)
    vol_e = E - 2
    with P.TravelTimeSolver(Cs.BIG_SHAPE, star818(P)) as sol:
        tdev = torch.from_numpy(tt).to(dev())
        pd = torch.from_numpy(picks).to(dev())
        wd = None if w is None else torch.from_numpy(w).to(dev())
        res = sol.locate(tdev, pd, wd, misfit_events=[vol_e])
        cell, mis, t0 = outputs(res)
        for r, (c, m, t) in ((r, v[:3]) for r, v in ref.items()):
            assert (cell[r], u64(mis[r]), u64(t0[r])) == (c, u64(m), u64(t)), (variant, "row", r)
        assert_periodic(cell, mis, t0, period, variant)
        for r, (kind, cells, _) in Cs.big_plants().items():
            assert np.all(cell[r::period] == min(cells)), (variant, kind)
        J, _ = Cs.misfit(tt, picks[vol_e], None if w is None else w[vol_e])
        assert np.array_equal(u64(res.volumes.cpu().numpy()[0]), u64(J)), "the volume of an event of the last batch"
        del res
        for lo, hi in [(s - 5, s + 6) for s in starts[1:]] + [(eb - 1, eb), (eb, eb + 1), (E - 7, E)]:
            s = sol.locate(tdev, pd[lo:hi], None if wd is None else wd[lo:hi])
            sc, sm, st = outputs(s)
            assert np.array_equal(sc, cell[lo:hi]), (variant, lo, hi)
            assert np.array_equal(u64(sm), u64(mis[lo:hi])) and np.array_equal(u64(st), u64(t0[lo:hi])), (lo, hi)


def test_more_events_than_one_launch_takes(P):
    """2 x 3 x 2 cells, K = 2, 65535 * 8 + 3 events that repeat 97 distinct rows: the last three events are a second
    batch.  The distinct rows against the restatement, every event against its row, four volumes around the edge."""
    import torch
    tt, rows_p, rows_w, _ = Cs.cap_case()
    E = Cs.CAP_E
    assert Cs.batches(Cs.CAP_SHAPE, E)[2] == [0, E - 3]
    picks, w = Cs.periodic(rows_p, E), Cs.periodic(rows_w, E)
    vols = [0, Cs.CAP - 1, Cs.CAP, E - 1]
    with P.TravelTimeSolver(Cs.CAP_SHAPE, star818(P)) as sol:
        res = sol.locate(torch.from_numpy(tt).to(dev()), picks, w, misfit_events=vols)
    cell, mis, t0 = outputs(res)
    rc, rm, rt, _ = Cs.locate_rows(tt, rows_p, rows_w)
    assert np.all(rc >= 0) and np.array_equal(cell[:Cs.CAP_P], rc)
    assert np.array_equal(u64(mis[:Cs.CAP_P]), u64(rm)) and np.array_equal(u64(t0[:Cs.CAP_P]), u64(rt))
    assert_periodic(cell, mis, t0, Cs.CAP_P, "cap")
    got = res.volumes.cpu().numpy()
    for v, e in enumerate(vols):
        assert np.array_equal(u64(got[v]), u64(Cs.misfit(tt, picks[e], w[e])[0])), e


@pytest.mark.parametrize("N", sorted(Cs.N_SHAPES))
def test_full_and_just_over_full_register_widths(P, N):
    """K in 1, 2, 7 ... 33 around every register instance of loc_kr() on a grid of N cells (around the 256-cell
    volume block and the 4096-cell tile): ten weighted events (dense, +0 at k = 0, +0 at k = K-1, -0.0 at a station
    whose box is partly at infinity, one station picked) and three with weights NULL, every volume."""
    with P.TravelTimeSolver(Cs.N_SHAPES[N], star818(P)) as sol:
        for K in Cs.K_EDGES:
            c = Cs.k_edge_case(K, N)
            check_locate(P, c["tt"], c["picks"], c["weights"], vol_events=tuple(range(Cs.K_E)), what=f"K={K} N={N}",
                         sol=sol)
            check_locate(P, c["tt"], c["none"]["picks"], None, vol_events=tuple(range(Cs.K_E_NONE)),
                         what=f"K={K} N={N}, weights NULL", sol=sol)


@pytest.mark.parametrize("route", Cs.RANGE_ROUTES)
def test_double_range_of_picks_and_weights(P, route):
    """Picks and weights at the ends of the double range (overflow of S1 and of (w r) r, INF - INF, W = INF with
    invW = 0, 1 / W = INF, subnormal weights and residuals): accepted, and the same bits as the restatement."""
    tt, picks, w = Cs.range_case(route)
    assert L.check(picks, w) is None
    res = check_locate(P, tt, picks, w, vol_events=tuple(range(len(picks))), what=route)
    cell, mis, t0 = outputs(res)
    assert np.all((cell >= 0) == (mis < np.inf)) and np.all(np.isnan(t0) == (cell < 0))
