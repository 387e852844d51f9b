"""GPU tier (-m gpu) of the confidence regions of located events (include/ttsweep.h, "locate confidence"):
ttsweep_locate_confidence_device through TravelTimeSolver.locate_confidence, every output equal to the numpy
restatement tests/confidence_reference.py integer for integer and bit for bit, with the reference level taken from
locate on the device; against the misfit volumes at full size; independent of the batch, deterministic, refusing bad
arguments without touching an output, leaving the boxes and the solve's state alone."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, Golden
import confidence_reference as R
import locate_cases as Cs

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
LEVELS = [1.0, 3.53, 7.81, np.inf]


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


def dev():
    import torch
    return torch.device("cuda:0")


def star818(P):
    return P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))


def synthetic_events(rng, tt, E, drop=0.15, noise=0.01, sigma_weights=False):
    """Picks T_k[cell] + t0 + noise at random cells that every box reaches, a share of them dropped (weight 0);
    weights 1 / noise^2 (sigma_weights) or uniform in [0.5, 2)."""
    K = tt.shape[0]
    flat = tt.reshape(K, -1)
    ok = np.flatnonzero(np.all(np.isfinite(flat), axis=0))
    cells = ok[rng.integers(0, len(ok), E)] if len(ok) else rng.integers(0, flat.shape[1], E)
    t0 = rng.uniform(-5, 5, E)
    T = flat[:, cells].T.astype(np.float64)
    picks = np.where(np.isfinite(T), T, 0.0) + t0[:, None] + noise * rng.standard_normal((E, K))
    w = np.full((E, K), 1.0 / noise ** 2) if sigma_weights else rng.uniform(0.5, 2.0, (E, K))
    w[rng.random((E, K)) < drop] = 0.0
    w[np.arange(E), rng.integers(0, K, E)] = w.max()      # at least one pick per event
    return picks, w


def host(res):
    return {f: getattr(res, f).cpu().numpy() for f in R.FIELDS}


def assert_same(got, want, what=""):
    for f in R.FIELDS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
        if not np.array_equal(g.view(np.uint8), w.view(np.uint8)):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {f} differs at {len(bad)} entries; first {bad[0].tolist()}: got "
                                 f"{g[tuple(bad[0])]!r} want {w[tuple(bad[0])]!r}")


def check_confidence(P, tt, picks, weights, delta, what=""):
    """locate then locate_confidence on the device == the restatement at locate's misfit; returns (result, host
    dict, misfit)."""
    import torch
    tt = np.ascontiguousarray(tt, dtype=F32)
    with P.TravelTimeSolver(tt.shape[1:], star818(P)) as sol:
        tdev = torch.from_numpy(tt).to(dev())
        loc = sol.locate(tdev, picks, weights)
        res = sol.locate_confidence(tdev, picks, weights, loc.misfit, delta)
    m = loc.misfit.cpu().numpy()
    E = len(picks)
    d = np.asarray(delta, np.float64)
    d = np.broadcast_to(d if d.ndim == 2 else np.atleast_1d(d)[None], (E, d.shape[-1] if d.ndim else 1))
    assert res.count.dtype == torch.int64 and res.lo.dtype == torch.int32 and res.t0_lo.dtype == torch.float64
    assert res.count.device == dev() and tuple(res.sum2.shape) == (E, d.shape[1], 6) and res.shape == tt.shape[1:]
    got = host(res)
    assert_same(got, R.confidence(tt, picks, weights, m, d), what)
    return res, got, m


def golden_star_stations():
    """The recorded boxes of g24 and g9, each star's boxes as the stations of one case."""
    out = []
    for name in ("g24", "g9"):
        by_star = {}
        for _, sname, _, _, tt, _ in Golden(name).cases():
            by_star.setdefault(sname, []).append(tt)
        out += [(f"{name}-star{s}", np.stack(b)) for s, b in sorted(by_star.items())]
    return out


GOLDEN_CASES = golden_star_stations()


@pytest.mark.parametrize("case", GOLDEN_CASES, ids=lambda c: c[0])
def test_golden_boxes_as_stations(P, case):
    name, tt = case
    finite = tt[np.isfinite(tt)]
    sigma = 0.05 * float(np.median(finite))
    rng = np.random.default_rng(11)
    picks, w = synthetic_events(rng, tt, 32, noise=sigma, sigma_weights=True)
    _, got, _ = check_confidence(P, tt, picks, w, LEVELS, name)
    _, one, _ = check_confidence(P, tt, picks[:5], None, 2.0 * sigma ** 2, name + " unweighted, one level")
    assert one["count"].shape == (5, 1)


def test_regions_of_the_golden_case_are_not_trivial(P):
    """The four star-5 boxes of g24 (5760 cells), sigma 5 % of the median finite travel time, 32 events from
    default_rng(11): at least three quarters of the (event, finite level) pairs have 2 <= count <= ncells / 2 (the
    restatement alone gives 96 of 96 with counts 4...624, 13...1237, 25...1936, checked on the CPU), so the bit-for-bit comparison above is not one of empty or full regions."""
    name, tt = next(c for c in GOLDEN_CASES if c[0] == "g24-star5")
    assert tt.shape[0] == 4 and tt[0].size == 5760
    sigma = 0.05 * float(np.median(tt[np.isfinite(tt)]))
    rng = np.random.default_rng(11)
    picks, w = synthetic_events(rng, tt, 32, noise=sigma, sigma_weights=True)
    _, got, _ = check_confidence(P, tt, picks, w, LEVELS, name)
    c = got["count"][:, :3]
    print("counts per level: min", c.min(0), "max", c.max(0))
    inside = (c >= 2) & (c <= tt[0].size // 2)
    print("pairs in range:", int(inside.sum()), "of", inside.size)
    assert inside.sum() >= 0.75 * inside.size
    assert np.all(got["count"][:, 3] == np.all(np.isfinite(tt), axis=0).sum())


FR = np.load(os.path.join(GOLDEN, "float_range.npz"))
FR_META = json.loads(bytes(FR["meta"]).decode())


@pytest.mark.parametrize("key", sorted(FR_META))
def test_float_range_boxes_as_stations(P, key):
    tt = FR[f"tt_{key}"]
    rng = np.random.default_rng(sum(map(ord, key)))
    picks, w = synthetic_events(rng, tt, 16, noise=1.0)
    check_confidence(P, tt, picks, w, [0.0, 5.0, 1e30, np.inf], key)


def test_boxes_partly_at_infinity_and_no_admissible_cell(P):
    rng = np.random.default_rng(6)
    tt = rng.uniform(0, 9, (6, 13, 9, 7)).astype(F32)
    tt[rng.random(tt.shape) < 0.3] = INF
    picks, w = synthetic_events(rng, tt, 30)
    per_event = rng.uniform(0, 40, (30, 3))
    per_event[::7, 1] = np.inf
    check_confidence(P, tt, picks, w, per_event)
    tt2 = np.full((2, 5, 4, 3), INF)
    tt2[0, 0, 0, 0] = 1.0
    tt2[1, 1, 1, 1] = 1.0               # no cell is reached by both
    _, got, m = check_confidence(P, tt2, np.array([[1.0, 1.0], [2.0, 3.0]]), None, [0.0, np.inf])
    assert np.all(np.isinf(m)) and np.all(got["count"] == 0)
    assert np.all(got["lo"] == [5, 4, 3]) and np.all(got["hi"] == -1)
    assert np.all(got["t0_lo"] == np.inf) and np.all(got["t0_hi"] == -np.inf)


def test_ties_and_a_level_below_the_minimum(P):
    import torch
    tt = np.zeros((3, 9, 8, 7), F32)
    tt[0] = 1.0
    tt[1] = 2.0
    tt[2, :, :, 3:] = 5.0               # J = 0 at every cell with z < 3 and at no other
    picks = np.array([[1.0, 2.0, 0.0], [3.0, 4.0, 2.0]])
    _, got, m = check_confidence(P, tt, picks, None, [0.0, np.inf])
    assert np.all(m == 0) and np.all(got["count"][:, 0] == 9 * 8 * 3) and np.all(got["count"][:, 1] == 9 * 8 * 7)
    assert np.all(got["hi"][:, 0] == [8, 7, 2])
    with P.TravelTimeSolver(tt.shape[1:], star818(P)) as sol:      # m is a level, not checked to be the minimum
        tdev = torch.from_numpy(tt).to(dev())
        for m_, want in ((np.array([0.0, -0.0]), 9 * 8 * 3), (np.array([np.inf, np.inf]), 0)):
            res = sol.locate_confidence(tdev, picks, None, m_, 0.0)
            assert_same(host(res), R.confidence(tt, picks, None, m_, np.zeros((2, 1))))
            assert np.all(res.count.cpu().numpy() == want)
    tt3 = np.stack([np.arange(60, dtype=F32).reshape(3, 4, 5), np.arange(60, 0, -1, dtype=F32).reshape(3, 4, 5)])
    with P.TravelTimeSolver((3, 4, 5), star818(P)) as sol:         # J > 0 everywhere: a too-low level is empty
        res = sol.locate_confidence(torch.from_numpy(tt3).to(dev()), np.array([[100.0, 7.0]]), None,
                                    np.array([0.0]), [0.0, 1e-9])
        assert torch.all(res.count == 0) and torch.all(res.hi == -1)


@pytest.mark.parametrize("K", [33, 200])
def test_many_stations_read_the_boxes_on_use(P, K):
    rng = np.random.default_rng(K)
    tt = rng.uniform(0, 20, (K, 12, 10, 9)).astype(F32)
    tt[rng.random(tt.shape) < 0.01] = INF
    picks, w = synthetic_events(rng, tt, 20, noise=0.5)
    check_confidence(P, tt, picks, w, [float(K), 3.0 * K, 10.0 * K, np.inf], f"K={K}")
    check_confidence(P, tt, picks[:9], w[:9], 2.0 * K, f"K={K}, one level")


@pytest.mark.parametrize("shape", [(1, 1, 1), (16, 16, 16), (17, 16, 16), (5, 41, 20), (1, 1, 4097)])
def test_grids_around_the_tile_size(P, shape):
    """Cell counts below, at and just above a multiple of the 4096-cell tile, register instances of every width."""
    rng = np.random.default_rng(sum(shape))
    for K in (3, 9, 17, 25):
        tt = rng.uniform(0, 5, (K,) + shape).astype(F32)
        picks, w = synthetic_events(rng, tt, 11, noise=0.3)
        check_confidence(P, tt, picks, w, [0.5, np.inf], f"{shape} K={K}")


def bench_stations(P):
    import torch
    shape = (241, 241, 51)
    starts = P.inputs.read_triples(P.inputs.starts_path("24"))
    v = P.inputs.velocity_model(*shape, seed=20160507)
    sol = P.TravelTimeSolver(shape, star818(P))
    sol.set_velocity(v)
    tt = torch.empty((len(starts),) + shape, dtype=torch.float32, device=dev())
    assert sol.solve_device(starts, tt, init=True) == 1
    return sol, starts, tt


def test_full_size_against_the_misfit_volumes_batches_and_state(P):
    """241x241x51, the 24 start-24 boxes as stations, 36 seeded events: a sparse level and delta = +inf against the
    misfit volumes locate returns (count, sums, moments and box from torch.nonzero on the device) and three events
    against the restatement (t0 as well); the same results one event at a time, in another order and in one call;
    two calls identical; boxes and the solve's state unchanged."""
    import torch
    sol, starts, tt = bench_stations(P)
    with sol:
        changed = sol.changed(len(starts))
        before = tt.clone()
        tth = tt.cpu().numpy()
        rng = np.random.default_rng(36)
        sigma = 0.05 * float(np.median(tth))      # a few cells' worth of travel time, as on the golden boxes
        picks, w = synthetic_events(rng, tth, 36, noise=sigma, sigma_weights=True)
        pd, wd = torch.from_numpy(picks).to(dev()), torch.from_numpy(w).to(dev())
        E = 36
        loc = sol.locate(tt, pd, wd, misfit_events=list(range(E)))
        delta = torch.tensor([3.53, float("inf")], dtype=torch.float64, device=dev())
        a = sol.locate_confidence(tt, pd, wd, loc.misfit, delta)
        b = sol.locate_confidence(tt, pd, wd, loc.misfit, delta)
        ha = host(a)
        assert_same(host(b), ha, "two calls")
        thr = loc.misfit[:, None] + delta[None, :]
        ncells = tth[0].size
        for e in range(E):
            for l in range(2):
                vol = loc.volumes[e]
                idx = torch.nonzero((vol <= thr[e, l]) & (vol < float("inf")))
                assert int(a.count[e, l]) == len(idx) > 0
                assert torch.equal(a.sum[e, l], idx.sum(0))
                x, y, z = idx[:, 0], idx[:, 1], idx[:, 2]
                want2 = torch.stack([(x * x).sum(), (y * y).sum(), (z * z).sum(), (x * y).sum(), (x * z).sum(),
                                     (y * z).sum()])
                assert torch.equal(a.sum2[e, l], want2)
                assert torch.equal(a.lo[e, l].to(torch.int64), idx.min(0).values)
                assert torch.equal(a.hi[e, l].to(torch.int64), idx.max(0).values)
        sparse = ha["count"][:, 0]
        print("cells inside at delta 3.53: min", sparse.min(), "median", int(np.median(sparse)), "max", sparse.max())
        assert np.all(ha["count"][:, 1] == ncells) and np.median(sparse) >= 2 and sparse.max() < ncells // 2
        del loc.volumes
        sample = [0, 17, 35]
        m = loc.misfit.cpu().numpy()
        want = R.confidence(tth, picks[sample], w[sample], m[sample], np.tile([3.53, np.inf], (3, 1)))
        assert_same({f: v[sample] for f, v in ha.items()}, want, "sample against the restatement")
        # batch independence: one at a time, reversed, and per-event deltas in one call
        for e in (0, 17, 35):
            s = sol.locate_confidence(tt, pd[e:e + 1], wd[e:e + 1], loc.misfit[e:e + 1], delta)
            assert_same(host(s), {f: v[e:e + 1] for f, v in ha.items()}, f"event {e} alone")
        rev = torch.arange(E - 1, -1, -1, device=dev())
        s = sol.locate_confidence(tt, pd[rev].contiguous(), wd[rev].contiguous(), loc.misfit[rev].contiguous(), delta)
        assert_same(host(s), {f: v[::-1] for f, v in ha.items()}, "reversed order")
        assert torch.equal(tt.view(torch.int32), before.view(torch.int32))
        assert sol.changed(len(starts)) == changed
        assert sol.solve_device(starts, tt, init=False) == 0          # still answered as a confirming pass


def test_bad_arguments_are_refused_and_leave_the_outputs(P):
    import torch
    rng = np.random.default_rng(1)
    tt = torch.from_numpy(rng.uniform(0, 5, (3, 6, 5, 4)).astype(F32)).to(dev())
    good = rng.uniform(0, 5, (4, 3))
    ones = np.ones((4, 3))
    m0 = np.full(4, 0.25)
    d0 = np.full((4, 2), 1.0)

    def spoil(a, v):
        a = np.array(a, np.float64)
        a.reshape(-1)[1] = v
        return a

    cases = [(spoil(good, np.nan), ones, m0, d0, "pick"), (spoil(good, np.inf), ones, m0, d0, "pick"),
             (good, spoil(ones, -1.0), m0, d0, "weight"), (good, spoil(ones, np.nan), m0, d0, "weight"),
             (good, np.array([[1.0] * 3, [0.0] * 3, [1.0] * 3, [1.0] * 3]), m0, d0, "no weight"),
             (good, ones, spoil(m0, np.nan), d0, "misfit"), (good, ones, spoil(m0, -1e-300), d0, "misfit"),
             (good, ones, spoil(m0, -np.inf), d0, "misfit"), (good, ones, m0, spoil(d0, np.nan), "delta"),
             (good, ones, m0, spoil(d0, -2.0), "delta")]
    with P.TravelTimeSolver((6, 5, 4), star818(P)) as sol:
        tp = sol._box_pointers(tt, 3)
        for picks, w, m, d, msg in cases:
            assert msg in ("pick", "weight", "no weight") or R.check(m, d) == msg
            t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev()) for x in (picks, w, m, d)]
            outs = [torch.full((4, 2) + tail, 77, dtype=dt, device=dev())
                    for dt, tail in ((torch.int64, ()), (torch.int64, (3,)), (torch.int64, (6,)), (torch.int32, (3,)),
                                     (torch.int32, (3,)), (torch.float64, ()), (torch.float64, ()))]
            rc = sol._L.ttsweep_locate_confidence_device(sol._ctx, 3, tp, 4, t[0].data_ptr(), t[1].data_ptr(),
                                                         t[2].data_ptr(), 2, t[3].data_ptr(),
                                                         *[o.data_ptr() for o in outs])
            assert rc < 0 and msg in P._lib.last_error(), (msg, P._lib.last_error())
            assert all(bool(torch.all(o == 77)) for o in outs), msg
            with pytest.raises(P.TTSweepError):
                sol.locate_confidence(tt, *t)
        for bad in ((good[:, :2], None, m0, 1.0), (good.astype(np.float32), None, m0, 1.0), (good, None, m0[:3], 1.0),
                    (good, None, m0, np.ones(5)), (good, None, m0, np.ones((3, 2)))):
            with pytest.raises(P.TTSweepError):
                sol.locate_confidence(tt, *bad)
        # every output may be NULL, and a -0.0 level is zero
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev()) for x in (good, ones, spoil(m0, -0.0), d0)]
        assert sol._L.ttsweep_locate_confidence_device(sol._ctx, 3, tp, 4, t[0].data_ptr(), t[1].data_ptr(),
                                                       t[2].data_ptr(), 2, t[3].data_ptr(), *([None] * 7)) == 0


def test_a_grid_whose_second_moments_could_overflow_is_refused(P):
    """1 x 1 x 2097152: ncells^3 = 2^63.  Refused before an output is touched; one cell fewer is accepted."""
    import torch
    for nz, ok in ((2097152, False), (2097151, True)):
        shape = (1, 1, nz)
        assert R.moments_fit(shape) == ok
        tt = torch.arange(nz, dtype=torch.float32, device=dev()).reshape((1,) + shape)
        picks = np.array([[1000.0]])
        with P.TravelTimeSolver(shape, star818(P)) as sol:
            if ok:
                res = sol.locate_confidence(tt, picks, None, np.zeros(1), np.inf)
                assert int(res.count[0, 0]) == nz and int(res.sum[0, 0, 2]) == nz * (nz - 1) // 2
                assert int(res.sum2[0, 0, 2]) == (nz - 1) * nz * (2 * nz - 1) // 6
                continue
            count = torch.full((1, 1), 77, dtype=torch.int64, device=dev())
            pd, md = torch.from_numpy(picks).to(dev()), torch.zeros(1, dtype=torch.float64, device=dev())
            rc = sol._L.ttsweep_locate_confidence_device(sol._ctx, 1, sol._box_pointers(tt, 1), 1, pd.data_ptr(), None,
                                                         md.data_ptr(), 1, md.data_ptr(), count.data_ptr(),
                                                         *([None] * 6))
            assert rc < 0 and "overflow" in P._lib.last_error()
            assert int(count[0, 0]) == 77


# ---- the cases of locate_cases.py (their claims are checked by the CPU tier, tests/test_confidence_cpu.py and
# tests/test_locate_cpu.py) ----
def check_regions(sol, tt, picks, weights, m, delta, what=""):
    """locate_confidence at the levels m, delta == the restatement, every output; returns the host dict"""
    import torch
    tdev = torch.from_numpy(np.ascontiguousarray(tt, dtype=F32)).to(dev())
    got = host(sol.locate_confidence(tdev, picks, weights, np.ascontiguousarray(m), np.ascontiguousarray(delta)))
    assert_same(got, Cs.confidence(tt, picks, weights, m, delta), what)
    return got


def test_more_events_than_one_launch_takes(P):
    """2 x 3 x 2 cells, K = 2, 65535 * 8 + 3 events that repeat 97 distinct rows, four levels: the last three events
    are the second launch of the search.  The distinct rows against the restatement, every event against its row."""
    import torch
    tt, rows_p, rows_w, rows_d = Cs.cap_case()
    E, period = Cs.CAP_E, Cs.CAP_P
    assert E - Cs.CAP == 3
    _, rows_m, _, _ = Cs.locate_rows(tt, rows_p, rows_w)
    picks, w, m, delta = (Cs.periodic(a, E) for a in (rows_p, rows_w, rows_m, rows_d))
    with P.TravelTimeSolver(Cs.CAP_SHAPE, star818(P)) as sol:
        got = host(sol.locate_confidence(torch.from_numpy(tt).to(dev()), picks, w, m, delta))
    assert_same({f: v[:period] for f, v in got.items()}, Cs.confidence(tt, rows_p, rows_w, rows_m, rows_d), "rows")
    first = np.arange(E) % period
    assert_same(got, {f: v[first] for f, v in got.items()}, "every event against its row")
    assert np.all(got["count"][-3:, 0] >= 1)


def test_regions_on_a_grid_of_many_tiles(P):
    """17 x 59 x 4095 (1003 tiles, the last partial): six rows of the planted case, among them the minimum at the
    last cell, the tie of one cell in every tile and an unplanted row; levels 0, 0.5 (the decoy), 4.5 (the cells
    planted for the neighbouring rows) and +inf."""
    rows = (1, 7, 14, 16, 17, 50)
    tt = np.array(Cs.big_box())
    picks = Cs.big_rows("unit")[0][list(rows)]
    ref = Cs.big_reference("unit", rows)
    m = np.array([ref[r][1] for r in rows])
    with P.TravelTimeSolver(Cs.BIG_SHAPE, star818(P)) as sol:
        got = check_regions(sol, tt, picks, None, m, np.tile([0.0, 0.5, 4.5, np.inf], (len(rows), 1)), "big")
    assert got["count"][:, 0].tolist() == [ref[r][5] for r in rows] and got["count"][4, 0] == 1003
    assert np.all(got["count"][:, 3] == tt[0].size) and np.all(got["count"][:5, 2] > got["count"][:5, 1])


@pytest.mark.parametrize("N", sorted(Cs.N_SHAPES))
def test_full_and_just_over_full_register_widths(P, N):
    """K in 1, 2, 7 ... 33 around every register instance on a grid of N cells with all three axes in play: the
    weighted events of every pattern and the events with weights NULL, levels 0, a sparse one and +inf at the
    restatement's minimum."""
    with P.TravelTimeSolver(Cs.N_SHAPES[N], star818(P)) as sol:
        for K in Cs.K_EDGES:
            c = Cs.k_edge_case(K, N)
            for call in ("weighted", "none"):
                d = c[call]
                got = check_regions(sol, c["tt"], d["picks"], d["weights"], d["m"], d["delta"], f"K={K} N={N} {call}")
                assert np.all(got["count"][:, 0] >= 1)


@pytest.mark.parametrize("route", Cs.RANGE_ROUTES)
def test_double_range_of_picks_and_weights(P, route):
    tt, picks, w = Cs.range_case(route)
    _, m, _, _ = Cs.locate_rows(tt, picks, w)
    delta = np.tile([0.0, 1.0, 1e300, np.inf], (len(picks), 1))
    with P.TravelTimeSolver(Cs.RANGE_SHAPE, star818(P)) as sol:
        got = check_regions(sol, tt, picks, w, m, delta, route)
        assert np.all((got["count"][:, 0] >= 1) == (m < np.inf))
        check_regions(sol, tt, picks, w, np.zeros(len(picks)), delta, route + ", m = 0")


@pytest.mark.parametrize("name", Cs.CONF_RANGE_CASES)
def test_double_range_of_levels(P, name):
    """m + delta at the largest finite double (exactly and by rounding), in the subnormal range, and one ulp below,
    at and one ulp above the J of a cell."""
    tt, picks, w, m, delta = Cs.conf_range_case(name)
    assert R.check(m, delta) is None
    with P.TravelTimeSolver(Cs.RANGE_SHAPE, star818(P)) as sol:
        check_regions(sol, tt, picks, w, m, delta, name)
