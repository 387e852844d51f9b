"""GPU tier (-m gpu): both ends of the float range, bit for bit against the reference's fixed points recorded in
tests/golden/float_range.npz (make_golden.py --float-range; the CPU pins are in test_float_range_cpu.py) and
against the CPU oracle, on every kernel and schedule.

  * travel times that overflow partway across the grid: the reference never stops there (INFINITY stored over
    INFINITY, serial_new/sweep-tt-multistart.c:228-237); the library returns the boxes it stands still at, then 0;
  * delays whose product d (v[c] + v[o]) overflows while d / 2 times the sum does not, and infinite pair sums:
    such volumes (v >= 2^126 / d_max) go to the per-cell kernel's instance that rounds as the reference does;
  * a star length whose half is not a float (subnormal, odd last bit), and two parallel entries one subnormal
    step apart: that instance, multiplying by d itself, for every volume;
  * lengths from delta = 0.37 and 2500 on the fast kernels.

Every solve runs with a sweep cap and a wait limit, so a schedule that never comes to rest fails quickly."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_equal
from tile_cases import tile_supports

pytestmark = pytest.mark.gpu

F32 = np.float32
FAIL_FAST = {"OPT_MAX_SWEEPS": 3000, "OPT_ASYNC_TIMEOUT_MILLI": 30000}

# kernel / schedule -> (options, the kernel_variant it reports on the fast path, one launch per solve)
SCHEDULES = {
    "cell": ({"OPT_KERNEL": 1}, 1, False),
    "strip1": ({"OPT_KERNEL": 2, "OPT_PAIR_MIN_STARTS": 1 << 20, "OPT_ASYNC": 1}, 2, True),
    "strip2": ({"OPT_KERNEL": 2, "OPT_PAIR_MIN_STARTS": 0, "OPT_ASYNC": 1}, 2, True),
    "strip1-passes": ({"OPT_KERNEL": 2, "OPT_PAIR_MIN_STARTS": 1 << 20, "OPT_ASYNC": 0}, 2, False),
    "strip2-passes": ({"OPT_KERNEL": 2, "OPT_PAIR_MIN_STARTS": 0, "OPT_ASYNC": 0}, 2, False),
    "tile": ({"OPT_KERNEL": 3}, 3, None),
    "tile-columns-padded": ({"OPT_KERNEL": 3, "OPT_TILE_IN_PLACE": 0}, 3, None),
    "tile-hyperplane-launches": ({"OPT_KERNEL": 3, "OPT_ASYNC": 0}, 3, False),
}


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


FR = np.load(os.path.join(GOLDEN, "float_range.npz"))
FR_META = json.loads(bytes(FR["meta"]).decode())


def star_of(z, key, m, make):
    fs = make(z[f"star_{m['star']}"], F32(np.uint32(m["delta_bits"]).view(F32)))
    if m["hand_made_d"]:
        fs["d"] = z[f"fsd_{key}"].view(F32)
    return fs


def solver(P, shape, fs, options):
    sol = P.TravelTimeSolver(shape, fs)
    for k, val in {**FAIL_FAST, **options}.items():
        sol.set_option(getattr(P, k), val)
    return sol


def exact_instance(v, fs):
    """The library's rule (ttsweep_set_velocity_device): the per-cell kernel's reference-rounding instance for a
    star with a live length whose half is not a float, or a volume with 0 < v < min(2^-124 / d_min, 1e30) or a
    finite v >= 2^126 / d_max."""
    d = fs["d"][:len(fs) - 1]
    if np.any((d * F32(0.5)) * F32(2) != d):
        return True
    pos = d[d > 0]
    if not len(pos):
        return False
    tiny = min(2.0 ** -124 / float(pos.min()), 1e30)
    huge = 2.0 ** 126 / float(pos.max())
    vv = v.astype(np.float64)
    return bool(np.any((vv > 0) & (vv < float(F32(tiny)))) or np.any(vv >= float(F32(huge))))


def boxes_for(shape, starts):
    out = []
    for st in starts:
        tt = np.full(shape, np.inf, dtype=F32)
        tt[tuple(st)] = 0
        out.append(tt)
    return out


def schedule_cases():
    """(schedule, case) pairs: TILE with the stars it accepts, its column drivers with the 6-neighbour star."""
    out = []
    for schedule, (_, variant, _) in SCHEDULES.items():
        for key, m in FR_META.items():
            if variant == 3 and not tile_supports(FR[f"star_{m['star']}"]):
                continue
            if schedule.startswith("tile-") and m["star"] != "six":
                continue
            out.append(pytest.param(schedule, key, id=f"{schedule}-{key}"))
    return out


@pytest.mark.parametrize("schedule,key", schedule_cases())
def test_float_range_cases_bit_exact(P, oracle, schedule, key):
    """Every recorded case on this kernel / schedule: the reference's boxes bit for bit (and the oracle's), a fresh
    solve returns 1 and a solve of the converged boxes 0 - the confirming call on the same context and a fresh
    context that does the device work - with ttsweep_get_changed agreeing; the kernel the routing rule names (and
    one launch without fallback where the schedule is one launch); the device validator and torch_checker report
    rest; the next ordinary volume gets the chosen kernel back."""
    import torch
    from torch_checker import fixed_point_counts
    options, variant, one_launch = SCHEDULES[schedule]
    z, m = FR, FR_META[key]
    dev = torch.device("cuda:0")
    v = z[f"v_{m['case']}"]
    starts = np.array(m["starts"], np.int32)
    nstart = len(starts)
    fs = star_of(z, key, m, P.inputs.make_fs)
    assert np.array_equal(fs["d"].view(np.uint32), z[f"fsd_{key}"]), key
    exact = exact_instance(v, fs)
    want = z[f"tt_{key}"]
    ofs = star_of(z, key, m, oracle.make_star)
    for s, st in enumerate(starts):
        o, _, _ = oracle.converge(v, ofs, st, order=1)
        assert_bit_equal(o, want[s], f"{key} start {st}: oracle")
    what = f"{key} ({schedule})"
    with solver(P, v.shape, fs, options) as sol:
        sol.set_velocity(v)
        tts = boxes_for(v.shape, starts)
        # (a start inside a block of infinite pair sums keeps its initial box: nothing improves)
        improved = [int(not np.array_equal(b.view(np.uint32), w.view(np.uint32))) for b, w in zip(tts, want)]
        assert sol.solve(starts, tts) == max(improved), what
        assert sol.changed(nstart) == improved, what
        stt = sol.stats()
        assert stt["kernel_variant"] == (1 if exact else variant), (what, stt["kernel_variant"])
        if not exact and one_launch is not False:
            if one_launch or m["star"] == "six":     # (TILE: the six-star column pipelines are one launch)
                assert stt["launches"] == 1 and stt["fallbacks"] == 0, (what, stt["launches"], stt["fallbacks"])
        for s in range(nstart):
            assert_bit_equal(tts[s], want[s], f"{what} start {starts[s]}")
        # the confirming call of a reference-style driver
        assert sol.solve(starts, tts) == 0 and sol.changed(nstart) == [0] * nstart, what
        for s in range(nstart):
            assert_bit_equal(tts[s], want[s], f"{what} start {starts[s]}, confirming call")
        # validators on the device
        tv = torch.from_numpy(v).to(dev)
        for s in range(nstart):
            box = torch.from_numpy(want[s].copy()).to(dev)
            rest = (0, m["ninf"][s], 0)
            assert sol.validate_device(starts[s], box) == rest, (what, starts[s])
            assert fixed_point_counts(tv, box, fs, starts[s]) == rest, (what, starts[s])
        if exact and not m["hand_made_d"] and not m["case"].startswith("odd_delta"):
            ordinary = (v.astype(np.float64) * 0 + 0.25).astype(F32)
            sol.set_velocity(ordinary)
            back = boxes_for(v.shape, starts[:1])
            assert sol.solve(starts[:1], back) == 1 and sol.stats()["kernel_variant"] == variant, what
            w, _, _ = oracle.converge(ordinary, ofs, starts[0], order=1)
            assert_bit_equal(back[0], w, f"{what}: back on the chosen kernel")
    # a fresh context, boxes in device memory: the device work finds nothing to change
    with solver(P, v.shape, fs, options) as sol:
        sol.set_velocity(v)
        tt = torch.from_numpy(want.copy()).to(dev)
        assert sol.solve_device(starts, tt, init=False) == 0, what
        assert sol.changed(nstart) == [0] * nstart and sol.stats()["sweeps_total"] > 0, what
        assert torch.equal(tt.view(torch.int32), torch.from_numpy(want.copy()).to(dev).view(torch.int32)), what
        # ... and the same context from the initial state, device-initialised
        assert sol.solve_device(starts, tt, init=True) == max(improved), what
        assert sol.changed(nstart) == improved, what
        got = tt.cpu().numpy()
        for s in range(nstart):
            assert_bit_equal(got[s], want[s], f"{what} start {starts[s]}, device boxes")


def test_every_schedule_meets_every_case():
    assert len(FR_META) == 24 and len(schedule_cases()) == 5 * 24 + 9 + 3 * 8


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -float("inf")])
def test_create_refuses_a_bad_live_length(P, bad):
    """ttsweep_create checks every live fs[].d: finite and >= 0 (a negative length makes a negative delay, for
    which the relaxation has no least fixed point; inf and NaN make NaN delays).  The entry the exclusive bound
    leaves out is not checked."""
    offs = P.inputs.read_triples(P.inputs.star_path("six"))
    fs = P.inputs.make_fs(offs)
    fs["d"][2] = bad
    with pytest.raises(P.TTSweepError, match="length"):
        P.TravelTimeSolver((8, 7, 6), fs)
    fs = P.inputs.make_fs(offs)
    fs["d"][-1] = bad                                   # (not live: starstop = len - 1)
    with P.TravelTimeSolver((8, 7, 6), fs) as sol:
        sol.set_velocity(np.full((8, 7, 6), 0.25, F32))
        assert sol.solve(np.array([[1, 2, 3]], np.int32), boxes_for((8, 7, 6), [[1, 2, 3]])) == 1


FULL_STARS = [pytest.param("818", 1, 1.5e36, id="818-1start"), pytest.param("818", 3, 1.5e36, id="818-3starts"),
              pytest.param("six", 2, 1.0e36, id="six-columns")]


@pytest.mark.parametrize("sname,nstart,scale", FULL_STARS)
def test_full_size_with_overflowing_travel_times(P, oracle, sname, nstart, scale):
    """241x241x51 under the default kernel choice, device-resident, velocities of the BASELINE model scaled so
    that a good part of every box overflows to INFINITY (yet below 2^126 / d_max: the fast kernels stay): one
    launch without fallback, the per-cell kernel's boxes bit for bit, torch_checker and the device validator at
    rest; six-FS also against the oracle."""
    import torch
    from torch_checker import fixed_point_counts
    shape = (241, 241, 51)
    v = (P.inputs.velocity_model(*shape, 20160507).astype(np.float64) * scale).astype(F32)
    offs = P.inputs.read_triples(P.inputs.star_path(sname))
    fs = P.inputs.make_fs(offs)
    assert not exact_instance(v, fs)
    starts = np.array([[120, 120, 50], [151, 19, 0], [34, 75, 0]][:nstart], np.int32)
    dev = torch.device("cuda:0")
    with solver(P, shape, fs, {}) as sol:
        sol.set_velocity(torch.from_numpy(v).to(dev))
        tt = torch.empty((nstart,) + shape, dtype=torch.float32, device=dev)
        assert sol.solve_device(starts, tt, init=True) == 1
        st = sol.stats()
        assert st["kernel_variant"] == (3 if sname == "six" else 2)
        assert st["launches"] == 1 and st["fallbacks"] == 0, (st["launches"], st["fallbacks"])
        assert sol.changed(nstart) == [1] * nstart
        tv = torch.from_numpy(v).to(dev)
        for s in range(nstart):
            ninf = int(torch.isinf(tt[s]).sum().item())
            assert 0.05 * v.size < ninf < 0.95 * v.size, (s, ninf / v.size)
            assert sol.validate_device(starts[s], tt[s]) == (0, ninf, 0), s
            assert fixed_point_counts(tv, tt[s], fs, starts[s]) == (0, ninf, 0), s
        again = tt.clone()
        assert sol.solve_device(starts, again, init=False) == 0
        assert torch.equal(again.view(torch.int32), tt.view(torch.int32))
    with solver(P, shape, fs, {"OPT_KERNEL": 1}) as cell:
        cell.set_velocity(torch.from_numpy(v).to(dev))
        want = torch.empty((nstart,) + shape, dtype=torch.float32, device=dev)
        assert cell.solve_device(starts, want, init=True) == 1
    got = tt.cpu().numpy()
    for s in range(nstart):
        assert_bit_equal(got[s], want[s].cpu().numpy(), f"{sname} start {starts[s]}: default kernel vs CELL")
    if sname == "six":
        for s in range(nstart):
            o, _, _ = oracle.converge(v, oracle.make_star(offs), starts[s], order=1)
            assert_bit_equal(got[s], o, f"six start {starts[s]}: oracle")
