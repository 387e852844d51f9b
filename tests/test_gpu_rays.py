"""GPU tier (-m gpu) of the ray calls (include/ttsweep.h, "rays"): ttsweep_predecessors_device and
ttsweep_trace_rays_device through TravelTimeSolver.predecessors / trace_rays, every case bit for bit against the
numpy restatement tests/ray_reference.py, and the replay of every OK / SEED ray ending at exactly its receiver's
time."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, Golden
import ray_reference as R

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


def dev():
    import torch
    return torch.device("cuda:0")


def all_cells(shape):
    return np.argwhere(np.ones(shape, bool)).astype(np.int32)


def check_box_rays(P, sol, v, fs, starts, tts, lo, hi, receivers=None, what=""):
    """pred and the rays from every cell (or `receivers`) of the boxes tts [nstart, ...] against the reference;
    returns (pred, rays)."""
    import torch
    starts = np.asarray(starts, np.int32).reshape(-1, 3)
    tt = torch.from_numpy(np.ascontiguousarray(tts, dtype=F32)).to(dev())
    pred = sol.predecessors(starts, tt)
    assert pred.dtype == torch.int32 and pred.shape == tt.shape and pred.device == tt.device
    got = pred.cpu().numpy()
    recv = all_cells(v.shape) if receivers is None else receivers
    rays = sol.trace_rays(starts, tt, recv, pred)
    n = len(recv)
    for s, st in enumerate(starts):
        want = R.predecessors(v, tts[s], fs, st, lo, hi)
        assert np.array_equal(got[s], want), f"{what} start {st}: pred differs at {np.argwhere(got[s] != want)[:5]}"
        offsets, cells, hop_d, status, t_recv = R.trace(v, tts[s], want, fs, st, recv, lo, hi)
        o = rays.offsets.numpy()[s * n:(s + 1) * n + 1]
        assert np.array_equal(o - o[0], offsets), what
        assert np.array_equal(rays.status.numpy()[s * n:(s + 1) * n], status), what
        assert np.array_equal(rays.t_recv.numpy()[s * n:(s + 1) * n].view(np.uint32), t_recv.view(np.uint32)), what
        assert np.array_equal(rays.cells[o[0]:o[-1]].cpu().numpy(), cells), what
        assert np.array_equal(rays.hop_d[o[0]:o[-1]].cpu().numpy().view(np.uint32), hop_d.view(np.uint32)), what
        end = R.replay(v, tts[s], offsets, cells, hop_d)
        ok = (status == R.RAY_OK) | (status == R.RAY_SEED)
        assert np.array_equal(end[ok].view(np.uint32), t_recv[ok].view(np.uint32)), what
    return got, rays


def golden_boxes():
    out = []
    for name in ("g24", "g9"):
        g = Golden(name)
        for key, sname, offs, start, tt, _ in g.cases():
            out.append((f"{name}/{key}", name, offs, start, tt, 0, len(offs) - 1))
        m = g.meta["3_range_5_60"]
        out.append((f"{name}/3_range_5_60", name, g.star("3"), m["start"], g.z["tt_3_range_5_60"], 5, 60))
    return out


GOLDEN_BOXES = golden_boxes()


@pytest.mark.parametrize("case", GOLDEN_BOXES, ids=[c[0] for c in GOLDEN_BOXES])
def test_golden_boxes_pred_and_rays(P, case):
    """Every recorded box uploaded as the reference left it, every star range the fixtures carry: pred and the
    rays from every cell equal the reference's, all OK, replay bit-exact."""
    key, name, offs, start, tt, lo, hi = case
    v = Golden(name).v
    fs = P.inputs.make_fs(offs)
    with P.TravelTimeSolver(v.shape, fs, lo, hi) as sol:
        sol.set_velocity(v)
        pred, rays = check_box_rays(P, sol, v, fs, [start], tt[None], lo, hi, what=key)
    assert not np.any(pred == P.PRED_SEED)
    assert np.all(rays.status.numpy() == P.RAY_OK)


FR = np.load(os.path.join(GOLDEN, "float_range.npz"))
FR_META = json.loads(bytes(FR["meta"]).decode())


@pytest.mark.parametrize("key", sorted(FR_META))
def test_float_range_pred_and_rays(P, key):
    """Overflowing and INFINITY cells (UNREACHED), subnormal and huge volumes (the exact delay), duplicate offsets
    (the hop_d tie-break): every box of every case, rays from every cell."""
    m = FR_META[key]
    v = FR[f"v_{m['case']}"]
    fs = P.inputs.make_fs(FR[f"star_{m['star']}"], F32(np.uint32(m["delta_bits"]).view(F32)))
    if m["hand_made_d"]:
        fs["d"] = FR[f"fsd_{key}"].view(F32)
    starts = np.array(m["starts"], np.int32)
    want = FR[f"tt_{key}"]
    with P.TravelTimeSolver(v.shape, fs) as sol:
        sol.set_velocity(v)
        pred, rays = check_box_rays(P, sol, v, fs, starts, want, 0, len(fs) - 1, what=key)
    for s in range(len(starts)):
        assert np.count_nonzero(pred[s] == P.PRED_UNREACHED) == m["ninf"][s], key
    if m["case"] == "dup_offset":        # (hop_d equal to the reference's: the smaller of the parallel lengths)
        assert np.all(rays.status.numpy() == P.RAY_OK)


def solver_for(P, v, fs):
    sol = P.TravelTimeSolver(v.shape, fs)
    sol.set_velocity(v)
    return sol


def test_seeded_box_rays_end_at_the_seeds(P):
    """A box solved from the caller's state (init = 0) with two extra finite sources: the seeds are SEED cells and
    the rays that reach them end there with status SEED."""
    import torch
    g = Golden("g24")
    v = g.v
    offs = g.star("5")
    fs = P.inputs.make_fs(offs)
    start = np.array([12, 10, 6], np.int32)
    seeds = [(2, 3, 1), (21, 17, 10)]
    box = np.full(v.shape, np.inf, F32)
    box[tuple(start)] = 0
    for p in seeds:
        box[p] = F32(0.5)
    with solver_for(P, v, fs) as sol:
        tt = torch.from_numpy(box[None].copy()).to(dev())
        assert sol.solve_device([start], tt, init=False) == 1
        solved = tt.cpu().numpy()
        pred, rays = check_box_rays(P, sol, v, fs, [start], solved, 0, len(fs) - 1, what="seeded")
    flat = lambda p: R.flat_index(v.shape, p)
    for p in seeds:
        assert pred[0].reshape(-1)[flat(p)] == P.PRED_SEED
    status = rays.status.numpy()
    assert np.count_nonzero(status == P.RAY_SEED) > 0 and np.count_nonzero(status == P.RAY_OK) > 0
    offsets, cells = rays.offsets.numpy(), rays.cells.cpu().numpy()
    first = cells[offsets[:-1][status == P.RAY_SEED]]
    assert set(first.tolist()) <= {flat(p) for p in seeds}


def test_zero_velocity_slab_reports_seed(P):
    """A slab of zero velocity: zero delays make plateaus of equal travel times, whose cells other than the entry
    have no strictly smaller neighbour - SEED, reported without any hang."""
    import torch
    g = Golden("g24")
    v = g.v.copy()
    v[:, 8:11, :] = 0
    fs = P.inputs.make_fs(g.star("3"))
    start = np.array([5, 2, 3], np.int32)
    with solver_for(P, v, fs) as sol:
        tt = torch.empty((1,) + v.shape, dtype=torch.float32, device=dev())
        assert sol.solve_device([start], tt, init=True) == 1
        pred, rays = check_box_rays(P, sol, v, fs, [start], tt.cpu().numpy(), 0, len(fs) - 1, what="zero slab")
    assert np.count_nonzero(pred == P.PRED_SEED) > 0
    assert np.count_nonzero(rays.status.numpy() == P.RAY_SEED) > 0


def test_bad_pred_gives_invalid_rays(P):
    """A hand-made pred: out of range, pointing uphill, a cycle onto itself, a SOURCE away from the start, an
    UNREACHED mark on a finite cell, and a lower cell that is no predecessor (as the reference judges it).  Rays through them are INVALID (and carry no
    cells), the others unchanged."""
    import torch
    g = Golden("g9")
    key = "818_mid"
    v, tt, start = g.v, g.z[f"tt_{key}"], g.z[f"start_{key}"]
    fs = P.inputs.make_fs(g.star("818"))
    good = R.predecessors(v, tt, fs, start)
    bad = good.copy().reshape(-1)
    N = bad.size
    order = np.argsort(tt.reshape(-1))
    far = order[-6:]                                    # the six latest cells: rays from them pass nowhere else
    bad[far[0]] = N + 5
    bad[far[1]] = far[2]                                # T[far[2]] >= T[far[1]]: not strictly decreasing
    bad[far[2]] = far[2]
    bad[far[3]] = P.PRED_SOURCE
    bad[far[4]] = P.PRED_UNREACHED
    bad[far[5]] = order[1]                              # a lower cell, but not through an edge whose candidate is T
    bad = bad.reshape(tt.shape)
    with solver_for(P, v, fs) as sol:
        t = torch.from_numpy(tt[None].copy()).to(dev())
        p = torch.from_numpy(bad[None].copy()).to(dev())
        recv = all_cells(v.shape)
        rays = sol.trace_rays([start], t, recv, p)
    offsets, cells, hop_d, status, t_recv = R.trace(v, tt, bad, fs, start, recv)
    assert np.array_equal(rays.status.numpy(), status)
    assert np.array_equal(rays.offsets.numpy(), offsets)
    assert np.array_equal(rays.cells.cpu().numpy(), cells)
    flat = [R.flat_index(v.shape, q) for q in recv]
    for c in far[:5]:
        assert status[flat.index(int(c))] == P.RAY_INVALID, c
    assert np.count_nonzero(status == P.RAY_OK) >= len(recv) - 6 - 10


def test_batched_calls_equal_single_calls(P):
    """Four boxes in one predecessors / trace_rays call give what four calls of one box give."""
    import torch
    g = Golden("g24")
    keys = ["818_mid", "818_corner", "818_deadin", "818_deadout"]
    starts = np.array([g.z[f"start_{k}"] for k in keys], np.int32)
    boxes = np.stack([g.z[f"tt_{k}"] for k in keys])
    fs = P.inputs.make_fs(g.star("818"))
    recv = all_cells(g.v.shape)[::5]
    with solver_for(P, g.v, fs) as sol:
        tt = torch.from_numpy(boxes).to(dev())
        pred = sol.predecessors(starts, tt)
        rays = sol.trace_rays(starts, tt, recv, pred)
        n = len(recv)
        for s in range(len(keys)):
            one = sol.predecessors(starts[s:s + 1], tt[s:s + 1].contiguous())
            assert torch.equal(one[0], pred[s]), keys[s]
            r1 = sol.trace_rays(starts[s:s + 1], tt[s:s + 1].contiguous(), recv)
            o = rays.offsets.numpy()[s * n:(s + 1) * n + 1]
            assert np.array_equal(o - o[0], r1.offsets.numpy())
            assert np.array_equal(rays.status.numpy()[s * n:(s + 1) * n], r1.status.numpy())
            assert torch.equal(rays.cells[o[0]:o[-1]], r1.cells)
            assert torch.equal(rays.hop_d[o[0]:o[-1]].view(torch.int32), r1.hop_d.view(torch.int32))


def test_solve_predecessors_solve_keeps_the_shortcut(P):
    """solve -> predecessors -> trace_rays -> solve of the same host boxes: the last solve is still the confirming
    pass answered with 0 without device work."""
    import torch
    g = Golden("g24")
    fs = P.inputs.make_fs(g.star("818"))
    starts = np.array([g.z["start_818_mid"], g.z["start_818_corner"]], np.int32)
    boxes = []
    for st in starts:
        b = np.full(g.v.shape, np.inf, F32)
        b[tuple(st)] = 0
        boxes.append(b)
    with solver_for(P, g.v, fs) as sol:
        assert sol.solve(starts, boxes) == 1
        sweeps = sol.stats()["sweeps_total"]
        assert sweeps > 0
        tt = torch.from_numpy(np.stack(boxes)).to(dev())
        pred = sol.predecessors(starts, tt)
        sol.trace_rays(starts, tt, all_cells(g.v.shape)[::9], pred)
        assert sol.solve(starts, boxes) == 0
        assert sol.stats()["sweeps_total"] == 0
        assert sol.changed(2) == [0, 0]


def test_full_size_rays_from_every_surface_cell(P):
    """241x241x51, 818-FS, the 24 BASELINE starts solved on the device; pred of all 24 boxes and the rays from
    every surface cell (z = 0): 1.39 M rays, all OK; replay on the device bit-exact for every ray; the Frechet rows
    reproduce t_recv within 1e-5; pred of 10 000 random cells equals the reference's, minimal index included."""
    import torch
    shape = (241, 241, 51)
    v = P.inputs.velocity_model(*shape, 20160507)
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))
    starts = P.inputs.read_triples(P.inputs.starts_path("24"))
    assert len(starts) == 24
    d = dev()
    with P.TravelTimeSolver(shape, fs) as sol:
        vd = torch.from_numpy(v).to(d)
        sol.set_velocity(vd)
        tt = torch.empty((24,) + shape, dtype=torch.float32, device=d)
        assert sol.solve_device(starts, tt, init=True) == 1
        pred = sol.predecessors(starts, tt)
        surf = np.argwhere(np.ones(shape[:2], bool))
        recv = np.concatenate([surf, np.zeros((len(surf), 1), np.int64)], axis=1).astype(np.int32)
        rays = sol.trace_rays(starts, tt, recv, pred)
    nrays = 24 * len(recv)
    assert len(rays) == nrays == 24 * 241 * 241
    assert torch.all(rays.status == P.RAY_OK)
    offsets = rays.offsets.to(d)
    counts = offsets[1:] - offsets[:-1]
    box = torch.arange(nrays, device=d) // len(recv)
    T = tt.reshape(24, -1)
    vf = vd.reshape(-1)
    cells = rays.cells.to(torch.int64)
    assert torch.all(cells[offsets[:-1]] == torch.from_numpy(
        np.array([R.flat_index(shape, s) for s in starts])).to(d)[box])
    # replay: t = fl(fl(fl(d * (v[a] + v[b])) / 2.0) + t), hop by hop, on the device
    t = T[box, cells[offsets[:-1]]].clone()
    for h in range(int(counts.max().item()) - 1):
        r = torch.nonzero(counts > h + 1).flatten()
        g = offsets[r] + h
        p = (rays.hop_d[g] * (vf[cells[g]] + vf[cells[g + 1]])).to(torch.float64) / 2.0
        t[r] = p.to(torch.float32) + t[r]
    t_recv = rays.t_recv.to(d)
    assert torch.equal(t.view(torch.int32), t_recv.view(torch.int32))
    G = P.rays_to_frechet(rays, shape)
    gv = torch.sparse.mm(G, vd.reshape(-1, 1).to(torch.float64)).flatten()
    rel = (gv - t_recv.to(torch.float64)).abs() / t_recv.to(torch.float64).abs()
    assert float(rel.max()) <= 1e-5
    rng = np.random.default_rng(7)
    for s in rng.choice(24, 4, replace=False):
        pick = np.stack([rng.integers(0, n, 2500) for n in shape], axis=1)
        box_s = tt[s].cpu().numpy()
        want = R.predecessors_at(v, box_s, fs, starts[s], pick)
        got = pred[s].cpu().numpy()[pick[:, 0], pick[:, 1], pick[:, 2]]
        assert np.array_equal(got, want), (s, np.argwhere(got != want)[:5])
