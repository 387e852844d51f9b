"""GPU tier (-m gpu) of the ray Frechet operators (include/ttsweep.h, "rays: the Frechet operators"):
ttsweep_ray_forward_device / ttsweep_ray_adjoint_device through TravelTimeSolver.frechet_operator, bit for bit
against the numpy restatement tests/ray_operator_reference.py on every case the ray tests cover, deterministic
from call to call, the adjoint of the forward, and the full-size workload against the explicit
trace_rays + rays_to_frechet path."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, Golden
import ray_operator_reference as O
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


def weights(rng, n):
    w = rng.standard_normal(n)
    w[rng.random(n) < 0.15] = 0.0
    w[rng.random(n) < 0.1] *= 2.0 ** -40
    return w


def check_operators(P, sol, v, fs, starts, tts, lo, hi, receivers=None, preds=None, what=""):
    """forward, adjoint, hits, status and t_recv of the operator of the boxes tts [nstart, ...] (rays from every
    cell, or `receivers`) equal to the restatement's, bit for bit; returns (op, reference rays)."""
    import torch
    starts = np.asarray(starts, np.int32).reshape(-1, 3)
    tt = torch.from_numpy(np.ascontiguousarray(tts, dtype=F32)).to(dev())
    recv = all_cells(v.shape) if receivers is None else receivers
    pred = None if preds is None else torch.from_numpy(np.ascontiguousarray(preds)).to(dev())
    op = sol.frechet_operator(starts, tt, recv, pred)
    offsets, cells, hop_d, status, t_recv = O.rays_of_boxes(v, tts, fs, starts, recv, lo, hi, preds)
    nrays, ncells = len(starts) * len(recv), v.size
    assert op.shape == (nrays, ncells), what
    assert np.array_equal(op.status.numpy(), status), what
    assert np.array_equal(op.t_recv.numpy().view(np.uint32), t_recv.view(np.uint32)), what
    rng = np.random.default_rng(len(what) + nrays)
    m = rng.uniform(0.5, 2.0, ncells)
    y = op.matvec(torch.from_numpy(m.reshape(v.shape)).to(dev()))
    assert y.dtype == torch.float64 and y.shape == (nrays,)
    want = O.forward(offsets, cells, hop_d, m)
    assert np.array_equal(y.cpu().numpy().view(np.uint64), want.view(np.uint64)), what
    w = weights(rng, nrays)
    g = op.rmatvec(torch.from_numpy(w).to(dev()))
    assert g.dtype == torch.float64 and tuple(g.shape) == v.shape
    gw, S = O.adjoint(offsets, cells, hop_d, w, ncells, O.entries_dmax(fs, v.shape, lo, hi))
    assert op.last_scale == S, what
    assert np.array_equal(g.cpu().numpy().reshape(-1).view(np.uint64), gw.view(np.uint64)), what
    h = op.hits()
    assert h.dtype == torch.int32 and tuple(h.shape) == v.shape
    assert np.array_equal(h.cpu().numpy().reshape(-1), O.hits(cells, ncells)), what
    return op, (offsets, cells, hop_d, status, t_recv)


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
def test_golden_boxes_operators(P, case):
    key, name, offs, start, tt, lo, hi = case
    v = Golden(name).v
    fs = P.inputs.make_fs(offs)
    with P.TravelTimeSolver(v.shape, fs, lo, hi) as sol:
        sol.set_velocity(v)
        op, _ = check_operators(P, sol, v, fs, [start], tt[None], lo, hi, what=key)
    assert np.all(op.status.numpy() == P.RAY_OK)


FR = np.load(os.path.join(GOLDEN, "float_range.npz"))
FR_META = json.loads(bytes(FR["meta"]).decode())


@pytest.mark.parametrize("key", sorted(FR_META))
def test_float_range_operators(P, key):
    m = FR_META[key]
    v = FR[f"v_{m['case']}"]
    fs = P.inputs.make_fs(FR[f"star_{m['star']}"], F32(np.uint32(m["delta_bits"]).view(F32)))
    if m["hand_made_d"]:
        fs["d"] = FR[f"fsd_{key}"].view(F32)
    starts = np.array(m["starts"], np.int32)
    with P.TravelTimeSolver(v.shape, fs) as sol:
        sol.set_velocity(v)
        check_operators(P, sol, v, fs, starts, FR[f"tt_{key}"], 0, len(fs) - 1, what=key)


def solver_for(P, v, fs):
    sol = P.TravelTimeSolver(v.shape, fs)
    sol.set_velocity(v)
    return sol


def test_seeded_box_operators(P):
    """SEED rays contribute the hops they walk."""
    import torch
    g = Golden("g24")
    v = g.v
    fs = P.inputs.make_fs(g.star("5"))
    start = np.array([12, 10, 6], np.int32)
    box = np.full(v.shape, np.inf, F32)
    box[tuple(start)] = 0
    for p in [(2, 3, 1), (21, 17, 10)]:
        box[p] = F32(0.5)
    with solver_for(P, v, fs) as sol:
        tt = torch.from_numpy(box[None].copy()).to(dev())
        assert sol.solve_device([start], tt, init=False) == 1
        solved = tt.cpu().numpy()
        op, _ = check_operators(P, sol, v, fs, [start], solved, 0, len(fs) - 1, what="seeded")
    assert np.count_nonzero(op.status.numpy() == P.RAY_SEED) > 0


def test_zero_velocity_slab_operators(P):
    import torch
    g = Golden("g24")
    v = g.v.copy()
    v[:, 8:11, :] = 0
    fs = P.inputs.make_fs(g.star("3"))
    start = np.array([5, 2, 3], np.int32)
    with solver_for(P, v, fs) as sol:
        tt = torch.empty((1,) + v.shape, dtype=torch.float32, device=dev())
        assert sol.solve_device([start], tt, init=True) == 1
        op, _ = check_operators(P, sol, v, fs, [start], tt.cpu().numpy(), 0, len(fs) - 1, what="zero slab")
    assert np.count_nonzero(op.status.numpy() == P.RAY_SEED) > 0


def test_bad_pred_invalid_rays_contribute_nothing(P):
    g = Golden("g9")
    key = "818_mid"
    v, tt, start = g.v, g.z[f"tt_{key}"], g.z[f"start_{key}"]
    fs = P.inputs.make_fs(g.star("818"))
    bad = R.predecessors(v, tt, fs, start).reshape(-1)
    N = bad.size
    order = np.argsort(tt.reshape(-1))
    far = order[-6:]
    bad[far[0]] = N + 5
    bad[far[1]] = far[2]
    bad[far[2]] = far[2]
    bad[far[3]] = P.PRED_SOURCE
    bad[far[4]] = P.PRED_UNREACHED
    bad[far[5]] = order[1]
    bad = bad.reshape(tt.shape)
    with solver_for(P, v, fs) as sol:
        op, ref = check_operators(P, sol, v, fs, [start], tt[None], 0, len(fs) - 1, preds=bad[None],
                                  what="bad pred")
    status = op.status.numpy()
    assert np.count_nonzero(status == P.RAY_INVALID) >= 5


def test_adjoint_is_deterministic_and_the_adjoint_of_forward(P):
    """Two adjoint calls are bit-identical; <G m, w> = <m, G^T w> within the fixed-point bound."""
    import torch
    g = Golden("g24")
    keys = ["818_mid", "818_corner", "818_deadin", "818_deadout"]
    starts = np.array([g.z[f"start_{k}"] for k in keys], np.int32)
    boxes = np.stack([g.z[f"tt_{k}"] for k in keys])
    fs = P.inputs.make_fs(g.star("818"))
    rng = np.random.default_rng(3)
    with solver_for(P, g.v, fs) as sol:
        tt = torch.from_numpy(boxes).to(dev())
        op = sol.frechet_operator(starts, tt, all_cells(g.v.shape))
        w = torch.from_numpy(weights(rng, op.shape[0])).to(dev())
        g1, h1 = op.rmatvec_hits(w)
        g2 = op.rmatvec(w)
        assert torch.equal(g1.view(torch.int64), g2.view(torch.int64))
        assert torch.equal(h1, op.hits())
        m = torch.from_numpy(rng.uniform(-1, 1, op.shape[1])).to(dev())
        lhs = float(torch.dot(op.matvec(m), w))
        rhs = float(torch.dot(m, g1.reshape(-1)))
        S = op.last_scale
        # each visit is rounded by at most 2^-S / 2; the rest is double rounding
        scale_ = float(torch.dot(m.abs(), h1.reshape(-1).to(torch.float64)))
        assert abs(lhs - rhs) <= 2.0 ** -S * scale_ + 1e-12 * abs(lhs) + 1e-12
        # nothing but zeros: g = 0, S = 0
        z = op.rmatvec(torch.zeros(op.shape[0], dtype=torch.float64, device=dev()))
        assert torch.count_nonzero(z) == 0 and op.last_scale == 0


def test_matvec_of_velocity_is_the_path_time(P):
    """G v = t_recv - T[path[0]] for OK and SEED rays, up to the float32 rounding of the solve's adds."""
    import torch
    g = Golden("g24")
    fs = P.inputs.make_fs(g.star("818"))
    key = "818_mid"
    tt, start = g.z[f"tt_{key}"], g.z[f"start_{key}"]
    with solver_for(P, g.v, fs) as sol:
        op = sol.frechet_operator([start], torch.from_numpy(tt[None].copy()).to(dev()), all_cells(g.v.shape))
        y = op.matvec(torch.from_numpy(g.v.astype(np.float64)).to(dev())).cpu().numpy()
    ok = (op.status.numpy() == P.RAY_OK) | (op.status.numpy() == P.RAY_SEED)
    assert ok.all()
    want = op.t_recv.numpy().astype(np.float64)
    assert np.all(np.abs(y - want) <= 1e-5 * np.abs(want))


def test_bad_operator_calls_are_refused(P):
    import torch
    g = Golden("g9")
    fs = P.inputs.make_fs(g.star("3"))
    key = "3_mid"
    tt, start = g.z[f"tt_{key}"], g.z[f"start_{key}"]
    with solver_for(P, g.v, fs) as sol:
        t = torch.from_numpy(tt[None].copy()).to(dev())
        op = sol.frechet_operator([start], t, all_cells(g.v.shape))
        w = torch.ones(op.shape[0], dtype=torch.float64, device=dev())
        w[7] = float("nan")
        with pytest.raises(P.TTSweepError, match="NaN or infinite"):
            op.rmatvec(w)
        w[7] = float("inf")
        with pytest.raises(P.TTSweepError, match="NaN or infinite"):
            op.rmatvec(w)
        with pytest.raises(P.TTSweepError):
            op.matvec(torch.zeros(3, dtype=torch.float64, device=dev()))
        with pytest.raises(P.TTSweepError):
            sol.frechet_operator([start], t, [[0, 0, g.v.shape[2]]])


def test_dense_refusals_leave_the_outputs_untouched(P):
    """The dense calls (forward, adjoint, trace) through the C ABI on the g9 grid with four starts, as
    test_refusals_leave_the_outputs_untouched of test_gpu_ray_pairs.py pins the pair calls: every output is filled
    with -7 and is still -7 after each refusal, the message names the function and the argument; then the accepted
    edge cases."""
    import ctypes as C
    import torch
    g = Golden("g9")
    v = g.v
    fs = P.inputs.make_fs(g.star("818"))
    starts = np.array([[4, 3, 2], [0, 0, 0], [8, 6, 4], [2, 5, 1]], np.int32)
    recv = np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4], [5, 5, 4], [8, 6, 4]], np.int32)
    n, nrecv, ncells = len(starts), len(recv), v.size
    nrays = n * nrecv
    lib = P._lib.lib()
    d = dev()
    with solver_for(P, v, fs) as sol, P.TravelTimeSolver(v.shape, fs) as no_velocity:
        tt = torch.empty((n,) + v.shape, dtype=torch.float32, device=d)
        assert sol.solve_device(starts, tt, init=True) == 1
        pred = sol.predecessors(starts, tt)
        arr, tp, pp = sol._starts_array(starts), sol._box_pointers(tt, n), sol._box_pointers(pred, n)
        rarr = sol._starts_array(recv)
        sent = {
            "y": torch.full((nrays,), -7.0, dtype=torch.float64, device=d),
            "g": torch.full((ncells,), -7.0, dtype=torch.float64, device=d),
            "hits": torch.full((ncells,), -7, dtype=torch.int32, device=d),
            "status": torch.full((nrays,), -7, dtype=torch.int32),
            "offsets": torch.full((nrays + 1,), -7, dtype=torch.int64),
            "t_recv": torch.full((nrays,), -7.0, dtype=torch.float32),
            "cells": torch.full((nrays * 16,), -7, dtype=torch.int32, device=d),
            "hop_d": torch.full((nrays * 16,), -7.0, dtype=torch.float32, device=d),
        }
        mdev = torch.ones(ncells, dtype=torch.float64, device=d)
        wdev = torch.ones(nrays, dtype=torch.float64, device=d)
        scale = C.c_int(-7)
        ptr = lambda t: None if t is None else t.data_ptr()
        torch.cuda.synchronize()

        def untouched(*names):
            torch.cuda.synchronize()
            return all(bool(torch.all(sent[k] == -7)) for k in (names or sent)) and (bool(names) or scale.value == -7)

        def reset():
            for t in sent.values():
                t.fill_(-7)
            scale.value = -7
            torch.cuda.synchronize()

        def calls(ctx=sol._ctx, nstart=n, arr_=arr, tp_=tp, nrecv_=nrecv, rarr_=rarr, m=mdev, y=sent["y"], w=wdev,
                  g_=sent["g"], offsets=sent["offsets"], capacity=nrays * 16):
            head = (ctx, nstart, arr_, tp_, pp, nrecv_, rarr_)
            return {
                "ray_forward": lambda: lib.ttsweep_ray_forward_device(*head, ptr(m), ptr(y), ptr(sent["status"])),
                "ray_adjoint": lambda: lib.ttsweep_ray_adjoint_device(*head, ptr(w), ptr(g_), ptr(sent["hits"]),
                                                                      C.byref(scale)),
                "trace_rays": lambda: lib.ttsweep_trace_rays_device(
                    *head, ptr(offsets), ptr(sent["status"]), ptr(sent["t_recv"]), ptr(sent["cells"]),
                    ptr(sent["hop_d"]), capacity),
            }

        def refused(message, only=("ray_forward", "ray_adjoint", "trace_rays"), **kw):
            for name, call in calls(**kw).items():
                if name not in only:
                    continue
                assert call() < 0, (name, message)
                err = P._lib.last_error()
                assert f"ttsweep_{name}_device" in err and message in err, (name, err)
                assert untouched(), (name, message)

        operators = ("ray_forward", "ray_adjoint")
        refused("null or bad argument", nstart=-1)
        refused("null or bad argument", nrecv_=-1)
        refused("null or bad argument", rarr_=None)
        refused("int32", only=operators, nstart=65536, nrecv_=65536)
        hole = sol._box_pointers(tt, n)
        hole[2] = None
        refused("null box pointer 2", tp_=hole)
        outside = sol._starts_array(np.concatenate([starts[:-1], [[0, v.shape[1], 0]]]))
        refused("start 3 ", arr_=outside)
        r2 = recv.copy()
        r2[1] = [2, 2, v.shape[2]]
        refused("receiver 1 ", rarr_=sol._starts_array(r2))
        r2[1], r2[5] = [2, 2, 2], [-1, 0, 0]
        refused("receiver 5 ", rarr_=sol._starts_array(r2))
        refused("velocity not set", ctx=no_velocity._ctx)
        refused("null or bad argument", only=("ray_forward",), m=None)
        refused("null or bad argument", only=("ray_forward",), y=None)
        refused("both", only=("ray_adjoint",), w=None)
        refused("both", only=("ray_adjoint",), g_=None)
        for badw in (float("nan"), float("inf")):
            wb = wdev.clone()
            wb[9] = badw
            refused("NaN or infinite", only=("ray_adjoint",), w=wb)
        refused("null or bad argument", only=("trace_rays",), offsets=None)
        # precedence: a bad receiver together with a NULL m reports the receiver
        refused("receiver 5 ", only=("ray_forward",), rarr_=sol._starts_array(r2), m=None)

        # accepted: no starts or no receivers.  forward writes nothing; adjoint zeroes g and hits, S = 0; the trace
        # sets offsets[0] = 0 and returns 0
        for kw in ({"nstart": 0}, {"nrecv_": 0}, {"nrecv_": 0, "rarr_": None}):
            for name, call in calls(**kw).items():
                assert call() == 0, (name, kw, P._lib.last_error())
            torch.cuda.synchronize()
            assert untouched("y", "status", "t_recv", "cells", "hop_d"), kw
            assert scale.value == 0 and not bool(torch.any(sent["g"] != 0)) and not bool(torch.any(sent["hits"] != 0))
            assert sent["offsets"][0] == 0 and bool(torch.all(sent["offsets"][1:] == -7)), kw
            reset()
        # adjoint with g and hits both NULL: S = 0, nothing else
        assert lib.ttsweep_ray_adjoint_device(sol._ctx, n, arr, tp, pp, nrecv, rarr, None, None, None,
                                              C.byref(scale)) == 0
        assert scale.value == 0 and untouched("y", "g", "hits", "status")
        reset()
        # a trace without room for the paths: the total, offsets, status and t_recv, and no cell
        for capacity in (0, 1):
            total = calls(capacity=capacity)["trace_rays"]()
            assert total > nrays and total == int(sent["offsets"][-1]) and sent["offsets"][0] == 0
            assert untouched("cells", "hop_d") and bool(torch.all(sent["status"] == P.RAY_OK))
            assert not bool(torch.any(sent["t_recv"] == -7))
            reset()
        assert total <= nrays * 16
        # the same arguments are accepted: every output is written
        for name, call in calls().items():
            assert call() == (total if name == "trace_rays" else 0), (name, P._lib.last_error())
        torch.cuda.synchronize()
        assert scale.value != -7
        for k in ("y", "g", "hits", "status", "offsets", "t_recv"):
            assert not bool(torch.any(sent[k] == -7)), k
        assert not bool(torch.any(sent["cells"][:total] == -7)) and not bool(torch.any(sent["hop_d"][:total] == -7))
        assert bool(torch.all(sent["cells"][total:] == -7)) and bool(torch.all(sent["hop_d"][total:] == -7))


def test_lsqr_on_a_golden_box_matches_scipy(P):
    """A short damped lsqr with the operator recovers scipy's lsqr on the dense G.  G is rank-deficient (a cell
    no ray crosses has a zero column), so the damping is a fair fraction of ||G|| (about 240): without it, loss of
    orthogonality lets any two implementations drift apart by percents within 20 iterations."""
    import torch
    from scipy.sparse.linalg import lsqr as scipy_lsqr
    g = Golden("g9")
    key = "818_mid"
    v, tt, start = g.v, g.z[f"tt_{key}"], g.z[f"start_{key}"]
    fs = P.inputs.make_fs(g.star("818"))
    recv = all_cells(v.shape)
    with solver_for(P, v, fs) as sol:
        op = sol.frechet_operator([start], torch.from_numpy(tt[None].copy()).to(dev()), recv)
        rng = np.random.default_rng(5)
        b = rng.standard_normal(op.shape[0])
        x, istop, itn, r1norm = P.lsqr(op, torch.from_numpy(b).to(dev()), damp=30.0, atol=1e-10, btol=1e-10,
                                       iter_lim=200)
    pred = R.predecessors(v, tt, fs, start)
    offsets, cells, hop_d, _, _ = R.trace(v, tt, pred, fs, start, recv)
    G = R.frechet_dense(offsets, cells, hop_d, v.size)
    want = scipy_lsqr(G, b, damp=30.0, atol=1e-10, btol=1e-10, iter_lim=200)
    assert x.device.type == "cuda" and (istop, itn) == (want[1], want[2]) and itn < 200
    assert np.linalg.norm(x.cpu().numpy() - want[0]) <= 1e-9 * np.linalg.norm(want[0])


def test_solve_operators_solve_keeps_the_shortcut(P):
    """solve -> operator (pred, forward, adjoint, hits) -> solve of the same host boxes: the last solve is
    still the confirming pass answered with 0 without device work."""
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
        assert sol.stats()["sweeps_total"] > 0
        tt = torch.from_numpy(np.stack(boxes)).to(dev())
        op = sol.frechet_operator(starts, tt, all_cells(g.v.shape)[::9])
        op.matvec(torch.ones(op.shape[1], dtype=torch.float64, device=dev()))
        op.rmatvec_hits(torch.ones(op.shape[0], dtype=torch.float64, device=dev()))
        assert sol.solve(starts, boxes) == 0
        assert sol.stats()["sweeps_total"] == 0
        assert sol.changed(2) == [0, 0]


def test_full_size_operators_match_the_explicit_path(P):
    """241x241x51, 818-FS, 24 starts, every surface cell a receiver: sum(hits) is the counting call's total, hits
    is the bincount of the traced cells, and G m / G^T w equal rays_to_frechet's within the bounds."""
    import torch
    shape = (241, 241, 51)
    v = P.inputs.velocity_model(*shape, 20160507)
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))
    starts = P.inputs.read_triples(P.inputs.starts_path("24"))
    d = dev()
    with P.TravelTimeSolver(shape, fs) as sol:
        vd = torch.from_numpy(v).to(d)
        sol.set_velocity(vd)
        tt = torch.empty((24,) + shape, dtype=torch.float32, device=d)
        assert sol.solve_device(starts, tt, init=True) == 1
        pred = sol.predecessors(starts, tt)
        surf = np.argwhere(np.ones(shape[:2], bool))
        recv = np.concatenate([surf, np.zeros((len(surf), 1), np.int64)], axis=1).astype(np.int32)
        op = sol.frechet_operator(starts, tt, recv, pred)
        hits = op.hits()
        rays = sol.trace_rays(starts, tt, recv, pred)
        gen = torch.Generator(device=d).manual_seed(9)
        m = torch.rand(op.shape[1], dtype=torch.float64, device=d, generator=gen) + 0.5
        w = torch.randn(op.shape[0], dtype=torch.float64, device=d, generator=gen)
        y = op.matvec(m)
        g, h2 = op.rmatvec_hits(w)
        S = op.last_scale
    assert torch.equal(hits, h2)
    assert torch.all(op.status == P.RAY_OK)
    total = int(rays.offsets[-1])
    assert int(hits.to(torch.int64).sum()) == total
    assert torch.equal(hits.reshape(-1), torch.bincount(rays.cells.to(torch.int64), minlength=op.shape[1])
                       .to(torch.int32))
    G = P.rays_to_frechet(rays, shape)
    del rays
    want = torch.sparse.mm(G, m.reshape(-1, 1)).flatten()
    assert float(((y - want).abs() / want.abs()).max()) <= 1e-12
    gt = torch.sparse.mm(G.t(), w.reshape(-1, 1)).flatten()
    absg = torch.sparse.mm(G.t(), w.abs().reshape(-1, 1)).flatten()
    bound = 2.0 ** -S * (hits.reshape(-1).to(torch.float64) + 1) + 1e-12 * absg
    assert torch.all((g.reshape(-1) - gt).abs() <= bound)
