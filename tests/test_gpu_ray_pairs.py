"""GPU tier (-m gpu) of the pair-list ray calls (include/ttsweep.h, "rays: pair lists"):
ttsweep_ray_pairs_forward_device / _adjoint_device through TravelTimeSolver.frechet_operator(pairs=...) and
ttsweep_ray_pairs_geometry_device through TravelTimeSolver.ray_geometry, bit for bit against the dense operator
calls on the cross-product list and against the numpy restatement tests/ray_pairs_reference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, Golden
import locate_reference as L
import ray_operator_reference as O
import ray_pairs_reference as PR
import ray_reference as R

pytestmark = pytest.mark.gpu

F32 = np.float32
GEO = ("t_recv", "hops", "length", "recv_hop", "recv_d", "recv_dt", "src_hop", "src_d", "src_dt", "deep")


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
    """weights() of test_gpu_ray_operators.py: zeros and 2^-40 scales among normal weights."""
    w = rng.standard_normal(n)
    w[rng.random(n) < 0.15] = 0.0
    w[rng.random(n) < 0.1] *= 2.0 ** -40
    return w


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def solver_for(P, v, fs, lo=0, hi=None):
    sol = P.TravelTimeSolver(v.shape, fs, lo, hi)
    sol.set_velocity(v)
    return sol


def run_pairs(sol, starts, tt, box, recv, m, w, pred=None):
    """Every output of the pair calls for one list, on the host: dict of numpy arrays (and S)."""
    import torch
    op = sol.frechet_operator(starts, tt, pred=pred, pairs=(box, recv))
    out = {"shape": op.shape, "status": op.status.numpy().copy(), "t_recv_op": op.t_recv.numpy().copy()}
    out["y"] = op.matvec(torch.from_numpy(m).to(dev())).cpu().numpy()
    g, h = op.rmatvec_hits(torch.from_numpy(w).to(dev()))
    out["g"], out["hits_both"], out["S"] = g.cpu().numpy().reshape(-1), h.cpu().numpy().reshape(-1), op.last_scale
    out["g_alone"] = op.rmatvec(torch.from_numpy(w).to(dev())).cpu().numpy().reshape(-1)
    out["hits"] = op.hits().cpu().numpy().reshape(-1)
    geo = sol.ray_geometry(starts, tt, box, recv, pred=op.pred)
    out["geo_status"] = geo.status.numpy().copy()
    for k in GEO:
        out[k] = getattr(geo, k).cpu().numpy()
    out["op"], out["geometry"] = op, geo
    return out


def check_against_restatement(got, rays, tts, fs, shape, box, recv, m, w, lo=0, hi=None, what=""):
    """The outputs of run_pairs equal to the restatement's, bit for bit."""
    ncells = int(np.prod(shape))
    offsets, cells, hop_d, status, t_recv = rays
    assert got["shape"] == (len(box), ncells), what
    assert same(got["status"], status) and same(got["geo_status"], status), what
    assert same(got["t_recv_op"], t_recv), what
    y, g, S, hits = PR.operators(rays, m, w, ncells, O.entries_dmax(fs, shape, lo, hi if hi is not None
                                                                     else len(fs) - 1))
    assert same(got["y"], y), what
    assert got["S"] == S, what
    assert same(got["g"], g) and same(got["g_alone"], g), what
    assert same(got["hits"], hits) and same(got["hits_both"], hits), what
    want = PR.geometry(tts, box, recv, rays)
    for k in GEO:
        assert same(got[k], want[k]), f"{what}: {k}"


# ---- 1. golden boxes: the cross-product pair list from every cell is the dense operator, and the restatement ----
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


def check_cross_product(P, sol, v, fs, starts, tts, lo, hi, what):
    import torch
    starts = np.asarray(starts, np.int32).reshape(-1, 3)
    recv = all_cells(v.shape)
    box, pr = PR.cross_product(len(starts), recv)
    rng = np.random.default_rng(len(what) + len(box))
    m, w = rng.uniform(0.5, 2.0, v.size), weights(rng, len(box))
    tt = torch.from_numpy(np.ascontiguousarray(tts, dtype=F32)).to(dev())
    got = run_pairs(sol, starts, tt, box, pr, m, w)
    dense = sol.frechet_operator(starts, tt, recv, got["op"].pred)
    assert dense.shape == got["shape"], what
    assert same(dense.status.numpy(), got["status"]) and same(dense.t_recv.numpy(), got["t_recv_op"]), what
    assert same(dense.matvec(torch.from_numpy(m).to(dev())).cpu().numpy(), got["y"]), what
    g, h = dense.rmatvec_hits(torch.from_numpy(w).to(dev()))
    assert dense.last_scale == got["S"], what
    assert same(g.cpu().numpy().reshape(-1), got["g"]) and same(h.cpu().numpy().reshape(-1), got["hits"]), what
    rays = O.rays_of_boxes(v, tts, fs, starts, recv, lo, hi)
    check_against_restatement(got, rays, tts, fs, v.shape, box, pr, m, w, lo, hi, what)
    return got


@pytest.mark.parametrize("case", GOLDEN_BOXES, ids=[c[0] for c in GOLDEN_BOXES])
def test_golden_boxes_cross_product_pairs(P, case):
    key, name, offs, start, tt, lo, hi = case
    v = Golden(name).v
    fs = P.inputs.make_fs(offs)
    with solver_for(P, v, fs, lo, hi) as sol:
        got = check_cross_product(P, sol, v, fs, [start], tt[None], lo, hi, key)
    assert np.all(got["status"] == P.RAY_OK)


FR = np.load(os.path.join(GOLDEN, "float_range.npz"))
FR_META = json.loads(bytes(FR["meta"]).decode())


@pytest.mark.parametrize("key", sorted(FR_META))
def test_float_range_cross_product_pairs(P, key):
    m = FR_META[key]
    v = FR[f"v_{m['case']}"]
    fs = P.inputs.make_fs(FR[f"star_{m['star']}"], F32(np.uint32(m["delta_bits"]).view(F32)))
    if m["hand_made_d"]:
        fs["d"] = FR[f"fsd_{key}"].view(F32)
    starts = np.array(m["starts"], np.int32)
    with solver_for(P, v, fs) as sol:
        check_cross_product(P, sol, v, fs, starts, FR[f"tt_{key}"], 0, len(fs) - 1, key)


# ---- 2. several boxes in one wave ----
@pytest.fixture(scope="module")
def g9_boxes(P):
    """Four starts on the g9 velocity with the 818 star, solved on the GPU: (v, fs, starts, boxes on the host, the
    restatement's rays from every cell of every box)."""
    import torch
    g = Golden("g9")
    v = g.v
    fs = P.inputs.make_fs(g.star("818"))
    starts = np.array([[4, 3, 2], [0, 0, 0], [8, 6, 4], [2, 5, 1]], np.int32)
    with solver_for(P, v, fs) as sol:
        tt = torch.empty((len(starts),) + v.shape, dtype=torch.float32, device=dev())
        assert sol.solve_device(starts, tt, init=True) == 1
        boxes = tt.cpu().numpy()
    every = O.rays_of_boxes(v, boxes, fs, starts, all_cells(v.shape))
    for a in (boxes,) + every:
        a.setflags(write=False)
    return v, fs, starts, boxes, every


def rays_from_every(every, shape, box, recv):
    """The rays of a pair list picked out of the rays from every cell of every box (ray s * ncells + q)."""
    offsets, cells, hop_d, status, t_recv = every
    ncells = int(np.prod(shape))
    r = np.asarray(box, np.int64) * ncells + (np.asarray(recv, np.int64) @ [shape[1] * shape[2], shape[2], 1])
    counts = (offsets[1:] - offsets[:-1])[r]
    idx = np.concatenate([np.arange(offsets[x], offsets[x + 1]) for x in r]) if len(r) else np.zeros(0, np.int64)
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), cells[idx], hop_d[idx], status[r], t_recv[r])


def mixed_pairs(rng, starts, shape, npair):
    """A pair list whose waves hold lanes of every box (box = r mod nstart, then a few swapped), with duplicated
    pairs and pairs whose receiver is the box's own start."""
    n = len(starts)
    box = (np.arange(npair) % n).astype(np.int32)
    recv = np.stack([rng.integers(0, s, npair) for s in shape], 1).astype(np.int32)
    for r in range(2, npair, 9):            # the box's own start as the receiver
        recv[r] = starts[box[r]]
    for r in range(5, npair, 11):           # a duplicate of an earlier pair
        box[r], recv[r] = box[r - 4], recv[r - 4]
    if npair == 1:
        box[0], recv[0] = 2, [1, 2, 3]
    return box, recv


@pytest.mark.parametrize("npair", [1, 63, 64, 65, 1000])
def test_several_boxes_in_one_wave(P, g9_boxes, npair):
    import torch
    v, fs, starts, boxes, every = g9_boxes
    rng = np.random.default_rng(100 + npair)
    box, recv = mixed_pairs(rng, starts, v.shape, npair)
    if npair >= 63:
        assert all(len(set(box[a:a + 64])) == len(starts) for a in range(0, npair - 3, 64))
        assert np.any(np.all(recv == starts[box], axis=1))
        assert len({(b, *q) for b, q in zip(box, recv)}) < npair
    m, w = rng.uniform(0.5, 2.0, v.size), weights(rng, npair)
    if npair == 1:
        w[0] = 0.75
    rays = rays_from_every(every, v.shape, box, recv)
    with solver_for(P, v, fs) as sol:
        tt = torch.from_numpy(boxes.copy()).to(dev())
        got = run_pairs(sol, starts, tt, box, recv, m, w)
        check_against_restatement(got, rays, boxes, fs, v.shape, box, recv, m, w, what=f"npair {npair}")
        # two calls: identical bits
        again = run_pairs(sol, starts, tt, box, recv, m, w, pred=got["op"].pred)
        for k in ("y", "g", "hits", "status") + GEO:
            assert same(again[k], got[k]), k
        # a permuted list: the same g, hits and S; y and status follow the permutation
        perm = rng.permutation(npair)
        other = run_pairs(sol, starts, tt, box[perm], recv[perm], m, w[perm], pred=got["op"].pred)
    assert other["S"] == got["S"] and same(other["g"], got["g"]) and same(other["hits"], got["hits"])
    assert same(other["y"], got["y"][perm]) and same(other["status"], got["status"][perm])
    for k in GEO:
        assert same(other[k], got[k][perm]), k
    if npair > 1:
        assert np.count_nonzero(got["hops"] == 0) >= 1 and got["hops"].max() >= 1


def test_one_context_many_shapes_of_call(P, g9_boxes):
    """The ray calls share one device buffer of the context, laid out anew by every call, grown when a call needs
    more and kept between calls.  One solver runs calls of very different sizes in a row - small after large, pair
    list after cross product, the trace's extra arrays in between - and every result equals, bit for bit, the same
    call on a fresh solver."""
    import torch
    v, fs, starts, boxes, _ = g9_boxes
    rng = np.random.default_rng(404)
    box, recv = mixed_pairs(rng, starts, v.shape, 1000)
    every = all_cells(v.shape)
    m = torch.from_numpy(rng.uniform(0.5, 2.0, v.size)).to(dev())
    w_dense = torch.from_numpy(weights(rng, len(starts) * len(every))).to(dev())
    host = lambda *ts: [t.cpu().numpy().copy() for t in ts]

    def geometry_of_one_pair(sol, tt, pred):
        geo = sol.ray_geometry(starts, tt, box[:1], recv[:1], pred=pred)
        return host(geo.status, *[getattr(geo, k) for k in GEO])

    def dense_adjoint_with_hits(sol, tt, pred):
        op = sol.frechet_operator(starts, tt, every, pred)
        g, hits = op.rmatvec_hits(w_dense)
        return host(op.status, g, hits) + [np.array(op.last_scale)]

    def trace_with_one_receiver(sol, tt, pred):
        rays = sol.trace_rays(starts, tt, recv[7:8], pred)
        return host(rays.offsets, rays.cells, rays.hop_d, rays.status, rays.t_recv)

    def pair_forward_of_1000_pairs(sol, tt, pred):
        op = sol.frechet_operator(starts, tt, pred=pred, pairs=(box, recv))
        return host(op.status, op.matvec(m))

    def predecessors(sol, tt, pred):
        return host(sol.predecessors(starts, tt))

    def dense_forward_with_one_receiver(sol, tt, pred):
        op = sol.frechet_operator(starts, tt, recv[3:4], pred)
        return host(op.status, op.matvec(m))

    def pair_adjoint_of_no_pairs(sol, tt, pred):
        # (through the C ABI: an empty weight tensor has no pointer to give)
        n = len(starts)
        g = torch.full((v.size,), -7.0, dtype=torch.float64, device=dev())
        hits = torch.full((v.size,), -7, dtype=torch.int32, device=dev())
        scale = C.c_int(-7)
        torch.cuda.synchronize()
        assert P._lib.lib().ttsweep_ray_pairs_adjoint_device(
            sol._ctx, n, sol._starts_array(starts), sol._box_pointers(tt, n), sol._box_pointers(pred, n), 0, None,
            None, m.data_ptr(), g.data_ptr(), hits.data_ptr(), C.byref(scale)) == 0, P._lib.last_error()
        return host(g, hits) + [np.array(scale.value)]

    calls = [geometry_of_one_pair, dense_adjoint_with_hits, trace_with_one_receiver, pair_forward_of_1000_pairs,
             predecessors, dense_forward_with_one_receiver, pair_adjoint_of_no_pairs]
    tt = torch.from_numpy(boxes.copy()).to(dev())
    with solver_for(P, v, fs) as sol:
        pred = sol.predecessors(starts, tt)
    want = []
    for call in calls:
        with solver_for(P, v, fs) as fresh:
            want.append(call(fresh, tt, pred))
    with solver_for(P, v, fs) as sol:
        got = [call(sol, tt, pred) for call in calls]
    for call, a, b in zip(calls, got, want):
        assert len(a) == len(b) and all(same(x, y) for x, y in zip(a, b)), call.__name__
    assert same(got[4][0], pred.cpu().numpy())
    assert got[2][0][-1] > len(starts) and len(got[3][1]) == 1000 and not got[6][0].any() and got[6][2] == 0


# ---- 3. statuses ----
def status_pairs(rng, starts, shape, must, npair=300):
    """Random pairs over every box, the cells `must` ([(box, flat cell)]) among them."""
    box = rng.integers(0, len(starts), npair).astype(np.int32)
    recv = np.stack([rng.integers(0, s, npair) for s in shape], 1).astype(np.int32)
    for r, (b, c) in enumerate(must):
        box[3 * r], recv[3 * r] = b, np.unravel_index(int(c), shape)
    return box, recv


def check_empty_rays(got, statuses):
    """The stated values of the rays without cells."""
    empty = np.isin(got["status"], statuses)
    assert empty.any()
    assert not got["hops"][empty].any() and not got["length"][empty].any() and np.all(got["deep"][empty] == -1)
    assert same(got["length"][empty], np.zeros(empty.sum()))
    for k in ("recv_hop", "recv_d", "recv_dt", "src_hop", "src_d", "src_dt"):
        assert not got[k][empty].any(), k
    assert same(got["y"][empty], np.zeros(empty.sum()))
    assert same(got["t_recv"], got["t_recv_op"])


def test_unreached_behind_a_wall(P):
    """A wall no travel time crosses: v is the slowness-like volume the delay d * (v[a] + v[b]) / 2 is linear in, so
    zero velocity is the largest float there, and every delay into the wall overflows to INFINITY (the inf_sum case
    of the float-range golden file).  The cells in it and behind it are UNREACHED."""
    import torch
    g = Golden("g24")
    v = g.v.copy()
    v[:, 8:11, :] = np.finfo(F32).max
    fs = P.inputs.make_fs(g.star("six"))
    starts = np.array([[5, 2, 3], [20, 4, 9], [11, 7, 0]], np.int32)
    rng = np.random.default_rng(31)
    with solver_for(P, v, fs) as sol:
        tt = torch.empty((3,) + v.shape, dtype=torch.float32, device=dev())
        assert sol.solve_device(starts, tt, init=True) == 1
        boxes = tt.cpu().numpy()
        assert np.all(np.isinf(boxes[:, :, 8:, :])) and np.all(np.isfinite(boxes[:, :, :8, :]))
        box, recv = status_pairs(rng, starts, v.shape, [])
        m, w = rng.uniform(0.5, 2.0, v.size), weights(rng, len(box))
        got = run_pairs(sol, starts, tt, box, recv, m, w)
    rays = PR.rays_of_pairs(v, boxes, fs, starts, box, recv)
    check_against_restatement(got, rays, boxes, fs, v.shape, box, recv, m, w, what="wall")
    assert set(got["status"]) == {P.RAY_OK, P.RAY_UNREACHED}
    check_empty_rays(got, [P.RAY_UNREACHED])
    assert np.all(np.isinf(got["t_recv"][got["status"] == P.RAY_UNREACHED]))


def test_seed_rays_of_a_seeded_box(P):
    import torch
    g = Golden("g24")
    v = g.v
    fs = P.inputs.make_fs(g.star("5"))
    starts = np.array([[12, 10, 6], [3, 3, 3]], np.int32)
    seeds = [(2, 3, 1), (21, 17, 10)]
    box0 = np.full((2,) + v.shape, np.inf, F32)
    for s, st in enumerate(starts):
        box0[s][tuple(st)] = 0
    for p in seeds:
        box0[0][p] = F32(0.5)
    rng = np.random.default_rng(32)
    with solver_for(P, v, fs) as sol:
        tt = torch.from_numpy(box0.copy()).to(dev())
        assert sol.solve_device(starts, tt, init=False) == 1
        boxes = tt.cpu().numpy()
        must = [(0, R.flat_index(v.shape, p)) for p in seeds]          # a receiver that is a SEED cell: no hop
        box, recv = status_pairs(rng, starts, v.shape, must)
        m, w = rng.uniform(0.5, 2.0, v.size), weights(rng, len(box))
        got = run_pairs(sol, starts, tt, box, recv, m, w)
    rays = PR.rays_of_pairs(v, boxes, fs, starts, box, recv)
    check_against_restatement(got, rays, boxes, fs, v.shape, box, recv, m, w, what="seeded")
    seed = got["status"] == P.RAY_SEED
    assert seed.sum() > 2 and np.any(got["status"] == P.RAY_OK)
    assert got["status"][0] == got["status"][3] == P.RAY_SEED and got["hops"][0] == got["hops"][3] == 0
    assert got["deep"][0] == must[0][1] and not got["recv_hop"][0].any()
    assert np.any(got["hops"][seed] > 0)


def test_invalid_rays_of_a_corrupted_pred(P):
    """pred corrupted as test_gpu_ray_operators.py builds it: the rays through the bad cells are INVALID, their
    adjoint terms are taken back out and their geometry is empty."""
    import torch
    g = Golden("g9")
    keys = ["818_mid", "818_corner"]
    v = g.v
    starts = np.array([g.z[f"start_{k}"] for k in keys], np.int32)
    boxes = np.stack([g.z[f"tt_{k}"] for k in keys])
    fs = P.inputs.make_fs(g.star("818"))
    preds = np.stack([R.predecessors(v, boxes[s], fs, starts[s]) for s in range(2)])
    bad = preds[0].reshape(-1)
    N = bad.size
    order = np.argsort(boxes[0].reshape(-1))
    far = order[-6:]
    bad[far[0]] = N + 5
    bad[far[1]] = far[2]
    bad[far[2]] = far[2]
    bad[far[3]] = P.PRED_SOURCE
    bad[far[4]] = P.PRED_UNREACHED
    bad[far[5]] = order[1]
    # a cell many rays pass: everything upstream of it becomes INVALID after hops that were already added
    hub = order[len(order) // 3]
    bad[hub] = hub
    rng = np.random.default_rng(33)
    box, recv = status_pairs(rng, starts, v.shape, [(0, c) for c in far], npair=400)
    m, w = rng.uniform(0.5, 2.0, v.size), weights(rng, len(box))
    with solver_for(P, v, fs) as sol:
        tt = torch.from_numpy(boxes.copy()).to(dev())
        got = run_pairs(sol, starts, tt, box, recv, m, w, pred=torch.from_numpy(preds).to(dev()))
    rays = PR.rays_of_pairs(v, boxes, fs, starts, box, recv, preds=preds)
    check_against_restatement(got, rays, boxes, fs, v.shape, box, recv, m, w, what="bad pred")
    assert np.count_nonzero(got["status"] == P.RAY_INVALID) >= 5 and np.any(got["status"] == P.RAY_OK)
    check_empty_rays(got, [P.RAY_INVALID])
    assert np.all(np.isfinite(got["t_recv"]))


# ---- 4. geometry by hand ----
def test_geometry_of_a_ray_straight_down_a_column(P):
    """Homogeneous 5 x 4 x 7 box, the 6-neighbour star: travel time is the Manhattan distance times the delay of one
    step, so the only shortest path between two cells of one column is the column itself."""
    import torch
    shape = (5, 4, 7)
    v = np.ones(shape, F32)
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("six")))
    d = F32(fs["d"][0])
    assert np.all(fs["d"][:6] == d)
    starts = np.array([[2, 1, 0], [2, 1, 6]], np.int32)         # the top and the bottom of one column
    flat = lambda p: (p[0] * 4 + p[1]) * 7 + p[2]
    box = np.array([0, 1, 0, 0, 1], np.int32)
    recv = np.array([[2, 1, 6], [2, 1, 0], [2, 1, 0], [2, 3, 0], [2, 1, 3]], np.int32)
    with solver_for(P, v, fs) as sol:
        tt = torch.empty((2,) + shape, dtype=torch.float32, device=dev())
        assert sol.solve_device(starts, tt, init=True) == 1
        geo = sol.ray_geometry(starts, tt, box, recv)
        T = tt.cpu().numpy()
    assert geo.status.tolist() == [P.RAY_OK] * 5
    # delay of one step: fl32(fl32(d * (1 + 1)) / 2) = d
    assert T[0][2, 1, 6] == F32(6) * d
    assert geo.hops.tolist() == [6, 6, 0, 2, 3]
    length = geo.length.cpu().numpy()
    assert length.dtype == np.float64 and length.tolist() == [6.0 * float(d), 6.0 * float(d), 0.0, 2.0 * float(d),
                                                               3.0 * float(d)]
    # ray 0 walks up the column from z = 6 to the start at z = 0: out of the receiver towards -z, out of the source
    # towards +z, deepest at the receiver; ray 1 is its mirror image: deepest at the end of the walk
    assert geo.recv_hop.tolist() == [[0, 0, -1], [0, 0, 1], [0, 0, 0], [0, -1, 0], [0, 0, 1]]
    assert geo.src_hop.tolist() == [[0, 0, 1], [0, 0, -1], [0, 0, 0], [0, 1, 0], [0, 0, -1]]
    assert geo.deep.tolist() == [flat((2, 1, 6)), flat((2, 1, 6)), flat((2, 1, 0)), flat((2, 3, 0)), flat((2, 1, 6))]
    for k in ("recv_d", "recv_dt", "src_d", "src_dt"):
        assert getattr(geo, k).tolist() == [float(d), float(d), 0.0, float(d), float(d)], k
    assert same(geo.t_recv.cpu().numpy(), np.array([6 * d, 6 * d, 0, 2 * d, 3 * d], F32))
    assert same(geo.receiver_gradient().cpu().numpy(),
                np.array([[0, 0, -float(d)], [0, 0, float(d)], [0, 0, 0], [0, -float(d), 0], [0, 0, float(d)]]) + 0.0)
    assert same(geo.takeoff().cpu().numpy(),
                np.array([[0, 0, 1.0], [0, 0, -1.0], [0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]]) + 0.0)


# ---- 5. adjointness ----
def test_pair_adjoint_is_the_adjoint_of_the_pair_forward(P, g9_boxes):
    """<G m, w> against <m, G^T w>.  The fixed point rounds every visit by at most 2^-S / 2 (include/ttsweep.h), so
    g[x] is within 2^-S * hits[x] / 2 of the exact sum: |m| . hits * 2^-S / 2 in the product.  The rest is double
    rounding: both sides are sums of the terms w_r * (d / 2) * m_x, whose absolute values add up to
    A = |m| . G^T |w|; a term passes through at most hops_max + 3 roundings on its ray, the last rounding of g, and
    then a dot product of npair or ncells entries, each step relative 2^-53."""
    import torch
    v, fs, starts, boxes, every = g9_boxes
    rng = np.random.default_rng(55)
    box, recv = mixed_pairs(rng, starts, v.shape, 1000)
    with solver_for(P, v, fs) as sol:
        tt = torch.from_numpy(boxes.copy()).to(dev())
        op = sol.frechet_operator(starts, tt, pairs=(box, recv))
        hops_max = int(sol.ray_geometry(starts, tt, box, recv, pred=op.pred).hops.max())
        w = torch.from_numpy(weights(rng, op.shape[0])).to(dev())
        m = torch.from_numpy(rng.uniform(-1, 1, op.shape[1])).to(dev())
        g, hits = op.rmatvec_hits(w)
        S = op.last_scale
        lhs = float(torch.dot(op.matvec(m), w))
        rhs = float(torch.dot(m, g.reshape(-1)))
        A = float(torch.dot(m.abs(), op.rmatvec(w.abs()).reshape(-1)))
    fixed = 2.0 ** -S * float(torch.dot(m.abs(), hits.reshape(-1).to(torch.float64))) / 2
    rounding = (hops_max + 4 + op.shape[0] + op.shape[1]) * 2.0 ** -53 * (A + fixed)
    print(f"adjointness: |lhs - rhs| = {abs(lhs - rhs):.3e}, fixed-point bound {fixed:.3e}, rounding {rounding:.3e}")
    assert abs(lhs - rhs) <= fixed + rounding


# ---- 6. refusals ----
def test_refusals_leave_the_outputs_untouched(P, g9_boxes):
    import torch
    v, fs, starts, boxes, _ = g9_boxes
    n, npair, ncells = len(starts), 6, v.size
    lib = P._lib.lib()
    box = np.array([0, 1, 2, 3, 0, 1], np.int32)
    recv = np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4], [5, 5, 4], [8, 6, 4]], np.int32)
    with solver_for(P, v, fs) as sol:
        tt = torch.from_numpy(boxes.copy()).to(dev())
        pred = sol.predecessors(starts, tt)
        arr, tp, pp = sol._starts_array(starts), sol._box_pointers(tt, n), sol._box_pointers(pred, n)
        d = dev()
        sent = {
            "y": torch.full((npair,), -7.0, dtype=torch.float64, device=d),
            "g": torch.full((ncells,), -7.0, dtype=torch.float64, device=d),
            "hits": torch.full((ncells,), -7, dtype=torch.int32, device=d),
            "status": torch.full((npair,), -7, dtype=torch.int32),
            "f32": [torch.full((npair,), -7.0, dtype=torch.float32, device=d) for _ in range(5)],
            "i32": [torch.full((npair,), -7, dtype=torch.int32, device=d) for _ in range(2)],
            "hop": [torch.full((npair, 3), -7, dtype=torch.int32, device=d) for _ in range(2)],
            "length": torch.full((npair,), -7.0, dtype=torch.float64, device=d),
        }
        mdev = torch.ones(ncells, dtype=torch.float64, device=d)
        wdev = torch.ones(npair, dtype=torch.float64, device=d)
        scale = C.c_int(-7)
        torch.cuda.synchronize()

        def untouched():
            torch.cuda.synchronize()
            flat = [sent["y"], sent["g"], sent["hits"], sent["status"], sent["length"]] + sent["f32"] + sent["i32"] \
                + sent["hop"]
            return all(bool(torch.all(t == -7)) for t in flat) and scale.value == -7

        def calls(nstart, arr_, np_, box_, recv_, w=wdev):
            """(name, the call as a function) of the three calls on these arguments; the arrays stay alive in it."""
            ba = None if box_ is None else np.ascontiguousarray(box_, np.int32)
            ra = None if recv_ is None else np.ascontiguousarray(recv_, np.int32)
            head = (sol._ctx, nstart, arr_, tp, pp, np_, None if ba is None else ba.ctypes.data,
                    None if ra is None else ra.ctypes.data)
            f32, i32, hop = sent["f32"], sent["i32"], sent["hop"]
            keep = (ba, ra, w)
            return [
                ("forward", lambda keep=keep: lib.ttsweep_ray_pairs_forward_device(
                    *head, mdev.data_ptr(), sent["y"].data_ptr(), sent["status"].data_ptr())),
                ("adjoint", lambda keep=keep: lib.ttsweep_ray_pairs_adjoint_device(
                    *head, w.data_ptr(), sent["g"].data_ptr(), sent["hits"].data_ptr(), C.byref(scale))),
                ("geometry", lambda keep=keep: lib.ttsweep_ray_pairs_geometry_device(
                    *head, sent["status"].data_ptr(), f32[0].data_ptr(), i32[0].data_ptr(),
                    sent["length"].data_ptr(), hop[0].data_ptr(), f32[1].data_ptr(), f32[2].data_ptr(),
                    hop[1].data_ptr(), f32[3].data_ptr(), f32[4].data_ptr(), i32[1].data_ptr())),
            ]

        def refused(message, *a, only=None, **kw):
            for name, call in calls(*a, **kw):
                if only and name != only:
                    continue
                assert call() < 0, (name, message)
                err = P._lib.last_error()
                assert f"ttsweep_ray_pairs_{name}_device" in err and message in err, err
                assert untouched(), (name, message)

        refused("null or bad argument", n, arr, -1, box, recv)
        refused("int32", n, arr, 2 ** 31, box, recv)
        refused("null or bad argument", n, arr, npair, None, recv)
        refused("null or bad argument", n, arr, npair, box, None)
        refused("null or bad argument", -1, arr, npair, box, recv)
        b2 = box.copy()
        b2[2] = n
        refused("pair 2 ", n, arr, npair, b2, recv)
        b2[2], b2[4] = 0, -1
        refused("pair 4 ", n, arr, npair, b2, recv)
        r2 = recv.copy()
        r2[3] = [4, 4, v.shape[2]]
        refused("pair 3 ", n, arr, npair, box, r2)
        r2[3], r2[5] = [4, 4, 4], [-1, 0, 0]
        refused("pair 5 ", n, arr, npair, box, r2)
        outside = sol._starts_array(np.concatenate([starts[:-1], [[0, v.shape[1], 0]]]))
        refused("start 3 ", n, outside, npair, box, recv)
        for badw in (float("nan"), float("inf")):
            wb = wdev.clone()
            wb[4] = badw
            refused("NaN or infinite", n, arr, npair, box, recv, only="adjoint", w=wb)
        # the Python layer raises with the library's message
        with pytest.raises(P.TTSweepError, match="pair 2 "):
            sol.frechet_operator(starts, tt, pred=pred, pairs=(b2 * 0 + [0, 1, n, 3, 0, 1], recv))
        with pytest.raises(P.TTSweepError, match="pair 5 "):
            sol.ray_geometry(starts, tt, box, r2, pred=pred)
        with pytest.raises(P.TTSweepError):
            sol.frechet_operator(starts, tt, recv, pred=pred, pairs=(box, recv))
        with pytest.raises(P.TTSweepError):
            sol.frechet_operator(starts, tt, pred=pred, pairs=(box[:3], recv))
        # the same arguments are accepted: every output is written
        for name, call in calls(n, arr, npair, box, recv):
            assert call() == 0, (name, P._lib.last_error())
        torch.cuda.synchronize()
        assert not untouched() and scale.value != -7
        assert not bool(torch.any(sent["y"] == -7)) and not bool(torch.any(sent["status"] == -7))
        # no pairs: as the dense calls with no receivers (nothing walked; g and hits zeroed, S = 0)
        for name, call in calls(n, arr, 0, None, None):
            assert call() == 0, (name, P._lib.last_error())
        torch.cuda.synchronize()
        assert scale.value == 0 and not bool(torch.any(sent["g"] != 0)) and not bool(torch.any(sent["hits"] != 0))
        empty = sol.frechet_operator(starts, tt, pred=pred, pairs=(box[:0], recv[:0]))
        assert empty.shape == (0, ncells) and len(sol.ray_geometry(starts, tt, box[:0], recv[:0], pred=pred)) == 0


# ---- 7. lsqr on a pair operator ----
def test_lsqr_on_a_pair_operator_matches_scipy(P, g9_boxes):
    """b = G m of a smooth m over a pair list on the g9 grid; the damped lsqr with the operator recovers scipy's lsqr
    on the dense G of the same rays: the settings and the tolerance (1e-9 relative, the same stop) are those of
    test_lsqr_on_a_golden_box_matches_scipy in test_gpu_ray_operators.py.

    The iteration count is not compared, unlike there.  This b lies in the range of a G of rank 289 and the atol
    test falls through 1e-10 only after 46 to 48 iterations, without decreasing monotonically; by then the Lanczos
    vectors have lost orthogonality, and the iteration at which the test is met is not a property of the problem to
    rounding: scipy's own lsqr on the dense G stops after 46, 47 or 48 iterations when entries of b move by one
    unit in the last place (4, 16 and 20 of 40 draws), while its x moves by at most 3.7e-10 relative.  (On the random
    b of the dense test it stops after 22 iterations in every draw.)  The stop reason, a count below the limit and x
    are what both sides determine."""
    import torch
    from scipy.sparse.linalg import lsqr as scipy_lsqr
    v, fs, starts, boxes, every = g9_boxes
    rng = np.random.default_rng(77)
    box, recv = mixed_pairs(rng, starts, v.shape, 700)
    x, y, z = np.meshgrid(*[np.linspace(0, 1, n) for n in v.shape], indexing="ij")
    smooth = (1.0 + 0.3 * np.sin(2 * x + y) + 0.2 * z).reshape(-1)
    offsets, cells, hop_d, _, _ = rays_from_every(every, v.shape, box, recv)
    G = R.frechet_dense(offsets, cells, hop_d, v.size)
    with solver_for(P, v, fs) as sol:
        op = sol.frechet_operator(starts, torch.from_numpy(boxes.copy()).to(dev()), pairs=(box, recv))
        b = op.matvec(torch.from_numpy(smooth).to(dev()))
        assert np.all(np.abs(b.cpu().numpy() - G @ smooth) <= 1e-12 * np.abs(G @ smooth))
        got, istop, itn, r1norm = P.lsqr(op, b, damp=30.0, atol=1e-10, btol=1e-10, iter_lim=200)
    want = scipy_lsqr(G, b.cpu().numpy(), damp=30.0, atol=1e-10, btol=1e-10, iter_lim=200)
    err = np.linalg.norm(got.cpu().numpy() - want[0]) / np.linalg.norm(want[0])
    print(f"lsqr on a pair operator: istop {istop} itn {itn}, scipy {want[1]} {want[2]}, relative difference {err:.3e}")
    assert got.device.type == "cuda" and istop == want[1] == 2 and itn < 200 and want[2] < 200
    assert err <= 1e-9
    assert r1norm < float(torch.linalg.vector_norm(b))


# ---- 8. from a locate result to the rows of the operator ----
def test_pairs_from_a_locate_result_line_up_with_the_picks(P):
    import torch
    g = Golden("g24")
    keys = ["818_mid", "818_corner", "818_deadin", "818_deadout"]
    v = g.v
    starts = np.array([g.z[f"start_{k}"] for k in keys], np.int32)
    boxes = np.stack([g.z[f"tt_{k}"] for k in keys])
    fs = P.inputs.make_fs(g.star("818"))
    K, E = len(keys), 14
    rng = np.random.default_rng(88)
    flat = boxes.reshape(K, -1)
    true = rng.integers(0, flat.shape[1], E)
    picks = flat[:, true].T.astype(np.float64) + rng.uniform(-5, 5, E)[:, None] + 0.01 * rng.standard_normal((E, K))
    w = rng.uniform(0.5, 2.0, (E, K))
    w[rng.random((E, K)) < 0.3] = 0.0
    w[np.arange(E), rng.integers(0, K, E)] = 1.0
    w[6] = 0.0
    w[6, 2] = 1.25                               # an event with one pick
    with solver_for(P, v, fs) as sol:
        tt = torch.from_numpy(boxes.copy()).to(dev())
        loc = sol.locate(tt, picks, w)
        box, recv, ev, stn = P.pairs_from_locations(loc, w)
        op = sol.frechet_operator(starts, tt, pairs=(box, recv))
        geo = sol.ray_geometry(starts, tt, box, recv, pred=op.pred)
        cell, t0 = loc.cell.cpu().numpy(), loc.t0.cpu().numpy()
    want = PR.pairs_from_locations_loop(loc.xyz.numpy() if hasattr(loc.xyz, "numpy") else loc.xyz, w)
    assert all(same(a, b) for a, b in zip((box, recv, ev, stn), want))
    assert len(box) == np.count_nonzero(w) and np.all(w[ev, stn] != 0) and np.all(cell >= 0)
    assert same((recv[:, 0].astype(np.int64) * v.shape[1] + recv[:, 1]) * v.shape[2] + recv[:, 2],
                cell[ev].astype(np.int64))
    assert np.all(op.status.numpy() == P.RAY_OK)
    t_recv = op.t_recv.numpy()
    assert same(t_recv, flat[stn, cell[ev]]) and same(geo.t_recv.cpu().numpy(), t_recv)
    # the restatement's cell, t0 and residuals r = (o - T) - t0 at the best cell
    rc, _, rt0, _ = L.locate(boxes, picks, w)
    assert same(cell, rc) and same(t0, rt0)
    r_want = np.subtract(np.subtract(picks[ev, stn], flat[stn, rc[ev]].astype(np.float64)), rt0[ev])
    r_got = (picks[ev, stn] - t_recv.astype(np.float64)) - t0[ev]
    assert same(r_got, r_want)
    J = np.zeros(E)
    np.add.at(J, ev, w[ev, stn] * r_got * r_got)
    assert np.all(np.abs(J - loc.misfit.cpu().numpy()) <= 1e-12 * np.maximum(J, 1e-300))
    assert J[6] == 0.0 or abs(r_got[ev == 6][0]) <= 1e-12


def test_solve_pair_calls_solve_keeps_the_shortcut(P):
    """solve -> pair operator and geometry -> solve of the same host boxes: still answered without device work."""
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
        box, recv = PR.cross_product(2, all_cells(g.v.shape)[::9])
        op = sol.frechet_operator(starts, tt, pairs=(box, recv))
        op.matvec(torch.ones(op.shape[1], dtype=torch.float64, device=dev()))
        op.rmatvec_hits(torch.ones(op.shape[0], dtype=torch.float64, device=dev()))
        sol.ray_geometry(starts, tt, box, recv, pred=op.pred)
        assert sol.solve(starts, boxes) == 0
        assert sol.stats()["sweeps_total"] == 0
        assert sol.changed(2) == [0, 0]
