"""CPU tier of the pair-list ray calls (include/ttsweep.h, "rays: pair lists"): the numpy restatement
(ray_pairs_reference.py) against the restatements it is built on, on the golden boxes of g9 / g24; the surface of the
C ABI (symbols, the macro, refusals that need no device); and pairs_from_locations against a loop."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, Golden
import ray_operator_reference as O
import ray_pairs_reference as PR
import ray_reference as R

F32 = np.float32


def golden_group(name, star, nbox=3):
    """(v, fs offsets, starts [n, 3], boxes [n, ...]) of the first boxes of one star in a golden file."""
    g = Golden(name)
    keys = [k for k, sname, *_ in g.cases() if sname == star][:nbox]
    assert len(keys) >= 2
    return g.v, g.star(star), np.array([g.z[f"start_{k}"] for k in keys], np.int32), \
        np.stack([g.z[f"tt_{k}"] for k in keys])


def some_cells(shape, rng, n):
    cells = np.argwhere(np.ones(shape, bool)).astype(np.int32)
    return cells[rng.choice(len(cells), n, replace=False)]


GROUPS = [("g9", "818"), ("g9", "3"), ("g24", "818"), ("g24", "5")]


@pytest.fixture(scope="module", params=GROUPS, ids=["/".join(g) for g in GROUPS])
def group(request, pkg):
    name, star = request.param
    v, offs, starts, boxes = golden_group(name, star)
    fs = pkg.inputs.make_fs(offs)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{star}".encode()))
    recv = some_cells(v.shape, rng, 60)
    recv[:len(starts)] = starts                 # receivers that are a box's own start
    dense = O.rays_of_boxes(v, boxes, fs, starts, recv)
    return v, fs, starts, boxes, recv, dense, rng


def test_cross_product_pair_list_is_the_dense_reference(group):
    v, fs, starts, boxes, recv, dense, rng = group
    box, pr = PR.cross_product(len(starts), recv)
    assert np.array_equal(box.reshape(len(starts), -1)[:, 0], np.arange(len(starts)))
    rays = PR.rays_of_pairs(v, boxes, fs, starts, box, pr)
    for a, b in zip(rays, dense):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    m = rng.uniform(0.5, 2.0, v.size)
    w = rng.standard_normal(len(box))
    w[::7] = 0
    dmax = O.entries_dmax(fs, v.shape)
    y, g, S, hits = PR.operators(rays, m, w, v.size, dmax)
    gd, Sd = O.adjoint(*dense[:3], w, v.size, dmax)
    assert S == Sd == O.scale(w, dmax, len(box))
    assert np.array_equal(y.view(np.uint64), O.forward(*dense[:3], m).view(np.uint64))
    assert np.array_equal(g.view(np.uint64), gd.view(np.uint64))
    assert np.array_equal(hits, O.hits(dense[1], v.size))


def test_geometry_against_the_stored_paths(group):
    """length is the step-by-step sum of hop_d in walk order; the hop times summed along the path are the replay's;
    hops, deep and the offsets are those of the path."""
    v, fs, starts, boxes, recv, dense, rng = group
    box, pr = PR.cross_product(len(starts), recv)
    rays = PR.rays_of_pairs(v, boxes, fs, starts, box, pr)
    offsets, cells, hop_d, status, t_recv = rays
    geo = PR.geometry(boxes, box, pr, rays)
    assert np.all(status == R.RAY_OK)
    assert np.array_equal(geo["t_recv"].view(np.uint32), t_recv.view(np.uint32))
    nz = v.shape[2]
    nohop = 0
    for r in range(len(box)):
        a, b = offsets[r], offsets[r + 1]
        path, d = cells[a:b], hop_d[a:b]
        assert geo["hops"][r] == len(path) - 1
        length = np.float64(0)
        for h in range(len(path) - 2, -1, -1):
            length = length + np.float64(d[h])
        assert geo["length"][r] == length
        z = path % nz
        assert geo["deep"][r] in path and geo["deep"][r] % nz == z.max()
        walk = path[::-1]
        assert geo["deep"][r] == walk[np.argmax(walk % nz)]
        if len(path) == 1:
            nohop += 1
            assert not geo["recv_hop"][r].any() and not geo["src_hop"][r].any() and geo["deep"][r] == path[0]
            assert geo["recv_d"][r] == geo["src_d"][r] == geo["recv_dt"][r] == geo["src_dt"][r] == 0
            continue
        T = boxes[box[r]].reshape(-1)
        assert geo["recv_d"][r] == d[-2] and geo["src_d"][r] == d[0]
        to = lambda c: np.array(np.unravel_index(int(c), v.shape))
        assert np.array_equal(geo["recv_hop"][r], to(path[-2]) - to(path[-1]))
        assert np.array_equal(geo["src_hop"][r], to(path[1]) - to(path[0]))
        assert geo["recv_dt"][r] == F32(T[path[-1]] - T[path[-2]]) and geo["recv_dt"][r] > 0
        assert geo["src_dt"][r] == F32(T[path[1]] - T[path[0]]) and geo["src_dt"][r] > 0
        # the first hop's time is the replayed delay of that hop: replaying the path without its last hop and
        # adding recv_dt gives the receiver's time up to the one rounding of the subtraction
        short = R.replay(v, boxes[box[r]], np.array([0, len(path) - 1]), path[:-1], d[:-1])
        assert short[0] == T[path[-2]]
        assert abs(np.float64(short[0]) + np.float64(geo["recv_dt"][r]) - np.float64(t_recv[r])) \
            <= np.spacing(t_recv[r])
    # the rays without a hop: a box's own start as its receiver
    assert nohop == sum(int(np.all(recv == st, axis=1).sum()) for st in starts) >= len(starts)
    full = R.replay(v, boxes[0], offsets[:len(recv) + 1], cells, hop_d)
    assert np.array_equal(full.view(np.uint32), t_recv[:len(recv)].view(np.uint32))


def test_adjoint_does_not_depend_on_the_order_of_the_pairs(group):
    v, fs, starts, boxes, recv, dense, rng = group
    box, pr = PR.cross_product(len(starts), recv)
    # duplicates: each occurrence is a ray of its own
    box = np.concatenate([box, box[:17]])
    pr = np.concatenate([pr, pr[:17]])
    w = rng.standard_normal(len(box))
    w[rng.random(len(box)) < 0.2] = 0
    m = rng.uniform(0.5, 2.0, v.size)
    dmax = O.entries_dmax(fs, v.shape)
    rays = PR.rays_of_pairs(v, boxes, fs, starts, box, pr)
    y, g, S, hits = PR.operators(rays, m, w, v.size, dmax)
    perm = rng.permutation(len(box))
    rays2 = PR.rays_of_pairs(v, boxes, fs, starts, box[perm], pr[perm])
    y2, g2, S2, hits2 = PR.operators(rays2, m, w[perm], v.size, dmax)
    assert S2 == S and np.array_equal(hits2, hits) and np.array_equal(g2.view(np.uint64), g.view(np.uint64))
    assert np.array_equal(y2.view(np.uint64), y[perm].view(np.uint64))
    assert np.array_equal(rays2[3], rays[3][perm])
    # a duplicated pair counts twice
    single = PR.rays_of_pairs(v, boxes, fs, starts, box[:-17], pr[:-17])
    assert int(hits.sum()) == int(O.hits(single[1], v.size).sum()) + int(np.diff(rays[0])[-17:].sum())


def test_pairs_from_locations_against_a_loop(pkg):
    rng = np.random.default_rng(8)
    E, K = 40, 7
    xyz = rng.integers(0, 9, (E, 3)).astype(np.int32)
    xyz[[3, 17, 39]] = -1                       # events without a cell
    w = rng.uniform(0.5, 2.0, (E, K))
    w[rng.random((E, K)) < 0.3] = 0.0
    w[5] = 0.0
    w[5, 4] = 1.5                               # an event with one pick
    w[17] = 1.0                                 # picked everywhere, but no cell
    w[0] = 0.0                                  # an event with no pick at all
    for weights, n in ((w, None), (None, K), (np.where(w != 0, -w, 0.0), None)):
        got = pkg.pairs_from_locations(xyz, weights, nstations=n)
        want = PR.pairs_from_locations_loop(xyz, weights, n)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    box, recv, ev, stn = pkg.pairs_from_locations(xyz, w)
    assert np.count_nonzero(ev == 5) == 1 and stn[ev == 5][0] == 4
    assert not np.isin(ev, [0, 3, 17, 39]).any()
    assert np.array_equal(box, stn) and np.array_equal(recv, xyz[ev]) and np.all(w[ev, stn] != 0)
    assert np.all(np.diff(ev * K + stn) > 0)    # (e, k) order
    n_all = pkg.pairs_from_locations(xyz, None, nstations=K)
    assert len(n_all[0]) == (E - 3) * K
    # a Locations result: its host xyz is used
    loc = pkg.Locations(cell=None, xyz=xyz, misfit=None, t0=None, volumes=None)
    assert all(np.array_equal(a, b) for a, b in zip(pkg.pairs_from_locations(loc, w), (box, recv, ev, stn)))
    with pytest.raises(pkg.TTSweepError):
        pkg.pairs_from_locations(xyz, None)
    empty = pkg.pairs_from_locations(np.zeros((0, 3), np.int32), np.zeros((0, K)))
    assert [len(a) for a in empty] == [0, 0, 0, 0] and empty[1].shape == (0, 3)


def test_ray_pair_symbols_exported_and_bound(pkg):
    L = pkg._lib.lib()
    bound = {n for n, _, _ in pkg._lib.SYMBOLS}
    for n in ("ttsweep_ray_pairs_forward_device", "ttsweep_ray_pairs_adjoint_device",
              "ttsweep_ray_pairs_geometry_device"):
        assert hasattr(L, n) and n in bound
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ttsweep.h")).read()
    assert "#define TTSWEEP_HAS_RAY_PAIRS 1" in hdr
    assert "#define TTSWEEP_ABI_VERSION 6" in hdr or "#define TTSWEEP_ABI_VERSION (6)" in hdr
    assert pkg.RayGeometry is pkg.solver.RayGeometry and pkg.pairs_from_locations is pkg.solver.pairs_from_locations
    assert "RayGeometry" in pkg.__all__ and "pairs_from_locations" in pkg.__all__
    assert hasattr(pkg.TravelTimeSolver, "ray_geometry")


def test_bad_pair_arguments_are_refused_without_a_device(pkg):
    L = pkg._lib.lib()
    st = (pkg._lib.Start * 1)(pkg._lib.Start(0, 0, 0))
    ptr = (C.c_void_p * 1)(None)
    box = (C.c_int * 1)(0)
    calls = {
        "ttsweep_ray_pairs_forward_device": lambda *a: L.ttsweep_ray_pairs_forward_device(*a, None, None, None),
        "ttsweep_ray_pairs_adjoint_device": lambda *a: L.ttsweep_ray_pairs_adjoint_device(*a, None, None, None, None),
        "ttsweep_ray_pairs_geometry_device": lambda *a: L.ttsweep_ray_pairs_geometry_device(*a, *([None] * 11)),
    }
    for name, call in calls.items():
        assert call(None, 1, st, ptr, ptr, 1, box, st) < 0                  # no context
        assert name in pkg._lib.last_error()
        assert call(None, -1, None, None, None, 0, None, None) < 0
        assert call(None, 0, None, None, None, -1, None, None) < 0
        assert "null or bad argument" in pkg._lib.last_error()
        assert call(None, 1, st, ptr, ptr, 1, None, st) < 0                 # pair_box NULL
        assert call(None, 1, st, ptr, ptr, 1, box, None) < 0                # pair_recv NULL
        assert "null or bad argument" in pkg._lib.last_error()
        # 2^31 pairs do not fit int32 ray indices: refused before the (one-element) arrays are read
        assert call(None, 1, st, ptr, ptr, 2 ** 31, box, st) < 0
        assert "int32" in pkg._lib.last_error()


def test_receiver_gradient_and_takeoff_are_plain_torch(pkg):
    import torch
    z = lambda *s: torch.zeros(*s)
    geo = pkg.RayGeometry(
        status=torch.zeros(3, dtype=torch.int32), t_recv=z(3), hops=torch.tensor([2, 0, 5], dtype=torch.int32),
        length=z(3).double(), recv_hop=torch.tensor([[1, -2, 2], [0, 0, 0], [0, 0, -1]], dtype=torch.int32),
        recv_d=z(3), recv_dt=torch.tensor([0.75, 0.0, 0.5]), src_hop=torch.tensor([[3, 4, 0], [0, 0, 0], [0, -1, 0]],
                                                                                   dtype=torch.int32),
        src_d=z(3), src_dt=z(3), deep=torch.zeros(3, dtype=torch.int32))
    g = geo.receiver_gradient()
    assert g.dtype == torch.float64 and g.shape == (3, 3)
    assert torch.equal(g, torch.tensor([[0.75 / 9, 0.75 * -2 / 9, 0.75 * 2 / 9], [0, 0, 0], [0, 0, -0.5]],
                                       dtype=torch.float64))
    t = geo.takeoff()
    assert torch.equal(t, torch.tensor([[0.6, 0.8, 0], [0, 0, 0], [0, -1, 0]], dtype=torch.float64))
    assert len(geo) == 3
