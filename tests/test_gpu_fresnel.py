"""GPU tier (-m gpu) of the Fresnel-volume calls (include/ttsweep.h, "fresnel"): ttsweep_fresnel_volume_device,
ttsweep_fresnel_forward_device and ttsweep_fresnel_adjoint_device, called as they are and through
TravelTimeSolver.fresnel_volumes / fresnel_operator, bit for bit against the numpy restatement
tests/fresnel_reference.py on boxes the library solved (or planted ones)."""
import ctypes as C

import numpy as np
import pytest

from conftest import Golden
import fresnel_reference as F

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64

# mirrored from csrc/ttsweep_fresnel.cpp and csrc/ttsweep_fresnel.hip
# (tests/test_fresnel_cpu.py::test_the_constants_mirror_the_sources)
LAUNCH_BLOCKS = 1 << 16
TILE_QUADS = 2048


@pytest.fixture(scope="module")
def P(pkg):
    assert pkg.device_count() > 0, "no HIP device: the GPU tier must run on an MI355X (there is no CPU fallback)"
    return pkg


def dev():
    import torch
    return torch.device("cuda:0")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def all_pairs(n):
    a, b = np.meshgrid(np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), indexing="ij")
    return a.reshape(-1), b.reshape(-1)


def four_starts(shape):
    """two near corners, two on faces"""
    nx, ny, nz = shape
    return np.array([[min(1, nx - 1), min(1, ny - 1), 1], [max(nx - 2, 0), max(ny - 2, 0), nz - 2],
                     [0, ny // 2, nz // 2], [nx // 2, ny - 1, nz // 3]], np.int32)


def solved(P, v, offs, starts):
    """(solver, boxes on the device, boxes on the host) of the starts, solved by the library"""
    import torch
    sol = P.TravelTimeSolver(v.shape, P.inputs.make_fs(offs))
    sol.set_velocity(np.ascontiguousarray(v, dtype=F32))
    tt = torch.empty((len(starts),) + tuple(v.shape), dtype=torch.float32, device=dev())
    sol.solve_device(starts, tt)
    return sol, tt, tt.cpu().numpy()


def weights(rng, n):
    """zeros, negatives and 2^-40 scales among normal values"""
    w = rng.standard_normal(n)
    w[rng.random(n) < 0.15] = 0.0
    w[rng.random(n) < 0.1] *= 2.0 ** -40
    return w


def raw_calls(sol, starts, tt, a, b, tau, lo=None, hi=None, m=None, w=None):
    """Every output of the three calls of the C ABI for one pair list, on the host: a dict of numpy arrays and
    scales.  Adjoint: g with hits, g alone, hits alone."""
    import torch
    args = sol._fresnel_args(starts, tt, a, b, tau, lo, hi)
    n = args[4]
    L = sol._L
    new = lambda dtype, *shape: torch.empty(tuple(shape), dtype=dtype, device=dev())
    out = {}
    st = np.full(n, -7, np.int32)
    t_ab, count, phi = new(torch.float32, n), new(torch.int64, n), new(torch.float64, n)
    blo, bhi = new(torch.int32, n, 3), new(torch.int32, n, 3)
    torch.cuda.synchronize()
    assert L.ttsweep_fresnel_volume_device(*args[:10], st.ctypes.data, t_ab.data_ptr(), count.data_ptr(),
                                           blo.data_ptr(), bhi.data_ptr(), phi.data_ptr()) == 0, P_err(sol)
    out["volume"] = dict(status=st, t_ab=t_ab.cpu().numpy(), count=count.cpu().numpy(), phi=phi.cpu().numpy(),
                         lo=blo.cpu().numpy(), hi=bhi.cpu().numpy())
    if m is not None:
        y, S, st2 = new(torch.float64, n), C.c_int(-99), np.full(n, -7, np.int32)
        md = to_dev(np.asarray(m, F64))
        torch.cuda.synchronize()
        assert L.ttsweep_fresnel_forward_device(*args[:10], md.data_ptr(), y.data_ptr(), st2.ctypes.data,
                                                C.byref(S)) == 0, P_err(sol)
        out["y"], out["S_m"], out["status_forward"] = y.cpu().numpy(), S.value, st2
    grid = sol.shape
    for key, use_w, use_h in (("both", True, True), ("g_alone", True, False), ("hits_alone", False, True)):
        if use_w and w is None:
            continue
        g = new(torch.float64, *grid) if use_w else None
        h = new(torch.int32, *grid) if use_h else None
        wd = to_dev(np.asarray(w, F64)) if use_w else None
        S, st3 = C.c_int(-99), np.full(n, -7, np.int32)
        torch.cuda.synchronize()
        assert L.ttsweep_fresnel_adjoint_device(
            *args[:10], None if wd is None else wd.data_ptr(), None if g is None else g.data_ptr(),
            None if h is None else h.data_ptr(), st3.ctypes.data, C.byref(S)) == 0, P_err(sol)
        out[key] = (None if g is None else g.cpu().numpy(), None if h is None else h.cpu().numpy(), S.value, st3)
    return out


def P_err(sol):
    return sol._L.ttsweep_last_error().decode()


def check(got, boxes, starts, a, b, tau, lo=None, hi=None, m=None, w=None, what=""):
    """The outputs of raw_calls equal to the restatement's, bit for bit"""
    vol = F.volume(boxes, starts, a, b, tau, lo, hi)
    for k in vol:
        assert same(got["volume"][k], vol[k]), f"{what}: volume {k}"
    if m is not None:
        y, S = F.forward(boxes, starts, a, b, tau, m, lo, hi)
        assert got["S_m"] == S and same(got["y"], y), f"{what}: forward"
        assert same(got["status_forward"], vol["status"]), what
    g, hits, S = F.adjoint(boxes, starts, a, b, tau, w, lo, hi)
    if w is not None:
        assert got["both"][2] == S and got["g_alone"][2] == S, f"{what}: S_w"
        assert same(got["both"][0], g) and same(got["g_alone"][0], g), f"{what}: g"
        assert same(got["both"][1], hits) and same(got["both"][3], vol["status"]), f"{what}: hits with g"
    assert same(got["hits_alone"][1], hits) and got["hits_alone"][2] == 0, f"{what}: hits alone"
    return vol


def taus(t_ab, mode):
    """tau per pair: a fraction of t_ab (0.5 where t_ab is 0: a == b), or one value for every pair"""
    if isinstance(mode, float):
        return np.full(len(t_ab), mode)
    return np.where(t_ab > 0, t_ab.astype(F64) / mode, 0.5)


# ---- 1. golden grids ----
GOLDEN_CASES = [(n, s) for n in ("g9", "g24") for s in ("six", "3", "5", "818")]


@pytest.mark.parametrize("name,star", GOLDEN_CASES, ids=["/".join(c) for c in GOLDEN_CASES])
def test_golden_grids(P, name, star):
    g = Golden(name)
    starts = four_starts(g.v.shape)
    sol, tt, boxes = solved(P, g.v, g.star(star), starts)
    with sol:
        a, b = all_pairs(4)
        t_ab, status = F.pair_times(boxes, starts, a, b)
        assert np.all(status == F.OK)
        rng = np.random.default_rng(len(name) + 10 * len(star))
        m = rng.uniform(-2.0, 2.0, g.v.shape)
        w = weights(rng, len(a))
        for mode in (64, 4, 1e-30, 1e30):
            tau = taus(t_ab, mode)
            got = raw_calls(sol, starts, tt, a, b, tau, m=m, w=w)
            vol = check(got, boxes, starts, a, b, tau, m=m, w=w, what=f"{name}/{star} tau {mode}")
            assert np.all(vol["count"] >= 1)
            if mode == 1e30:
                assert np.all(vol["count"] == g.v.size)
        # forward of ones is phi
        got = raw_calls(sol, starts, tt, a, b, tau, m=np.ones(g.v.shape))
        assert same(got["y"], got["volume"]["phi"]) and got["S_m"] == 60 - F.ceil_log2(g.v.size)


# ---- 2. ragged rows ----
@pytest.mark.parametrize("shape", [(3, 5, 67), (2, 3, 130)], ids=["3x5x67", "2x3x130"])
def test_ragged_rows_and_windows(P, shape):
    rng = np.random.default_rng(shape[2])
    v = rng.uniform(0.5, 2.0, shape).astype(F32)
    starts = four_starts(shape)
    sol, tt, boxes = solved(P, v, Golden("g9").star("3"), starts)
    with sol:
        a, b = all_pairs(4)
        t_ab, _ = F.pair_times(boxes, starts, a, b)
        tau = taus(t_ab, 8)
        m, w = rng.uniform(-2.0, 2.0, shape), weights(rng, len(a))
        top = np.asarray(shape) - 1
        lo_r = rng.integers(0, top // 2 + 1, (len(a), 3))
        hi_r = np.minimum(lo_r + rng.integers(0, top + 1, (len(a), 3)), top)
        windows = {
            "whole": (None, None),
            "one cell": ((1, 2, 33), (1, 2, 33)),
            "z segment": ((1, 2, 1), (1, 2, 65)),
            "x slab": ((1, 0, 0), (1, top[1], top[2])),
            "per pair": (lo_r, hi_r),
        }
        base = None
        for name, (lo, hi) in windows.items():
            got = raw_calls(sol, starts, tt, a, b, tau, lo, hi, m=m, w=w)
            check(got, boxes, starts, a, b, tau, lo, hi, m=m, w=w, what=f"{shape} {name}")
            if name == "whole":
                base = got
        # the volume's own bounding boxes as windows: the bits of the call without windows
        vols = sol.fresnel_volumes(starts, tt, a, b, tau)
        lo, hi = vols.windows()
        assert np.all(lo <= hi) and same(vols.phi.cpu().numpy(), base["volume"]["phi"])
        again = raw_calls(sol, starts, tt, a, b, tau, lo, hi, m=m, w=w)
        for k in base["volume"]:
            assert same(again["volume"][k], base["volume"][k]), k
        assert same(again["y"], base["y"]) and again["S_m"] == base["S_m"]
        for k in ("both", "g_alone", "hits_alone"):
            assert all(x is None and y is None or same(x, y) for x, y in zip(again[k], base[k])), k


# ---- 3. planted boxes ----
def test_planted_boxes(P):
    rng = np.random.default_rng(5)
    shape = (4, 3, 9)
    boxes = rng.uniform(0.0, 3.0, (3,) + shape).astype(F32)
    starts = np.array([[0, 0, 0], [3, 2, 8], [1, 1, 1]], np.int32)
    boxes[0, 1, 1, 2] = np.inf
    boxes[1, 2, 0, 0] = np.nan
    boxes[1, 2, 0, 1] = F32(np.uint32(0xffc00001).view(F32))        # a negative NaN with a payload
    # ... and in whole quads that start at a flat index divisible by 4 (rows 0 and 4 of 9 cells: quads at 0 and 40),
    # which the kernel reads with one 16-byte load per box; the cells above lie in quads it reads cell by cell
    assert ((0 * 3 + 0) * 9 + 0) % 4 == 0 and ((1 * 3 + 1) * 9 + 4) % 4 == 0 and boxes[0].size % 4 == 0
    boxes[1, 0, 0, 1] = np.nan
    boxes[0, 1, 1, 5] = np.nan
    boxes[1, 1, 1, 6] = np.inf
    boxes[0, 0, 2, 3] = -0.0
    boxes[1, 3, 1, 4] = -1.5
    boxes[0, 2, 2, 2] = -np.inf
    boxes[2, 0, 0, 0] = np.inf                  # t_ab of (2, 0)
    boxes[2, 3, 2, 8] = np.nan                  # t_ab of (2, 1)
    boxes[1, 1, 1, 1] = -np.inf                 # t_ab of (1, 2): below INFINITY, the pair is OK
    boxes[2, 2, 2, 2] = -np.inf                 # ... and -INF - -INF on one of its cells
    a, b = all_pairs(3)
    tau = np.full(len(a), 1.5)
    m, w = rng.uniform(-1.0, 1.0, shape), rng.uniform(-1.0, 1.0, len(a))
    w[0] = 1.5                                  # the largest weight is a kept pair's: E_w does not change below
    with P.TravelTimeSolver(shape, P.inputs.make_fs(Golden("g9").star("six"))) as sol:
        got = raw_calls(sol, starts, to_dev(boxes), a, b, tau, m=m, w=w)
        vol = check(got, boxes, starts, a, b, tau, m=m, w=w, what="planted")
        dead = (a == 2) & (b < 2)
        assert np.all(vol["status"][dead] == F.UNREACHED) and np.all(vol["status"][~dead] == F.OK)
        v = got["volume"]
        assert not v["count"][dead].any() and not v["phi"][dead].any() and not got["y"][dead].any()
        assert np.all(v["lo"][dead] == shape) and np.all(v["hi"][dead] == -1)
        assert np.isnan(v["t_ab"][(a == 2) & (b == 1)]).all() and np.isinf(v["t_ab"][(a == 2) & (b == 0)]).all()
        # they add nothing to hits: the list without them counts the same
        keep = ~dead
        less = raw_calls(sol, starts, to_dev(boxes), a[keep], b[keep], tau[keep], w=w[keep])
        assert same(less["both"][1], got["both"][1]) and same(less["hits_alone"][1], got["hits_alone"][1])
        # ... and nothing to g: with two pairs of weight zero in their place (K_p and E_w as before) the same bits
        pad = lambda x, v: np.concatenate([x[keep], np.full(2, v, x.dtype)])
        padded = raw_calls(sol, starts, to_dev(boxes), pad(a, 0), pad(b, 0), pad(tau, 1.5), w=pad(w, 0.0))
        assert padded["both"][2] == got["both"][2] and same(padded["both"][0], got["both"][0])
        assert np.isfinite(got["both"][0]).all() and np.isfinite(got["y"]).all()


# ---- 4. scales ----
def test_scales_and_degenerate_lists(P):
    import torch
    g = Golden("g9")
    starts = four_starts(g.v.shape)
    sol, tt, boxes = solved(P, g.v, g.star("5"), starts)
    rng = np.random.default_rng(44)
    with sol:
        a, b = all_pairs(4)
        t_ab, _ = F.pair_times(boxes, starts, a, b)
        tau = taus(t_ab, 4)
        for scale in (1.0, 2.0 ** -40, 2.0 ** 30):
            m = weights(rng, g.v.size).reshape(g.v.shape) * scale
            w = weights(rng, len(a)) * scale
            check(raw_calls(sol, starts, tt, a, b, tau, m=m, w=w), boxes, starts, a, b, tau, m=m, w=w,
                  what=f"scale {scale}")
        # all zero
        m0, w0 = np.zeros(g.v.shape), np.zeros(len(a))
        m0[1, 1, 1] = -0.0
        got = raw_calls(sol, starts, tt, a, b, tau, m=m0, w=w0)
        check(got, boxes, starts, a, b, tau, m=m0, w=w0, what="all zero")
        assert got["S_m"] == 0 and not got["y"].any() and got["both"][2] == 0 and not got["both"][0].any()
        assert got["both"][1].any()
        # no pair at all: g and hits zeroed, S = 0
        e = np.zeros(0, np.int32)
        got = raw_calls(sol, starts, tt, e, e, np.zeros(0), m=np.ones(g.v.shape), w=np.zeros(0))
        assert got["both"][2] == 0 and not got["both"][0].any() and not got["both"][1].any()
        assert got["both"][0].shape == g.v.shape and got["S_m"] == 60 - F.ceil_log2(g.v.size)
        assert not got["hits_alone"][1].any()
        # one pair: K_p = 0
        check(raw_calls(sol, starts, tt, a[6:7], b[6:7], tau[6:7], m=m, w=np.array([-3.0])), boxes, starts, a[6:7],
              b[6:7], tau[6:7], m=m, w=np.array([-3.0]), what="one pair")
        # a pair three times: each occurrence counts
        a3, b3, tau3 = np.repeat(a[6:8], 3), np.repeat(b[6:8], 3), np.repeat(tau[6:8], 3)
        w3 = weights(rng, 6)
        got = raw_calls(sol, starts, tt, a3, b3, tau3, m=m, w=w3)
        vol = check(got, boxes, starts, a3, b3, tau3, m=m, w=w3, what="repeated")
        assert int(got["hits_alone"][1].sum()) == int(vol["count"].sum()) == 3 * int(vol["count"][::3].sum())
    # one pair and one cell: K_c = K_p = 0
    one = np.zeros((1, 1, 1, 1), F32)
    with P.TravelTimeSolver((1, 1, 1), P.inputs.make_fs(g.star("six"))) as sol:
        z = np.zeros(1, np.int32)
        st = np.zeros((1, 3), np.int32)
        m, w = np.full((1, 1, 1), 1.75), np.array([-0.3])
        got = raw_calls(sol, st, to_dev(one), z, z, np.array([2.0]), m=m, w=w)
        check(got, one, st, z, z, np.array([2.0]), m=m, w=w, what="one cell")
        assert got["volume"]["count"][0] == 1 and got["volume"]["phi"][0] == 1.0 and got["y"][0] == 1.75
        assert got["S_m"] == 60 and got["both"][2] == 62 and got["both"][0][0, 0, 0] == -0.3


# ---- 5. order and repeatability ----
def test_order_repeatability_and_the_solve_shortcut(P):
    import torch
    g = Golden("g24")
    starts = four_starts(g.v.shape)
    sol, tt, boxes = solved(P, g.v, g.star("818"), starts)
    rng = np.random.default_rng(3)
    with sol:
        changed = sol.changed(len(starts))
        before = tt.clone()
        a, b = all_pairs(4)
        a, b = np.concatenate([a, a[:5]]), np.concatenate([b, b[:5]])
        t_ab, _ = F.pair_times(boxes, starts, a, b)
        tau = taus(t_ab, 16)
        m, w = rng.uniform(-2.0, 2.0, g.v.shape), weights(rng, len(a))
        one = raw_calls(sol, starts, tt, a, b, tau, m=m, w=w)
        two = raw_calls(sol, starts, tt, a, b, tau, m=m, w=w)
        p = rng.permutation(len(a))
        perm = raw_calls(sol, starts, tt, a[p], b[p], tau[p], m=m, w=w[p])
        check(one, boxes, starts, a, b, tau, m=m, w=w, what="order")
        for k in one["volume"]:
            assert same(one["volume"][k], two["volume"][k]) and same(one["volume"][k][p], perm["volume"][k]), k
        assert same(one["y"], two["y"]) and same(one["y"][p], perm["y"]) and one["S_m"] == perm["S_m"]
        for k in ("both", "g_alone", "hits_alone"):
            for x, y, z in zip(one[k][:3], two[k][:3], perm[k][:3]):
                assert x is None and y is None and z is None or (same(x, y) and same(x, z)), k
        assert torch.equal(tt.view(torch.int32), before.view(torch.int32))
        assert sol.changed(len(starts)) == changed
        assert sol.solve_device(starts, tt, init=False) == 0          # still answered as a confirming pass
    # host boxes: the solve after the calls is answered without device work
    hb = []
    for st in starts[:2]:
        box = np.full(g.v.shape, np.inf, F32)
        box[tuple(st)] = 0
        hb.append(box)
    with P.TravelTimeSolver(g.v.shape, P.inputs.make_fs(g.star("818"))) as sol:
        sol.set_velocity(g.v)
        assert sol.solve(starts[:2], hb) == 1 and sol.stats()["sweeps_total"] > 0
        op = sol.fresnel_operator(starts[:2], to_dev(np.stack(hb)), [0, 1], [1, 0], 0.5)
        op.matvec(torch.ones(op.shape[1], dtype=torch.float64, device=dev()))
        op.rmatvec_hits(torch.ones(op.shape[0], dtype=torch.float64, device=dev()))
        assert sol.solve(starts[:2], hb) == 0 and sol.stats()["sweeps_total"] == 0
        assert sol.changed(2) == [0, 0]


# ---- 6. the launch edge ----
def test_a_launch_edge(P):
    """LAUNCH_BLOCKS + 1 pairs on a grid of one tile per pair (5 x 5 x 64: 400 quads), so the blocks of the call are
    one full launch and a second one of a single block, the last pair's.  The pairs cycle through the sixteen (a, b),
    two windows and five weights, which the restatement evaluates once each."""
    shape = (5, 5, 64)
    assert shape[0] * shape[1] * (shape[2] // 4) <= TILE_QUADS
    rng = np.random.default_rng(6)
    v = rng.uniform(0.5, 2.0, shape).astype(F32)
    starts = four_starts(shape)
    sol, tt, boxes = solved(P, v, Golden("g9").star("six"), starts)
    with sol:
        n = LAUNCH_BLOCKS + 1
        i = np.arange(n)
        a, b = ((i % 16) // 4).astype(np.int32), (i % 4).astype(np.int32)
        t_ab, _ = F.pair_times(boxes, starts, a, b)
        tau = taus(t_ab, 16)
        sub = (i // 16) % 2 == 1
        lo = np.where(sub[:, None], np.array([1, 0, 3]), np.array([0, 0, 0])).astype(np.int32)
        hi = np.where(sub[:, None], np.array([3, 4, 40]), np.array(shape) - 1).astype(np.int32)
        w = np.array([1.0, -0.5, 0.0, 2.0 ** -20, 3.25])[(i // 32) % 5]
        m = rng.uniform(-2.0, 2.0, shape)
        got = raw_calls(sol, starts, tt, a, b, tau, lo, hi, m=m, w=w)
        vol = check(got, boxes, starts, a, b, tau, lo, hi, m=m, w=w, what="launch edge")
        assert vol["count"][-1] >= 1 and got["both"][2] == 61 - 2 - 17


def test_a_launch_edge_inside_a_pair_and_the_tile_edge(P):
    """Pairs of four tiles past LAUNCH_BLOCKS blocks, so that the second launch begins in the middle of a pair whose
    first tiles closed the first launch.  The grid is 1 x 3 x 4 (TILE_QUADS + 1): a row holds one quad more than a
    tile, the whole grid three full tiles and a tile of three quads.  In front of those pairs, two whose windows hold
    exactly TILE_QUADS quads (one full tile) and TILE_QUADS + 1 (a full tile and a tile of one quad).  Planted boxes:
    the calls are defined for any floats, and no solve is needed."""
    T = TILE_QUADS
    shape = (1, 3, 4 * (T + 1))
    rng = np.random.default_rng(66)
    boxes = rng.uniform(0.0, 3.0, (4,) + shape).astype(F32)
    starts = np.array([[0, 0, 0], [0, 1, 5], [0, 2, 77], [0, 1, 4 * T]], np.int32)
    top = np.array(shape, np.int32) - 1
    edge_lo = np.array([[0, 1, 4], [0, 2, 0]], np.int32)
    edge_hi = np.array([[0, 1, 4 * T + 3], [0, 2, top[2]]], np.int32)
    quads = lambda l, h: int((h[0] - l[0] + 1) * (h[1] - l[1] + 1) * ((h[2] - l[2] + 1 + 3) // 4))
    assert [quads(l, h) for l, h in zip(edge_lo, edge_hi)] == [T, T + 1]
    whole = quads((0, 0, 0), top)
    per = -(-whole // T)
    assert per == 4 and whole % T == 3
    n = 2 + LAUNCH_BLOCKS // per + 1
    tiles = np.concatenate([[1, 2], np.full(n - 2, per)])
    first = np.concatenate([[0], np.cumsum(tiles)])
    r = int(np.searchsorted(first, LAUNCH_BLOCKS, side="right")) - 1         # the pair that holds block LAUNCH_BLOCKS
    assert r >= 2 and first[r] < LAUNCH_BLOCKS < first[r + 1] - 1 and first[-1] > LAUNCH_BLOCKS
    i = np.arange(n)
    a, b = ((i % 16) // 4).astype(np.int32), (i % 4).astype(np.int32)
    tau = np.where(a == b, 0.5, 0.75)
    lo, hi = np.zeros((n, 3), np.int32), np.tile(top, (n, 1))
    lo[:2], hi[:2] = edge_lo, edge_hi
    w = np.array([1.0, -0.5, 0.0, 2.0 ** -20, 3.25])[(i // 16) % 5]
    m = rng.uniform(-2.0, 2.0, shape)
    with P.TravelTimeSolver(shape, P.inputs.make_fs(Golden("g9").star("six"))) as sol:
        got = raw_calls(sol, starts, to_dev(boxes), a, b, tau, lo, hi, m=m, w=w)
        vol = check(got, boxes, starts, a, b, tau, lo, hi, m=m, w=w, what="launch edge inside a pair")
        assert vol["count"][r] >= 1 and vol["count"][0] >= 1 and vol["count"][1] >= 1


# ---- 7. refusals ----
def test_refusals_leave_the_outputs(P):
    import torch
    rng = np.random.default_rng(1)
    shape = (6, 5, 4)
    N = int(np.prod(shape))
    tt = to_dev(rng.uniform(0, 5, (3,) + shape).astype(F32))
    starts = np.array([[0, 0, 0], [5, 4, 3], [2, 2, 2]], np.int32)
    good = dict(nbox=3, starts=starts, a=np.array([0, 1, 2, 0], np.int32), b=np.array([1, 2, 0, 0], np.int32),
                tau=np.array([1.0, 2.0, 0.5, 1.0]), lo=np.zeros((4, 3), np.int32),
                hi=np.tile(np.array(shape, np.int32) - 1, (4, 1)), npair=4, m=np.ones(N), w=np.ones(4),
                null=(), ctx=True, boxnull=False)

    def edit(key, idx, val):
        arr = good[key].copy()
        arr[idx] = val
        return {key: arr}

    cases = [
        (dict(nbox=0), "bad argument"), (dict(npair=-1), "bad argument"), (dict(npair=2 ** 31), "int32"),
        (dict(null=("starts",)), "bad argument"), (dict(null=("tt",)), "bad argument"),
        (dict(null=("a",)), "bad argument"), (dict(null=("b",)), "bad argument"),
        (dict(null=("tau",)), "bad argument"), (dict(ctx=False), "bad argument"),
        (dict(null=("lo",)), "both"), (dict(null=("hi",)), "both"), (dict(boxnull=True), "null box pointer 1"),
        (edit("starts", (1, 0), 6), "start 1"), (edit("starts", (2, 2), -1), "start 2"),
        (edit("a", 2, 3), "pair 2"), (edit("b", 1, -1), "pair 1"),
        (edit("tau", 3, np.nan), "pair 3"), (edit("tau", 0, np.inf), "pair 0"), (edit("tau", 1, 0.0), "pair 1"),
        (edit("tau", 1, -0.0), "pair 1"), (edit("tau", 2, -1.0), "pair 2"),
        (edit("lo", (1, 1), -1), "pair 1"), (edit("hi", (2, 0), 6), "pair 2"), (edit("lo", (3, 2), 3), None),
        (dict(lo=edit("lo", (3, 2), 3)["lo"], hi=edit("hi", (3, 2), 2)["hi"]), "pair 3"),
    ]
    device_cases = [(edit("m", 7, np.nan), "forward", "m"), (edit("m", N - 1, -np.inf), "forward", "m"),
                    (edit("w", 2, np.nan), "adjoint", "w"), (edit("w", 0, np.inf), "adjoint", "w")]

    with P.TravelTimeSolver(shape, P.inputs.make_fs(Golden("g9").star("six"))) as sol:
        L = sol._L

        def attempt(change, which):
            c = {**good, **change}
            n = 4
            keep = [np.ascontiguousarray(c[k]) for k in ("a", "b", "tau", "lo", "hi")]
            ptr = {k: (None if k in c["null"] else arr.ctypes.data) for k, arr in zip(("a", "b", "tau", "lo", "hi"), keep)}
            sarr = sol._starts_array(c["starts"])
            boxes = sol._box_pointers(tt, 3)
            if c["boxnull"]:
                boxes[1] = None
            shared = (sol._ctx if c["ctx"] else None, c["nbox"], None if "starts" in c["null"] else sarr,
                      None if "tt" in c["null"] else boxes, c["npair"], ptr["a"], ptr["b"], ptr["tau"], ptr["lo"],
                      ptr["hi"])
            st = np.full(n, -7, np.int32)
            S = C.c_int(-99)
            outs = {"t_ab": torch.full((n,), 9.5, dtype=torch.float32, device=dev()),
                    "count": torch.full((n,), 77, dtype=torch.int64, device=dev()),
                    "lo": torch.full((n, 3), 77, dtype=torch.int32, device=dev()),
                    "hi": torch.full((n, 3), 77, dtype=torch.int32, device=dev()),
                    "phi": torch.full((n,), 3.5, dtype=torch.float64, device=dev()),
                    "y": torch.full((n,), 3.5, dtype=torch.float64, device=dev()),
                    "g": torch.full(shape, 3.5, dtype=torch.float64, device=dev()),
                    "hits": torch.full(shape, 77, dtype=torch.int32, device=dev())}
            md, wd = to_dev(np.asarray(c["m"], F64)), to_dev(np.asarray(c["w"], F64))
            torch.cuda.synchronize()
            if which == "volume":
                rc = L.ttsweep_fresnel_volume_device(*shared, st.ctypes.data, outs["t_ab"].data_ptr(),
                                                     outs["count"].data_ptr(), outs["lo"].data_ptr(),
                                                     outs["hi"].data_ptr(), outs["phi"].data_ptr())
            elif which == "forward":
                rc = L.ttsweep_fresnel_forward_device(*shared, md.data_ptr(), outs["y"].data_ptr(), st.ctypes.data,
                                                      C.byref(S))
            else:
                rc = L.ttsweep_fresnel_adjoint_device(*shared, wd.data_ptr(), outs["g"].data_ptr(),
                                                      outs["hits"].data_ptr(), st.ctypes.data, C.byref(S))
            msg = P_err(sol)
            torch.cuda.synchronize()
            untouched = np.all(st == -7) and S.value == -99 and all(
                bool((t == (77 if t.dtype in (torch.int32, torch.int64) else 9.5 if t.dtype == torch.float32 else 3.5))
                     .all()) for t in outs.values())
            return rc, msg, untouched

        names = {"volume": "ttsweep_fresnel_volume_device", "forward": "ttsweep_fresnel_forward_device",
                 "adjoint": "ttsweep_fresnel_adjoint_device"}
        for which, name in names.items():
            rc, msg, untouched = attempt({}, which)
            assert rc == 0 and not untouched, which                     # the unedited call is accepted
            for change, text in cases:
                rc, msg, untouched = attempt(change, which)
                if text is None:                                        # lo == hi: a one-cell extent is a window
                    assert rc == 0, (which, change, msg)
                    continue
                assert rc < 0 and untouched, (which, change, msg)
                assert name in msg and text in msg, (which, change, msg)
        for change, which, text in device_cases:
            rc, msg, untouched = attempt(change, which)
            assert rc < 0 and untouched and names[which] in msg and f"{text} holds a NaN or infinite" in msg, msg
        # w without g, g without w, a NULL m, a NULL y
        args = sol._fresnel_args(starts, tt, good["a"], good["b"], good["tau"], None, None)
        buf = torch.full(shape, 3.5, dtype=torch.float64, device=dev())
        assert L.ttsweep_fresnel_adjoint_device(*args[:10], buf.data_ptr(), None, None, None, None) < 0
        assert "both" in P_err(sol)
        assert L.ttsweep_fresnel_adjoint_device(*args[:10], None, buf.data_ptr(), None, None, None) < 0
        assert L.ttsweep_fresnel_forward_device(*args[:10], None, buf.data_ptr(), None, None) < 0
        assert L.ttsweep_fresnel_forward_device(*args[:10], buf.data_ptr(), None, None, None) < 0
        assert "bad argument" in P_err(sol) and bool((buf == 3.5).all())
        # the Python layer refuses what would be an out-of-bounds read
        with pytest.raises(P.TTSweepError):
            sol.fresnel_volumes(starts, tt, [0, 1], [1], 1.0)
        with pytest.raises(P.TTSweepError):
            sol.fresnel_volumes(starts, tt, [0, 5], [1, 0], 1.0)
        with pytest.raises(P.TTSweepError):
            sol.fresnel_volumes(starts, tt.double(), [0], [1], 1.0)


def test_a_grid_beyond_int32_cells_is_refused(P):
    """2048 x 1024 x 1024 = 2^31 cells, one more than INT32_MAX: each call refuses before it reads a box or touches
    an output.  The context of such a grid holds one padded velocity volume (8.7 GB, allocated and never written);
    the boxes handed over are small ones, which a refusal never reads, the pair is (0, 0) with a one-cell window."""
    import torch
    shape = (2048, 1024, 1024)
    assert int(np.prod(shape, dtype=np.int64)) == 2 ** 31
    small = to_dev(np.zeros((1, 4, 4, 4), F32))
    with P.TravelTimeSolver(shape, P.inputs.make_fs(Golden("g9").star("six"))) as sol:
        L = sol._L
        st = sol._starts_array(np.zeros((1, 3), np.int32))
        boxes = sol._box_pointers(small, 1)
        z, tau, win = np.zeros(1, np.int32), np.ones(1), np.zeros((1, 3), np.int32)
        shared = (sol._ctx, 1, st, boxes, 1, z.ctypes.data, z.ctypes.data, tau.ctypes.data, win.ctypes.data,
                  win.ctypes.data)
        full = lambda dtype, val, *s: torch.full(s, val, dtype=dtype, device=dev())
        outs = [full(torch.float32, 9.5, 1), full(torch.int64, 77, 1), full(torch.int32, 77, 1, 3),
                full(torch.int32, 77, 1, 3), full(torch.float64, 3.5, 1)]
        y, g, hits = full(torch.float64, 3.5, 1), full(torch.float64, 3.5, 64), full(torch.int32, 77, 64)
        mw = full(torch.float64, 1.0, 64)
        status, S = np.full(1, -7, np.int32), C.c_int(-99)
        torch.cuda.synchronize()
        calls = {
            "ttsweep_fresnel_volume_device": lambda: L.ttsweep_fresnel_volume_device(
                *shared, status.ctypes.data, *(t.data_ptr() for t in outs)),
            "ttsweep_fresnel_forward_device": lambda: L.ttsweep_fresnel_forward_device(
                *shared, mw.data_ptr(), y.data_ptr(), status.ctypes.data, C.byref(S)),
            "ttsweep_fresnel_adjoint_device": lambda: L.ttsweep_fresnel_adjoint_device(
                *shared, mw.data_ptr(), g.data_ptr(), hits.data_ptr(), status.ctypes.data, C.byref(S)),
        }
        for name, call in calls.items():
            assert call() < 0, name
            msg = P_err(sol)
            assert name in msg and "2048 x 1024 x 1024 cells do not fit int32" in msg, msg
        torch.cuda.synchronize()
        assert status[0] == -7 and S.value == -99
        for t, val in zip(outs + [y, g, hits], (9.5, 77, 77, 77, 3.5, 3.5, 3.5, 77)):
            assert bool((t == val).all())


# ---- 8. the operator ----
def test_the_operator(P):
    import torch
    g = Golden("g24")
    shape = g.v.shape
    starts = four_starts(shape)
    sol, tt, boxes = solved(P, g.v, g.star("5"), starts)
    rng = np.random.default_rng(12)
    with sol:
        a, b = all_pairs(4)
        recv = starts[b]
        geo = sol.ray_geometry(starts, tt, a, recv)
        t_ab, _ = F.pair_times(boxes, starts, a, b)
        tau = taus(t_ab, 8)
        op = sol.fresnel_operator(starts, tt, a, b, tau, norm=geo.length)
        plain = sol.fresnel_operator(starts, tt, a, b, tau, norm=geo.length, windows=False)
        unit = sol.fresnel_operator(starts, tt, a, b, tau)
        assert op.shape == (16, g.v.size) and same(op.status.numpy(), np.zeros(16, np.int32))
        vol = F.volume(boxes, starts, a, b, tau)
        for k in ("t_ab", "count", "phi", "lo", "hi"):
            assert same(getattr(op.volumes, k).cpu().numpy(), vol[k]), k
        lo, hi = op.volumes.windows()
        assert same(lo, vol["lo"]) and same(hi, vol["hi"])
        # matvec is coef * y_raw formed in torch, bit for bit; a == b has length 0, so a zero row
        m = to_dev(rng.uniform(0.5, 2.0, shape))
        w = to_dev(weights(rng, 16))
        coef = torch.where(op.volumes.phi > 0, geo.length / op.volumes.phi, torch.zeros_like(op.volumes.phi))
        assert torch.equal(op.coef, coef) and torch.equal(unit.coef, 1.0 / unit.volumes.phi)
        y_raw, S_m = F.forward(boxes, starts, a, b, tau, m.cpu().numpy())
        y = op.matvec(m)
        assert same(y.cpu().numpy(), (coef * to_dev(y_raw)).cpu().numpy()) and op.last_forward_scale == S_m
        assert not y.cpu().numpy()[a == b].any()
        # a row sums to the thin ray's length: matvec of ones
        ones = torch.ones(shape, dtype=torch.float64, device=dev())
        rows = op.matvec(ones).cpu().numpy()
        assert np.allclose(rows, geo.length.cpu().numpy(), rtol=1e-12, atol=0)
        assert np.allclose(unit.matvec(ones).cpu().numpy(), 1.0, rtol=1e-12, atol=0)
        # rmatvec is F^T (coef * w)
        gw, hits = op.rmatvec_hits(w)
        want_g, want_h, S_w = F.adjoint(boxes, starts, a, b, tau, (coef * w).cpu().numpy())
        assert op.last_scale == S_w and same(gw.cpu().numpy(), want_g) and same(hits.cpu().numpy(), want_h)
        assert same(op.rmatvec(w).cpu().numpy(), want_g) and same(op.hits().cpu().numpy(), want_h)
        # windows=True and windows=False: equal bits
        assert same(plain.matvec(m).cpu().numpy(), y.cpu().numpy())
        gp, hp = plain.rmatvec_hits(w)
        assert torch.equal(gp, gw) and torch.equal(hp, hits) and plain.last_scale == op.last_scale
        # the adjoint identity <F m, w'> = <m, F^T w'> with w' = coef * w, within the rounding of the fixed-point
        # terms (half a unit of 2^-S per visit: at most ncells visits per pair, npair per cell) and of the two dot
        # products in float64 (n terms: n * eps * sum |x_i y_i|, Higham's gamma_n to first order)
        wp = (coef * w).cpu().numpy()
        mh = m.cpu().numpy().reshape(-1)
        lhs_terms = unit.forward_raw(m).cpu().numpy() * wp
        rhs_terms = mh * gw.cpu().numpy().reshape(-1)
        eps = np.finfo(F64).eps
        bound = (2.0 ** -S_m * g.v.size / 2 * np.abs(wp).sum() + 2.0 ** -S_w * 16 / 2 * np.abs(mh).sum()
                 + 16 * eps * np.abs(lhs_terms).sum() + g.v.size * eps * np.abs(rhs_terms).sum())
        gap = abs(float(np.sum(lhs_terms)) - float(np.sum(rhs_terms)))
        print(f"adjoint identity: gap {gap:.3e}, bound {bound:.3e}")
        assert gap <= bound
        # lsqr takes the operator as it is
        m_true = to_dev(rng.uniform(0.5, 2.0, g.v.size))
        rhs = op.matvec(m_true)
        x, istop, itn, r1norm = P.lsqr(op, rhs, iter_lim=8)
        start = float(torch.linalg.vector_norm(rhs))
        print(f"lsqr: istop {istop}, itn {itn}, r1norm {r1norm:.3e} from {start:.3e}")
        assert x.shape == (g.v.size,) and itn >= 1 and r1norm < start
