"""GPU tier (-m gpu) of sub-cell event location (include/ttsweep.h, "locate subcell"): ttsweep_locate_subcell_device
through TravelTimeSolver.locate_subcell and the driver locate_fine, bit for bit (through u64, no tolerances) against
the numpy restatement tests/locate_subcell_reference.py, and against locate / locate_window where the header says they
agree."""
import numpy as np
import pytest

import locate_cases as Cs
import locate_subcell_reference as S
import locate_window_reference as W

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)
TILE = 8 * 256              # LOC_SC * LOC_BLOCK: nodes of one block of locate_subcell_search_kernel
STAGE = 4096                # LOC_SUB_STAGE: floats (stations x cells of a window) a block stages in LDS, at most
ET = 8                      # LOC_WIN_ET: events of a group, at most
PARTIALS = 1 << 24          # LOC_PARTIALS and LOC_WIN_BLOCKS of ttsweep_locate.cpp: partials and blocks of a batch
BLOCKS = 1 << 22


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


def outputs(res):
    return res.node.cpu().numpy(), res.misfit.cpu().numpy(), res.t0.cpu().numpy()


def same(got, want, what=""):
    """(node or cell, misfit, t0) equal on the bits; the NaN of t0 is the quiet NaN 0x7ff8000000000000 on both sides"""
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(u64(got[1]), u64(want[1])), what
    assert np.array_equal(u64(got[2]), u64(want[2])), what


def staged(K, lo, hi):
    """the blocks of a window stage it in LDS (the host's rule, mirrored)"""
    return K * int(np.prod(np.asarray(hi) - np.asarray(lo) + 1)) <= STAGE


def check_subcell(sol, tt, picks, w=None, lo=None, hi=None, sub=8, what=""):
    """locate_subcell on the device == the restatement; returns the device outputs as numpy"""
    import torch
    tt = np.ascontiguousarray(tt, dtype=F32)
    res = sol.locate_subcell(torch.from_numpy(tt).to(dev()), picks, w, lo, hi, sub)
    assert res.node.dtype == torch.int32 and res.node.device == dev() and tuple(res.node.shape) == (len(picks), 3)
    assert res.sub == sub
    got = outputs(res)
    same(got, S.locate_subcell(tt, picks, w, lo, hi, sub), what)
    none = np.all(got[0] == -1, axis=1)
    assert np.all(np.isnan(res.position[none])) and np.array_equal(res.position[~none], got[0][~none] / float(sub))
    return got


def random_box(seed, K=4, shape=Cs.RANGE_SHAPE, inf_share=0.05):
    rng = np.random.default_rng(seed)
    tt = rng.uniform(0, 9, (K,) + tuple(shape)).astype(F32)
    tt[rng.random(tt.shape) < inf_share] = INF
    return rng, tt


def events(rng, E, K, drop=0.2):
    picks = rng.uniform(0, 12, (E, K))
    w = rng.uniform(0.5, 2.0, (E, K))
    w[rng.random((E, K)) < drop] = 0.0
    w[np.arange(E), rng.integers(0, K, E)] = 1.0      # at least one pick per event
    return picks, w


def seeded_windows(rng, shape, E):
    lo = np.stack([rng.integers(0, n, E) for n in shape], 1)
    hi = np.stack([rng.integers(lo[:, a], shape[a]) for a in range(3)], 1)
    return lo, hi


# ---- sub = 1 is locate_window, and on the whole grid locate ----
def test_whole_grid_sub_one_equals_locate_and_locate_window(P):
    import torch
    shape = Cs.RANGE_SHAPE
    rng, tt = random_box(11)
    tt[1, 2, 3, 4] = F32(-0.0)
    picks, w = events(rng, 12, 4)
    lo, hi = seeded_windows(rng, shape, 12)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        tdev = torch.from_numpy(tt).to(dev())
        for ww in (w, None):
            got = check_subcell(sol, tt, picks, ww, sub=1)
            for other in (sol.locate(tdev, picks, ww), sol.locate_window(tdev, picks, ww)):
                same((got[0], got[1], got[2]), (other.xyz.numpy(), other.misfit.cpu().numpy(), other.t0.cpu().numpy()))
        got = check_subcell(sol, tt, picks, w, lo, hi, sub=1, what="windows")
        other = sol.locate_window(tdev, picks, w, lo, hi)
        same(got, (other.xyz.numpy(), other.misfit.cpu().numpy(), other.t0.cpu().numpy()), "windows")
        for sub in (2, 3, 16):                          # property 3
            finer = check_subcell(sol, tt, picks, w, lo, hi, sub=sub, what=f"sub {sub}")
            assert np.all(u64(finer[1]) <= u64(got[1])), "J >= +0: the order of the bits is the order of the values"


# ---- the register instances ----
@pytest.mark.parametrize("K", [8, 9, 24, 33])
def test_register_widths(P, K):
    """a full register instance, one over, the 24 of the bench and the interpolate-on-use instance, at sub = 3 on
    17 x 1 x 241: lo = hi along y, whose upper corner must never be read.  The whole grid reads its corners from the
    boxes, the window from LDS."""
    c = Cs.k_edge_case(K, 4097)
    lo, hi = (3, 0, 100), (6, 0, 125)
    assert c["shape"][1] == 1 and not staged(K, (0, 0, 0), np.array(c["shape"]) - 1) and staged(K, lo, hi)
    with P.TravelTimeSolver(c["shape"], star818(P)) as sol:
        for picks, w in ((c["picks"], c["weights"]), (c["none"]["picks"], None)):
            check_subcell(sol, c["tt"], picks, w, sub=3, what=f"K={K}")
            check_subcell(sol, c["tt"], picks, w, lo, hi, sub=3, what=f"K={K} window")


# ---- windows on the upper faces, both corner paths ----
@pytest.mark.parametrize("sub", [2, 8, 64])
def test_windows_that_touch_the_upper_faces(P, sub):
    """hi = n - 1 on every axis: a wrong j reads out of the box or out of the window.  A single cell (one node), the
    corner's 2 x 2 x 2 cells, a column; at sub 2 and 8, with 24 stations, also a window of 140 cells and the whole
    grid, which is beyond the staging limit"""
    shape = Cs.RANGE_SHAPE
    K = 24 if sub < 64 else 6
    rng, tt = random_box(sub, K=K, inf_share=0.01)
    top = np.array(shape) - 1
    los = [top, top - 1, (top[0], top[1], 0)] + ([(1, 2, 4), (0, 0, 0)] if sub < 64 else [])
    assert sub == 64 or (staged(K, los[3], top) and not staged(K, los[4], top))
    lo = np.array(los)
    hi = np.tile(top, (len(lo), 1))
    picks, w = events(rng, len(lo), K)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        node, _, _ = check_subcell(sol, tt, picks, w, lo, hi, sub)
        check_subcell(sol, tt, picks[:3], None, lo[:3], hi[:3], sub, "no weights")
    assert np.all(node[0] == top * sub) or np.all(node[0] == -1), "a single cell is a single node"


def test_both_corner_paths(P):
    """one call with windows on either side of the staging limit, interleaved; the same window scored from LDS and,
    among more stations, from the boxes gives the same bits where the extra stations are not picked"""
    import torch
    shape = Cs.RANGE_SHAPE
    K = 24
    rng, tt = random_box(77, K=K, inf_share=0.01)
    small, large = ((1, 2, 3), (4, 6, 9)), ((0, 0, 0), (4, 6, 10))
    assert staged(K, *small) and K * 4 * 5 * 7 == 3360 and not staged(K, *large)
    E = 4
    lo = np.array([small[0], large[0]] * 2)
    hi = np.array([small[1], large[1]] * 2)
    picks, w = events(rng, E, K)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        check_subcell(sol, tt, picks, w, lo, hi, 4)
        # 30 stations: the small window is 4200 floats, not staged; the six new stations are not picked
        assert not staged(30, *small)
        tt30 = np.concatenate([tt, rng.uniform(0, 9, (6,) + shape).astype(F32)])
        p30, w30 = np.concatenate([picks, np.ones((E, 6))], 1), np.concatenate([w, np.zeros((E, 6))], 1)
        a = outputs(sol.locate_subcell(torch.from_numpy(tt).to(dev()), picks, w, lo, hi, 4))
        b = outputs(sol.locate_subcell(torch.from_numpy(tt30).to(dev()), p30, w30, lo, hi, 4))
        same(a, b)


# ---- node counts around the tile ----
TILE_CASES = {TILE - 1: (62, 33), TILE: (23, 89), TILE + 1: (8, 256), 2 * TILE + 1: (8, 512)}     # nodes: (sub, cells - 1)


@pytest.mark.parametrize("count", sorted(TILE_CASES), ids=lambda c: f"{c}nodes")
def test_node_counts_around_the_tile(P, count):
    """T - 1, T, T + 1 and 2T + 1 nodes along one axis, the other two single; T0 = 0 and T1 the coordinate along the
    axis, picks (0, the last coordinate): J = +0 at the window's last node alone"""
    sub, m = TILE_CASES[count]
    assert m * sub + 1 == count
    shape = (520, 2, 600)
    g = np.meshgrid(*(np.arange(n, dtype=F32) for n in shape), indexing="ij")
    rng = np.random.default_rng(count)
    for axis in (2, 0):
        tt = np.stack([np.zeros(shape, F32), g[axis]])
        lo = np.array([3, 1, 5])
        hi = lo.copy()
        hi[axis] += m
        picks = np.array([[0.0, float(hi[axis])], list(rng.uniform(0, 9, 2))])
        with P.TravelTimeSolver(shape, star818(P)) as sol:
            node, mis, _ = check_subcell(sol, tt, picks, None, np.tile(lo, (2, 1)), np.tile(hi, (2, 1)), sub, f"axis {axis}")
        assert np.array_equal(node[0], hi * sub) and mis[0] == 0.0


# ---- ties ----
def test_ties_go_to_the_smallest_node(P):
    """T0 = 0 and T1 a function of x alone: every (qy, qz) ties on the bits, 41 x 65 nodes over three tiles at sub 8;
    where two neighbouring x hold the minimum the nodes between them tie as well"""
    shape = (4, 6, 9)
    tt = np.zeros((2,) + shape, F32)
    picks = np.array([[0.0, 1.0]] * 2)
    lo = np.array([[0, 0, 0], [1, 2, 3]])
    hi = np.array([[3, 5, 8], [3, 5, 8]])
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        tt[1] = np.array([5, 3, 1, 4], F32)[:, None, None]
        assert 41 * 65 > TILE and (16 * 41 * 65) // TILE != (17 * 41 * 65 - 1) // TILE
        node, mis, _ = check_subcell(sol, tt, picks, None, lo, hi, 8)
        assert np.array_equal(node, [[16, 0, 0], [16, 16, 24]]) and np.all(mis == 0)
        tt[1] = np.array([5, 1, 1, 4], F32)[:, None, None]
        node, mis, _ = check_subcell(sol, tt, picks, None, lo, hi, 8)
        assert np.array_equal(node, [[8, 0, 0], [8, 16, 24]]) and np.all(mis == 0)
        node, _, _ = check_subcell(sol, tt, picks, None, lo, hi, 3, "sub 3")
        assert np.array_equal(node, [[3, 0, 0], [3, 6, 9]])


# ---- a planted sub-cell minimum ----
def test_planted_subcell_minimum(P):
    tt, picks, planted, lo, hi = S.planted_case()
    with P.TravelTimeSolver(tt.shape[1:], star818(P)) as sol:
        node, mis, _ = check_subcell(sol, tt, picks, None, lo, hi, 8)
        cell = outputs(sol.locate_subcell(__import__("torch").from_numpy(tt).to(dev()), picks, None, lo, hi, 1))
    assert np.array_equal(node[0], planted) and np.all(planted % 8 != 0)
    want = S.locate_subcell(tt, picks, None, lo, hi, 8)[1][0] / W.locate_window(tt, picks, None, lo, hi, 1)[1][0]
    print(f"planted node: J = {mis[0]:.3e}, best cell J = {cell[1][0]:.3e}, ratio {mis[0] / cell[1][0]:.3e}")
    assert mis[0] / cell[1][0] == want and mis[0] < 2e-9 and cell[1][0] > 1e-2     # the bounds of the CPU tier


# ---- nothing admissible ----
def test_nothing_admissible(P):
    shape = (6, 7, 8)
    rng = np.random.default_rng(8)
    tt = rng.uniform(0, 9, (3,) + shape).astype(F32)
    tt[1, :3] = INF                             # x < 3 is not reached by station 1
    picks = rng.uniform(0, 12, (5, 3))
    w = np.ones((5, 3))
    w[3, 1] = 0.0                               # event 3 does not pick station 1
    lo = np.array([[3, 0, 0], [0, 1, 2], [2, 1, 2], [0, 1, 2], [3, 2, 2]])
    hi = np.array([[5, 6, 7], [2, 5, 6], [4, 5, 6], [2, 5, 6], [5, 6, 7]])
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        node, mis, t0 = check_subcell(sol, tt, picks, w, lo, hi, 4)
        alone = check_subcell(sol, tt, picks[[0, 2, 3, 4]], w[[0, 2, 3, 4]], lo[[0, 2, 3, 4]], hi[[0, 2, 3, 4]], 4)
    assert np.all(node[1] == -1) and mis[1] == np.inf and u64(t0[1]) == 0x7ff8000000000000
    same(tuple(a[[0, 2, 3, 4]] for a in (node, mis, t0)), alone, "the neighbours of the unplaced event")
    assert np.all(node[[0, 2, 3, 4], 0] >= 0) and node[2, 0] >= 3 * 4, "event 2: only the nodes with ix >= 3"
    assert node[3, 0] <= 2 * 4


# ---- grouping and order ----
def test_grouping_and_order(P):
    """the same events with every window distinct, in runs of equal windows (1, 7, 8, 9 and 17: groups of 8 and
    less), permuted and one at a time: identical outputs per event; two calls are bit-identical"""
    import torch
    shape = Cs.RANGE_SHAPE
    rng, tt = random_box(7, K=5)
    runs = (1, 7, 8, 9, 17)
    E = sum(runs)
    picks, w = events(rng, E, 5)
    rlo, rhi = seeded_windows(rng, shape, len(runs))
    rlo[2], rhi[2] = (0, 0, 0), (4, 6, 10)
    lo, hi = np.repeat(rlo, runs, axis=0), np.repeat(rhi, runs, axis=0)
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        tdev = torch.from_numpy(tt).to(dev())
        every = check_subcell(sol, tt, picks, w, lo, hi, 3)
        same(outputs(sol.locate_subcell(tdev, picks, w, lo, hi, 3)), every, "call to call")
        perm = rng.permutation(E)                       # equal windows no longer follow each other
        got = outputs(sol.locate_subcell(tdev, picks[perm], w[perm], lo[perm], hi[perm], 3))
        same(got, tuple(a[perm] for a in every), "permuted")
        for e in range(0, E, 5):
            one = outputs(sol.locate_subcell(tdev, picks[e:e + 1], w[e:e + 1], lo[e:e + 1], hi[e:e + 1], 3))
            same(one, tuple(a[e:e + 1] for a in every), f"event {e} alone")
        dlo, dhi = seeded_windows(rng, shape, E)
        dlo[:, 0] = np.arange(E) % 5                    # consecutive windows differ
        dhi[:, 0] = np.maximum(dhi[:, 0], dlo[:, 0])
        distinct = check_subcell(sol, tt, picks, w, dlo, dhi, 3, "distinct windows")
        r = slice(None, None, -1)
        same(outputs(sol.locate_subcell(tdev, picks[r].copy(), w[r].copy(), dlo[r], dhi[r], 3)),
             tuple(a[r] for a in distinct), "reversed")


# ---- a batch edge ----
def test_a_batch_edge(P):
    """BLOCKS + 1 events whose windows alternate, so that every event is a group of its own with one block: the block
    table of the first batch is full and the last event is a second batch.  The rows are periodic (Cs.cap_case), so
    the restatement runs on one period of (row, window).  The other budget, PARTIALS partials, is first crossed by
    four times as many events and is not run here; both are one comparison in cut_batches of ttsweep_locate.cpp."""
    import torch
    tt, rows, wrows, _ = Cs.cap_case()
    E = BLOCKS + 1
    assert E * 1 <= PARTIALS and int(np.prod(Cs.CAP_SHAPE)) * 2 ** 3 <= TILE
    wins = (((0, 0, 0), (1, 2, 1)), ((0, 1, 0), (1, 2, 1)))
    period = 2 * Cs.CAP_P
    idx = np.arange(period)
    lo = np.array([wins[i % 2][0] for i in idx], np.int32)
    hi = np.array([wins[i % 2][1] for i in idx], np.int32)
    want = S.locate_subcell(tt, rows[idx % Cs.CAP_P], wrows[idx % Cs.CAP_P], lo, hi, 2)
    every = np.arange(E)
    with P.TravelTimeSolver(Cs.CAP_SHAPE, star818(P)) as sol:
        res = sol.locate_subcell(torch.from_numpy(tt).to(dev()), Cs.periodic(rows, E), Cs.periodic(wrows, E),
                                 lo[every % 2], hi[every % 2], 2)
        got = outputs(res)
    same(got, tuple(a[every % period] for a in want))


# ---- refusals ----
def test_refusals_leave_the_outputs(P):
    import torch
    rng = np.random.default_rng(1)
    shape = (6, 5, 4)
    tt = torch.from_numpy(rng.uniform(0, 5, (3,) + shape).astype(F32)).to(dev())
    good = rng.uniform(0, 5, (4, 3))
    ones = np.ones((4, 3))
    LO, HI = np.zeros((4, 3), np.int32), np.tile(np.array(shape, np.int32) - 1, (4, 1))

    def edit(a, e, axis, v):
        b = a.copy()
        b[e, axis] = v
        return b

    def refused(sol, K, tdev, picks, w, lo, hi, sub, msg):
        E = len(picks)
        pd, wd = torch.from_numpy(picks).to(dev()), torch.from_numpy(w).to(dev())
        node = torch.full((E, 3), 77, dtype=torch.int32, device=dev())
        mis = torch.full((E,), 3.5, dtype=torch.float64, device=dev())
        t0 = torch.full((E,), -2.5, dtype=torch.float64, device=dev())
        lo, hi = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
        rc = sol._L.ttsweep_locate_subcell_device(
            sol._ctx, K, sol._box_pointers(tdev, K), E, pd.data_ptr(), wd.data_ptr(), lo.ctypes.data, hi.ctypes.data,
            sub, node.data_ptr(), mis.data_ptr(), t0.data_ptr())
        assert rc < 0 and msg in P._lib.last_error(), (msg, P._lib.last_error())
        assert torch.all(node == 77) and torch.all(mis == 3.5) and torch.all(t0 == -2.5), msg
        with pytest.raises(P.TTSweepError):
            sol.locate_subcell(tdev, pd, wd, lo, hi, sub)

    with P.TravelTimeSolver(shape, star818(P)) as sol:
        cases = ((good, ones, LO, HI, 0, "sub 0"),
                 (good, ones, LO, HI, 65, "sub 65"),
                 (good, ones, edit(LO, 2, 1, 4), edit(HI, 2, 1, 3), 8, "event 2"),      # lo > hi
                 (good, ones, LO, edit(HI, 3, 0, 6), 8, "event 3"),                       # hi = n
                 (good, ones, edit(LO, 1, 2, -1), HI, 8, "event 1"),                      # lo < 0
                 (np.where(np.eye(4, 3) > 0, np.inf, good), ones, LO, HI, 8, "pick"),
                 (good, np.where(np.eye(4, 3) > 0, -1.0, 1.0), LO, HI, 8, "weight"),
                 (good, np.array([[1.0] * 3, [0.0] * 3, [1.0] * 3, [1.0] * 3]), LO, HI, 8, "no weight"))
        for picks, w, lo, hi, sub, msg in cases:
            refused(sol, 3, tt, picks, w, lo, hi, sub, msg)
        with pytest.raises(P.TTSweepError):
            sol.locate_subcell(tt, good, None, LO[:3], HI[:3])          # [E, 3] with the wrong E
        with pytest.raises(P.TTSweepError):
            sol.locate_subcell(tt, good, None, LO, HI, sub=2.0)         # a float sub
        got = outputs(sol.locate_subcell(tt, good, ones, LO, HI, 2))    # a correct call works afterwards
        same(got, S.locate_subcell(tt.cpu().numpy(), good, ones, LO, HI, 2))
    # an event with more nodes than int32 holds: (39 * 64 + 1)^3; the event before it is fine
    big = (40, 40, 40)
    with P.TravelTimeSolver(big, star818(P)) as sol:
        tb = torch.zeros((1,) + big, dtype=torch.float32, device=dev())
        lo, hi = np.zeros((2, 3), np.int32), np.array([[1, 1, 1], [39, 39, 39]], np.int32)
        refused(sol, 1, tb, good[:2, :1], ones[:2, :1], lo, hi, 64, "event 1")
        assert "nodes" in P._lib.last_error()
    # an axis whose nodes overflow int32: (2^25 + 1 - 1) * 64 = 2^31.  A star along z alone: the solver's own
    # neighbour offsets must fit 32 bits for it to accept such a grid (its padded velocity image is 13 GB, untouched)
    long = (1, 1, 2 ** 25 + 1)
    along_z = P.inputs.make_fs(np.array([[0, 0, 1], [0, 0, -1], [0, 0, 2]], np.int32))
    with P.TravelTimeSolver(long, along_z) as sol:
        tb = torch.empty((1,) + long, dtype=torch.float32, device=dev())
        lo, hi = np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32)
        refused(sol, 1, tb, good[:1, :1], ones[:1, :1], lo, hi, 64, "axis 2")
        tb[0, 0, 0, :2] = torch.tensor([1.0, 2.0])
        res = sol.locate_subcell(tb, np.array([[1.5]]), None, [0, 0, 0], [0, 0, 1], sub=32)    # 32 fits
        assert res.misfit.cpu().numpy()[0] == 0.0


# ---- locate_fine ----
def test_locate_fine(P):
    import torch
    shape = (9, 8, 7)
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(*(np.arange(float(n)) for n in shape), indexing="ij"))
    stations = np.array([[0, 0, 0], [8, 0, 0], [0, 7, 6], [8, 7, 0], [4, 3, 6]], float)
    tt = np.stack([np.sqrt(((g - s[:, None, None, None]) ** 2).sum(0)) for s in stations]).astype(F32)
    tt[0, :2, :2, :2] = INF
    E = 7
    pos = rng.uniform(1, 5, (E, 3))
    picks = np.stack([np.sqrt(((pos - s) ** 2).sum(1)) for s in stations], 1) + rng.uniform(-3, 3, (E, 1))
    w = np.ones((E, 5))
    w[1:6, 0] = 0.0                             # only events 0 and 6 pick station 0 ...
    w[6, 1:] = 0.0                              # ... and event 6 nothing else
    with P.TravelTimeSolver(shape, star818(P)) as sol:
        tdev = torch.from_numpy(tt).to(dev())
        none = torch.from_numpy(np.full_like(tt, INF)).to(dev())
        first = sol.locate(tdev, picks, w)
        for radius in (1, (2, 1, 0)):
            fine = sol.locate_fine(tdev, picks, w, sub=8, radius=radius)
            assert fine.cell is first.cell or torch.equal(fine.cell, first.cell)
            assert torch.equal(fine.cell_misfit.view(torch.int64), first.misfit.view(torch.int64))
            lo, hi = S.fine_windows(shape, first.cell.cpu().numpy(), radius)
            by_hand = sol.locate_subcell(tdev, picks, w, lo, hi, 8)
            same(outputs(fine), outputs(by_hand), str(radius))
            same(outputs(fine), S.locate_subcell(tt, picks, w, lo, hi, 8), str(radius))
            assert np.all(u64(fine.misfit.cpu().numpy()) <= u64(fine.cell_misfit.cpu().numpy()))
        near = np.abs(fine.position - pos).max(1)
        print("locate_fine: largest distance from the true position per event, in cells:", np.round(near, 3))
        # cells from locate_refine, on the device and as numpy
        refined = sol.locate_refine(tdev, picks, w, stride=2)
        for cells in (refined.cell, refined.cell.cpu().numpy()):
            fine = sol.locate_fine(tdev, picks, w, sub=4, cells=cells)
            lo, hi = S.fine_windows(shape, refined.cell.cpu().numpy(), 1)
            same(outputs(fine), S.locate_subcell(tt, picks, w, lo, hi, 4), "cells from locate_refine")
            assert fine.cell_misfit is None and fine.cell is cells
            assert np.all(u64(fine.misfit.cpu().numpy()) <= u64(refined.misfit.cpu().numpy()))
        # no cell is admissible: the event stays unplaced, beside one that is placed
        mixed = torch.cat([tdev[:1], none[1:]])
        wm = np.zeros((2, 5))
        wm[0, 0], wm[1, 1] = 1.0, 1.0           # event 0 picks the real box, event 1 a box of infinities
        fine = sol.locate_fine(mixed, picks[:2], wm, sub=8)
        node, mis, t0 = outputs(fine)
        assert fine.cell.cpu().numpy()[1] == -1 and np.all(node[1] == -1) and mis[1] == np.inf
        assert u64(t0[1]) == 0x7ff8000000000000 and np.all(np.isnan(fine.position[1]))
        assert np.all(node[0] >= 0) and np.isfinite(mis[0])
        with pytest.raises(P.TTSweepError):
            sol.locate_fine(tdev, picks, w, cells=np.full(E, 9 * 8 * 7, np.int32))
