"""CPU tier of sub-cell event location (include/ttsweep.h, "locate subcell"): the numpy restatement
(locate_subcell_reference.py) against its per-node pure-Python loop on a tiny box; the properties the header states,
against locate_reference and locate_window_reference; the C ABI's surface; the refusals that come before any device
work."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
import locate_cases as Cs
import locate_reference as L
import locate_subcell_reference as S
import locate_window_reference as W

F32 = np.float32
INF = F32(np.inf)
SUBS = (1, 2, 3, 8, 16)         # 3 makes u inexact


def u64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_t0(a, b):
    return (np.isnan(a) and np.isnan(b)) or u64(a) == u64(b)


def range_case(K=4, E=9, seed=5):
    """a random box on Cs.RANGE_SHAPE with 5 % of the cells at infinity and one -0.0; weighted events, some picks
    dropped; seeded windows, the first the whole grid, the second a single cell"""
    rng = np.random.default_rng(seed)
    shape = Cs.RANGE_SHAPE
    tt = rng.uniform(0, 9, (K,) + shape).astype(F32)
    tt[rng.random(tt.shape) < 0.05] = INF
    tt[1, 2, 3, 4] = F32(-0.0)
    picks = rng.uniform(0, 12, (E, K))
    w = rng.uniform(0.5, 2.0, (E, K))
    w[rng.random((E, K)) < 0.25] = 0.0
    w[:, 1] = 1.0                   # the station of the -0.0 is picked
    lo = np.stack([rng.integers(0, n, E) for n in shape], 1)
    hi = np.stack([rng.integers(lo[:, a], shape[a]) for a in range(3)], 1)
    lo[0], hi[0] = 0, np.array(shape) - 1
    lo[1], hi[1] = (2, 3, 4), (2, 3, 4)
    return tt, picks, w, lo, hi


def test_restatement_equals_the_per_node_loop():
    rng = np.random.default_rng(2)
    shape = (3, 4, 5)
    tt = rng.uniform(0, 9, (3,) + shape).astype(F32)
    tt[0, 1, 2, 3] = INF
    tt[2, 0, 0, 0] = F32(-0.0)
    picks = rng.uniform(0, 12, (4, 3))
    w = np.array([[1.0, 1.0, 1.0], [0.5, 0.0, 2.0], [0.0, 0.0, 1.5], [1.0, 2.0, -0.0]])
    lo = np.array([[0, 0, 0], [1, 1, 2], [0, 3, 0], [2, 0, 4]])
    hi = np.array([[2, 3, 4], [2, 3, 3], [2, 3, 4], [2, 3, 4]])
    for sub in (1, 2, 3, 5):
        node, mis, t0 = S.locate_subcell(tt, picks, w, lo, hi, sub)
        for e in range(len(picks)):
            q, J, t = S.subcell_slow(tt, picks[e], w[e], lo[e], hi[e], sub)
            assert tuple(node[e]) == q, (sub, e)
            assert u64(mis[e]) == u64(J) and same_t0(t0[e], t), (sub, e)
    node, _, _ = S.locate_subcell(tt, picks[:1], None, sub=3)
    assert tuple(node[0]) == S.subcell_slow(tt, picks[0], None, (0, 0, 0), (2, 3, 4), 3)[0]


@pytest.mark.parametrize("sub", SUBS)
def test_nodes_on_cells_carry_the_bits_of_locate(sub):
    """property 1: f = 0 on all three axes, the -0.0 included"""
    tt, picks, w, _, _ = range_case()
    shape = tt.shape[1:]
    That, q = S.interpolate(tt, (0, 0, 0), np.array(shape) - 1, sub)
    assert That.shape[1:] == tuple((n - 1) * sub + 1 for n in shape)
    on = That[:, ::sub, ::sub, ::sub]
    fin = np.isfinite(tt)
    assert np.array_equal(u64(on[fin]), u64(tt[fin].astype(np.float64) + 0.0)) and not np.any(np.isfinite(on[~fin]))
    assert u64(on[1, 2, 3, 4]) == 0, "the -0.0 becomes +0.0"
    for e in range(len(picks)):
        J, t0 = S.misfit(That, picks[e], w[e])
        Jc, t0c = Cs.misfit(tt, picks[e], w[e])
        assert np.array_equal(u64(J[::sub, ::sub, ::sub]), u64(Jc))
        adm = Jc < np.inf
        assert adm.any() and np.array_equal(u64(t0[::sub, ::sub, ::sub][adm]), u64(t0c[adm]))


@pytest.mark.parametrize("sub", SUBS)
def test_sub_one_is_locate_window_and_no_sub_is_worse(sub):
    """properties 2 and 3"""
    tt, picks, w, lo, hi = range_case()
    shape = tt.shape[1:]
    node, mis, t0 = S.locate_subcell(tt, picks, w, lo, hi, sub)
    cell, cm, ct = W.locate_window(tt, picks, w, lo, hi, 1)
    assert cell[0] >= 0
    assert np.all(u64(mis) <= u64(cm)), "J >= +0: the order of the bits is the order of the values"
    assert np.array_equal(np.all(node == -1, axis=1), cell < 0), "the base cell is a corner of every node"
    ok = cell >= 0
    assert np.all(node[ok] >= lo[ok] * sub) and np.all(node[ok] <= hi[ok] * sub)
    if sub == 1:
        assert np.array_equal(node[ok], np.array(np.unravel_index(cell[ok], shape)).T)
        assert np.array_equal(u64(mis), u64(cm)) and np.array_equal(u64(t0[ok]), u64(ct[ok]))
        assert np.all(np.isnan(t0[~ok]))
        whole = S.locate_subcell(tt, picks, w, sub=1)
        rc, rm, rt, _ = L.locate(tt, picks, w)
        assert np.array_equal(whole[0], np.array(np.unravel_index(rc, shape)).T) and np.array_equal(u64(whole[1]), u64(rm))


@pytest.mark.parametrize("sub", SUBS)
def test_a_node_is_inadmissible_exactly_when_a_picked_corner_is_not_finite(sub):
    tt, picks, w, _, _ = range_case()
    shape = tt.shape[1:]
    top = np.array(shape) - 1
    That, _ = S.interpolate(tt, (0, 0, 0), top, sub)
    (_, ix, jx, _), (_, iy, jy, _), (_, iz, jz, _) = (S.axis(0, top[a], sub) for a in range(3))
    fin = np.isfinite(tt)
    corners = np.ones(That.shape, bool)
    for x in (ix, jx):
        for y in (iy, jy):
            for z in (iz, jz):
                corners &= fin[np.ix_(np.arange(tt.shape[0]), x, y, z)]
    assert not np.any(np.isfinite(That[~corners])) and np.all(np.isfinite(That[corners]))
    seen = 0
    for e in range(len(picks)):
        J, _ = S.misfit(That, picks[e], w[e])
        want = np.all(corners[w[e] != 0], axis=0)
        assert np.array_equal(J < np.inf, want), e
        seen += int((~want).sum())
    assert seen > 0


def test_planted_node_on_a_linear_field():
    """The search recovers the planted node.  Every float32 value is below 64, so within 2^-18 of the linear field;
    an interpolated time is a convex combination of such values up to rounding, so every residual at the planted
    node is below 2^-16 after the origin time is removed and J < 6 * 2^-32 < 2e-9, while the best cell is 3/8 of a
    cell or more away on every axis and its J is above 1e-2 (the restatement's claim about this case)."""
    tt, picks, node, lo, hi = S.planted_case()
    assert np.all(node % 8 != 0) and float(np.abs(tt).max()) < 64
    got, mis, _ = S.locate_subcell(tt, picks, None, lo, hi, 8)
    assert np.array_equal(got[0], node)
    _, cm, _ = W.locate_window(tt, picks, None, lo, hi, 1)
    print(f"planted node: J = {mis[0]:.3e}, best cell J = {cm[0]:.3e}")
    assert mis[0] < 2e-9 and cm[0] > 1e-2


def test_subcell_symbol_exported_and_bound(pkg):
    lib = pkg._lib.lib()
    assert hasattr(lib, "ttsweep_locate_subcell_device")
    assert "ttsweep_locate_subcell_device" in {n for n, _, _ in pkg._lib.SYMBOLS}
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ttsweep.h")).read()
    assert "#define TTSWEEP_HAS_LOCATE_SUBCELL 1" in hdr and "int ttsweep_locate_subcell_device(" in hdr
    assert "#define TTSWEEP_ABI_VERSION 6" in hdr or "#define TTSWEEP_ABI_VERSION (6)" in hdr
    assert lib.ttsweep_abi_version() == 6
    assert callable(pkg.TravelTimeSolver.locate_subcell) and callable(pkg.TravelTimeSolver.locate_fine)
    assert pkg.SubcellLocations is pkg.solver.SubcellLocations and "SubcellLocations" in pkg.__all__
    loc = pkg.SubcellLocations(1, 8, 2, 3, 4)
    assert loc.cell is None and loc.cell_misfit is None
    assert [f for f in pkg.Locations.__dataclass_fields__] == ["cell", "xyz", "misfit", "t0", "volumes", "coarse_cell",
                                                               "coarse_misfit"], "Locations is unchanged"


def test_bad_subcell_arguments_are_refused_without_a_device(pkg):
    lib = pkg._lib.lib()
    loc = lib.ttsweep_locate_subcell_device
    ptr = (C.c_void_p * 1)(None)
    d = C.c_void_p(8)                           # never read: every call below is refused first

    def last():
        return pkg._lib.last_error()

    def ints(*v):
        return (C.c_int * len(v))(*v)

    # the checks below come before the context is read, so a NULL context is refused for the reason given
    for args in ((0, ptr, 1, d), (1, ptr, 0, d), (-1, ptr, 1, d), (1, None, 1, d), (1, ptr, 1, None)):
        assert loc(None, *args, None, None, None, 8, None, None, None) < 0
        assert "ttsweep_locate_subcell_device" in last() and "null or bad argument" in last()
    assert loc(None, 65536, ptr, 65536, d, None, None, None, 8, None, None, None) < 0
    assert "int32" in last()
    lo, hi = ints(0, 0, 0, 1, 1, 1), ints(2, 2, 2, 3, 3, 3)
    assert loc(None, 1, ptr, 2, d, None, lo, None, 8, None, None, None) < 0
    assert "lo and hi" in last()
    assert loc(None, 1, ptr, 2, d, None, None, hi, 8, None, None, None) < 0
    assert "lo and hi" in last()
    for sub in (0, 65, -3):
        assert loc(None, 1, ptr, 2, d, None, lo, hi, sub, None, None, None) < 0
        assert f"sub {sub}" in last() and "1..64" in last()
    assert loc(None, 1, ptr, 2, d, None, ints(0, 0, 0, 1, -1, 1), hi, 8, None, None, None) < 0
    assert "event 1" in last() and "window" in last()
    assert loc(None, 1, ptr, 2, d, None, ints(0, 0, 3, 1, 1, 1), hi, 8, None, None, None) < 0       # lo > hi
    assert "event 0" in last() and "window" in last()
    # acceptable windows and sub reach the context check
    for sub in (1, 64):
        assert loc(None, 1, ptr, 2, d, None, lo, hi, sub, None, None, None) < 0
        assert "null or bad argument" in last()


def test_locate_subcell_checks_arguments_before_the_library(pkg):
    sol = pkg.TravelTimeSolver.__new__(pkg.TravelTimeSolver)
    sol.shape, sol.device = (2, 2, 2), 0
    with pytest.raises(pkg.TTSweepError):
        sol.locate_subcell(np.zeros((1, 2, 2, 2), np.float32), np.zeros((1, 1)))
    with pytest.raises(pkg.TTSweepError):
        sol.locate_fine(np.zeros((1, 2, 2, 2), np.float32), np.zeros((1, 1)))
    with pytest.raises(pkg.TTSweepError):
        sol.locate_fine(np.zeros((1, 2, 2, 2), np.float32), np.zeros((1, 1)), radius=-1)
