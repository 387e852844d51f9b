"""CPU tier of windowed, strided event location (include/ttsweep.h, "locate window"): the numpy restatement
(locate_window_reference.py) against an argmin over locate_reference's misfit volume masked to the candidate set, on
tiny hand-made boxes; the C ABI's surface (symbol exported and bound, the macro); every refusal that concerns the
arguments, windows and strides, which come before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
import locate_reference as L
import locate_window_reference as W

INF = np.float32(np.inf)


def u64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def masked_argmin(tt, o, w, lo, hi, stride):
    """(cell, J, t0) from the whole misfit volume of locate_reference, every cell off the candidate set masked."""
    J, t0 = L.misfit(tt, o, w)
    shape = tt.shape[1:]
    mask = np.zeros(shape, bool)
    mask[tuple(slice(int(lo[a]), int(hi[a]) + 1, int(stride[a])) for a in range(3))] = True
    Jm = np.where(mask, J, np.inf).reshape(-1)
    if not np.any(Jm < np.inf):
        return -1, np.inf, np.nan
    x = int(np.argmin(Jm))
    return x, Jm[x], t0.reshape(-1)[x]


def test_restatement_equals_the_masked_argmin_of_the_volume():
    rng = np.random.default_rng(11)
    shape = (4, 5, 6)
    for K in (1, 3):
        tt = rng.uniform(0, 10, (K,) + shape).astype(np.float32)
        tt[rng.random(tt.shape) < 0.15] = INF
        E = 12
        picks = rng.uniform(0, 20, (E, K))
        w = rng.uniform(0.1, 2, (E, K))
        w[rng.random((E, K)) < 0.3] = 0
        w[:, 0] = 1.0
        lo = np.stack([rng.integers(0, n, E) for n in shape], 1)
        hi = np.stack([rng.integers(lo[:, a], shape[a]) for a in range(3)], 1)
        lo[0], hi[0] = 0, np.array(shape) - 1
        for stride in ((1, 1, 1), (2, 1, 3), (7, 7, 7)):
            cell, mis, t0 = W.locate_window(tt, picks, w, lo, hi, stride)
            for e in range(E):
                x, J, t = masked_argmin(tt, picks[e], w[e], lo[e], hi[e], stride)
                assert cell[e] == x, (K, stride, e)
                assert u64(mis[e]) == u64(J) and (np.isnan(t) and np.isnan(t0[e]) or u64(t0[e]) == u64(t))
        # the whole grid with stride 1 is locate
        cell, mis, t0 = W.locate_window(tt, picks, w)
        rc, rm, rt, _ = L.locate(tt, picks, w)
        assert np.array_equal(cell, rc) and np.array_equal(u64(mis), u64(rm))
        assert np.array_equal(np.isnan(t0), np.isnan(rt)) and np.array_equal(u64(t0[rc >= 0]), u64(rt[rc >= 0]))


def test_ties_go_to_the_lo_corner_and_stay_on_the_lattice():
    tt = np.ones((2, 5, 5, 5), np.float32)
    o = np.array([[3.0, 3.0]])
    cell, _, _ = W.locate_window(tt, o, None, [1, 2, 1], [4, 4, 3], 1)
    assert cell[0] == (1 * 5 + 2) * 5 + 1
    tt[1] = 2.0                              # J > 0, the same at every cell ...
    tt[1, 2::2, 1::2, 2::2] = 1.0            # ... but J = 0 at cells off the lattice from (1, 2, 1) with stride 2
    cell, mis, _ = W.locate_window(tt, o, None, [1, 2, 1], [4, 4, 3], 2)
    assert cell[0] == (1 * 5 + 2) * 5 + 1 and mis[0] > 0
    assert L.locate(tt, o)[1][0] == 0.0


def test_refine_restatement_on_a_smooth_misfit():
    """Two stages on a box set with one basin: the lattice node next to the minimum leads to it; misfit <= coarse."""
    g = np.stack(np.meshgrid(np.arange(9.0), np.arange(8.0), np.arange(7.0), indexing="ij"))
    stations = np.array([[0, 0, 0], [8, 0, 0], [0, 7, 6], [8, 7, 0], [4, 3, 6]], float)
    tt = np.stack([np.sqrt(((g - s[:, None, None, None]) ** 2).sum(0)) for s in stations]).astype(np.float32)
    true = (5, 3, 2)
    o = tt[(slice(None),) + true].astype(np.float64)[None] + 1.5
    cell, mis, t0, cc, cm = W.refine(tt, o, None, stride=4)
    assert cell[0] == np.ravel_multi_index(true, tt.shape[1:]) and mis[0] == 0.0 and mis[0] <= cm[0]
    assert tuple(np.array(np.unravel_index(cc[0], tt.shape[1:])) % 4) == (0, 0, 0)
    tt[:, ::4, ::4, ::4] = INF               # no admissible lattice node: stage 2 is the whole grid
    cell, mis, _, cc, cm = W.refine(tt, o, None, stride=4)
    assert cc[0] == -1 and cm[0] == np.inf and cell[0] == L.locate(tt, o)[0][0] >= 0


def test_window_symbol_exported_and_bound(pkg):
    lib = pkg._lib.lib()
    assert hasattr(lib, "ttsweep_locate_window_device")
    assert "ttsweep_locate_window_device" in {n for n, _, _ in pkg._lib.SYMBOLS}
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ttsweep.h")).read()
    assert "#define TTSWEEP_HAS_LOCATE_WINDOW 1" in hdr
    assert "#define TTSWEEP_ABI_VERSION 6" in hdr or "#define TTSWEEP_ABI_VERSION (6)" in hdr
    assert lib.ttsweep_abi_version() == 6
    assert callable(pkg.TravelTimeSolver.locate_window) and callable(pkg.TravelTimeSolver.locate_refine)
    loc = pkg.Locations(1, 2, 3, 4, None)
    assert loc.coarse_cell is None and loc.coarse_misfit is None


def test_bad_window_arguments_are_refused_without_a_device(pkg):
    lib = pkg._lib.lib()
    loc = lib.ttsweep_locate_window_device
    ptr = (C.c_void_p * 1)(None)
    d = C.c_void_p(8)                           # never read: every call below is refused first

    def last():
        return pkg._lib.last_error()

    def ints(*v):
        return (C.c_int * len(v))(*v)

    # the checks below come before the context is read, so a NULL context is refused for the reason given
    for args in ((0, ptr, 1, d), (1, ptr, 0, d), (-1, ptr, 1, d), (1, None, 1, d), (1, ptr, 1, None)):
        assert loc(None, *args, None, None, None, None, None, None, None) < 0
        assert "ttsweep_locate_window_device" in last() and "null or bad argument" in last()
    assert loc(None, 65536, ptr, 65536, d, None, None, None, None, None, None, None) < 0
    assert "int32" in last()
    lo, hi = ints(0, 0, 0, 1, 1, 1), ints(2, 2, 2, 3, 3, 3)
    assert loc(None, 1, ptr, 2, d, None, lo, None, None, None, None, None) < 0
    assert "lo and hi" in last()
    assert loc(None, 1, ptr, 2, d, None, None, hi, None, None, None, None) < 0
    assert "lo and hi" in last()
    for stride in (ints(1, 0, 1), ints(-2, 1, 1), ints(1, 1, 0)):
        assert loc(None, 1, ptr, 2, d, None, lo, hi, stride, None, None, None) < 0
        assert "stride" in last() and "below 1" in last()
    assert loc(None, 1, ptr, 2, d, None, ints(0, 0, 0, 1, -1, 1), hi, None, None, None, None) < 0
    assert "event 1" in last() and "window" in last()
    assert loc(None, 1, ptr, 2, d, None, ints(0, 0, 3, 1, 1, 1), hi, None, None, None, None) < 0       # lo > hi
    assert "event 0" in last() and "window" in last()
    # an acceptable window reaches the context check
    assert loc(None, 1, ptr, 2, d, None, lo, hi, ints(1, 2, 3), None, None, None) < 0
    assert "null or bad argument" in last()


def test_locate_window_checks_arguments_before_the_library(pkg):
    """TravelTimeSolver.locate_window / locate_refine refuse a wrong tt before they reach C (no device needed)."""
    sol = pkg.TravelTimeSolver.__new__(pkg.TravelTimeSolver)
    sol.shape, sol.device = (2, 2, 2), 0
    with pytest.raises(pkg.TTSweepError):
        sol.locate_window(np.zeros((1, 2, 2, 2), np.float32), np.zeros((1, 1)))
    with pytest.raises(pkg.TTSweepError):
        sol.locate_refine(np.zeros((1, 2, 2, 2), np.float32), np.zeros((1, 1)))
