"""CPU tier of event location (include/ttsweep.h, "locate"): the numpy restatement (locate_reference.py) against a
per-cell pure-Python loop on tiny hand-made boxes, the C ABI's surface (symbol exported and bound, the macro, bad
arguments refused before any device work) and the Python exports."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
import locate_reference as L

INF = np.float32(np.inf)


def agree(tt, o, w=None):
    cell, mis, t0, _ = L.locate(tt, np.asarray(o, np.float64)[None], None if w is None else np.asarray(w)[None])
    x, J, t = L.locate_slow(tt, o, w)
    assert cell[0] == x
    assert np.float64(mis[0]).tobytes() == np.float64(J).tobytes()
    assert np.float64(t0[0]).tobytes() == np.float64(t).tobytes()
    return cell[0], mis[0], t0[0]


def test_reference_agrees_with_a_cell_loop_on_random_boxes():
    rng = np.random.default_rng(3)
    for K in (1, 2, 5):
        tt = rng.uniform(0, 10, (K, 3, 4, 2)).astype(np.float32)
        tt[rng.random(tt.shape) < 0.1] = INF
        for _ in range(5):
            o = rng.uniform(0, 20, K)
            w = rng.uniform(0.1, 2, K)
            w[rng.random(K) < 0.3] = 0
            if not np.any(w):
                w[0] = 1.0
            agree(tt, o, w)
            agree(tt, o)


def test_ties_go_to_the_smallest_index():
    tt = np.array([[[0, 1, 0, 1]], [[2, 3, 2, 3]]], np.float32)     # [2, 1, 4]: cells 0 and 2 equal, 1 and 3 equal
    cell, J, t0 = agree(tt, [5.0, 7.0])
    assert cell == 0 and J == 0.0 and t0 == 5.0
    cell, _, _ = agree(tt[:, :, 1:], [5.0, 7.0])
    assert cell == 0


def test_single_pick_gives_the_smallest_admissible_cell():
    tt = np.array([[[INF, INF, 4, 1, 0]], [[0, 0, INF, 0, 0]]], np.float32)
    cell, J, t0 = agree(tt, [9.0, 1.0], [1.0, 0.0])
    assert cell == 2 and J == 0.0 and t0 == 5.0


def test_zero_weight_station_with_an_all_inf_box_is_skipped():
    tt = np.stack([np.full((2, 2, 2), INF), np.arange(8, dtype=np.float32).reshape(2, 2, 2),
                   np.arange(8, 0, -1, dtype=np.float32).reshape(2, 2, 2)])
    cell, J, _ = agree(tt, [1.0, 3.0, 5.0], [0.0, 1.0, 2.0])
    assert cell >= 0 and np.isfinite(J)


def test_no_admissible_cell():
    tt = np.array([[[INF, 1]], [[2, INF]]], np.float32)
    cell, J, t0 = agree(tt, [1.0, 1.0])
    assert cell == -1 and J == np.inf and np.isnan(t0)
    Jv, _ = L.misfit(tt, [1.0, 1.0])
    assert np.all(Jv == np.inf)


def test_refusals_of_the_reference():
    o = np.zeros((2, 3))
    assert L.check(o) is None
    assert L.check(np.where(np.eye(2, 3) > 0, np.nan, o)) == "pick"
    assert L.check(o, np.array([[1, -1, 1], [1, 1, 1]], float)) == "weight"
    assert L.check(o, np.array([[1, np.inf, 1], [1, 1, 1]], float)) == "weight"
    assert L.check(o, np.array([[0, 0, 0], [1, 1, 1]], float)) == "no weight"


def test_locate_symbol_exported_and_bound(pkg):
    lib = pkg._lib.lib()
    assert hasattr(lib, "ttsweep_locate_device")
    assert "ttsweep_locate_device" in {n for n, _, _ in pkg._lib.SYMBOLS}
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ttsweep.h")).read()
    assert "#define TTSWEEP_HAS_LOCATE 1" in hdr
    assert "#define TTSWEEP_ABI_VERSION 6" in hdr or "#define TTSWEEP_ABI_VERSION (6)" in hdr
    assert lib.ttsweep_abi_version() == 6
    assert pkg.Locations is pkg.solver.Locations and "Locations" in pkg.__all__
    assert callable(pkg.TravelTimeSolver.locate)


def test_bad_locate_arguments_are_refused_without_a_device(pkg):
    lib = pkg._lib.lib()
    loc = lib.ttsweep_locate_device
    ptr = (C.c_void_p * 1)(None)
    ev = (C.c_int * 1)(0)
    d = C.c_void_p(8)                           # never read: every call below is refused first

    def last():
        return pkg._lib.last_error()

    assert loc(None, 1, ptr, 1, d, None, None, None, None, 0, None, None) < 0
    assert "ttsweep_locate_device" in last() and "null or bad argument" in last()
    # the checks below come before the context is read, so a NULL context is refused for the reason given
    for args in ((0, ptr, 1, d), (1, ptr, 0, d), (-1, ptr, 1, d), (1, None, 1, d), (1, ptr, 1, None)):
        assert loc(None, *args, None, None, None, None, 0, None, None) < 0
        assert "null or bad argument" in last()
    assert loc(None, 1, ptr, 1, d, None, None, None, None, -1, None, None) < 0
    assert loc(None, 1, ptr, 1, d, None, None, None, None, 1, None, ptr) < 0
    assert loc(None, 1, ptr, 1, d, None, None, None, None, 1, ev, None) < 0
    assert "null or bad argument" in last()
    # 65536 x 65536 picks do not fit int32 indices: refused before the (one-element) box list is read
    assert loc(None, 65536, ptr, 65536, d, None, None, None, None, 0, None, None) < 0
    assert "int32" in last()


def test_locate_checks_arguments_before_the_library(pkg):
    """TravelTimeSolver.locate refuses a wrong tt before it reaches C (no device needed to get there)."""
    sol = pkg.TravelTimeSolver.__new__(pkg.TravelTimeSolver)
    sol.shape, sol.device = (2, 2, 2), 0
    with pytest.raises(pkg.TTSweepError):
        sol.locate(np.zeros((1, 2, 2, 2), np.float32), np.zeros((1, 1)))
