"""CPU tier of event location (include/ttsweep.h, "locate"): the numpy restatement (locate_reference.py) against a
per-cell pure-Python loop on tiny hand-made boxes, the C ABI's surface (symbol exported and bound, the macro, bad
arguments refused before any device work) and the Python exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
import locate_cases as Cs
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


# ---- the claims of the cases of locate_cases.py, checked with the restatement alone (the GPU tier runs the same
# inputs through the library) ----
CSRC = os.path.join(os.path.dirname(GOLDEN), "..", "uoparallel-seismic-project_amd", "csrc")


def test_case_constants_mirror_the_sources():
    hip = open(os.path.join(CSRC, "ttsweep_locate.hip")).read()
    cpp = open(os.path.join(CSRC, "ttsweep_locate.cpp")).read()

    def const(src, name):
        return re.search(r"constexpr\s+[\w ]+\s" + name + r"\s*=\s*([^;]+);", src).group(1).strip()

    assert int(const(hip, "LOC_BLOCK")) == Cs.STEP and int(const(hip, "LOC_ET")) == Cs.ET
    assert int(const(hip, "LOC_C")) * Cs.STEP == Cs.TILE
    assert const(cpp, "LOC_PARTIALS") == "1LL << 24" and Cs.PARTIALS == 1 << 24
    assert "LOC_PARTIALS / ntiles, 65535LL * 8" in cpp and "const int eb = 65535 * 8;" in cpp and Cs.CAP == 65535 * 8
    assert "K <= 8 ? 8 : K <= 16 ? 16 : K <= 24 ? 24 : K <= 32 ? 32 : 0" in hip
    assert set(Cs.KR_WIDTHS) | {1, 33} <= set(Cs.K_EDGES)
    assert all(k + 1 in Cs.K_EDGES and k - 1 in Cs.K_EDGES for k in Cs.KR_WIDTHS)


def test_big_case_makes_three_batches_that_end_in_partial_event_blocks():
    ntiles, eb, starts = Cs.batches(Cs.BIG_SHAPE, Cs.BIG_E)
    assert ntiles == 1003 and int(np.prod(Cs.BIG_SHAPE)) % Cs.TILE != 0
    assert eb == 16727 and eb % Cs.ET != 0 and len(starts) >= 3 and starts == [0, eb, 2 * eb]
    assert 0 < Cs.BIG_E - starts[-1] < Cs.ET                                # the last batch is one partial block
    assert len({s % Cs.BIG_P for s in starts}) == len(starts)              # the edges fall on different rows
    assert all(Cs.BIG_P % d for d in range(2, Cs.BIG_P))
    # the existing largest case, for comparison: one batch
    assert Cs.batches((241, 241, 51), 4097) == (724, 4097, [0])
    ntiles, eb, starts = Cs.batches(Cs.CAP_SHAPE, Cs.CAP_E)
    assert (ntiles, eb, starts) == (1, Cs.CAP, [0, Cs.CAP]) and Cs.CAP_E - Cs.CAP == 3 and Cs.CAP % Cs.CAP_P != 0


def test_planted_cells_sit_where_their_kind_says():
    N = int(np.prod(Cs.BIG_SHAPE))
    pl = Cs.big_plants()
    tile, step, tid = (lambda x: x // Cs.TILE), (lambda x: x % Cs.TILE // Cs.STEP), (lambda x: x % Cs.STEP)
    assert pl[1][1] == [N - 1] and tile(N - 1) == 1002 and tid(N - 1) == (N - 1002 * Cs.TILE) % Cs.STEP - 1
    assert [tile(pl[r][1][0]) for r in (4, 5, 6, 7)] == [5, 261, 300, 1002]
    a, b = pl[8][1]
    assert tile(a) == tile(b) and tid(a) == tid(b) and step(b) == step(a) + 1
    a, b = pl[9][1]
    assert tile(a) == tile(b) and step(a) == step(b) and tid(b) == tid(a) + 64
    a, b = pl[10][1]
    assert tile(a) == tile(b) and (step(a), tid(a), step(b), tid(b)) == (0, 1, 1, 0)
    for r, lanes in ((11, (5, 5)), (12, (1, 0)), (13, (70, 0))):
        a, b = pl[r][1]
        assert a < b and (tile(a) % 256, tile(b) % 256) == lanes and tile(b) >= 256
    a, b = pl[16][1]
    assert tile(a) == tile(b) == 1002 and step(a) == step(b) == (N - 1 - 1002 * Cs.TILE) // Cs.STEP and tid(a) == 0
    assert sorted(tile(x) for x in pl[17][1]) == list(range(1003))


@pytest.mark.slow
@pytest.mark.parametrize("variant", ["unit", "weighted"])
def test_planted_minima_and_ties_of_the_big_case(variant):
    """The restatement on the 4 107 285 cells: every planted row has its minimum exactly at its planted cells, all
    of them with the same J bits, and the smallest of them is the located cell.  "unit": the minimum is +0 and the
    decoy 0.5.  "weighted": the minimum is not zero and nothing is assumed but equal bits."""
    ref = Cs.big_reference(variant)
    pl = Cs.big_plants()
    assert set(pl) <= set(ref) and len(pl) == 18
    for r, (kind, cells, decoy) in pl.items():
        cell, m, t0, Jc, Jd, nmin = ref[r]
        assert cell == min(cells) and nmin == len(cells), (r, kind)
        assert np.all(Cs.u64(Jc) == Cs.u64(m)), (r, kind)
        if variant == "unit":
            assert Cs.u64(m) == 0 and (decoy is None or Jd == 0.5)
        else:
            assert 0 < m < 0.1 and (decoy is None or Jd > m)
    assert all(v[0] >= 0 and np.isfinite(v[1]) for v in ref.values())
    assert len({v[0] for v in ref.values()}) >= 18                          # the rows do not share one answer


def test_cap_case_rows():
    tt, picks, w, delta = Cs.cap_case()
    assert L.check(picks, w) is None and int((w == 0).sum()) >= 5 and not np.any(np.all(w == 0, axis=1))
    cell, m, t0, _ = Cs.locate_rows(tt, picks, w)
    assert np.all(cell >= 0) and len(set(cell.tolist())) >= 6 and len(np.unique(m)) > Cs.CAP_P // 2
    assert len(set(zip(cell.tolist(), m.tolist(), t0.tolist()))) == Cs.CAP_P          # every row has its own answer


@pytest.mark.parametrize("N", sorted(Cs.N_SHAPES))
def test_k_edge_cases_carry_their_weight_patterns(N):
    assert int(np.prod(Cs.N_SHAPES[N])) == N
    for K in Cs.K_EDGES:
        c = Cs.k_edge_case(K, N)
        w, s0 = c["weights"], c["s0"]
        assert L.check(c["picks"], w) is None
        seen = set()
        for e, p in enumerate(c["patterns"]):
            seen.add(p)
            bits = Cs.u64(w[e])
            if p == "dense":
                assert np.all(w[e] > 0)
            elif p == "zero_first":
                assert bits[0] == 0 and np.all(w[e, 1:] > 0)
            elif p == "zero_last":
                assert bits[K - 1] == 0 and np.all(w[e, :K - 1] > 0)
            elif p == "neg_zero":
                assert bits[s0] == 1 << 63 and np.all(np.delete(w[e], s0) > 0)
                J, _ = Cs.misfit(c["tt"], c["picks"][e], w[e])
                if N >= 255:        # cells only the station without a pick does not reach are admissible, and win
                    hidden = ~np.isfinite(c["tt"][s0])
                    assert np.any(J[hidden] < np.inf)
                    assert K == 2 or hidden.reshape(-1)[int(np.argmin(J))]      # K = 2 leaves one pick: J ~ 0
            else:
                assert int((w[e] != 0).sum()) == 1
        assert seen == (set(Cs.PATTERNS) if K > 1 else {"dense", "single"})
        assert c["none"]["weights"] is None and len(c["none"]["picks"]) == Cs.K_E_NONE
        if N >= 255:
            assert np.all(np.isfinite(c["weighted"]["m"])) and np.any(~np.isfinite(c["tt"]))


@pytest.mark.parametrize("route", Cs.RANGE_ROUTES)
def test_float_range_routes_are_taken(route):
    """Each route of the double range is really taken by the restatement (Cs.range_claim), the case is not one the
    library refuses, and the restatement agrees with the per-cell Python loop on it."""
    admissible = Cs.range_claim(route)
    tt, picks, w = Cs.range_case(route)
    for e in range(len(picks)):
        with np.errstate(all="ignore"):
            cell, m, _ = agree(tt, picks[e], None if w is None else w[e])
        assert (cell >= 0) == (admissible[e] > 0) and (m < np.inf) == (admissible[e] > 0)
