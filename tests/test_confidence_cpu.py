"""CPU tier of the confidence regions of located events (include/ttsweep.h, "locate confidence"): the numpy
restatement (confidence_reference.py) against a per-cell pure-Python loop and on hand-made cases, the host-side helpers
of ConfidenceRegions against exact rational arithmetic, the C ABI's surface (symbol exported and bound, the macro,
bad arguments refused before any device work) and the Python exports."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN
import confidence_reference as R
import locate_cases as Cs
import locate_reference as L

INF = np.float32(np.inf)


def one(tt, o, w, m, deltas):
    """confidence() of one event; every field also checked against the cell loop."""
    out = R.confidence(tt, np.asarray(o, np.float64)[None], None if w is None else np.asarray(w, np.float64)[None],
                       [m], np.asarray(deltas, np.float64)[None])
    slow = R.confidence_slow(tt, o, w, m, deltas)
    blank = R.empty(np.asarray(tt).shape[1:], 1, len(deltas))
    for l, s in enumerate(slow):
        for f in R.FIELDS:
            want = blank[f][0, l] if s is None else np.asarray(s[f], blank[f].dtype)
            assert np.asarray(out[f][0, l]).tobytes() == np.asarray(want).tobytes(), (f, l)
    return {f: v[0] for f, v in out.items()}


def test_reference_agrees_with_a_cell_loop_on_random_boxes():
    rng = np.random.default_rng(3)
    seen = 0
    for K in (1, 2, 5):
        tt = rng.uniform(0, 10, (K, 3, 4, 2)).astype(np.float32)
        tt[rng.random(tt.shape) < 0.1] = INF
        for _ in range(5):
            o = rng.uniform(0, 20, K)
            w = rng.uniform(0.1, 2, K)
            w[rng.random(K) < 0.3] = 0
            if not np.any(w):
                w[0] = 1.0
            _, m, _, _ = L.locate(tt, o[None], w[None])
            for deltas in ([3.0], [0.0, 2.0, 50.0, np.inf]):
                r = one(tt, o, w, m[0], deltas)
                seen += int(r["count"].max())
            one(tt, o, None, 1.0, [0.5, 7.0, 1.0, 0.0])
    assert seen > 50


def test_delta_zero_gives_the_cells_at_the_minimum_and_a_tie_counts_two():
    tt = np.array([[[[0, 1, 0, 1]]], [[[2, 4, 2, 4]]]], np.float32)     # [2, 1, 1, 4]: cells 0 and 2 fit both picks
    cell, m, _, _ = L.locate(tt, np.array([[5.0, 7.0]]))
    r = one(tt, [5.0, 7.0], None, m[0], [0.0])
    J, _ = L.misfit(tt, [5.0, 7.0])
    assert r["count"][0] == 2 == int((J == m[0]).sum()) and J.reshape(-1)[cell[0]] == m[0]
    assert r["lo"][0].tolist() == [0, 0, 0] and r["hi"][0].tolist() == [0, 0, 2]
    assert r["sum"][0].tolist() == [0, 0, 2] and r["sum2"][0].tolist() == [0, 0, 4, 0, 0, 0]


def test_infinite_delta_gives_every_admissible_cell_and_levels_are_nested():
    rng = np.random.default_rng(5)
    tt = rng.uniform(0, 10, (3, 4, 3, 5)).astype(np.float32)
    tt[rng.random(tt.shape) < 0.15] = INF
    o = rng.uniform(0, 20, 3)
    _, m, _, _ = L.locate(tt, o[None])
    r = one(tt, o, None, m[0], [0.0, 4.0, 30.0, np.inf])
    J, _ = L.misfit(tt, o)
    assert r["count"][3] == int((J < np.inf).sum()) > 0
    assert np.all(np.diff(r["count"]) >= 0) and r["count"][0] >= 1
    assert np.all(np.diff(r["lo"], axis=0) <= 0) and np.all(np.diff(r["hi"], axis=0) >= 0)
    assert np.all(np.diff(r["t0_lo"]) <= 0) and np.all(np.diff(r["t0_hi"]) >= 0)


def test_empty_regions_have_the_values_of_the_table():
    tt = np.arange(24, dtype=np.float32).reshape(1, 2, 3, 4)
    for m, deltas in ((np.inf, [0.0, np.inf]), (0.0, [0.0, 0.0])):
        tt2 = np.concatenate([tt, tt[:, ::-1]])                     # two stations: J > 0 everywhere
        r = one(tt2, [100.0, 90.0], None, m, deltas)
        assert np.all(r["count"] == 0) and np.all(r["sum"] == 0) and np.all(r["sum2"] == 0)
        assert np.all(r["lo"] == [2, 3, 4]) and np.all(r["hi"] == -1)
        assert np.all(r["t0_lo"] == np.inf) and np.all(r["t0_hi"] == -np.inf)
    none = np.array([[[[INF, 1]]], [[[2, INF]]]], np.float32)         # no admissible cell at all
    r = one(none, [1.0, 1.0], None, 0.0, [np.inf])
    assert r["count"][0] == 0 and np.all(r["lo"] == [1, 1, 2])


def test_origin_times_of_both_zeros_order_as_total_order():
    r = R.region(np.zeros((1, 1, 2)), np.array([[[0.0, -0.0]]]), 0.0, 0.0)
    assert r["count"] == 2
    assert np.signbit(r["t0_lo"]) and not np.signbit(r["t0_hi"]) and r["t0_lo"] == 0.0 == r["t0_hi"]
    r = R.region(np.zeros((1, 1, 2)), np.array([[[-0.0, 0.0]]]), 0.0, 0.0)
    assert np.signbit(r["t0_lo"]) and not np.signbit(r["t0_hi"])
    k = R.t0_key(np.array([-np.inf, -1.0, -0.0, 0.0, 5e-324, 1.0, np.inf]))
    assert np.all(np.diff(k.astype(object)) > 0)


def test_refusals_of_the_reference():
    assert R.check([0.0, np.inf], [[0.0, np.inf], [1.0, 2.0]]) is None
    assert R.check([0.0, np.nan], [[0.0], [1.0]]) == "misfit"
    assert R.check([0.0, -1.0], [[0.0], [1.0]]) == "misfit"
    assert R.check([0.0, 1.0], [[0.0], [np.nan]]) == "delta"
    assert R.check([0.0, 1.0], [[-1e-300], [1.0]]) == "delta"
    assert R.moments_fit((241, 241, 51)) and R.moments_fit((1024, 1024, 512))
    assert not R.moments_fit((1, 1, 2097152)) and R.moments_fit((1, 1, 2097151))


def regions(pkg, count, s, q, lo, hi, shape):
    import torch
    t = torch.from_numpy
    E = len(count)
    return pkg.ConfidenceRegions(t(np.asarray(count, np.int64).reshape(E, 1)), t(np.asarray(s, np.int64).reshape(E, 1, 3)),
                                 t(np.asarray(q, np.int64).reshape(E, 1, 6)), t(np.asarray(lo, np.int32).reshape(E, 1, 3)),
                                 t(np.asarray(hi, np.int32).reshape(E, 1, 3)), t(np.zeros((E, 1))), t(np.zeros((E, 1))),
                                 shape)


def test_centroid_and_covariance_against_exact_rationals(pkg):
    rng = np.random.default_rng(7)
    shape = (1000, 900, 800)
    counts, sums, sum2s = [], [], []
    for n in (1, 2, 7, 500, 20000):
        c = np.stack([rng.integers(0, s, n) for s in shape], 1).astype(np.int64)
        if n == 500:
            c = c // 50 + np.array([900, 800, 700])                 # a small cloud far from the origin
        counts.append(n)
        sums.append(c.sum(0))
        sum2s.append([int((c[:, a] * c[:, b]).sum()) for a, b in R.SUM2])
    counts.append(0)
    sums.append([0, 0, 0])
    sum2s.append([0] * 6)
    r = regions(pkg, counts, sums, sum2s, np.zeros((6, 3)), np.zeros((6, 3)), shape)
    cen, cov = r.centroid(), r.covariance()
    assert cen.shape == (6, 1, 3) and cov.shape == (6, 1, 3, 3) and cen.dtype == cov.dtype == np.float64
    assert np.all(np.isnan(cen[5])) and np.all(np.isnan(cov[5]))
    assert np.array_equal(cov[:5], np.swapaxes(cov[:5], -1, -2))
    for e in range(5):
        n, s, q = counts[e], [int(x) for x in sums[e]], sum2s[e]
        sq = {ab: q[i] for i, ab in enumerate(R.SUM2)}
        for a in range(3):
            assert abs(Fraction(float(cen[e, 0, a])) - Fraction(s[a], n)) <= Fraction(s[a], n) * Fraction(1, 2 ** 52)
            for b in range(3):
                exact = Fraction(sq[(min(a, b), max(a, b))], n) - Fraction(s[a] * s[b], n * n)
                bound = 8 * Fraction(1, 2 ** 52) * Fraction(max(sq[(a, a)], sq[(b, b)]), n)
                assert abs(Fraction(float(cov[e, 0, a, b])) - exact) <= bound, (e, a, b)


def test_open_on_each_of_the_six_faces(pkg):
    shape = (9, 8, 7)
    lo, hi, want = [[3, 3, 3]], [[5, 4, 4]], [False]
    for a in range(3):
        l, h = [3, 3, 3], [5, 4, 4]
        l[a] = 0
        lo.append(l), hi.append([5, 4, 4]), want.append(True)
        h[a] = shape[a] - 1
        lo.append([3, 3, 3]), hi.append(h), want.append(True)
    lo.append(list(shape)), hi.append([-1, -1, -1]), want.append(False)     # the empty region
    count = [1] * 7 + [0]
    r = regions(pkg, count, np.zeros((8, 3)), np.zeros((8, 6)), lo, hi, shape)
    assert r.open().shape == (8, 1) and r.open()[:, 0].tolist() == want
    assert len(r) == 8


def test_confidence_symbol_exported_and_bound(pkg):
    lib = pkg._lib.lib()
    assert hasattr(lib, "ttsweep_locate_confidence_device")
    assert "ttsweep_locate_confidence_device" in {n for n, _, _ in pkg._lib.SYMBOLS}
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ttsweep.h")).read()
    assert "#define TTSWEEP_HAS_LOCATE_CONFIDENCE 1" in hdr
    assert "#define TTSWEEP_ABI_VERSION 6" in hdr or "#define TTSWEEP_ABI_VERSION (6)" in hdr
    assert lib.ttsweep_abi_version() == 6
    assert pkg.ConfidenceRegions is pkg.solver.ConfidenceRegions and "ConfidenceRegions" in pkg.__all__
    assert callable(pkg.TravelTimeSolver.locate_confidence)


def test_bad_confidence_arguments_are_refused_without_a_device(pkg):
    conf = pkg._lib.lib().ttsweep_locate_confidence_device
    ptr = (C.c_void_p * 1)(None)
    d = C.c_void_p(8)                           # never read: every call below is refused first
    outs = (None,) * 7

    def last():
        return pkg._lib.last_error()

    assert conf(None, 1, ptr, 1, d, None, d, 1, d, *outs) < 0       # only the context is missing
    assert "ttsweep_locate_confidence_device" in last() and "null or bad argument" in last()
    # the checks below come before the context is read, so a NULL context is refused for the reason given
    for nbox, tt, nev, picks, m, nlevel, delta in ((0, ptr, 1, d, d, 1, d), (1, ptr, 0, d, d, 1, d), (-1, ptr, 1, d, d, 1, d),
                                                   (1, None, 1, d, d, 1, d), (1, ptr, 1, None, d, 1, d),
                                                   (1, ptr, 1, d, None, 1, d), (1, ptr, 1, d, d, 1, None),
                                                   (1, ptr, 1, d, d, 0, d), (1, ptr, 1, d, d, 5, d)):
        assert conf(None, nbox, tt, nev, picks, None, m, nlevel, delta, *outs) < 0
        assert "null or bad argument" in last()
    # 65536 x 65536 picks do not fit int32 indices: refused before the (one-element) box list is read
    assert conf(None, 65536, ptr, 65536, d, None, d, 1, d, *outs) < 0
    assert "int32" in last()


def test_locate_confidence_checks_arguments_before_the_library(pkg):
    """TravelTimeSolver.locate_confidence refuses a wrong tt before it reaches C (no device needed to get there)."""
    sol = pkg.TravelTimeSolver.__new__(pkg.TravelTimeSolver)
    sol.shape, sol.device = (2, 2, 2), 0
    with pytest.raises(pkg.TTSweepError):
        sol.locate_confidence(np.zeros((1, 2, 2, 2), np.float32), np.zeros((1, 1)), None, np.zeros(1), 1.0)


# ---- the claims of the confidence cases of locate_cases.py, checked with the restatement alone ----

def test_k_edge_regions_are_not_trivial():
    """Every (K, N) of the K-edge cases, both calls, the sparse level: the restatement's region is neither empty nor
    every admissible cell for at least three quarters of the events.  The restatement gives 1253 of 1456 here (counts 5 ... 7592): every event
    on the seven grids of 255 cells and more but the K = 1 events with unit weights (J = +0 at every cell), none on
    the grid of one cell, where no region can be.  Level 0 holds the located cell and delta = +inf every admissible cell."""
    inside = total = 0
    lo, hi = 10 ** 9, 0
    for N in Cs.N_SHAPES:
        for K in Cs.K_EDGES:
            c = Cs.k_edge_case(K, N)
            for call in ("weighted", "none"):
                d = c[call]
                assert R.check(d["m"], d["delta"]) is None
                got = Cs.confidence(c["tt"], d["picks"], d["weights"], d["m"], d["delta"])["count"]
                ok = (got[:, 1] > 0) & (got[:, 1] < got[:, 2])       # full: every admissible cell
                inside, total = inside + int(ok.sum()), total + len(ok)
                if N > 1 and (K > 1 or call == "weighted"):      # K = 1 with unit weights: J = +0 everywhere
                    lo, hi = min(lo, int(got[:, 1].min())), max(hi, int(got[:, 1].max()))
                    assert np.all(got[:, 0] >= 1) and np.all(got[:, 0] <= got[:, 1]) and np.all(got[:, 1] < got[:, 2])
    print("sparse regions neither empty nor full:", inside, "of", total, "counts", lo, "...", hi)
    assert inside >= 0.75 * total


def test_cap_case_levels():
    tt, picks, w, delta = Cs.cap_case()
    _, m, _, _ = Cs.locate_rows(tt, picks, w)
    assert R.check(m, delta) is None and delta.shape == (Cs.CAP_P, 4)
    got = Cs.confidence(tt, picks, w, m, delta)["count"]
    assert np.all(got[:, 0] >= 1) and np.all(np.diff(got, axis=1) >= 0) and len(np.unique(got[:, 2])) >= 4


def test_thresholds_at_the_largest_finite_double():
    tt, picks, w, m, delta = Cs.conf_range_case("thr_largest_finite")
    assert R.check(m, delta) is None
    with np.errstate(all="ignore"):
        thr = m[:, None] + delta
    inf_bits = Cs.u64(np.inf)
    for e, l in ((0, 0), (1, 0), (1, 2), (2, 0), (3, 0)):       # (1, 0) gets there by rounding up
        assert thr[e, l] == Cs.DBL_MAX and Cs.u64(thr[e, l]) + 1 == inf_bits, (e, l)
    assert m[1] + delta[1, 0] > m[1] and delta[1, 0] < 2.0 ** 971
    assert thr[0, 2] == np.inf and thr[2, 2] == np.inf
    got = Cs.confidence(tt, picks, w, m, delta)["count"]
    adm = int(np.all(np.isfinite(tt), axis=0).sum())
    J, _ = Cs.misfit(tt, picks[0])
    assert m[2] == J[J < np.inf].max() and np.all(got[:3] == adm) and got[3].tolist() == [adm, adm, 0]


def test_thresholds_in_the_subnormal_range():
    tt, picks, w, m, delta = Cs.conf_range_case("thr_subnormal")
    assert R.check(m, delta) is None
    thr = m[:, None] + delta
    assert np.all(thr > 0) and np.all(thr < Cs.DBL_TINY) and np.all(delta[:, 1:] > 0) and np.all(m < Cs.DBL_TINY)
    got = Cs.confidence(tt, picks, w, m, delta)["count"]
    adm = int((Cs.misfit(tt, picks[0], w[0])[0] < np.inf).sum())
    assert np.all(got[:, 0] >= 1) and np.all(got[:, 2] > got[:, 0]) and np.all(got[:, 3] > got[:, 2])
    assert np.all(got[:, 3] < adm)


def test_thresholds_one_ulp_around_a_cell():
    tt, picks, w, m, delta = Cs.conf_range_case("thr_one_ulp")
    assert R.check(m, delta) is None and np.all(delta == 0)
    J, _ = Cs.misfit(tt, picks[0], w[0])
    got = Cs.confidence(tt, picks, w, m, delta)["count"][:, 0].reshape(-1, 3)
    at = m.reshape(-1, 3)[:, 1]
    for (below, exact, above), Jx in zip(got.tolist(), at):
        assert exact == above == int((J <= Jx).sum()) and exact - below == int((J == Jx).sum()) >= 1
    assert got[0, 0] == 0 and got[-1, 1] == J.size
