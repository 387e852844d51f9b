"""Case builders shared by the CPU and GPU tiers of locate and locate confidence (no fixtures, no conftest).

Every input is built from seeded numpy.  Beside the input each builder returns what the case claims to exercise
(batch edges, planted minima and ties, weight patterns, float-range routes).  The CPU tier checks those claims with
the restatements (locate_reference.py, confidence_reference.py) alone; the GPU tier compares the library with the
restatements on the same inputs.  The constants below mirror the library's (ttsweep_locate.hip / ttsweep_locate.cpp);
the sources name the tests that depend on them."""
import functools

import numpy as np

import confidence_reference as R
import locate_reference as L

F32 = np.float32
F32_INF = F32(np.inf)
DBL_MAX = np.finfo(np.float64).max
DBL_TINY = np.finfo(np.float64).tiny       # the smallest normal double

STEP = 256                  # LOC_BLOCK: cells of one step of a search block, and of one volume block
TILE = 16 * STEP            # LOC_C * LOC_BLOCK: cells per search block
ET = 8                      # LOC_ET: events per search block
PARTIALS = 1 << 24          # LOC_PARTIALS: per-tile partials of one batch of events, at most
CAP = 65535 * ET            # the launch limit on grid.y, in events
KR_WIDTHS = (8, 16, 24, 32)  # loc_kr(): the register instances; above 32 the boxes are read on use


def u64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def batches(shape, E):
    """(ntiles, eb, first event of every batch) of ttsweep_locate_device for E events on a grid of this shape."""
    N = int(np.prod([int(n) for n in shape], dtype=object))
    ntiles = -(-N // TILE)
    eb = max(1, min(E, PARTIALS // ntiles, CAP))
    return ntiles, eb, list(range(0, E, eb))


def locate_rows(tt, picks, weights=None, probe=None):
    """The restatement's (cell, misfit, t0) of every row, one event at a time so that only one J volume is alive;
    probe(e, J) -> anything is kept per row (the claims' view of the volume)."""
    picks = np.asarray(picks, np.float64)
    E = len(picks)
    cell, mis, t0 = np.empty(E, np.int32), np.empty(E), np.empty(E)
    kept = []
    with np.errstate(all="ignore"):
        for e in range(E):
            w = None if weights is None else np.asarray(weights, np.float64)[e:e + 1]
            c, m, t, vols = L.locate(tt, picks[e:e + 1], w, volumes=(0,))
            cell[e], mis[e], t0[e] = c[0], m[0], t[0]
            if probe is not None:
                kept.append(probe(e, vols[0]))
    return cell, mis, t0, kept


def misfit(tt, o, w=None):
    with np.errstate(all="ignore"):
        return L.misfit(tt, o, w)


def confidence(tt, picks, weights, m, delta):
    with np.errstate(all="ignore"):
        return R.confidence(tt, picks, weights, m, delta)


# ---- 1. second and third batches of locate: a grid of many tiles, periodic events, planted minima and ties ----
BIG_SHAPE = (17, 59, 4095)          # 4 107 285 cells: 1003 tiles, the last one partial
BIG_P = 97                          # distinct event rows, prime: batch edges fall on different rows
BIG_BACKGROUND = (300, 1000)        # a[x] of the cells nothing is planted in; rows use c = 3 * row <= 288


def big_plants():
    """{row: (kind, cells of the tied minimum, a decoy cell one step worse or None)} on BIG_SHAPE.  lane / wave /
    step are those of locate_search_kernel (x = tile * 4096 + j * 256 + tid), thread those of locate_final_kernel
    (tile % 256)."""
    N = int(np.prod(BIG_SHAPE))
    last = (N - 1) // TILE          # 1002
    b = lambda t: t * TILE
    laststep = b(last) + (N - b(last) - 1) // STEP * STEP      # first cell of the partial last step
    every = [b(t) + (t * 37 + 11) % 3000 for t in range(last + 1)]
    return {
        0: ("cell 0", [0], 1),
        1: ("cell N-1: the last lane of the partial step of the partial tile", [N - 1], 5),
        2: ("cell 4095: the last cell of tile 0", [4095], 4094),
        3: ("cell 4096: the first cell of tile 1", [4096], 4097),
        4: ("tile 5", [b(5) + 1234], b(5) + 1233),
        5: ("tile 261: the thread of tile 5 in the final kernel", [b(261) + 77], b(5) + 78),
        6: ("tile 300", [b(300) + 4000], b(299) + 4000),
        7: ("tile 1002: the partial tile", [b(last) + 100], b(last - 1) + 100),
        8: ("tie in one lane at two steps: x, x + 256", [b(5) + 7, b(5) + 7 + STEP], None),
        9: ("tie in two waves: x, x + 64", [b(5) + 2 * STEP + 9, b(5) + 2 * STEP + 9 + 64], None),
        10: ("tie of lane 1 step 0 with lane 0 step 1", [b(300) + 1, b(300) + STEP], None),
        11: ("tie in tiles 5 and 261: one thread of the final kernel", [b(5) + 300, b(261) + 2], None),
        12: ("tie in tiles 1 and 256: lanes 1 and 0 of the final kernel", [b(1) + 50, b(256) + 50], None),
        13: ("tie in tiles 70 and 256: waves 1 and 0 of the final kernel", [b(70) + 9, b(256) + 9], None),
        14: ("tie of three in tiles 300 and 1002", [b(300) + 3333, b(last) + 5, b(last) + 3000], None),
        15: ("tie of the second cell and the second-to-last cell", [2, N - 2], None),
        16: ("tie inside the partial last step: its first lane and a later one", [laststep, N - 3], None),
        17: ("tie of one cell in every tile", every, None),
    }


@functools.lru_cache(maxsize=None)
def big_box():
    """[2, 17, 59, 4095] float32: T0 = 0, T1 = a, small integers; a = 3 * row at the cells planted for a row,
    3 * row + 1 at its decoy, BIG_BACKGROUND elsewhere."""
    N = int(np.prod(BIG_SHAPE))
    rng = np.random.default_rng(1003)
    a = rng.integers(*BIG_BACKGROUND, N).astype(F32)
    used = set()
    for row, (_, cells, decoy) in big_plants().items():
        for x in cells + ([] if decoy is None else [decoy]):
            assert 0 <= x < N and x not in used, (row, x)
            used.add(x)
        a[cells] = 3 * row
        if decoy is not None:
            a[decoy] = 3 * row + 1
    tt = np.zeros((2, N), F32)
    tt[1] = a
    tt = tt.reshape((2,) + BIG_SHAPE)
    tt.setflags(write=False)
    return tt


def big_rows(variant):
    """(picks [P, 2], weights [P, 2] or None) of the P distinct rows.
    "unit": weights None, picks (0, c) with c = 3 * row: J(x) = (c - a[x])^2 / 2 exactly, +0 at the planted cells,
    0.5 at the decoy, >= 2 at every other cell.
    "weighted": weights (0.7 + row / 100, 1.9 - row / 100), picks (0.3, c + 0.1): J is a function of a[x] alone, so
    the planted cells still tie, at a minimum that is not zero; nothing is taken from the algebra, the claims come
    from the restatement's J bits."""
    row = np.arange(BIG_P, dtype=np.float64)
    if variant == "unit":
        return np.stack([np.zeros(BIG_P), 3.0 * row], 1), None
    assert variant == "weighted"
    return (np.stack([np.full(BIG_P, 0.3), 3.0 * row + 0.1], 1),
            np.stack([0.7 + row / 100.0, 1.9 - row / 100.0], 1))


BIG_E = 2 * (PARTIALS // 1003) + 5          # three batches of locate on BIG_SHAPE


def periodic(rows, E):
    return None if rows is None else np.ascontiguousarray(rows[np.arange(E) % len(rows)])


@functools.lru_cache(maxsize=None)
def big_reference(variant, rows=None):
    """The restatement on the distinct rows (all, or the tuple rows): {row: (cell, misfit, t0, J at the planted
    cells, J at the decoy, number of cells at the minimum)}."""
    tt = big_box()
    picks, w = big_rows(variant)
    idx = list(range(BIG_P)) if rows is None else list(rows)
    plants = big_plants()

    def probe(i, J):
        _, cells, decoy = plants.get(idx[i], ("", [], None))
        Jf = J.reshape(-1)
        return Jf[cells].copy(), None if decoy is None else Jf[decoy], int((Jf == Jf.min()).sum())

    c, m, t, kept = locate_rows(tt, picks[idx], None if w is None else w[idx], probe)
    return {r: (int(c[i]), m[i], t[i]) + kept[i] for i, r in enumerate(idx)}


# ---- 2. the 65535 * 8 cap: a tiny grid, periodic events, two launches of the search ----
CAP_SHAPE = (2, 3, 2)
CAP_E = CAP + 3
CAP_P = 97


@functools.lru_cache(maxsize=None)
def cap_case():
    """(tt [2, 2, 3, 2], picks [P, 2], weights [P, 2], delta [P, 4]) of the distinct rows; a fifth of the rows have
    one station without a pick, one cell of a box is at infinity."""
    rng = np.random.default_rng(524283)
    tt = rng.uniform(0, 9, (2,) + CAP_SHAPE).astype(F32)
    tt[1, 1, 2, 0] = F32_INF
    picks = rng.uniform(-3, 12, (CAP_P, 2))
    w = rng.uniform(0.5, 2.0, (CAP_P, 2))
    drop = np.flatnonzero(rng.random(CAP_P) < 0.2)
    w[drop, rng.integers(0, 2, len(drop))] = 0.0
    delta = np.stack([np.zeros(CAP_P), rng.uniform(0, 3, CAP_P), rng.uniform(3, 30, CAP_P), np.full(CAP_P, np.inf)], 1)
    return tt, picks, w, delta


# ---- 3. K edges: full and just-over-full register instances against cell counts around the block sizes ----
K_EDGES = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33)
N_SHAPES = {1: (1, 1, 1), 255: (3, 5, 17), 256: (4, 8, 8), 257: (1, 257, 1), 4095: (5, 9, 91), 4096: (16, 16, 16),
            4097: (17, 1, 241), 8193: (3, 2731, 1)}
PATTERNS = ("dense", "zero_first", "zero_last", "neg_zero", "single")
K_E = 10                    # weighted events: two of every pattern, a full event block and a partial one
K_E_NONE = 3                # events of the call with weights None


def sparse_delta(J, m, share=16):
    """A level for which the restatement's region is neither empty nor full: thr halfway between the q-th and the
    (q+1)-th smallest admissible J, q = max(2, admissible / share).  1.0 when fewer than four cells are admissible."""
    Ja = np.sort(J[J < np.inf])
    if len(Ja) < 4 or not np.isfinite(m):
        return 1.0
    q = max(2, len(Ja) // share)
    return float(max(0.0, 0.5 * Ja[q - 1] + 0.5 * Ja[q] - m))


@functools.lru_cache(maxsize=None)
def k_edge_case(K, N):
    """Random boxes [K, shape of N cells] with 2 % of the cells at infinity (none when N = 1) and, for K > 1, a
    quarter of the cells of station `s0` at infinity; K_E weighted events, event e of pattern PATTERNS[e % 5]
    ("dense" for what K cannot carry), whose -0.0 sits at station s0 and whose true cell has T_s0 = INF; K_E_NONE
    events for weights None.  Returns a dict: tt, picks, weights, patterns, s0, and per call ("weighted", "none")
    the restatement's m and the levels delta = (0, sparse, INF)."""
    shape = N_SHAPES[N]
    rng = np.random.default_rng([3, K, N])
    tt = rng.uniform(0, 20, (K,) + shape).astype(F32)
    if N > 1:
        tt[rng.random(tt.shape) < 0.02] = F32_INF
    s0 = int(rng.integers(0, K))
    flat = tt.reshape(K, -1)
    if K > 1 and N > 1:
        flat[s0, rng.random(N) < 0.25] = F32_INF
    others = np.all(np.isfinite(np.delete(flat, s0, 0)), axis=0) if K > 1 else np.isfinite(flat[0])
    every = others & np.isfinite(flat[s0])
    hidden = others & ~np.isfinite(flat[s0])          # reached by every station but s0

    def cell_from(mask):
        ok = np.flatnonzero(mask)
        return int(ok[rng.integers(0, len(ok))]) if len(ok) else int(rng.integers(0, N))

    patterns = [PATTERNS[e % 5] if K > 1 else ("dense", "single")[e % 2] for e in range(K_E)]
    picks = np.empty((K_E, K))
    w = rng.uniform(0.5, 2.0, (K_E, K))
    for e, p in enumerate(patterns):
        x = cell_from(hidden if p == "neg_zero" else every)
        T = flat[:, x].astype(np.float64)
        picks[e] = np.where(np.isfinite(T), T, 0.0) + rng.uniform(-5, 5) + 0.3 * rng.standard_normal(K)
        if p == "zero_first":
            w[e, 0] = 0.0
        elif p == "zero_last":
            w[e, K - 1] = 0.0
        elif p == "neg_zero":
            w[e, s0] = -0.0
        elif p == "single":
            keep = w[e, (s0 + 1) % K]
            w[e] = 0.0
            w[e, (s0 + 1) % K] = keep
    out = {"tt": tt, "shape": shape, "patterns": patterns, "s0": s0, "picks": picks, "weights": w}
    for name, o, ww in (("weighted", picks, w), ("none", picks[:K_E_NONE], None)):
        m = np.empty(len(o))
        delta = np.empty((len(o), 3))
        for e in range(len(o)):
            J, _ = misfit(tt, o[e], None if ww is None else ww[e])
            m[e] = J.min()
            delta[e] = (0.0, sparse_delta(J, m[e]), np.inf)
        out[name] = {"picks": o, "weights": ww, "m": m, "delta": delta}
    return out


# ---- 4. the double range of picks, weights, m and delta ----
RANGE_SHAPE = (5, 7, 11)            # 385 cells: two steps of one tile, the second partial; two volume blocks


def partial_sums(tt, o, w=None):
    """(W, invW, S1 [shape]) of one event: the first pass of the contract's formula, for the route claims (the
    restatement returns t0 = S1 * invW only).  The same numpy operations in the same order."""
    tt = np.asarray(tt, F32)
    K = tt.shape[0]
    w = np.ones(K) if w is None else np.asarray(w, np.float64)
    o = np.asarray(o, np.float64)
    with np.errstate(all="ignore"):
        W = np.float64(0.0)
        S1 = np.zeros(tt.shape[1:])
        for k in range(K):
            if w[k] != 0:
                W = W + w[k]
                S1 = np.add(S1, np.multiply(w[k], np.subtract(o[k], tt[k].astype(np.float64))))
        return W, np.float64(1.0) / W, S1


def range_box(rng, K, inf_share=0.03):
    tt = rng.uniform(1, 2, (K,) + RANGE_SHAPE).astype(F32)
    tt[rng.random(tt.shape) < inf_share] = F32_INF
    return tt


def _near(tt, rng, E, spread):
    """picks within `spread` of the travel times of a cell every station reaches"""
    flat = tt.reshape(tt.shape[0], -1)
    ok = np.flatnonzero(np.all(np.isfinite(flat), axis=0))
    x = ok[rng.integers(0, len(ok), E)]
    return flat[:, x].T.astype(np.float64) + rng.uniform(-spread, spread, (E, tt.shape[0]))


RANGE_ROUTES = ("s1_overflows", "wrr_overflows", "huge_finite_misfit", "s1_inf_minus_inf", "w_overflows_invw_zero",
                "invw_overflows", "subnormal_weights", "subnormal_residuals")


@functools.lru_cache(maxsize=None)
def range_case(route):
    """(tt, picks [E, K], weights [E, K] or None) of one float-range route of locate; what the route must show is
    checked by range_claim()."""
    rng = np.random.default_rng([4, RANGE_ROUTES.index(route)])
    big = 1.7e308
    if route == "s1_overflows":                 # S1 = 1.7e308 + 1.7e308 = +INF (and -INF for the second event)
        tt = range_box(rng, 3)
        return tt, np.array([[big] * 3, [-big] * 3, [big, big, 1.0]]), None
    if route == "wrr_overflows":                # S1 and t0 finite, r = 1e160: (w * r) * r = +INF
        tt = range_box(rng, 4)
        return tt, np.array([[1e160, -1e160, 3.0, 1.0], [2.0, 1e155, 1.0, -1e155]]), np.array([[1.0] * 4, [2.0, 0.5, 0.0, 0.5]])
    if route == "huge_finite_misfit":           # r ~ 1e153: J ~ 1e306, finite, the boxes' values absorbed; 1e9: not
        tt = range_box(rng, 4)
        return tt, np.array([[1e153, -1e153, 3.0, 1.0], [3e153, 1.0, 2.0, -1e153], [1e9, -1e9, 2.0, 1.0]]), None
    if route == "s1_inf_minus_inf":             # w * (o - T) = +INF and -INF both enter S1: NaN
        tt = range_box(rng, 4)
        return (tt, np.array([[big, -big, 1.0, 2.0], [1.0, -big, big, 2.0]]),
                np.array([[10.0, 10.0, 1.0, 1.0], [1.0, 4.0, 4.0, 0.0]]))
    if route == "w_overflows_invw_zero":        # W = 3e308 = +INF, invW = 0, t0 = S1 * 0
        tt = range_box(rng, 3)
        return tt, _near(tt, rng, 4, 0.2), np.full((4, 3), 1e308)
    if route == "invw_overflows":               # W = 3e-310, 1.0 / W = +INF
        tt = range_box(rng, 3)
        return tt, _near(tt, rng, 3, 0.5), np.full((3, 3), 1e-310)
    if route == "subnormal_weights":            # every weight subnormal, W normal, J subnormal
        tt = range_box(rng, 5)
        w = np.tile([3e-309, 2e-309, 4e-309, 0.0, 2.5e-309], (4, 1))
        w[1, 0] = 5e-324
        return tt, _near(tt, rng, 4, 0.5), w
    assert route == "subnormal_residuals"       # T = 0 on half of the cells, picks subnormal: r^2 underflows to +0
    tt = range_box(rng, 3, inf_share=0.0)
    zero = rng.random(RANGE_SHAPE) < 0.5
    zero[0, 0, :3] = False
    tt[:, zero] = 0.0
    return tt, np.array([[1e-310, 3e-310, 2e-310], [4e-320, -4e-320, 0.0], [5e-324, 5e-324, 5e-324]]), None


def range_claim(route):
    """Raises AssertionError unless the restatement takes the route on range_case(route); returns a short record."""
    tt, picks, w = range_case(route)
    E = len(picks)
    assert L.check(picks, w) is None, "the case must not be refused"
    rec = []
    for e in range(E):
        we = None if w is None else w[e]
        W, invW, S1 = partial_sums(tt, picks[e], we)
        J, t0 = misfit(tt, picks[e], we)
        with np.errstate(all="ignore"):
            assert np.array_equal(u64(np.multiply(S1, invW))[J < np.inf], u64(t0)[J < np.inf])
        adm = int((J < np.inf).sum())
        rec.append(adm)
        fin = np.all(np.isfinite(tt), axis=0)        # the cells every box reaches
        if route == "s1_overflows":
            assert fin.sum() > 300 and adm == 0 and np.all(S1[fin] == (np.inf if picks[e, 0] > 0 else -np.inf))
        elif route == "wrr_overflows":
            assert np.all(np.isfinite(S1[np.all(np.isfinite(tt[np.asarray(we) != 0]), axis=0)])) and adm == 0
            assert np.isfinite(invW)
        elif route == "huge_finite_misfit":
            assert adm == int(np.all(np.isfinite(tt), axis=0).sum()) > 300
            assert np.all(J[J < np.inf] > (1e300 if e < 2 else 1e18))
            if e == 2:
                assert len(np.unique(J[J < np.inf])) > 300     # the boxes' values are not absorbed
        elif route == "s1_inf_minus_inf":
            assert fin.sum() > 300 and np.all(np.isnan(S1[fin])) and adm == 0
        elif route == "w_overflows_invw_zero":
            assert W == np.inf and invW == 0.0
            assert 0 < adm < J.size and np.all(t0[J < np.inf] == 0.0)
            assert np.any(np.isinf(S1)), "some cells overflow S1: t0 = INF * 0 = NaN there"
        elif route == "invw_overflows":
            assert 0 < W < DBL_TINY and invW == np.inf and adm == 0
        elif route == "subnormal_weights":
            assert np.all(np.asarray(we)[np.asarray(we) != 0] < DBL_TINY) and np.isfinite(invW)
            Ja = J[J < np.inf]
            assert adm > 300 and np.all(Ja < 1e-307) and (Ja < DBL_TINY).sum() > adm // 2
            assert len(np.unique(Ja)) > adm // 4
        elif route == "subnormal_residuals":
            zero = np.all(tt == 0, axis=0)
            assert zero.sum() > 100 and np.all(J[zero] == 0.0) and np.all(J[~zero] > 0.0)
            assert np.all(np.abs(picks[e]) < DBL_TINY)
    return rec


CONF_RANGE_CASES = ("thr_largest_finite", "thr_subnormal", "thr_one_ulp")


@functools.lru_cache(maxsize=None)
def conf_range_case(name):
    """(tt, picks, weights, m [E], delta [E, L]) of one float-range case of locate confidence."""
    if name == "thr_largest_finite":            # m + delta = DBL_MAX: bits + 1 are the bits of +INF
        tt, picks, _ = range_case("huge_finite_misfit")
        picks = picks[[0, 1, 0, 1]]
        J0, _ = misfit(tt, picks[0])
        top = float(J0[J0 < np.inf].max())
        m = np.array([DBL_MAX / 2, np.nextafter(DBL_MAX, 0.0), top, 0.0])
        ulp = 2.0 ** 971                         # of DBL_MAX: m + 0.75 ulp rounds up to it, m + ulp is it exactly
        delta = np.array([[DBL_MAX / 2, 0.0, DBL_MAX], [0.75 * ulp, 0.0, ulp],
                          [DBL_MAX - top, 0.0, np.inf], [DBL_MAX, np.nextafter(DBL_MAX, 0.0), 1e306]])
        return tt, picks, None, m, delta
    if name == "thr_subnormal":                 # J, m, delta and m + delta all subnormal
        tt, picks, w = range_case("subnormal_weights")
        E = len(picks)
        m = np.empty(E)
        delta = np.empty((E, 4))
        for e in range(E):
            J, _ = misfit(tt, picks[e], w[e])
            m[e] = J.min()
            delta[e] = (0.0, 5e-324, sparse_delta(J, m[e]), sparse_delta(J, m[e], share=3))
        return tt, picks, w, m, delta
    assert name == "thr_one_ulp"                # thr one ulp below, at and one ulp above the J of a cell
    rng = np.random.default_rng(41)
    tt = rng.uniform(0, 20, (4,) + RANGE_SHAPE).astype(F32)
    o = _near(tt, rng, 1, 1.0)[0]
    wt = rng.uniform(0.5, 2.0, 4)
    J, _ = misfit(tt, o, wt)
    Js = np.sort(J.reshape(-1))
    m = []
    for rank in (0, 1, 40, 200, 384):
        m += [np.nextafter(Js[rank], 0.0), Js[rank], np.nextafter(Js[rank], np.inf)]
    m = np.array(m)
    return tt, np.tile(o, (len(m), 1)), np.tile(wt, (len(m), 1)), m, np.zeros((len(m), 1))
