"""Independent numpy restatement of sub-cell event location (include/ttsweep.h, "locate subcell") and of the driver
TravelTimeSolver.locate_fine.

Vectorised over the nodes of a window, one ufunc per operation (numpy has no fused multiply-add), so every double is
rounded as the library rounds it and the GPU must agree bit for bit.  The misfit is restated here on the interpolated
double times; locate_reference is used by the tests for comparison only.  subcell_slow is a per-node pure-Python loop
over the same formulas for tiny cases."""
import numpy as np


def axis(lo, hi, sub):
    """(q, i, j, u) of the nodes lo * sub .. hi * sub of one axis"""
    q = np.arange(int(lo) * sub, int(hi) * sub + 1, dtype=np.int64)
    i = q // sub
    f = q % sub
    j = i + (f != 0)
    u = np.divide(f.astype(np.float64), np.float64(sub))
    return q, i, j, u


def lerp(a, b, u):
    return np.add(a, np.multiply(u, np.subtract(b, a)))


def interpolate(tt, lo, hi, sub):
    """That [K, Nx', Ny', Nz'] float64 on the nodes of the window, and the node coordinates per axis"""
    tt = np.asarray(tt, dtype=np.float32)
    K = tt.shape[0]
    (qx, ix, jx, ux), (qy, iy, jy, uy), (qz, iz, jz, uz) = (axis(lo[a], hi[a], sub) for a in range(3))
    for a, j in enumerate((jx, jy, jz)):
        assert j.max() <= hi[a], "the upper corner never leaves the window"
    ks = np.arange(K)

    def T(x, y, z):
        return tt[np.ix_(ks, x, y, z)].astype(np.float64)

    ux, uy, uz = ux[None, :, None, None], uy[None, None, :, None], uz[None, None, None, :]
    with np.errstate(all="ignore"):
        c00 = lerp(T(ix, iy, iz), T(ix, iy, jz), uz)
        c01 = lerp(T(ix, jy, iz), T(ix, jy, jz), uz)
        c10 = lerp(T(jx, iy, iz), T(jx, iy, jz), uz)
        c11 = lerp(T(jx, jy, iz), T(jx, jy, jz), uz)
        c0 = lerp(c00, c01, uy)
        c1 = lerp(c10, c11, uy)
        return lerp(c0, c1, ux), (qx, qy, qz)


def misfit(That, o, w=None):
    """(J, t0) of one event on interpolated times That [K, ...] float64: the formulas of "locate", stations ascending,
    zero weights skipped.  J is +inf where the node is inadmissible (J not below +inf)."""
    K = That.shape[0]
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    o = np.asarray(o, dtype=np.float64)
    picked = [k for k in range(K) if w[k] != 0]
    W = np.float64(0.0)
    for k in picked:
        W = W + w[k]
    with np.errstate(all="ignore"):
        invW = np.float64(1.0) / W
        S1 = np.zeros(That.shape[1:], np.float64)
        for k in picked:
            S1 = np.add(S1, np.multiply(w[k], np.subtract(o[k], That[k])))
        t0 = np.multiply(S1, invW)
        J = np.zeros(That.shape[1:], np.float64)
        for k in picked:
            r = np.subtract(np.subtract(o[k], That[k]), t0)
            J = np.add(J, np.multiply(np.multiply(w[k], r), r))
    return np.where(J < np.inf, J, np.inf), t0


def windows(shape, E, lo=None, hi=None):
    n = np.asarray(shape, np.int64)
    lo = np.zeros(3, np.int64) if lo is None else np.asarray(lo, np.int64)
    hi = n - 1 if hi is None else np.asarray(hi, np.int64)
    return np.broadcast_to(lo, (E, 3)), np.broadcast_to(hi, (E, 3))


def locate_subcell(tt, picks, weights=None, lo=None, hi=None, sub=8):
    """(node [E, 3] int32, misfit [E], t0 [E]) of every event over the nodes of its window"""
    tt = np.asarray(tt, dtype=np.float32)
    picks = np.asarray(picks, dtype=np.float64)
    E = picks.shape[0]
    lo, hi = windows(tt.shape[1:], E, lo, hi)
    node = np.full((E, 3), -1, np.int32)
    mis = np.full(E, np.inf)
    t0s = np.full(E, np.nan)
    last = None
    for e in range(E):
        if last != (tuple(lo[e]), tuple(hi[e])):        # the interpolation of a window shared with the previous event is kept
            last = (tuple(lo[e]), tuple(hi[e]))
            That, q = interpolate(tt, lo[e], hi[e], sub)
        J, t0 = misfit(That, picks[e], None if weights is None else weights[e])
        if np.any(J < np.inf):
            i = int(np.argmin(J))           # the first of the minimum in C order: the smallest (qx, qy, qz)
            a, b, c = np.unravel_index(i, J.shape)
            node[e] = (q[0][a], q[1][b], q[2][c])
            mis[e], t0s[e] = J.reshape(-1)[i], t0.reshape(-1)[i]
    return node, mis, t0s


def fine_windows(shape, cells, radius=1):
    """(lo, hi) [E, 3] of locate_fine: cell +- radius clipped to the grid; the cell (0, 0, 0) alone for cell -1"""
    n = np.asarray(shape, np.int64)
    radius = np.broadcast_to(np.asarray(radius, np.int64), (3,))
    cells = np.asarray(cells, np.int64)
    lo, hi = np.zeros((len(cells), 3), np.int64), np.zeros((len(cells), 3), np.int64)
    for e in np.flatnonzero(cells >= 0):
        xyz = np.array(np.unravel_index(int(cells[e]), shape), np.int64)
        lo[e], hi[e] = np.maximum(xyz - radius, 0), np.minimum(xyz + radius, n - 1)
    return lo, hi


def subcell_slow(tt, o, w, lo, hi, sub):
    """(node, J, t0) of one event by a per-node pure-Python loop over the same formulas (tiny boxes only)"""
    tt = np.asarray(tt, dtype=np.float32)
    K = tt.shape[0]
    w = [1.0] * K if w is None else [float(x) for x in w]
    o = [float(x) for x in o]
    inf = float("inf")
    W = 0.0
    for k in range(K):
        if w[k] != 0:
            W += w[k]
    invW = 1.0 / W
    best = ((-1, -1, -1), inf, float("nan"))

    def parts(q):
        i, f = q // sub, q % sub
        return i, i + (1 if f else 0), float(f) / float(sub)

    def lp(a, b, u):
        return a + u * (b - a)

    for qx in range(lo[0] * sub, hi[0] * sub + 1):
        ix, jx, ux = parts(qx)
        for qy in range(lo[1] * sub, hi[1] * sub + 1):
            iy, jy, uy = parts(qy)
            for qz in range(lo[2] * sub, hi[2] * sub + 1):
                iz, jz, uz = parts(qz)
                That = []
                for k in range(K):
                    T = lambda x, y, z: float(tt[k, x, y, z])
                    c00 = lp(T(ix, iy, iz), T(ix, iy, jz), uz)
                    c01 = lp(T(ix, jy, iz), T(ix, jy, jz), uz)
                    c10 = lp(T(jx, iy, iz), T(jx, iy, jz), uz)
                    c11 = lp(T(jx, jy, iz), T(jx, jy, jz), uz)
                    That.append(lp(lp(c00, c01, uy), lp(c10, c11, uy), ux))
                s1 = 0.0
                for k in range(K):
                    if w[k] != 0:
                        s1 += w[k] * (o[k] - That[k])
                t0 = s1 * invW
                J = 0.0
                for k in range(K):
                    if w[k] != 0:
                        r = (o[k] - That[k]) - t0
                        J += (w[k] * r) * r
                if J < inf and J < best[1]:
                    best = ((qx, qy, qz), J, t0)
    return best


# ---- a case both tiers use ----
def planted_case():
    """six boxes linear in the coordinates, stored as float32; the picks of the one event are the linear field itself
    (in double) at a node with f != 0 on every axis, sub = 8, plus an origin time; the window is the +-1 window of the
    node's nearest cell.  Returns tt, picks, the node, lo, hi."""
    g = np.stack(np.meshgrid(np.arange(9.0), np.arange(8.0), np.arange(7.0), indexing="ij"))
    rng = np.random.default_rng(6)
    coef = rng.uniform(-1, 1, (6, 3))
    coef[:3] += 2 * np.eye(3)
    const = rng.uniform(10, 20, 6)
    tt = (np.tensordot(coef, g, 1) + const[:, None, None, None]).astype(np.float32)
    node = np.array([4 * 8 + 3, 3 * 8 + 5, 2 * 8 + 6])
    picks = (coef @ (node / 8.0) + const + 1.25)[None]
    return tt, picks, node, np.array([[3, 3, 2]]), np.array([[5, 5, 4]])
