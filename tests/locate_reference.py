"""Independent numpy restatement of event location (include/ttsweep.h, "locate").

Vectorised over cells, stations in ascending k, one ufunc per operation (numpy has no fused multiply-add), so every
double is rounded as the library rounds it and the GPU must agree bit for bit."""
import numpy as np


def check(picks, weights=None):
    """The refusals of ttsweep_locate_device on picks / weights [E, K]: None when the call is accepted, else the
    reason."""
    o = np.asarray(picks, dtype=np.float64)
    w = np.ones_like(o) if weights is None else np.asarray(weights, dtype=np.float64)
    if not np.all(np.isfinite(o)):
        return "pick"
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        return "weight"
    if np.any(np.all(w == 0, axis=1)):
        return "no weight"
    return None


def misfit(tt, o, w=None):
    """(J, t0) of one event over every cell: tt [K, ...] float32, o / w [K] float64.  J is +inf where the cell is
    inadmissible."""
    tt = np.asarray(tt, dtype=np.float32)
    K = tt.shape[0]
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    o = np.asarray(o, dtype=np.float64)
    picked = [k for k in range(K) if w[k] != 0]
    W = np.float64(0.0)
    for k in picked:
        W = W + w[k]
    invW = np.float64(1.0) / W
    shape = tt.shape[1:]
    with np.errstate(all="ignore"):
        S1 = np.zeros(shape, np.float64)
        bad = np.zeros(shape, bool)
        for k in picked:
            T = tt[k].astype(np.float64)
            bad |= T >= np.inf
            d = np.subtract(o[k], T)
            S1 = np.add(S1, np.multiply(w[k], d))
        t0 = np.multiply(S1, invW)
        J = np.zeros(shape, np.float64)
        for k in picked:
            T = tt[k].astype(np.float64)
            r = np.subtract(np.subtract(o[k], T), t0)
            J = np.add(J, np.multiply(np.multiply(w[k], r), r))
    bad |= ~(J < np.inf)
    J = np.where(bad, np.inf, J)
    return J, t0


def locate(tt, picks, weights=None, volumes=()):
    """(cell [E] int32, misfit [E], t0 [E], {e: J volume}) of every event."""
    picks = np.asarray(picks, dtype=np.float64)
    E = picks.shape[0]
    cell = np.full(E, -1, np.int32)
    mis = np.full(E, np.inf)
    t0s = np.full(E, np.nan)
    vols = {}
    for e in range(E):
        J, t0 = misfit(tt, picks[e], None if weights is None else weights[e])
        Jf = J.reshape(-1)
        if e in volumes:
            vols[e] = J
        if np.any(Jf < np.inf):
            x = int(np.argmin(Jf))          # the first index of the minimum
            cell[e], mis[e], t0s[e] = x, Jf[x], t0.reshape(-1)[x]
    return cell, mis, t0s, vols


def locate_slow(tt, o, w=None):
    """(cell, J, t0) of one event by a per-cell pure-Python loop over the same formula (tiny boxes only)."""
    tt = np.asarray(tt, dtype=np.float32)
    K = tt.shape[0]
    w = [1.0] * K if w is None else [float(x) for x in w]
    o = [float(x) for x in o]
    flat = tt.reshape(K, -1)
    best = (-1, float("inf"), float("nan"))
    W = 0.0
    for k in range(K):
        if w[k] != 0:
            W += w[k]
    invW = 1.0 / W
    for x in range(flat.shape[1]):
        T = [float(flat[k, x]) for k in range(K)]
        if any(T[k] >= float("inf") for k in range(K) if w[k] != 0):
            continue
        s1 = 0.0
        for k in range(K):
            if w[k] != 0:
                s1 += w[k] * (o[k] - T[k])
        t0 = s1 * invW
        J = 0.0
        for k in range(K):
            if w[k] != 0:
                r = (o[k] - T[k]) - t0
                J += (w[k] * r) * r
        if not J < float("inf"):
            continue
        if J < best[1]:
            best = (x, J, t0)
    return best
