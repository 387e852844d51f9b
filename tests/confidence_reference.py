"""Independent numpy restatement of the confidence regions of located events (include/ttsweep.h, "locate
confidence").

J, t0 and admissibility come from locate_reference.misfit (the restatement of locate, unchanged); the region of level
l is the admissible cells with J <= m + delta[l] (one double addition).  Counts, coordinate sums and second moments
are integer numpy (int64: the library refuses grids on which they could overflow), the t0 extremes are taken through
a key whose unsigned order is IEEE totalOrder (-0 below +0)."""
import numpy as np

from locate_reference import misfit

SUM2 = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))        # xx, yy, zz, xy, xz, yz
FIELDS = ("count", "sum", "sum2", "lo", "hi", "t0_lo", "t0_hi")


def check(m, delta):
    """The refusals of ttsweep_locate_confidence_device on m [E] / delta [E, L]: None when accepted."""
    m, delta = np.asarray(m, np.float64), np.asarray(delta, np.float64)
    if np.any(np.isnan(m)) or np.any(m < 0):
        return "misfit"
    if np.any(np.isnan(delta)) or np.any(delta < 0):
        return "delta"
    return None


def moments_fit(shape):
    """ncells * max(nx, ny, nz)^2 < 2^63 (Python ints): the second moments cannot overflow int64."""
    nx, ny, nz = (int(n) for n in shape)
    return nx * ny * nz * max(nx, ny, nz) ** 2 < 2 ** 63


def t0_key(t):
    """uint64 keys of doubles whose unsigned order is totalOrder."""
    u = np.ascontiguousarray(np.asarray(t, np.float64)).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def empty(shape, E, L):
    nx, ny, nz = shape
    return {"count": np.zeros((E, L), np.int64), "sum": np.zeros((E, L, 3), np.int64),
            "sum2": np.zeros((E, L, 6), np.int64), "lo": np.tile(np.array([nx, ny, nz], np.int32), (E, L, 1)),
            "hi": np.full((E, L, 3), -1, np.int32), "t0_lo": np.full((E, L), np.inf), "t0_hi": np.full((E, L), -np.inf)}


def region(J, t0, m, d):
    """The summary of one (event, level) from the volumes J, t0 [nx, ny, nz]: None for the empty region."""
    if m == np.inf:
        return None
    thr = np.float64(m) + np.float64(d)
    R = (J < np.inf) & (J <= thr)
    if not R.any():
        return None
    c = [a.astype(np.int64) for a in np.nonzero(R)]
    tr = t0[R]
    k = t0_key(tr)
    return {"count": int(R.sum()), "sum": [int(a.sum()) for a in c],
            "sum2": [int((c[a] * c[b]).sum()) for a, b in SUM2], "lo": [int(a.min()) for a in c],
            "hi": [int(a.max()) for a in c], "t0_lo": tr[int(np.argmin(k))], "t0_hi": tr[int(np.argmax(k))]}


def confidence(tt, picks, weights, m, delta):
    """Every output of ttsweep_locate_confidence_device as a dict of numpy arrays; tt [K, nx, ny, nz] float32,
    picks / weights [E, K] (weights None: all 1.0), m [E], delta [E, L]."""
    tt = np.asarray(tt, np.float32)
    picks = np.asarray(picks, np.float64)
    E = picks.shape[0]
    m = np.asarray(m, np.float64)
    delta = np.asarray(delta, np.float64).reshape(E, -1)
    L = delta.shape[1]
    out = empty(tt.shape[1:], E, L)
    for e in range(E):
        J, t0 = misfit(tt, picks[e], None if weights is None else weights[e])
        for l in range(L):
            r = region(J, t0, m[e], delta[e, l])
            if r:
                for f, v in r.items():
                    out[f][e, l] = v
    return out


def confidence_slow(tt, o, w, m, deltas):
    """One event by a per-cell pure-Python loop over locate's formula, Python ints and struct-packed keys (tiny boxes
    only): a list of per-level dicts in the layout of region(), None for an empty region."""
    import struct
    tt = np.asarray(tt, np.float32)
    K, nx, ny, nz = tt.shape
    w = [1.0] * K if w is None else [float(x) for x in w]
    o = [float(x) for x in o]
    inf = float("inf")

    def key(t):
        u = struct.unpack("<Q", struct.pack("<d", t))[0]
        return (~u) & (2 ** 64 - 1) if u >> 63 else u | 1 << 63

    W = 0.0
    for k in range(K):
        if w[k] != 0:
            W += w[k]
    invW = 1.0 / W
    res = [None] * len(deltas)
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                T = [float(tt[k, x, y, z]) for k in range(K)]
                if any(T[k] >= inf for k in range(K) if w[k] != 0):
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
                if not J < inf or m == inf:
                    continue
                for l, d in enumerate(deltas):
                    if not J <= float(m) + float(d):
                        continue
                    c = (x, y, z)
                    if res[l] is None:
                        res[l] = {"count": 0, "sum": [0] * 3, "sum2": [0] * 6, "lo": list(c), "hi": list(c),
                                  "t0_lo": t0, "t0_hi": t0}
                    r_ = res[l]
                    r_["count"] += 1
                    for a in range(3):
                        r_["sum"][a] += c[a]
                        r_["lo"][a] = min(r_["lo"][a], c[a])
                        r_["hi"][a] = max(r_["hi"][a], c[a])
                    for q, (a, b) in enumerate(SUM2):
                        r_["sum2"][q] += c[a] * c[b]
                    if key(t0) < key(r_["t0_lo"]):
                        r_["t0_lo"] = t0
                    if key(t0) > key(r_["t0_hi"]):
                        r_["t0_hi"] = t0
    return res
