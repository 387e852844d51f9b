"""Independent numpy restatement of windowed, strided event location (include/ttsweep.h, "locate window") and of
the two-stage driver TravelTimeSolver.locate_refine.

The candidate index set is built from lo, hi and stride; locate_reference.misfit (imported, not copied) is evaluated
on those cells only, and the lexicographic minimum of (J, index) is taken."""
import numpy as np

import locate_reference as L


def candidates(shape, lo, hi, stride=(1, 1, 1)):
    """The FLOATBOX indices of C = { lo + i * stride <= hi, per axis }, ascending."""
    ax = [np.arange(int(lo[a]), int(hi[a]) + 1, int(stride[a]), dtype=np.int64) for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    return ((x * shape[1] + y) * shape[2] + z).reshape(-1)


def windows(shape, E, lo=None, hi=None, stride=1):
    """(lo [E,3], hi [E,3], stride [3]) as int64, with the broadcasts of TravelTimeSolver.locate_window."""
    n = np.asarray(shape, np.int64)
    lo = np.zeros(3, np.int64) if lo is None else np.asarray(lo, np.int64)
    hi = n - 1 if hi is None else np.asarray(hi, np.int64)
    return (np.broadcast_to(lo, (E, 3)), np.broadcast_to(hi, (E, 3)), np.broadcast_to(np.asarray(stride, np.int64), (3,)))


def locate_window(tt, picks, weights=None, lo=None, hi=None, stride=1):
    """(cell [E] int32, misfit [E], t0 [E]) of every event over its candidates."""
    tt = np.asarray(tt, dtype=np.float32)
    K, shape = tt.shape[0], tt.shape[1:]
    flat = tt.reshape(K, -1)
    picks = np.asarray(picks, dtype=np.float64)
    E = picks.shape[0]
    lo, hi, stride = windows(shape, E, lo, hi, stride)
    cell = np.full(E, -1, np.int32)
    mis = np.full(E, np.inf)
    t0s = np.full(E, np.nan)
    last = None
    for e in range(E):
        if last != (tuple(lo[e]), tuple(hi[e])):        # the gather of a window shared with the previous event is kept
            last = (tuple(lo[e]), tuple(hi[e]))
            idx = candidates(shape, lo[e], hi[e], stride)
            T = flat[:, idx]
        with np.errstate(all="ignore"):
            J, t0 = L.misfit(T, picks[e], None if weights is None else weights[e])
        if np.any(J < np.inf):
            i = int(np.argmin(J))           # the first of the minimum: idx ascends, so the smallest index
            cell[e], mis[e], t0s[e] = idx[i], J[i], t0[i]
    return cell, mis, t0s


def refine(tt, picks, weights=None, stride=4, radius=None):
    """The two stages of locate_refine: (cell, misfit, t0, coarse_cell, coarse_misfit)."""
    tt = np.asarray(tt, dtype=np.float32)
    shape = tt.shape[1:]
    n = np.asarray(shape, np.int64)
    stride = np.broadcast_to(np.asarray(stride, np.int64), (3,))
    radius = stride if radius is None else np.broadcast_to(np.asarray(radius, np.int64), (3,))
    cc, cm, _ = locate_window(tt, picks, weights, stride=stride)
    E = len(cc)
    lo, hi = np.zeros((E, 3), np.int64), np.tile(n - 1, (E, 1))
    for e in np.flatnonzero(cc >= 0):
        xyz = np.array(np.unravel_index(int(cc[e]), shape), np.int64)
        lo[e], hi[e] = np.maximum(xyz - radius, 0), np.minimum(xyz + radius, n - 1)
    cell, mis, t0 = locate_window(tt, picks, weights, lo, hi, 1)
    return cell, mis, t0, cc, cm
