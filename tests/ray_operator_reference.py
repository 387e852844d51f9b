"""Independent numpy restatement of the ray Frechet operators (include/ttsweep.h, "rays: the Frechet operators"):
y = G m, g = G^T w in the library's int64 fixed point, and hit counts.

Written from the header's rules on top of ray_reference.trace (the same rays, in the library's path format), so
that the GPU results can be compared bit for bit: every step is IEEE double arithmetic or integer arithmetic."""
import numpy as np

import ray_reference as R


def entries_dmax(fs, shape, starstart=0, starstop=None):
    """The largest d among the star's ray entries (offsets that fit the grid; 0 when there is none)."""
    if starstop is None:
        starstop = len(fs) - 1
    dmax = np.float32(0)
    for di, dj, dk, d, _ in R.pull_entries(fs, starstart, starstop):
        if abs(di) < shape[0] and abs(dj) < shape[1] and abs(dk) < shape[2]:
            dmax = max(dmax, np.float32(d))
    return dmax


def scale(w, dmax, nrays):
    """S = 61 - E_w - E_d - K (0 when every weight is zero)."""
    w = np.asarray(w, dtype=np.float64)
    nz = w[w != 0]
    if nz.size == 0:
        return 0
    e_w = int(np.frexp(nz)[1].max())
    e_d = int(np.frexp(np.float64(dmax))[1])
    k = 0
    while (1 << k) < nrays:
        k += 1
    return 61 - e_w - e_d - k


def forward(offsets, cells, hop_d, m):
    """y [nrays]: per ray, from y = 0.0 in walk order (receiver -> source), y = y + (0.5 * d) * (m[c] + m[p])
    for every hop p -> c.  Rays without cells (UNREACHED, INVALID) give 0."""
    offsets = np.asarray(offsets, dtype=np.int64)
    cells = np.asarray(cells, dtype=np.int64)
    hop_d = np.asarray(hop_d, dtype=np.float32)
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    counts = offsets[1:] - offsets[:-1]
    y = np.zeros(len(counts), dtype=np.float64)
    for h in range(int(counts.max()) - 1 if len(counts) and counts.max() > 0 else 0):
        r = np.nonzero(counts > h + 1)[0]
        g = offsets[r + 1] - 2 - h                      # the hop cells[g] -> cells[g + 1], h hops from the receiver
        c, p = cells[g + 1], cells[g]
        y[r] = y[r] + (0.5 * hop_d[g].astype(np.float64)) * (m[c] + m[p])
    return y


def _terms(offsets, hop_d, w, S):
    """The fixed-point term of every path cell: llrint(ldexp(w_r * (0.5 * (d_in + d_out)), S))."""
    offsets = np.asarray(offsets, dtype=np.int64)
    hop_d = np.asarray(hop_d, dtype=np.float32).astype(np.float64)
    counts = offsets[1:] - offsets[:-1]
    ray = np.repeat(np.arange(len(counts)), counts)
    first = np.zeros(len(hop_d), dtype=bool)
    first[offsets[:-1][counts > 0]] = True
    d_out = hop_d                                       # 0 at a ray's last cell (the receiver)
    d_in = np.where(first, 0.0, np.concatenate([[0.0], hop_d[:-1]]))
    x = np.asarray(w, dtype=np.float64)[ray] * (0.5 * (d_in + d_out))
    return np.rint(np.ldexp(x, S)).astype(np.int64)


def adjoint(offsets, cells, hop_d, w, ncells, dmax):
    """(g [ncells] float64, S): G^T w summed in int64 fixed point, then g = ldexp((double)acc, -S)."""
    nrays = len(offsets) - 1
    S = scale(w, dmax, nrays)
    acc = np.zeros(ncells, dtype=np.int64)
    if np.any(np.asarray(w) != 0):
        np.add.at(acc, np.asarray(cells, dtype=np.int64), _terms(offsets, hop_d, w, S))
    return np.ldexp(acc.astype(np.float64), -S), S


def hits(cells, ncells):
    """int32 [ncells]: the number of rays (with cells: OK or SEED) whose path holds each cell."""
    return np.bincount(np.asarray(cells, dtype=np.int64), minlength=ncells).astype(np.int32)


def rays_of_boxes(v, tts, fs, starts, receivers, lo=0, hi=None, preds=None):
    """ray_reference.trace of every box, concatenated in ray order r = s * nrecv + q:
    (offsets, cells, hop_d, status, t_recv)."""
    parts = []
    for s, st in enumerate(starts):
        pred = R.predecessors(v, tts[s], fs, st, lo, hi) if preds is None else preds[s]
        parts.append(R.trace(v, tts[s], pred, fs, st, receivers, lo, hi))
    offsets = [np.zeros(1, np.int64)]
    base = 0
    for o, *_ in parts:
        offsets.append(o[1:] + base)
        base += o[-1]
    return (np.concatenate(offsets), np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]),
            np.concatenate([p[4] for p in parts]))
