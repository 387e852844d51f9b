"""Plain numpy restatement of the three Fresnel-volume calls (include/ttsweep.h, "fresnel"), written from the
definitions there: phi per (pair, cell) in float64 with every operation rounded on its own, and int64 fixed-point
sums.  Two forms: the vectorised one the GPU tests compare against, and a per-cell loop in Python floats and
Python integers (`*_loop`) that checks the vectorised one.

The vectorised form evaluates each distinct (a, b, tau, window) once and, in the adjoint, each distinct weight of
such a group once, multiplied by the number of its occurrences: the sums are integer sums, so n equal terms are n
times the term, whatever the order."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
OK, UNREACHED = 0, 2


def ceil_log2(n):
    k = 0
    while (1 << k) < n:
        k += 1
    return k


def max_exponent(a):
    """The largest frexp exponent of the nonzero entries of a, None when there is none."""
    a = np.asarray(a, dtype=F64).reshape(-1)
    a = a[a != 0]
    return int(np.frexp(a)[1].max()) if a.size else None


def flat_index(shape, p):
    return (int(p[0]) * shape[1] + int(p[1])) * shape[2] + int(p[2])


def pair_times(boxes, starts, pair_a, pair_b):
    """(t_ab float32 [npair], status int32 [npair])"""
    shape = boxes.shape[1:]
    flat = np.array([flat_index(shape, s) for s in starts], dtype=np.int64)
    t = boxes.reshape(len(boxes), -1)[np.asarray(pair_a, dtype=np.int64), flat[np.asarray(pair_b, dtype=np.int64)]]
    t = t.astype(F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        status = np.where(t < np.inf, OK, UNREACHED).astype(np.int32)
    return t, status


def windows_of(shape, npair, lo, hi):
    """lo, hi as int64 [npair, 3]; None: the whole grid"""
    if lo is None:
        assert hi is None
        return np.zeros((npair, 3), np.int64), np.tile(np.asarray(shape, np.int64) - 1, (npair, 1))
    return (np.broadcast_to(np.asarray(lo, np.int64), (npair, 3)).copy(),
            np.broadcast_to(np.asarray(hi, np.int64), (npair, 3)).copy())


def phi_window(Ta, Tb, t_ab, tau, lo, hi):
    """phi of the cells of the window [lo, hi] of one pair, float64, the window's shape"""
    w = tuple(slice(int(l), int(h) + 1) for l, h in zip(lo, hi))
    A, B = Ta[w].astype(F64), Tb[w].astype(F64)
    with np.errstate(all="ignore"):
        ok = (A < np.inf) & (B < np.inf)
        delta = (A + B) - F64(t_ab)
        phi = F64(1.0) - delta / F64(tau)
        phi = np.where(phi > 1.0, 1.0, phi)
        phi = np.where(phi > 0.0, phi, 0.0)
    return np.where(ok, phi, 0.0)


def _groups(pair_a, pair_b, tau, lo, hi):
    """The distinct (a, b, tau, window): (first pair of each group, the group of every pair)"""
    key = np.concatenate([np.asarray(pair_a, np.int64)[:, None], np.asarray(pair_b, np.int64)[:, None],
                          np.ascontiguousarray(tau, F64).view(np.int64)[:, None], lo, hi], axis=1)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return first, inverse.reshape(-1)


def _fixed(x, S):
    """llrint(ldexp(x, S)) as int64"""
    return np.rint(np.ldexp(x, S)).astype(np.int64)


def volume(boxes, starts, pair_a, pair_b, tau, lo=None, hi=None):
    """dict of status, t_ab, count (int64), lo, hi (int32 [npair, 3]), phi (float64)"""
    shape = boxes.shape[1:]
    npair = len(pair_a)
    tau = np.broadcast_to(np.asarray(tau, F64), (npair,))
    t_ab, status = pair_times(boxes, starts, pair_a, pair_b)
    lo, hi = windows_of(shape, npair, lo, hi)
    S = 60 - ceil_log2(int(np.prod(shape)))
    out = dict(status=status, t_ab=t_ab, count=np.zeros(npair, np.int64), phi=np.zeros(npair, F64),
               lo=np.tile(np.asarray(shape, np.int32), (npair, 1)), hi=np.full((npair, 3), -1, np.int32))
    if npair == 0:
        return out
    first, group = _groups(pair_a, pair_b, tau, lo, hi)
    for g, r in enumerate(first):
        if status[r] != OK:
            continue
        phi = phi_window(boxes[pair_a[r]], boxes[pair_b[r]], t_ab[r], tau[r], lo[r], hi[r])
        at = np.argwhere(phi > 0)
        if not len(at):
            continue
        members = group == g
        out["count"][members] = len(at)
        out["phi"][members] = np.ldexp(F64(int(_fixed(phi, S).sum())), -S)
        out["lo"][members] = (at.min(axis=0) + lo[r]).astype(np.int32)
        out["hi"][members] = (at.max(axis=0) + lo[r]).astype(np.int32)
    return out


def forward(boxes, starts, pair_a, pair_b, tau, m, lo=None, hi=None):
    """(y float64 [npair], S_m)"""
    shape = boxes.shape[1:]
    npair = len(pair_a)
    tau = np.broadcast_to(np.asarray(tau, F64), (npair,))
    m = np.asarray(m, F64).reshape(shape)
    y = np.zeros(npair, F64)
    E = max_exponent(m)
    if E is None:
        return y, 0
    S = 61 - E - ceil_log2(int(np.prod(shape)))
    if npair == 0:
        return y, S
    t_ab, status = pair_times(boxes, starts, pair_a, pair_b)
    lo, hi = windows_of(shape, npair, lo, hi)
    first, group = _groups(pair_a, pair_b, tau, lo, hi)
    for g, r in enumerate(first):
        if status[r] != OK:
            continue
        phi = phi_window(boxes[pair_a[r]], boxes[pair_b[r]], t_ab[r], tau[r], lo[r], hi[r])
        mw = m[tuple(slice(int(l), int(h) + 1) for l, h in zip(lo[r], hi[r]))]
        terms = _fixed((phi * mw)[phi > 0], S)
        y[group == g] = np.ldexp(F64(int(terms.sum())), -S)
    return y, S


def adjoint(boxes, starts, pair_a, pair_b, tau, w, lo=None, hi=None):
    """(g float64 grid or None when w is None, hits int32 grid, S_w)"""
    shape = boxes.shape[1:]
    npair = len(pair_a)
    tau = np.broadcast_to(np.asarray(tau, F64), (npair,))
    hits = np.zeros(shape, np.int64)
    acc = np.zeros(shape, np.int64)
    E = None if w is None else max_exponent(w)
    S = 0 if E is None else 61 - E - ceil_log2(npair)
    if npair:
        t_ab, status = pair_times(boxes, starts, pair_a, pair_b)
        lo, hi = windows_of(shape, npair, lo, hi)
        first, group = _groups(pair_a, pair_b, tau, lo, hi)
        for g, r in enumerate(first):
            if status[r] != OK:
                continue
            phi = phi_window(boxes[pair_a[r]], boxes[pair_b[r]], t_ab[r], tau[r], lo[r], hi[r])
            win = tuple(slice(int(l), int(h) + 1) for l, h in zip(lo[r], hi[r]))
            members = np.nonzero(group == g)[0]
            hits[win] += len(members) * (phi > 0)
            if E is None:
                continue
            wv, n = np.unique(np.asarray(w, F64)[members].view(np.int64), return_counts=True)
            for bits, k in zip(wv, n):
                acc[win] += int(k) * np.where(phi > 0, _fixed(np.int64(bits).view(F64) * phi, S), 0)
    gout = None if w is None else np.ldexp(acc.astype(F64), -S)
    return gout, hits.astype(np.int32), S


# ---- the per-cell loop: Python floats (IEEE doubles) and Python integers ----

def _phi_cell(A, B, t_ab, tau):
    if not A < math.inf or not B < math.inf:
        return 0.0
    delta = (A + B) - t_ab
    phi = 1.0 - delta / tau
    if phi > 1.0:
        phi = 1.0
    if not phi > 0.0:
        return 0.0
    return phi


def _visits(boxes, starts, pair_a, pair_b, tau, lo, hi):
    """yields (pair, None) for every pair and then (pair, (x, y, z), phi) for each of its cells with phi > 0, the
    pairs in order"""
    shape = boxes.shape[1:]
    npair = len(pair_a)
    tau = np.broadcast_to(np.asarray(tau, F64), (npair,))
    lo, hi = windows_of(shape, npair, lo, hi)
    for r in range(npair):
        Ta, Tb = boxes[pair_a[r]], boxes[pair_b[r]]
        t_ab = float(Ta[tuple(int(c) for c in starts[pair_b[r]])])
        yield r, None, t_ab
        if not t_ab < math.inf:
            continue
        for x in range(lo[r][0], hi[r][0] + 1):
            for y in range(lo[r][1], hi[r][1] + 1):
                for z in range(lo[r][2], hi[r][2] + 1):
                    phi = _phi_cell(float(Ta[x, y, z]), float(Tb[x, y, z]), t_ab, float(tau[r]))
                    if phi > 0.0:
                        yield r, (x, y, z), phi


def volume_loop(boxes, starts, pair_a, pair_b, tau, lo=None, hi=None):
    shape = boxes.shape[1:]
    npair = len(pair_a)
    S = 60 - ceil_log2(int(np.prod(shape)))
    status = np.zeros(npair, np.int32)
    t = np.zeros(npair, F32)
    count = [0] * npair
    total = [0] * npair
    blo = np.tile(np.asarray(shape, np.int32), (npair, 1))
    bhi = np.full((npair, 3), -1, np.int32)
    for r, cell, val in _visits(boxes, starts, pair_a, pair_b, tau, lo, hi):
        if cell is None:
            t[r] = F32(val)
            status[r] = OK if val < math.inf else UNREACHED
            continue
        count[r] += 1
        total[r] += round(math.ldexp(val, S))
        blo[r] = np.minimum(blo[r], cell)
        bhi[r] = np.maximum(bhi[r], cell)
    phi = np.array([math.ldexp(float(s), -S) for s in total], F64).reshape(npair)
    return dict(status=status, t_ab=t, count=np.array(count, np.int64).reshape(npair), phi=phi, lo=blo, hi=bhi)


def forward_loop(boxes, starts, pair_a, pair_b, tau, m, lo=None, hi=None):
    shape = boxes.shape[1:]
    npair = len(pair_a)
    m = np.asarray(m, F64).reshape(shape)
    E = max_exponent(m)
    if E is None:
        return np.zeros(npair, F64), 0
    S = 61 - E - ceil_log2(int(np.prod(shape)))
    total = [0] * npair
    for r, cell, val in _visits(boxes, starts, pair_a, pair_b, tau, lo, hi):
        if cell is not None:
            total[r] += round(math.ldexp(val * float(m[cell]), S))
    return np.array([math.ldexp(float(s), -S) for s in total], F64).reshape(npair), S


def adjoint_loop(boxes, starts, pair_a, pair_b, tau, w, lo=None, hi=None):
    shape = boxes.shape[1:]
    npair = len(pair_a)
    E = None if w is None else max_exponent(w)
    S = 0 if E is None else 61 - E - ceil_log2(npair)
    acc = np.zeros(shape, dtype=object)
    acc[...] = 0
    hits = np.zeros(shape, np.int32)
    for r, cell, val in _visits(boxes, starts, pair_a, pair_b, tau, lo, hi):
        if cell is None:
            continue
        hits[cell] += 1
        if E is not None:
            acc[cell] += round(math.ldexp(float(w[r]) * val, S))
    g = None
    if w is not None:
        g = np.array([math.ldexp(float(a), -S) for a in acc.reshape(-1)], F64).reshape(shape)
    return g, hits, S
