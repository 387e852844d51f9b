"""Independent numpy restatement of the ray calls (include/ttsweep.h, "rays"): predecessors, trace and replay.

Written from the semantics, not from the library: the reference's own delay rule (float32 product, halved in
float64, rounded back to float32: serial_new/sweep-tt-multistart.c:216), its liveness rule (no edge centred on the
start, :219-221; the exclusive star bound), the FLOATBOX layout x*ny*nz + y*nz + z.  Every star entry l gives two
pull entries: +f_l (the edge centred on the cell: dead at the start) and -f_l (centred on the neighbour: dead when
the neighbour is the start).  Offsets that do not fit the grid are skipped."""
import numpy as np

F32 = np.float32
PRED_SOURCE, PRED_SEED, PRED_UNREACHED = -1, -2, -3
RAY_OK, RAY_SEED, RAY_UNREACHED, RAY_INVALID = 0, 1, 2, 3
FWD, REV = 1, 2


def delay(d, vsum):
    """fl32((double) fl32(d * vsum) / 2.0), elementwise."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = (F32(d) * np.asarray(vsum, dtype=F32)).astype(F32)
        return (p.astype(np.float64) / 2.0).astype(F32)


def pull_entries(fs, starstart, starstop):
    """[(di, dj, dk, d, kind)] of the live star entries fs[starstart:starstop], zero offsets dropped."""
    out = []
    for l in range(starstart, starstop):
        e = (int(fs["i"][l]), int(fs["j"][l]), int(fs["k"][l]))
        if e == (0, 0, 0):
            continue
        d = F32(fs["d"][l])
        out.append((e[0], e[1], e[2], d, FWD))
        out.append((-e[0], -e[1], -e[2], d, REV))
    return out


def _slices(n, e):
    """(cell slice, neighbour slice) along one axis for offset e, or None when nothing fits."""
    if abs(e) >= n:
        return None
    return (slice(max(0, -e), min(n, n - e)), slice(max(0, e), min(n, n + e)))


def flat_index(shape, p):
    return (int(p[0]) * shape[1] + int(p[1])) * shape[2] + int(p[2])


def predecessors(v, tt, fs, start, starstart=0, starstop=None):
    """pred box (int32, shape of tt) of one box."""
    if starstop is None:
        starstop = len(fs) - 1
    v = np.asarray(v, dtype=F32)
    T = np.asarray(tt, dtype=F32)
    shape = T.shape
    S = flat_index(shape, start)
    idx = np.arange(T.size, dtype=np.int64).reshape(shape)
    big = np.iinfo(np.int64).max
    best = np.full(shape, big, dtype=np.int64)
    for di, dj, dk, d, kind in pull_entries(fs, starstart, starstop):
        sl = [_slices(n, e) for n, e in zip(shape, (di, dj, dk))]
        if any(s is None for s in sl):
            continue
        cs = tuple(s[0] for s in sl)
        os_ = tuple(s[1] for s in sl)
        tc, to = T[cs], T[os_]
        with np.errstate(over="ignore", invalid="ignore"):
            cand = (delay(d, v[cs] + v[os_]) + to).astype(F32)
            match = (to < tc) & (cand == tc)
        live = (idx[cs] != S) if kind == FWD else (idx[os_] != S)
        match &= live
        oi = idx[os_]
        view = best[cs]
        best[cs] = np.where(match & (oi < view), oi, view)
    with np.errstate(invalid="ignore"):
        unreached = ~(T < np.inf)
    pred = np.where(best == big, PRED_SEED, best)
    pred = np.where(unreached, PRED_UNREACHED, pred)
    pred.reshape(-1)[S] = PRED_SOURCE
    return pred.astype(np.int32)


def _offset_table(fs, starstart, starstop):
    """offset -> [(d, kind)] sorted by d."""
    table = {}
    for di, dj, dk, d, kind in pull_entries(fs, starstart, starstop):
        table.setdefault((di, dj, dk), []).append((d, kind))
    for k in table:
        table[k].sort(key=lambda x: float(x[0]))
    return table


def trace(v, tt, pred, fs, start, receivers, starstart=0, starstop=None):
    """Rays of one box to receivers [(i, j, k)]: (offsets int64, cells int32, hop_d float32, status int32,
    t_recv float32) in the library's format (hop_d aligned with cells, 0 at a ray's last cell)."""
    if starstop is None:
        starstop = len(fs) - 1
    v = np.asarray(v, dtype=F32).reshape(-1)
    shape = tt.shape
    T = np.asarray(tt, dtype=F32).reshape(-1)
    P = np.asarray(pred).reshape(-1)
    N = T.size
    S = flat_index(shape, start)
    table = _offset_table(fs, starstart, starstop)
    nyz = shape[1] * shape[2]

    def coords(c):
        return c // nyz, (c % nyz) // shape[2], c % shape[2]

    def hop_length(c, p):
        cx, cy, cz = coords(c)
        px, py, pz = coords(p)
        for d, kind in table.get((px - cx, py - cy, pz - cz), []):
            live = (c != S) if kind == FWD else (p != S)
            with np.errstate(over="ignore", invalid="ignore"):
                if live and F32(delay(d, v[c] + v[p]) + T[p]) == T[c]:
                    return d
        return None

    paths, hops, status, t_recv = [], [], [], []
    for q in receivers:
        c = flat_index(shape, q)
        t_recv.append(T[c])
        if not T[c] < np.inf:
            status.append(RAY_UNREACHED)
            paths.append([])
            hops.append([])
            continue
        path, hd = [c], []
        st = None
        while st is None:
            p = int(P[c])
            if p == PRED_SOURCE:
                st = RAY_OK if c == S else RAY_INVALID
            elif p == PRED_SEED:
                st = RAY_SEED
            elif p < 0 or p >= N or not T[p] < T[c]:
                st = RAY_INVALID
            else:
                d = hop_length(c, p)
                if d is None:
                    st = RAY_INVALID
                else:
                    path.append(p)
                    hd.append(d)
                    c = p
        status.append(st)
        if st in (RAY_OK, RAY_SEED):
            paths.append(path[::-1])
            hops.append(hd[::-1] + [F32(0)])
        else:
            paths.append([])
            hops.append([])
    counts = np.array([len(p) for p in paths], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cells = np.array([c for p in paths for c in p], dtype=np.int32)
    hop_d = np.array([d for h in hops for d in h], dtype=F32)
    return offsets, cells, hop_d, np.array(status, dtype=np.int32), np.array(t_recv, dtype=F32)


def replay(v, tt, offsets, cells, hop_d):
    """Travel time at the end of every ray, replayed from T[path[0]] with the reference's delay rule
    (NaN for a ray without cells)."""
    v = np.asarray(v, dtype=F32).reshape(-1)
    T = np.asarray(tt, dtype=F32).reshape(-1)
    offsets = np.asarray(offsets)
    cells = np.asarray(cells, dtype=np.int64)
    hop_d = np.asarray(hop_d, dtype=F32)
    nrays = len(offsets) - 1
    counts = offsets[1:] - offsets[:-1]
    out = np.full(nrays, np.nan, dtype=F32)
    have = counts > 0
    t = np.zeros(nrays, dtype=F32)
    t[have] = T[cells[offsets[:-1][have]]]
    for h in range(int(counts.max()) - 1 if nrays and counts.max() > 0 else 0):
        r = np.nonzero(counts > h + 1)[0]
        g = offsets[r] + h
        with np.errstate(over="ignore", invalid="ignore"):
            t[r] = (delay(hop_d[g], v[cells[g]] + v[cells[g + 1]]) + t[r]).astype(F32)
    out[have] = t[have]
    return out


def frechet_dense(offsets, cells, hop_d, ncells):
    """Dense float64 G [nrays, ncells]: every hop of length d between cells a and b adds d / 2 at a and at b."""
    nrays = len(offsets) - 1
    G = np.zeros((nrays, ncells), dtype=np.float64)
    for r in range(nrays):
        for g in range(int(offsets[r]), int(offsets[r + 1]) - 1):
            h = float(hop_d[g]) / 2
            G[r, cells[g]] += h
            G[r, cells[g + 1]] += h
    return G


def predecessors_at(v, tt, fs, start, cells, starstart=0, starstop=None):
    """pred of the listed cells only ((n, 3) coordinates): the same rule as predecessors(), for boxes too large
    for a whole-grid restatement."""
    if starstop is None:
        starstop = len(fs) - 1
    v = np.asarray(v, dtype=F32)
    T = np.asarray(tt, dtype=F32)
    shape = T.shape
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    S = flat_index(shape, start)
    cf = (cells[:, 0] * shape[1] + cells[:, 1]) * shape[2] + cells[:, 2]
    tc = T.reshape(-1)[cf]
    vc = v.reshape(-1)[cf]
    big = np.iinfo(np.int64).max
    best = np.full(len(cells), big, dtype=np.int64)
    for di, dj, dk, d, kind in pull_entries(fs, starstart, starstop):
        o3 = cells + np.array([di, dj, dk])
        ok = np.all((o3 >= 0) & (o3 < np.array(shape)), axis=1)
        of = np.where(ok, (o3[:, 0] * shape[1] + o3[:, 1]) * shape[2] + o3[:, 2], 0)
        to = T.reshape(-1)[of]
        with np.errstate(over="ignore", invalid="ignore"):
            cand = (delay(d, vc + v.reshape(-1)[of]) + to).astype(F32)
            match = ok & (to < tc) & (cand == tc)
        match &= (cf != S) if kind == FWD else (of != S)
        best = np.where(match & (of < best), of, best)
    with np.errstate(invalid="ignore"):
        unreached = ~(tc < np.inf)
    pred = np.where(best == big, PRED_SEED, best)
    pred = np.where(unreached, PRED_UNREACHED, pred)
    pred = np.where(cf == S, PRED_SOURCE, pred)
    return pred.astype(np.int32)
