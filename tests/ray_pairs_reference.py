"""Independent numpy restatement of the pair-list ray calls (include/ttsweep.h, "rays: pair lists"): the rays of a
list of (box, receiver) pairs, the operators over them and the geometry of each ray.

The rays are ray_reference.trace's, box by box, put in pair order; the operators are the functions of
ray_operator_reference.py (forward, adjoint, hits, scale) with nrays = npair.  geometry() derives every output of
ttsweep_ray_pairs_geometry_device from the stored path of each pair with the roundings the header states: integers,
one float32 subtraction, a step-by-step float64 sum."""
import numpy as np

import ray_operator_reference as O
import ray_reference as R

F32 = np.float32


def cross_product(nstart, receivers):
    """The pair list of the dense calls: pair_box[s * nrecv + q] = s, pair_recv[s * nrecv + q] = receivers[q]."""
    receivers = np.asarray(receivers, np.int32).reshape(-1, 3)
    return (np.repeat(np.arange(nstart, dtype=np.int32), len(receivers)),
            np.tile(receivers, (nstart, 1)))


def rays_of_pairs(v, tts, fs, starts, pair_box, pair_recv, lo=0, hi=None, preds=None):
    """ray_reference.trace of every pair, in pair order: (offsets, cells, hop_d, status, t_recv).  Every box is
    traced once, to the distinct receivers its pairs name."""
    pair_box = np.asarray(pair_box, np.int64).reshape(-1)
    pair_recv = np.asarray(pair_recv, np.int64).reshape(-1, 3)
    npair = len(pair_box)
    paths, hops = [None] * npair, [None] * npair
    status = np.zeros(npair, np.int32)
    t_recv = np.zeros(npair, F32)
    for s in np.unique(pair_box):
        rows = np.nonzero(pair_box == s)[0]
        recv, inverse = np.unique(pair_recv[rows], axis=0, return_inverse=True)
        pred = R.predecessors(v, tts[s], fs, starts[s], lo, hi) if preds is None else preds[s]
        o, c, d, st, tr = R.trace(v, tts[s], pred, fs, starts[s], recv, lo, hi)
        for r, u in zip(rows, np.asarray(inverse).reshape(-1)):
            paths[r], hops[r] = c[o[u]:o[u + 1]], d[o[u]:o[u + 1]]
            status[r], t_recv[r] = st[u], tr[u]
    counts = np.array([len(p) for p in paths], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cells = np.concatenate(paths).astype(np.int32) if npair else np.zeros(0, np.int32)
    hop_d = np.concatenate(hops).astype(F32) if npair else np.zeros(0, F32)
    return offsets, cells, hop_d, status, t_recv


def geometry(tts, pair_box, pair_recv, rays):
    """The outputs of ttsweep_ray_pairs_geometry_device as a dict of arrays, from the stored paths `rays` (of
    rays_of_pairs: source -> receiver, hop_d[i] the hop from cell i to cell i + 1).  The walk runs the other way,
    receiver -> source."""
    offsets, cells, hop_d, status, _ = rays
    shape = tts[0].shape
    nyz, nz = shape[1] * shape[2], shape[2]
    npair = len(status)
    pair_recv = np.asarray(pair_recv, np.int64).reshape(-1, 3)
    out = {
        "t_recv": np.zeros(npair, F32), "hops": np.zeros(npair, np.int32), "length": np.zeros(npair, np.float64),
        "recv_hop": np.zeros((npair, 3), np.int32), "recv_d": np.zeros(npair, F32), "recv_dt": np.zeros(npair, F32),
        "src_hop": np.zeros((npair, 3), np.int32), "src_d": np.zeros(npair, F32), "src_dt": np.zeros(npair, F32),
        "deep": np.full(npair, -1, np.int32),
    }

    def xyz(c):
        return np.array([c // nyz, (c % nyz) // nz, c % nz], np.int64)

    for r in range(npair):
        T = np.asarray(tts[pair_box[r]], F32).reshape(-1)
        q = R.flat_index(shape, pair_recv[r])
        out["t_recv"][r] = T[q]
        path = [int(c) for c in cells[offsets[r]:offsets[r + 1]]][::-1]      # walk order: receiver first
        if not path:
            continue                                                         # UNREACHED or INVALID
        assert path[0] == q
        d = hop_d[offsets[r]:offsets[r + 1]][:-1][::-1]                      # d of the hops in walk order
        out["hops"][r] = len(path) - 1
        length = np.float64(0.0)
        for x in d:
            length = length + np.float64(x)
        out["length"][r] = length
        deep = path[0]
        for c in path[1:]:
            if c % nz > deep % nz:
                deep = c
        out["deep"][r] = deep
        if len(path) > 1:
            c, p = path[0], path[1]                                          # the hop out of the receiver
            out["recv_hop"][r] = xyz(p) - xyz(c)
            out["recv_d"][r] = d[0]
            out["recv_dt"][r] = F32(T[c] - T[p])
            c, p = path[-2], path[-1]                                        # the hop into the end cell
            out["src_hop"][r] = xyz(c) - xyz(p)
            out["src_d"][r] = d[-1]
            out["src_dt"][r] = F32(T[c] - T[p])
    return out


def operators(rays, m, w, ncells, dmax):
    """(y, g, S, hits) of the pair list's rays: ray_operator_reference's functions with nrays = npair."""
    offsets, cells, hop_d, _, _ = rays
    g, S = O.adjoint(offsets, cells, hop_d, w, ncells, dmax)
    return O.forward(offsets, cells, hop_d, m), g, S, O.hits(cells, ncells)


def pairs_from_locations_loop(xyz, weights, nstations=None):
    """pairs_from_locations written out as a loop over events and stations."""
    xyz = np.asarray(xyz).reshape(-1, 3)
    K = nstations if weights is None else np.asarray(weights).shape[1]
    box, recv, ev, stn = [], [], [], []
    for e in range(len(xyz)):
        if np.any(xyz[e] < 0):
            continue
        for k in range(K):
            if weights is None or weights[e][k] != 0:
                box.append(k)
                recv.append(xyz[e])
                ev.append(e)
                stn.append(k)
    return (np.array(box, np.int32), np.array(recv, np.int32).reshape(-1, 3), np.array(ev, np.int64),
            np.array(stn, np.int64))
