"""Cost and accuracy gain of sub-cell event location (include/ttsweep.h, "locate subcell"; INTEGRATION.md "Locating
events").

Stations and events are those of tools/locate_bench.py (its events() is imported): the boxes of bench.py's workload
solved on the device, --events seeded events, 15 % of the picks dropped.  Before anything is timed the numpy
restatement (tests/locate_subcell_reference.py) must return the planted node on noise-free picks, on the CPU.  Then,
all in one process, picks and weights already on the device, HIP events on the current stream, median of --reps after
one warm-up call of each shape:
  locate_ms        TravelTimeSolver.locate, the yardstick
  window_ms        locate_window in the +-1 windows around locate's cells, one window per event
  subcell8_ms      locate_subcell in the same windows at --sub (8: 17^3 nodes in a full window)
  subcell1_ms      locate_subcell in the same windows at sub = 1: the candidates of window_ms
  fine_ms          locate_fine, both stages and the host work between them
  triple_ratio     time per (event, node, picked station) of subcell8 over that of window; the picks are the same, so
                   (subcell8_ms / nodes) / (window_ms / cells)
  count_ratio      what the operation counts predict: (21 K + 8 K') / (8 K'), K stations, K' picked per event
Accuracy: --events events at seeded positions between the cells, picks from the trilinear field plus N(0, 0.01):
the median distance in cells from the true position of locate's cell, of centroid() of the confidence region
J <= misfit + 3.53 * 0.01^2, and of locate_fine's position.
Fails unless locate_fine's median distance is below locate's.  Prints one JSON line.

    python tools/locate_subcell_bench.py [--grid 241,241,51] [--star 818] [--nstarts 24] [--events 4096] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from locate_bench import events        # noqa: E402
from locate_window_bench import timed  # noqa: E402
import locate_subcell_reference as S   # noqa: E402


def trilinear(tt, pos):
    """[E, K] float64: the K boxes interpolated at the positions pos [E, 3] (in cells, inside the grid)"""
    n = np.array(tt.shape[1:])
    i = np.minimum(np.floor(pos).astype(np.int64), n - 2)
    u = pos - i
    out = np.zeros((len(pos), tt.shape[0]))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wgt = np.prod(np.where(np.array([dx, dy, dz]) == 1, u, 1 - u), axis=1)
                out += wgt[:, None] * tt[:, i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz].T.astype(np.float64)
    return out


def planted_check(tth, sub, rng, count=8):
    """noise-free picks formed at a node: the restatement returns that node in the +-1 window of its base cell"""
    n = np.array(tth.shape[1:])
    done = 0
    while done < count:
        cell = np.array([rng.integers(1, m - 1) for m in n])
        node = cell * sub + rng.integers(1, sub, 3)
        lo, hi = cell - 1, cell + 1
        if not np.all(np.isfinite(tth[(slice(None),) + tuple(slice(a, b + 1) for a, b in zip(lo, hi))])):
            continue
        That, q = S.interpolate(tth, lo, hi, sub)
        at = tuple(int(np.flatnonzero(q[a] == node[a])[0]) for a in range(3))
        picks = That[(slice(None),) + at][None] + rng.uniform(-5, 5)
        got, mis, _ = S.locate_subcell(tth, picks, None, lo[None], hi[None], sub)
        if not np.array_equal(got[0], node):
            sys.exit(f"the restatement places noise-free picks of node {node} at {got[0]} (J = {mis[0]:.3e})")
        done += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="241,241,51")
    ap.add_argument("--star", default="818")
    ap.add_argument("--starts", default="24")
    ap.add_argument("--nstarts", type=int, default=0)
    ap.add_argument("--events", type=int, default=4096)
    ap.add_argument("--sub", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libttsweep.so (A/B builds)")
    args = ap.parse_args()
    import torch
    import ttsweep_pkg
    P = ttsweep_pkg.load()
    if args.lib:
        P._lib.use_library(args.lib)
    nx, ny, nz = (int(x) for x in args.grid.split(","))
    shape = (nx, ny, nz)
    n = np.array(shape, np.int64)
    dev = torch.device("cuda:0")
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path(args.star)))
    starts = P.inputs.read_triples(P.inputs.starts_path(args.starts))
    if args.nstarts:
        starts = starts[:args.nstarts]
    if shape != (241, 241, 51):
        starts = P.inputs.scaled_starts(starts, nx, ny, nz)
        v = P.inputs.velocity_model_device(nx, ny, nz, 20160507, dev)
    else:
        v = torch.from_numpy(P.inputs.velocity_model(nx, ny, nz, 20160507)).to(dev)
    K = len(starts)
    E, sub = args.events, args.sub
    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((K,) + shape, dtype=torch.float32, device=dev)
        assert sol.solve_device(starts, tt, init=True) == 1
        del v
        tth = tt.cpu().numpy()
        planted_check(tth, sub, np.random.default_rng(8))

        picks, w, _ = events(tt, E, 1)
        loc_ms, loc_all, full = timed(lambda: sol.locate(tt, picks, w), args.reps)
        lo, hi = S.fine_windows(shape, full.cell.cpu().numpy(), 1)
        cells = np.prod(hi - lo + 1, axis=1)
        nodes = np.prod((hi - lo) * sub + 1, axis=1)
        distinct = len({tuple(a) + tuple(b) for a, b in zip(lo, hi)})
        win_ms, win_all, win = timed(lambda: sol.locate_window(tt, picks, w, lo=lo, hi=hi), args.reps)
        s8_ms, s8_all, s8 = timed(lambda: sol.locate_subcell(tt, picks, w, lo=lo, hi=hi, sub=sub), args.reps)
        s1_ms, s1_all, s1 = timed(lambda: sol.locate_subcell(tt, picks, w, lo=lo, hi=hi, sub=1), args.reps)
        fine_ms, fine_all, fine = timed(lambda: sol.locate_fine(tt, picks, w, sub=sub), args.reps)
        assert torch.equal(s1.misfit.view(torch.int64), win.misfit.view(torch.int64))
        assert torch.equal(fine.node, s8.node) and torch.equal(fine.misfit.view(torch.int64), s8.misfit.view(torch.int64))
        assert bool(torch.all(s8.misfit <= win.misfit))
        kp = float((w != 0).sum(1).double().mean())
        ratio = (s8_ms / float(nodes.sum())) / (win_ms / float(cells.sum()))

        # accuracy: true positions between the cells, at least one cell from the faces
        rng = np.random.default_rng(3)
        pos = np.stack([rng.uniform(1, m - 2, E) for m in n], 1)
        clean = trilinear(tth, pos)
        ok = np.all(np.isfinite(clean), axis=1)
        pos, clean = pos[ok], clean[ok]
        noisy = clean + rng.uniform(-5, 5, (len(pos), 1)) + 0.01 * rng.standard_normal(clean.shape)
        wa = np.ones_like(noisy)
        first = sol.locate(tt, noisy, wa)
        conf = sol.locate_confidence(tt, noisy, wa, first.misfit, 3.53 * 0.01 ** 2)
        fine_a = sol.locate_fine(tt, noisy, wa, sub=sub)

        def median_distance(p):
            d = np.sqrt(((p - pos) ** 2).sum(1))
            return round(float(np.median(d[np.isfinite(d)])), 4)

        d_cell = median_distance(first.xyz.numpy().astype(np.float64))
        d_centroid = median_distance(conf.centroid()[:, 0, :])
        d_fine = median_distance(fine_a.position)
        out = {"grid": list(shape), "star": args.star, "stations": K, "events": E, "sub": sub,
               "picked_mean": round(kp, 2), "distinct_windows": distinct,
               "cells_mean": round(float(cells.mean()), 1), "nodes_mean": round(float(nodes.mean()), 1),
               "locate_ms": round(loc_ms, 3), "locate_ms_all": loc_all,
               "window_ms": round(win_ms, 3), "window_ms_all": win_all,
               "subcell8_ms": round(s8_ms, 3), "subcell8_ms_all": s8_all,
               "subcell1_ms": round(s1_ms, 3), "subcell1_ms_all": s1_all,
               "fine_ms": round(fine_ms, 3), "fine_ms_all": fine_all,
               "triple_ratio": round(ratio, 3), "count_ratio": round((21 * K + 8 * kp) / (8 * kp), 3),
               "accuracy_events": int(len(pos)), "median_distance_cell": d_cell,
               "median_distance_centroid": d_centroid, "median_distance_fine": d_fine}
    out["library"] = os.path.relpath(P._lib.LIB_PATH, ROOT)
    print(json.dumps(out))
    if not d_fine < d_cell:
        sys.exit(f"locate_fine's median distance ({d_fine}) is not below locate's ({d_cell})")


if __name__ == "__main__":
    main()
