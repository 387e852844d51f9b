"""Cost of windowed event location and of the coarse-to-fine search (include/ttsweep.h, "locate window";
INTEGRATION.md "Locating events").

Stations and events are those of tools/locate_bench.py (its events() is imported): the boxes of bench.py's workload
solved on the device, --events seeded events, 15 % of the picks dropped.  All in one process, picks and weights
already on the device, HIP events on the current stream, median of --reps after one warm-up call of each shape:
  locate_ms          TravelTimeSolver.locate, the yardstick
  window_full_ms     locate_window over the whole grid with stride 1: the same work as locate
  stage1_ms          locate_window over the whole grid on the lattice of --stride
  stage2_ms          locate_window with stride 1 in the windows locate_refine builds from stage 1
  refine_ms          locate_refine, both stages and the host work between them
  distinct_ms        locate_window with one +-4 window per event around seeded cells, every window different
  refined_equal      the share of events whose refined cell is locate's
  max_misfit_excess  the largest misfit_refine - misfit_locate
Fails unless refine_ms < locate_ms.  Prints one JSON line.

    python tools/locate_window_bench.py [--grid 241,241,51] [--star 818] [--nstarts 24] [--events 4096] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from locate_bench import events        # noqa: E402


def timed(fn, reps):
    """(median ms, every ms, the last result) of fn() after one warm-up call"""
    import torch
    fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [round(x, 3) for x in times], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="241,241,51")
    ap.add_argument("--star", default="818")
    ap.add_argument("--starts", default="24")
    ap.add_argument("--nstarts", type=int, default=0)
    ap.add_argument("--events", type=int, default=4096)
    ap.add_argument("--stride", type=int, default=4)
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
    E, s = args.events, args.stride
    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((K,) + shape, dtype=torch.float32, device=dev)
        assert sol.solve_device(starts, tt, init=True) == 1
        del v
        picks, w, _ = events(tt, E, 1)
        loc_ms, loc_all, full = timed(lambda: sol.locate(tt, picks, w), args.reps)
        win_ms, win_all, whole = timed(lambda: sol.locate_window(tt, picks, w), args.reps)
        assert torch.equal(whole.cell, full.cell) and torch.equal(whole.misfit.view(torch.int64),
                                                                  full.misfit.view(torch.int64))
        s1_ms, _, coarse = timed(lambda: sol.locate_window(tt, picks, w, lo=[0, 0, 0], hi=n - 1, stride=s), args.reps)
        xyz = coarse.xyz.numpy().astype(np.int64)
        placed = (xyz[:, 0] >= 0)[:, None]
        lo2 = np.where(placed, np.maximum(xyz - s, 0), 0)
        hi2 = np.where(placed, np.minimum(xyz + s, n - 1), n - 1)
        s2_ms, _, _ = timed(lambda: sol.locate_window(tt, picks, w, lo=lo2, hi=hi2), args.reps)
        ref_ms, ref_all, fine = timed(lambda: sol.locate_refine(tt, picks, w, stride=s), args.reps)
        # one +-4 window per event around its own seeded centre, every window different
        rng = np.random.default_rng(2)
        flat = np.unique(rng.integers(0, int(np.prod(n)), 2 * E))
        assert len(flat) >= E
        centre = np.array(np.unravel_index(rng.permutation(flat)[:E], shape), np.int64).T
        lo3, hi3 = np.maximum(centre - 4, 0), np.minimum(centre + 4, n - 1)
        distinct = len({tuple(a) + tuple(b) for a, b in zip(lo3, hi3)})
        d_ms, _, _ = timed(lambda: sol.locate_window(tt, picks, w, lo=lo3, hi=hi3), args.reps)
        excess = (fine.misfit - full.misfit)
        excess = excess[torch.isfinite(excess)]
        cand1 = int(np.prod((n - 1) // s + 1))
        out = {"grid": list(shape), "star": args.star, "stations": K, "events": E, "stride": s,
               "locate_ms": round(loc_ms, 3), "locate_ms_all": loc_all,
               "window_full_ms": round(win_ms, 3), "window_full_ms_all": win_all,
               "window_full_over_locate": round(win_ms / loc_ms, 4),
               "stage1_ms": round(s1_ms, 3), "stage1_candidates": cand1,
               "stage2_ms": round(s2_ms, 3), "stage2_candidates_mean": round(float(np.prod(hi2 - lo2 + 1, axis=1).mean()), 1),
               "refine_ms": round(ref_ms, 3), "refine_ms_all": ref_all,
               "locate_over_refine": round(loc_ms / ref_ms, 2),
               "distinct_ms": round(d_ms, 3), "distinct_windows": distinct,
               "refined_equal": round(float((fine.cell == full.cell).double().mean()), 4),
               "max_misfit_excess": float(excess.max()) if len(excess) else 0.0,
               "coarse_without_cell": int((coarse.cell < 0).sum())}
    out["library"] = os.path.relpath(P._lib.LIB_PATH, ROOT)
    print(json.dumps(out))
    if not ref_ms < loc_ms:
        sys.exit(f"locate_refine ({ref_ms:.3f} ms) is not faster than locate ({loc_ms:.3f} ms)")


if __name__ == "__main__":
    main()
