"""Cost of confidence regions (include/ttsweep.h, "locate confidence") beside the search of locate itself.

The case of tools/locate_bench.py: the stations are the boxes of bench.py's workload (241x241x51, 818-FS, the 24
starts of start-24 solved on the device), --events seeded events with noise 0.01 and 15 % of the picks dropped.  All
times are from this process, HIP events on the current stream, median of --reps after one warm-up call:
  locate_ms             TravelTimeSolver.locate, unchanged: the yardstick
  confidence_ms_l1/_l4  locate_confidence at locate's misfit with 1 and 4 levels, delta = c * sigma^2 * (mean weight
                        above zero), c = 3.53 and (1, 3.53, 7.81, 11.34), sigma = the pick noise: sparse regions
  inside_share_l1/_l4   the mean share of the grid's cells inside a region (all levels)
  confidence_dense_ms   one level, delta = +inf: every admissible cell of every event
  peak_call_bytes       device memory in use during a confidence call above the level before it (a thread samples
                        hipMemGetInfo while the call runs), beside what misfit volumes of these events would take
With --grid 1024,1024,512 --star six --nstarts 14 --events 256 the stations are scaled as bench.py scales them.
Prints one JSON line.

    python tools/confidence_bench.py [--grid 241,241,51] [--star 818] [--nstarts 24] [--events 4096] [--reps 5]
"""
import argparse
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from locate_bench import events          # the same seeded events as the locate benchmark

SIGMA = 0.01


def timed(fn, reps):
    import torch
    fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [round(t, 3) for t in times], out


def peak_bytes(fn):
    """Device bytes in use during fn() above the level before it."""
    import torch
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    low, stop = [free0], threading.Event()

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])

    t = threading.Thread(target=sample)
    t.start()
    try:
        fn()
    finally:
        stop.set()
        t.join()
    return free0 - low[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="241,241,51")
    ap.add_argument("--star", default="818")
    ap.add_argument("--starts", default="24")
    ap.add_argument("--nstarts", type=int, default=0)
    ap.add_argument("--events", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libttsweep.so (A/B builds)")
    args = ap.parse_args()
    import torch
    import ttsweep_pkg
    P = ttsweep_pkg.load()
    if args.lib:
        P._lib.use_library(args.lib)
    nx, ny, nz = (int(x) for x in args.grid.split(","))
    shape = (nx, ny, nz)
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
    K, N, E = len(starts), nx * ny * nz, args.events
    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((K,) + shape, dtype=torch.float32, device=dev)
        assert sol.solve_device(starts, tt, init=True) == 1
        del v
        picks, w, _ = events(tt, E, 1)
        loc_ms, loc_all, loc = timed(lambda: sol.locate(tt, picks, w), args.reps)
        unit = SIGMA ** 2 * float(w[w != 0].mean())
        d1 = torch.tensor([3.53 * unit], dtype=torch.float64, device=dev)
        d4 = torch.tensor([1.0, 3.53, 7.81, 11.34], dtype=torch.float64, device=dev) * unit
        out = {"grid": list(shape), "star": args.star, "stations": K, "events": E,
               "picked_station_events": int((w != 0).sum()), "locate_ms": round(loc_ms, 3), "locate_ms_all": loc_all,
               "delta_unit": unit}
        for name, d in (("l1", d1), ("l4", d4)):
            ms, allms, res = timed(lambda: sol.locate_confidence(tt, picks, w, loc.misfit, d), args.reps)
            out.update({f"confidence_ms_{name}": round(ms, 3), f"confidence_ms_{name}_all": allms,
                        f"confidence_over_locate_{name}": round(ms / loc_ms, 4),
                        f"inside_share_{name}": float(res.count.double().mean() / N),
                        f"count_median_{name}": res.count.double().median(dim=0).values.tolist(),
                        f"count_max_{name}": res.count.max(dim=0).values.tolist(),
                        f"open_share_{name}": float(res.open().mean())})
        out["peak_call_bytes"] = peak_bytes(lambda: sol.locate_confidence(tt, picks, w, loc.misfit, d4))
        out["volume_bytes_per_event"] = 8 * N
        out["volume_bytes_all_events"] = 8 * N * E
        if not args.no_dense:
            inf = torch.tensor([float("inf")], dtype=torch.float64, device=dev)
            ms, allms, res = timed(lambda: sol.locate_confidence(tt, picks, w, loc.misfit, inf), max(1, args.reps // 2))
            out.update({"confidence_dense_ms": round(ms, 3), "confidence_dense_ms_all": allms,
                        "dense_over_sparse_l1": round(ms / out["confidence_ms_l1"], 3),
                        "dense_inside_share": float(res.count.double().mean() / N)})
    out["library"] = os.path.relpath(P._lib.LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
