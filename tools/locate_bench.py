"""Cost of event location (include/ttsweep.h, "locate"; INTEGRATION.md "Locating events").

The stations are the boxes of bench.py's workload: 241x241x51, 818-FS, the 24 starts of start-24 solved on the
device.  --events seeded events (default 4096) at random cells every box reaches, picks T_k[cell] + t0 + noise, 15 %
of the picks dropped (weight 0).  locate_ms: one TravelTimeSolver.locate call (picks and weights already on the
device), HIP events on the current stream, median of --reps after one warm-up call.  torch_ms: the same formula in
plain torch on the same device, --chunk events at a time ([chunk, ncells] float64 tensors, stations in order, picked
stations masked), timed once after a warm-up chunk; speedup = torch_ms / locate_ms.  f64_ops is the work of the
formula, 8 double operations per (event, picked station, cell).  With --grid 1024,1024,512 --star six --nstarts 14
the stations are scaled as bench.py scales them (no torch baseline: --no-torch).  Prints one JSON line.

    python tools/locate_bench.py [--grid 241,241,51] [--star 818] [--nstarts 24] [--events 4096] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events(tt, E, seed):
    """picks, weights [E, K] (float64 torch on tt's device) and the true cells."""
    import torch
    K = tt.shape[0]
    flat = tt.reshape(K, -1)
    ok = torch.nonzero(torch.all(torch.isfinite(flat), dim=0)).flatten()
    g = torch.Generator(device=tt.device).manual_seed(seed)
    cells = ok[torch.randint(0, len(ok), (E,), device=tt.device, generator=g)]
    t0 = torch.rand(E, dtype=torch.float64, device=tt.device, generator=g) * 10 - 5
    picks = flat[:, cells].T.to(torch.float64) + t0[:, None]
    picks += 0.01 * torch.randn(E, K, dtype=torch.float64, device=tt.device, generator=g)
    w = 0.5 + 1.5 * torch.rand(E, K, dtype=torch.float64, device=tt.device, generator=g)
    w[torch.rand(E, K, device=tt.device, generator=g) < 0.15] = 0.0
    w[torch.arange(E), torch.randint(0, K, (E,), device=tt.device, generator=g)] = 1.0
    return picks.contiguous(), w.contiguous(), cells


def torch_locate(T64, picks, w, chunk):
    """The formula in plain torch: (cell, J) per event, chunk events at a time."""
    import torch
    K, N = T64.shape
    cells, Js = [], []
    for a in range(0, len(picks), chunk):
        o, ww = picks[a:a + chunk], w[a:a + chunk]
        invW = 1.0 / ww.sum(dim=1, keepdim=True)
        S1 = torch.zeros(len(o), N, dtype=torch.float64, device=T64.device)
        for k in range(K):
            d = o[:, k:k + 1] - T64[k]
            S1 += torch.where(ww[:, k:k + 1] != 0, ww[:, k:k + 1] * d, 0.0)
        t0 = S1 * invW
        J = torch.zeros_like(S1)
        for k in range(K):
            r = (o[:, k:k + 1] - T64[k]) - t0
            J += torch.where(ww[:, k:k + 1] != 0, ww[:, k:k + 1] * r * r, 0.0)
        J = torch.nan_to_num(J, nan=float("inf"))
        m, c = J.min(dim=1)
        cells.append(c)
        Js.append(m)
    return torch.cat(cells), torch.cat(Js)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="241,241,51")
    ap.add_argument("--star", default="818")
    ap.add_argument("--starts", default="24")
    ap.add_argument("--nstarts", type=int, default=0)
    ap.add_argument("--events", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--no-torch", action="store_true")
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
    K = len(starts)
    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((K,) + shape, dtype=torch.float32, device=dev)
        assert sol.solve_device(starts, tt, init=True) == 1
        del v
        picks, w, true = events(tt, args.events, 1)
        sol.locate(tt, picks, w)
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = sol.locate(tt, picks, w)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        loc_ms = float(np.median(times))
        picked = int((w != 0).sum())
        N = nx * ny * nz
        out = {"grid": list(shape), "star": args.star, "stations": K, "events": args.events,
               "picked_station_events": picked, "f64_ops": 8 * picked * N,
               "locate_ms": round(loc_ms, 3), "locate_ms_all": [round(x, 3) for x in times],
               "f64_ops_per_s": round(8 * picked * N / (loc_ms * 1e-3), 1),
               "true_cell_recovered": round(float((res.cell.to(torch.int64) == true).double().mean()), 4),
               "no_admissible_cell": int((res.cell < 0).sum())}
        if not args.no_torch:
            T64 = tt.reshape(K, -1).to(torch.float64)
            torch_locate(T64, picks[:args.chunk], w[:args.chunk], args.chunk)
            torch.cuda.synchronize(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tc, tj = torch_locate(T64, picks, w, args.chunk)
            b.record()
            b.synchronize()
            torch_ms = a.elapsed_time(b)
            out.update({"torch_ms": round(torch_ms, 1), "torch_chunk_events": args.chunk,
                        "speedup_over_torch": round(torch_ms / loc_ms, 2),
                        "torch_cells_agree": round(float((tc.to(torch.int32) == res.cell).double().mean()), 4)})
    out["library"] = os.path.relpath(P._lib.LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
