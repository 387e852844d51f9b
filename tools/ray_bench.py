"""Cost of the ray calls on the bench workload (include/ttsweep.h, "rays"; INTEGRATION.md "Rays").

  (a) predecessors of every box: TravelTimeSolver.predecessors (one ttsweep_predecessors_device call)
  (b) rays from every surface cell (z = 0) of every box: TravelTimeSolver.trace_rays with pred given (both ABI
      calls: count, host scan, fill), including the allocation of the path buffers
on 241x241x51, 818-FS, the 24 starts of start-24 solved on the device (bench.py's default workload), and with
--grid 1024,1024,512 --star six --nstarts N on the HBM-regime grid (scaled starts, as bench.py).  Times are HIP
events on the current stream around each call (the calls synchronise before they return), median of --reps after
one warm-up call.  trace_rays_phases_ms splits (b) into the steps trace_rays takes, each timed on the host clock
(every step ends synchronised): the receiver list to its C array, the counting call of the C ABI, the allocation
of the path buffers, the filling call.

The Frechet operators of the same rays (TravelTimeSolver.frechet_operator, pred given):
  (c) frechet_forward_ms G m, frechet_adjoint_ms G^T w, frechet_hits_ms the hit counts alone,
      frechet_adjoint_hits_ms G^T w and the hit counts of one walk (m, w random float64 on the device);
  (d) the explicit path for comparison: explicit_trace_frechet_ms = trace_rays + rays_to_frechet (the sparse COO
      matrix, coalesced), explicit_forward_ms / explicit_adjoint_ms = torch.sparse.mm with G / G^T.
frechet_peak_bytes is the peak of torch's device allocator over (c), the boxes and pred included.  --no-trace
leaves out (b) and (d), the legs that store paths: with --grid 1024,1024,512 --star six --nstarts 14 the paths of
every surface cell would need ~150 GB.  Prints one JSON line.

    python tools/ray_bench.py [--grid 241,241,51] [--star 818] [--nstarts 24] [--reps 5] [--no-trace] [--lib LIB]

--lib LIB: another build of the library (an A/B build of the same sources); the line's "library" names the one in use.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="241,241,51")
    ap.add_argument("--star", default="818")
    ap.add_argument("--starts", default="24")
    ap.add_argument("--nstarts", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="leave out the legs that store paths: (b) and (d)")
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
    nstart = len(starts)
    surf = np.argwhere(np.ones((nx, ny), bool))
    recv = np.concatenate([surf, np.zeros((len(surf), 1), np.int64)], axis=1).astype(np.int32)

    def timed(fn):
        fn()
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return float(np.median(out)), out, res

    def phases(sol, tt, pred):
        """trace_rays step by step (solver.py), each step timed: ms per step."""
        out = {}
        t0 = time.perf_counter()
        arr, recv_arr = sol._starts_array(starts), sol._starts_array(recv)
        t1 = time.perf_counter()
        nrays = nstart * len(recv_arr)
        offsets = torch.zeros(nrays + 1, dtype=torch.int64)
        status = torch.empty(nrays, dtype=torch.int32)
        t_recv = torch.empty(nrays, dtype=torch.float32)
        tptr, pptr = sol._box_pointers(tt, nstart), sol._box_pointers(pred, nstart)

        def call(cells, hop_d, cap):
            return sol._L.ttsweep_trace_rays_device(sol._ctx, nstart, arr, tptr, pptr, len(recv_arr), recv_arr,
                                                    offsets.data_ptr(), status.data_ptr(), t_recv.data_ptr(),
                                                    cells, hop_d, cap)
        t2 = time.perf_counter()
        total = call(None, None, 0)
        t3 = time.perf_counter()
        cells = torch.empty(total, dtype=torch.int32, device=dev)
        hop_d = torch.empty(total, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        t4 = time.perf_counter()
        assert call(cells.data_ptr(), hop_d.data_ptr(), total) == total
        t5 = time.perf_counter()
        out["receivers_to_c_array"] = (t1 - t0) * 1e3
        out["count_call"] = (t3 - t2) * 1e3
        out["alloc_paths"] = (t4 - t3) * 1e3
        out["fill_call"] = (t5 - t4) * 1e3
        return out

    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((nstart,) + shape, dtype=torch.float32, device=dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert sol.solve_device(starts, tt, init=True) == 1
        b.record()
        b.synchronize()
        solve_ms = a.elapsed_time(b)
        pred_ms, pred_all, pred = timed(lambda: sol.predecessors(starts, tt))
        out = {}
        if not args.no_trace:
            rays_ms, rays_all, rays = timed(lambda: sol.trace_rays(starts, tt, recv, pred))
            steps = [phases(sol, tt, pred) for _ in range(args.reps + 1)][1:]
            counts = (rays.offsets[1:] - rays.offsets[:-1]).numpy()
            out.update({
                "trace_rays_ms": round(rays_ms, 3), "trace_rays_ms_all": [round(x, 3) for x in rays_all],
                "trace_rays_phases_ms": {k: round(float(np.median([s[k] for s in steps])), 3) for k in steps[0]},
                "rays": int(len(rays)), "path_cells": int(counts.sum()), "hops_max": int(counts.max() - 1),
                "hops_mean": round(float(counts.mean() - 1), 2),
                "status_ok_seed_unreached_invalid": [int(x) for x in np.bincount(rays.status.numpy(), minlength=4)],
            })
            del rays
        kernel = sol.stats()["kernel_variant"]
        out.update(operator_legs(P, sol, starts, tt, recv, pred, timed, dev))
        if not args.no_trace:
            out.update(explicit_legs(P, sol, starts, tt, recv, pred, shape, timed, dev))
    npull = len(P.build_pull_star(fs))
    print(json.dumps({
        "grid": list(shape), "star": args.star, "nstart": nstart, "solve_kernel_variant": kernel,
        "solve_ms_first_call": round(solve_ms, 3),
        "predecessors_ms": round(pred_ms, 3), "predecessors_ms_all": [round(x, 3) for x in pred_all],
        "predecessor_candidates": int(nstart * nx * ny * nz * npull), **out,
        "library": os.path.relpath(P._lib.LIB_PATH, ROOT)}))


def operator_legs(P, sol, starts, tt, recv, pred, timed, dev):
    """(c): the Frechet operators, pred given."""
    import torch
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    build_ms, _, op = timed(lambda: sol.frechet_operator(starts, tt, recv, pred))
    gen = torch.Generator(device=dev).manual_seed(1)
    m = torch.rand(op.shape[1], dtype=torch.float64, device=dev, generator=gen)
    w = torch.randn(op.shape[0], dtype=torch.float64, device=dev, generator=gen)
    fwd_ms, fwd_all, _ = timed(lambda: op.matvec(m))
    del m
    adj_ms, adj_all, g = timed(lambda: op.rmatvec(w))
    del g
    hits_ms, hits_all, hits = timed(op.hits)
    both_ms, both_all, _ = timed(lambda: op.rmatvec_hits(w))
    status = np.bincount(op.status.numpy(), minlength=4)
    r = lambda xs: [round(x, 3) for x in xs]
    return {
        "frechet_operator_ms": round(build_ms, 3),
        "frechet_forward_ms": round(fwd_ms, 3), "frechet_forward_ms_all": r(fwd_all),
        "frechet_adjoint_ms": round(adj_ms, 3), "frechet_adjoint_ms_all": r(adj_all),
        "frechet_hits_ms": round(hits_ms, 3), "frechet_hits_ms_all": r(hits_all),
        "frechet_adjoint_hits_ms": round(both_ms, 3), "frechet_adjoint_hits_ms_all": r(both_all),
        "frechet_scale": op.last_scale, "frechet_rays": op.shape[0],
        "frechet_path_cells": int(hits.to(torch.int64).sum()),
        "frechet_status_ok_seed_unreached_invalid": [int(x) for x in status],
        "frechet_peak_bytes": int(torch.cuda.max_memory_allocated(dev)),
    }


def explicit_legs(P, sol, starts, tt, recv, pred, shape, timed, dev):
    """(d): trace_rays + rays_to_frechet, then torch.sparse.mm with G and G^T."""
    import torch
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    build_ms, build_all, G = timed(lambda: P.rays_to_frechet(sol.trace_rays(starts, tt, recv, pred), shape))
    gen = torch.Generator(device=dev).manual_seed(1)
    m = torch.rand(G.shape[1], 1, dtype=torch.float64, device=dev, generator=gen)
    w = torch.randn(G.shape[0], 1, dtype=torch.float64, device=dev, generator=gen)
    Gt = G.t()
    fwd_ms, fwd_all, _ = timed(lambda: torch.sparse.mm(G, m))
    adj_ms, adj_all, _ = timed(lambda: torch.sparse.mm(Gt, w))
    r = lambda xs: [round(x, 3) for x in xs]
    return {
        "explicit_trace_frechet_ms": round(build_ms, 3), "explicit_trace_frechet_ms_all": r(build_all),
        "explicit_forward_ms": round(fwd_ms, 3), "explicit_forward_ms_all": r(fwd_all),
        "explicit_adjoint_ms": round(adj_ms, 3), "explicit_adjoint_ms_all": r(adj_all),
        "explicit_nnz": int(G._nnz()), "explicit_peak_bytes": int(torch.cuda.max_memory_allocated(dev)),
    }


if __name__ == "__main__":
    main()
