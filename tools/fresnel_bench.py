"""Cost of the Fresnel-volume calls (include/ttsweep.h, "fresnel"; INTEGRATION.md "Fat rays").

Stations: the boxes of bench.py's workload (241x241x51, 818-FS, the 24 starts of start-24) solved on the device.
Events: --events boxes solved from seeded cells (their solve is timed too).  Pairs: (event box, station box), 15 % of
them dropped at random; tau = t_ab / --tau-div for every pair.  Times are HIP events on the current stream around
each call (the calls synchronise before they return), median of --reps after one warm-up call.

  volume_ms                    ttsweep_fresnel_volume_device over whole grids: the call the windows come from
  forward_ms / adjoint_ms / adjoint_hits_ms, each without windows (*_whole_*) and with the volumes' bounding boxes
                               as windows (*_window_*): FresnelOperator.matvec / rmatvec / rmatvec_hits
  visits                       (pair, cell) visits of a call: pairs x cells, or the sum of the windows' cells
  *_gvisits_s                  visits per second / 1e9
  *_hbm_share                  8 bytes (two floats) per visit over the time, against the 8.0 TB/s HBM3E peak of the
                               MI355X (its measured streaming rate is about 6.3 TB/s).  Pairs that share a box re-read
                               it from the caches, so this is the rate at which the kernel consumes travel times, an
                               upper bound on what HBM delivered.
  adjoint_*_atomic_share       8 bytes per int64 atomic (the cells with phi > 0: hits summed) over the time, against
                               the 1.3 TB/s of added bytes the memory-side atomics sustain.  The adjoint_hits rows
                               count the same 8 bytes: the 4-byte hits atomic each of those cells also issues is
                               not in the figure (with it: 1.5 times the share)
  torch_*                      the same sums (phi, F m, F^T w, in float64, not fixed point) in plain torch in the same
                               process over the first --torch-pairs pairs, whole grids and windows, next to the
                               library's time for that sub-list (lib_sub_*), and the ratio

Prints one JSON line.

    python tools/fresnel_bench.py [--events 256] [--tau-div 32] [--reps 5] [--torch-pairs 256] [--nstarts 0] [--lib LIB]

--nstarts N: only the first N of the 24 stations (0: all), for a short run.  --lib LIB: another build of the library
(an A/B build of the same sources); the line's "library" names the one in use.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from locate_window_bench import timed  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s
ATOMIC_ROOF = 1.3e12       # added bytes/s


def torch_sums(tt, starts_flat, a, b, tau, m, w, lo, hi):
    """(y, g) of the pairs in plain torch float64; lo / hi None: whole grids"""
    import torch
    shape = tuple(tt.shape[1:])
    y = torch.zeros(len(a), dtype=torch.float64, device=tt.device)
    g = torch.zeros(shape, dtype=torch.float64, device=tt.device)
    flat = tt.reshape(len(tt), -1)
    for r in range(len(a)):
        win = (slice(None),) * 3 if lo is None else tuple(slice(int(l), int(h) + 1) for l, h in zip(lo[r], hi[r]))
        A, B = tt[int(a[r])][win].double(), tt[int(b[r])][win].double()
        t_ab = flat[int(a[r]), int(starts_flat[b[r]])].double()
        phi = (1.0 - ((A + B) - t_ab) / float(tau[r])).clamp(0.0, 1.0)
        y[r] = (phi * m[win]).sum()
        g[win] += w[r] * phi
    return y, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=256)
    ap.add_argument("--tau-div", type=float, default=32.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-pairs", type=int, default=256)
    ap.add_argument("--nstarts", type=int, default=0)
    ap.add_argument("--lib", default=None, help="another build of libttsweep.so (A/B builds)")
    args = ap.parse_args()
    import torch
    import ttsweep_pkg
    P = ttsweep_pkg.load()
    if args.lib:
        P._lib.use_library(args.lib)
    shape = (241, 241, 51)
    nx, ny, nz = shape
    ncells = nx * ny * nz
    dev = torch.device("cuda:0")
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))
    stations = P.inputs.read_triples(P.inputs.starts_path("24"))
    if args.nstarts:
        stations = stations[:args.nstarts]
    K, E = len(stations), args.events
    rng = np.random.default_rng(20160507)
    cells = np.stack([rng.integers(8, n - 8, E) for n in shape], 1).astype(np.int32)
    starts = np.concatenate([np.asarray(stations, np.int32).reshape(-1, 3), cells])
    v = torch.from_numpy(P.inputs.velocity_model(nx, ny, nz, 20160507)).to(dev)
    out = {"grid": list(shape), "star": "818", "stations": K, "events": E, "tau": f"t_ab / {args.tau_div:g}",
           "reps": args.reps}
    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((K + E,) + shape, dtype=torch.float32, device=dev)
        assert sol.solve_device(stations, tt[:K], init=True) == 1
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for e0 in range(0, E, 24):
            sol.solve_device(cells[e0:e0 + 24], tt[K + e0:K + min(e0 + 24, E)], init=True)
        a1.record()
        a1.synchronize()
        out["event_boxes_solve_ms"] = round(a0.elapsed_time(a1), 3)
        del v

        ev, st = np.meshgrid(np.arange(E), np.arange(K), indexing="ij")
        keep = rng.random(E * K) >= 0.15
        a = (K + ev.reshape(-1)[keep]).astype(np.int32)
        b = st.reshape(-1)[keep].astype(np.int32)
        npair = len(a)
        sflat = (starts[:, 0].astype(np.int64) * ny + starts[:, 1]) * nz + starts[:, 2]
        t_ab = tt.reshape(K + E, -1)[torch.from_numpy(a.astype(np.int64)).to(dev),
                                     torch.from_numpy(sflat[b]).to(dev)].double().cpu().numpy()
        assert np.all(np.isfinite(t_ab)) and np.all(t_ab > 0)
        tau = t_ab / args.tau_div

        gen = torch.Generator(device=dev).manual_seed(1)
        m = torch.rand(shape, dtype=torch.float64, device=dev, generator=gen)
        w = torch.randn(npair, dtype=torch.float64, device=dev, generator=gen)
        out["volume_ms"], out["volume_ms_all"], vols = timed(
            lambda: sol.fresnel_volumes(starts, tt, a, b, tau), args.reps)
        count = vols.count.cpu().numpy()
        lo, hi = vols.windows()
        win_cells = np.prod(hi.astype(np.int64) - lo + 1, axis=1)
        visits = {"whole": npair * ncells, "window": int(win_cells.sum())}
        out.update({"pairs": npair, "support_mean": round(float(count.mean()) / ncells, 5),
                    "window_cells_mean": round(float(win_cells.mean()) / ncells, 5),
                    "visits_whole": visits["whole"], "visits_window": visits["window"],
                    "cells_with_phi": int(count.sum())})
        ops = {"whole": sol.fresnel_operator(starts, tt, a, b, tau, windows=False),
               "window": sol.fresnel_operator(starts, tt, a, b, tau, windows=True)}
        res = {}
        for kind, op in ops.items():
            legs = {"forward": lambda op=op: op.matvec(m), "adjoint": lambda op=op: op.rmatvec(w),
                    "adjoint_hits": lambda op=op: op.rmatvec_hits(w)}
            for leg, fn in legs.items():
                ms, every, res[leg, kind] = timed(fn, args.reps)
                key = f"{leg}_{kind}"
                out[f"{key}_ms"], out[f"{key}_ms_all"] = round(ms, 3), every
                out[f"{key}_gvisits_s"] = round(visits[kind] / ms * 1e-6, 2)
                out[f"{key}_hbm_share"] = round(8.0 * visits[kind] / (ms * 1e-3) / HBM_PEAK, 4)
                if leg != "forward":
                    out[f"{key}_atomic_share"] = round(8.0 * float(count.sum()) / (ms * 1e-3) / ATOMIC_ROOF, 4)
        out["volume_gvisits_s"] = round(visits["whole"] / out["volume_ms"] * 1e-6, 2)
        out["volume_hbm_share"] = round(8.0 * visits["whole"] / (out["volume_ms"] * 1e-3) / HBM_PEAK, 4)
        out["volume_ms"] = round(out["volume_ms"], 3)
        out["windows_change_no_bit"] = bool(
            torch.equal(res["forward", "whole"].view(torch.int64), res["forward", "window"].view(torch.int64))
            and torch.equal(res["adjoint", "whole"].view(torch.int64), res["adjoint", "window"].view(torch.int64))
            and torch.equal(res["adjoint_hits", "whole"][1], res["adjoint_hits", "window"][1]))
        out["hits_sum_is_count_sum"] = int(res["adjoint_hits", "whole"][1].sum()) == int(count.sum())

        # the same sums in plain torch over a sub-list, and the library on that sub-list
        n = min(args.torch_pairs, npair)
        sa, sb, stau = a[:n], b[:n], tau[:n]
        sub = {"whole": sol.fresnel_operator(starts, tt, sa, sb, stau, windows=False),
               "window": sol.fresnel_operator(starts, tt, sa, sb, stau, windows=True)}
        coef_w = sub["whole"].coef * w[:n]
        out["torch_pairs"] = n
        for kind, op in sub.items():
            wl, wh = (None, None) if kind == "whole" else (lo[:n], hi[:n])
            t_ms, _, (ty, tg) = timed(lambda: torch_sums(tt, sflat, sa, sb, stau, m, coef_w, wl, wh), 1)
            f_ms, _, y = timed(lambda op=op: op.forward_raw(m), args.reps)
            g_ms, _, g = timed(lambda op=op: op.rmatvec(w[:n]), args.reps)
            out[f"torch_{kind}_ms"] = round(t_ms, 3)
            out[f"lib_sub_{kind}_ms"] = round(f_ms + g_ms, 3)
            out[f"torch_over_lib_{kind}"] = round(t_ms / (f_ms + g_ms), 1)
            out[f"torch_{kind}_y_max_rel"] = float(((ty - y).abs() / y.abs().clamp_min(1e-300)).max())
            out[f"torch_{kind}_g_max_abs"] = float((tg - g).abs().max())
    out["library"] = os.path.relpath(P._lib.LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
