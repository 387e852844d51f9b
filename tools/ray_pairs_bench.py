"""Cost of the pair-list ray calls (include/ttsweep.h, "rays: pair lists"; INTEGRATION.md "Rays").

The boxes are those of tools/ray_bench.py: 241x241x51, 818-FS, the 24 starts of start-24 solved on the device, pred
computed once.  Times are HIP events on the current stream around each call (the calls synchronise before they
return), median of --reps after one warm-up call.

  (a) cross product: every surface cell (z = 0) of every box, the rays of tools/ray_bench.py, once through the dense
      calls (dense_*_ms) and once as a pair list (pairs_*_ms) in the same process: forward, adjoint, adjoint with
      hits; the outputs are compared bit for bit (cross_product_equal); *_ratio = pairs / dense.
  (b) located events: the --events seeded events of tools/locate_bench.py (random cells every box reaches, 15 % of
      the picks dropped) and pairs_from_locations of their true cells: events_*_ms for forward, adjoint, adjoint with
      hits and geometry, the time of pairs_from_locations itself (host), and the dense calls that would be needed to
      cover the same picks (24 boxes x the events' cells: cover_*_ms), with the rays each walks.

Prints one JSON line.

    python tools/ray_pairs_bench.py [--events 4096] [--reps 5] [--lib LIB]

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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nstarts", type=int, default=0)
    ap.add_argument("--lib", default=None, help="another build of libttsweep.so (A/B builds)")
    args = ap.parse_args()
    import torch
    import ttsweep_pkg
    from locate_bench import events
    P = ttsweep_pkg.load()
    if args.lib:
        P._lib.use_library(args.lib)
    shape = (241, 241, 51)
    nx, ny, nz = shape
    dev = torch.device("cuda:0")
    fs = P.inputs.make_fs(P.inputs.read_triples(P.inputs.star_path("818")))
    starts = P.inputs.read_triples(P.inputs.starts_path("24"))
    if args.nstarts:
        starts = starts[:args.nstarts]
    K = len(starts)
    v = torch.from_numpy(P.inputs.velocity_model(nx, ny, nz, 20160507)).to(dev)
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
        return float(np.median(out)), res

    def legs(op, m, w, prefix, out):
        """forward, adjoint, adjoint with hits of one operator: times into out, results returned."""
        out[f"{prefix}_forward_ms"], y = timed(lambda: op.matvec(m))
        out[f"{prefix}_adjoint_ms"], g = timed(lambda: op.rmatvec(w))
        out[f"{prefix}_adjoint_hits_ms"], gh = timed(lambda: op.rmatvec_hits(w))
        return y, g, gh[1]

    out = {"grid": list(shape), "star": "818", "nstart": K, "reps": args.reps}
    with P.TravelTimeSolver(shape, fs) as sol:
        sol.set_velocity(v)
        tt = torch.empty((K,) + shape, dtype=torch.float32, device=dev)
        assert sol.solve_device(starts, tt, init=True) == 1
        pred = sol.predecessors(starts, tt)
        gen = torch.Generator(device=dev).manual_seed(1)
        m = torch.rand(nx * ny * nz, dtype=torch.float64, device=dev, generator=gen)

        # (a) the cross product of tools/ray_bench.py, dense and as a pair list
        box = np.repeat(np.arange(K, dtype=np.int32), len(recv))
        dense = sol.frechet_operator(starts, tt, recv, pred)
        pairs = sol.frechet_operator(starts, tt, pred=pred, pairs=(box, np.tile(recv, (K, 1))))
        w = torch.randn(dense.shape[0], dtype=torch.float64, device=dev, generator=gen)
        a = legs(dense, m, w, "dense", out)
        b = legs(pairs, m, w, "pairs", out)
        out["cross_product_rays"] = dense.shape[0]
        out["cross_product_equal"] = bool(
            torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
            and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)) and torch.equal(a[2], b[2])
            and torch.equal(dense.status, pairs.status) and dense.last_scale == pairs.last_scale)
        for k in ("forward", "adjoint", "adjoint_hits"):
            out[f"{k}_ratio"] = round(out[f"pairs_{k}_ms"] / out[f"dense_{k}_ms"], 4)
        del dense, pairs, a, b, w

        # (b) the locate bench's events: the picks that exist against the cross product that covers them
        _, wts, true = events(tt, args.events, 1)
        true = true.cpu().numpy()
        xyz = np.stack([true // (ny * nz), true // nz % ny, true % nz], 1).astype(np.int32)
        wts = wts.cpu().numpy()
        t0 = time.perf_counter()
        pbox, precv, ev, stn = P.pairs_from_locations(xyz, wts)
        out["pairs_from_locations_ms"] = (time.perf_counter() - t0) * 1e3
        op = sol.frechet_operator(starts, tt, pred=pred, pairs=(pbox, precv))
        w = torch.randn(op.shape[0], dtype=torch.float64, device=dev, generator=gen)
        legs(op, m, w, "events", out)
        out["events_geometry_ms"], geo = timed(lambda: sol.ray_geometry(starts, tt, pbox, precv, pred=pred))
        hops = geo.hops.to(torch.float64)
        out.update({"events": args.events, "events_pairs": op.shape[0],
                    "events_hops_mean": round(float(hops.mean()), 2), "events_hops_max": int(hops.max()),
                    "events_status_ok_seed_unreached_invalid":
                        [int(x) for x in np.bincount(op.status.numpy(), minlength=4)]})
        cover = sol.frechet_operator(starts, tt, xyz, pred)
        wc = torch.randn(cover.shape[0], dtype=torch.float64, device=dev, generator=gen)
        legs(cover, m, wc, "cover", out)
        out["cover_rays"] = cover.shape[0]
        out["rays_walked_ratio"] = round(op.shape[0] / cover.shape[0], 4)
        for k in ("forward", "adjoint", "adjoint_hits"):
            out[f"events_over_cover_{k}"] = round(out[f"events_{k}_ms"] / out[f"cover_{k}_ms"], 4)
        out["geometry_over_forward"] = round(out["events_geometry_ms"] / out["events_forward_ms"], 4)
    out = {k: round(x, 3) if isinstance(x, float) and k.endswith("_ms") else x for k, x in out.items()}
    out["library"] = os.path.relpath(P._lib.LIB_PATH, ROOT)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
