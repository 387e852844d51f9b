"""CPU tier of the ray calls (include/ttsweep.h, "rays"): the numpy restatement (ray_reference.py) on every
converged box the reference recorded - no SEED cell, only OK rays, a bit-exact replay, a Frechet row per ray
that reproduces the receiver's time - and the C ABI's surface: symbols exported and bound, NULL arguments
refused with a message before any device work."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, Golden
import ray_reference as R


def golden_cases():
    """(name, v, fs, start, tt, starstart, starstop) of every converged box in g24 / g9 / live_ref."""
    import ttsweep_pkg
    P = ttsweep_pkg.load()
    out = []
    for name in ("g24", "g9"):
        g = Golden(name)
        for key, sname, offs, start, tt, _ in g.cases():
            fs = P.inputs.make_fs(offs)
            out.append((f"{name}/{key}", g.v, fs, start, tt, 0, len(fs) - 1))
        m = g.meta["3_range_5_60"]
        out.append((f"{name}/3_range_5_60", g.v, P.inputs.make_fs(g.star("3")), m["start"],
                    g.z["tt_3_range_5_60"], 5, 60))
    z = np.load(os.path.join(GOLDEN, "live_ref.npz"))
    for n in json.loads(bytes(z["meta"]).decode()):
        fs = P.inputs.make_fs(z[f"offs_{n}"])
        out.append((f"live_ref/{n}", z[f"v_{n}"], fs, z[f"start_{n}"], z[f"tt_{n}"], 0, len(fs) - 1))
    return out


CASES = golden_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_rays_of_recorded_boxes(case):
    name, v, fs, start, tt, lo, hi = case
    pred = R.predecessors(v, tt, fs, start, lo, hi)
    assert not np.any(pred == R.PRED_SEED), name
    assert np.count_nonzero(pred == R.PRED_SOURCE) == 1 and pred[tuple(start)] == R.PRED_SOURCE
    assert np.all(pred[np.isfinite(tt)] != R.PRED_UNREACHED)
    finite = pred >= 0
    assert np.all(tt.reshape(-1)[pred[finite]] < tt[finite]), name
    recv = np.argwhere(np.isfinite(tt))
    if len(recv) > 2000:
        recv = recv[::3]
    offsets, cells, hop_d, status, t_recv = R.trace(v, tt, pred, fs, start, recv, lo, hi)
    assert np.all(status == R.RAY_OK), name
    assert np.all(cells[offsets[:-1]] == R.flat_index(tt.shape, start)), name
    got = R.replay(v, tt, offsets, cells, hop_d)
    assert np.array_equal(got.view(np.uint32), t_recv.view(np.uint32)), name
    # the Frechet rows: G @ v is the sum of the delays, the receiver's time up to rounding
    sub = slice(0, min(len(recv), 300))
    G = R.frechet_dense(offsets[:len(recv[sub]) + 1], cells, hop_d, v.size)
    gv = G @ v.reshape(-1).astype(np.float64)
    want = t_recv[sub].astype(np.float64)
    assert np.all(np.abs(gv - want) <= 1e-5 * np.maximum(np.abs(want), 1e-30)), name


def test_rays_to_frechet_matches_dense_rows(pkg):
    """rays_to_frechet (torch, here on the CPU) against the dense restatement."""
    import torch
    name, v, fs, start, tt, lo, hi = CASES[8]        # g24/818_mid
    pred = R.predecessors(v, tt, fs, start, lo, hi)
    recv = np.argwhere(np.isfinite(tt))[::11]
    offsets, cells, hop_d, status, t_recv = R.trace(v, tt, pred, fs, start, recv, lo, hi)
    rays = pkg.Rays(torch.from_numpy(offsets), torch.from_numpy(cells), torch.from_numpy(hop_d),
                    torch.from_numpy(status), torch.from_numpy(t_recv))
    G = pkg.rays_to_frechet(rays, v.shape)
    assert G.shape == (len(recv), v.size) and G.dtype == torch.float64
    assert np.allclose(G.to_dense().numpy(), R.frechet_dense(offsets, cells, hop_d, v.size), rtol=0, atol=0)
    gv = torch.sparse.mm(G, torch.from_numpy(v.reshape(-1, 1).astype(np.float64))).flatten().numpy()
    assert np.all(np.abs(gv - t_recv) <= 1e-5 * np.abs(t_recv.astype(np.float64)))


def test_ray_symbols_exported_and_bound(pkg):
    L = pkg._lib.lib()
    bound = {n for n, _, _ in pkg._lib.SYMBOLS}
    for n in ("ttsweep_predecessors_device", "ttsweep_trace_rays_device"):
        assert hasattr(L, n) and n in bound
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ttsweep.h")).read()
    for macro, val in (("TTSWEEP_HAS_RAYS", 1), ("TTSWEEP_PRED_SOURCE", -1), ("TTSWEEP_PRED_SEED", -2),
                       ("TTSWEEP_PRED_UNREACHED", -3), ("TTSWEEP_RAY_OK", 0), ("TTSWEEP_RAY_SEED", 1),
                       ("TTSWEEP_RAY_UNREACHED", 2), ("TTSWEEP_RAY_INVALID", 3)):
        assert f"#define {macro} ({val})" in hdr or f"#define {macro} {val}" in hdr, macro
    assert (pkg.PRED_SOURCE, pkg.PRED_SEED, pkg.PRED_UNREACHED) == (-1, -2, -3)
    assert (pkg.RAY_OK, pkg.RAY_SEED, pkg.RAY_UNREACHED, pkg.RAY_INVALID) == (0, 1, 2, 3)


def test_null_arguments_are_refused_without_a_device(pkg):
    import ctypes as C
    L = pkg._lib.lib()
    st = (pkg._lib.Start * 1)(pkg._lib.Start(0, 0, 0))
    ptr = (C.c_void_p * 1)(None)
    off = (C.c_longlong * 2)()
    assert L.ttsweep_predecessors_device(None, 1, st, ptr, ptr) < 0
    assert "ttsweep_predecessors_device" in pkg._lib.last_error()
    assert L.ttsweep_predecessors_device(None, -1, None, None, None) < 0
    assert L.ttsweep_trace_rays_device(None, 1, st, ptr, ptr, 1, st, off, None, None, None, None, 0) < 0
    assert "ttsweep_trace_rays_device" in pkg._lib.last_error()
    assert L.ttsweep_trace_rays_device(None, 0, None, None, None, -1, None, None, None, None, None, None, 0) < 0
