"""CPU tier of the ray Frechet operators (include/ttsweep.h, "rays: the Frechet operators"): the numpy
restatement (ray_operator_reference.py) against the dense G of ray_reference.py on every recorded box, the C ABI's
surface (symbols exported and bound, the macro, bad arguments refused before any device work) and lsqr against
scipy's on a dense CPU operator."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, Golden
import ray_operator_reference as O
import ray_reference as R


def golden_cases():
    """(name, v, fs, start, tt, starstart, starstop) of every converged box in g24 / g9 / live_ref."""
    import ttsweep_pkg
    P = ttsweep_pkg.load()
    out = []
    for name in ("g24", "g9"):
        g = Golden(name)
        for key, sname, offs, start, tt, _ in g.cases():
            out.append((f"{name}/{key}", g.v, P.inputs.make_fs(offs), start, tt, 0, len(offs) - 1))
        m = g.meta["3_range_5_60"]
        out.append((f"{name}/3_range_5_60", g.v, P.inputs.make_fs(g.star("3")), m["start"],
                    g.z["tt_3_range_5_60"], 5, 60))
    z = np.load(os.path.join(GOLDEN, "live_ref.npz"))
    for n in json.loads(bytes(z["meta"]).decode()):
        fs = P.inputs.make_fs(z[f"offs_{n}"])
        out.append((f"live_ref/{n}", z[f"v_{n}"], fs, z[f"start_{n}"], z[f"tt_{n}"], 0, len(fs) - 1))
    return out


CASES = golden_cases()


def random_weights(rng, n):
    """Normal weights with zeros, negatives and tiny values among them."""
    w = rng.standard_normal(n)
    w[rng.random(n) < 0.15] = 0.0
    tiny = rng.random(n) < 0.1
    w[tiny] *= 2.0 ** -40
    return w


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restated_operators_equal_the_dense_frechet_matrix(case):
    name, v, fs, start, tt, lo, hi = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pred = R.predecessors(v, tt, fs, start, lo, hi)
    recv = np.argwhere(np.isfinite(tt))
    if len(recv) > 400:
        recv = recv[rng.choice(len(recv), 400, replace=False)]
    offsets, cells, hop_d, status, t_recv = R.trace(v, tt, pred, fs, start, recv, lo, hi)
    G = R.frechet_dense(offsets, cells, hop_d, v.size)
    m = rng.uniform(0.5, 2.0, v.size)
    y = O.forward(offsets, cells, hop_d, m)
    want = G @ m
    assert np.all(np.abs(y - want) <= 1e-12 * np.abs(want)), name
    w = random_weights(rng, len(recv))
    g, S = O.adjoint(offsets, cells, hop_d, w, v.size, O.entries_dmax(fs, v.shape, lo, hi))
    want = G.T @ w
    h = O.hits(cells, v.size)
    assert np.all(h[np.any(G != 0, axis=0)] > 0)
    bound = 2.0 ** -S * (h + 1) + 1e-12 * (np.abs(G).T @ np.abs(w))
    assert np.all(np.abs(g - want) <= bound), name
    # the restated sum fits the bound it is built on: every |acc| < 2^61
    assert np.all(np.abs(np.ldexp(g, S)) < 2.0 ** 61)


def test_scale_rule():
    assert O.scale(np.zeros(5), np.float32(1.5), 5) == 0
    # E_w = frexp(3.0) = 2, E_d = frexp(1.5) = 1, K = ceil(log2(5)) = 3
    assert O.scale(np.array([0.0, -3.0, 1e-300, 0.5, 0.0]), np.float32(1.5), 5) == 61 - 2 - 1 - 3
    assert O.scale(np.array([1.0]), np.float32(0.75), 1) == 61 - 1 - 0 - 0


def test_ray_operator_symbols_exported_and_bound(pkg):
    L = pkg._lib.lib()
    bound = {n for n, _, _ in pkg._lib.SYMBOLS}
    for n in ("ttsweep_ray_forward_device", "ttsweep_ray_adjoint_device"):
        assert hasattr(L, n) and n in bound
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ttsweep.h")).read()
    assert "#define TTSWEEP_HAS_RAY_OPERATORS 1" in hdr
    assert "#define TTSWEEP_ABI_VERSION 6" in hdr or "#define TTSWEEP_ABI_VERSION (6)" in hdr
    assert pkg.FrechetOperator is pkg.solver.FrechetOperator and pkg.lsqr is pkg.solver.lsqr
    assert "FrechetOperator" in pkg.__all__ and "lsqr" in pkg.__all__


def test_bad_operator_arguments_are_refused_without_a_device(pkg):
    L = pkg._lib.lib()
    st = (pkg._lib.Start * 1)(pkg._lib.Start(0, 0, 0))
    ptr = (C.c_void_p * 1)(None)
    fwd, adj = L.ttsweep_ray_forward_device, L.ttsweep_ray_adjoint_device
    assert fwd(None, 1, st, ptr, ptr, 1, st, None, None, None) < 0
    assert "ttsweep_ray_forward_device" in pkg._lib.last_error()
    assert adj(None, 1, st, ptr, ptr, 1, st, None, None, None, None) < 0
    assert "ttsweep_ray_adjoint_device" in pkg._lib.last_error()
    for call in (lambda *a: fwd(*a, None, None, None), lambda *a: adj(*a, None, None, None, None)):
        assert call(None, -1, None, None, None, 0, None) < 0
        assert call(None, 0, None, None, None, -1, None) < 0
        assert "null or bad argument" in pkg._lib.last_error()
        assert call(None, 1, st, ptr, ptr, 1, None) < 0          # receivers NULL
        # 65536 x 65536 rays do not fit int32 ray indices: refused before the (one-element) arrays are read
        assert call(None, 65536, st, ptr, ptr, 65536, st) < 0
        assert "int32" in pkg._lib.last_error()


class Dense:
    """A dense torch matrix as an lsqr operator."""

    def __init__(self, A):
        self.A = A
        self.shape = tuple(A.shape)

    def matvec(self, x):
        return self.A @ x

    def rmatvec(self, y):
        return self.A.T @ y


@pytest.mark.parametrize("damp", [0.0, 0.3])
def test_lsqr_matches_scipy_on_a_dense_operator(pkg, damp):
    import torch
    from scipy.sparse.linalg import lsqr as scipy_lsqr
    rng = np.random.default_rng(11)
    A = rng.standard_normal((80, 30))
    A[:, 3] *= 1e-3
    b = rng.standard_normal(80)
    want = scipy_lsqr(A, b, damp=damp, atol=1e-10, btol=1e-10, iter_lim=200)
    x, istop, itn, r1norm = pkg.lsqr(Dense(torch.from_numpy(A)), torch.from_numpy(b), damp=damp, atol=1e-10,
                                     btol=1e-10, iter_lim=200)
    assert x.dtype == torch.float64 and x.device == torch.device("cpu")
    assert (istop, itn) == (want[1], want[2])
    assert np.linalg.norm(x.numpy() - want[0]) <= 1e-9 * np.linalg.norm(want[0])
    assert abs(r1norm - want[3]) <= 1e-9 * abs(want[3])
    # a consistent system: stops on btol with the exact solution
    xs = rng.standard_normal(30)
    x, istop, itn, _ = pkg.lsqr(Dense(torch.from_numpy(A)), torch.from_numpy(A @ xs), iter_lim=200)
    want = scipy_lsqr(A, A @ xs, atol=1e-8, btol=1e-8, iter_lim=200)     # (scipy's defaults are 1e-6)
    assert (istop, itn) == (want[1], want[2])
    assert np.linalg.norm(x.numpy() - want[0]) <= 1e-9 * np.linalg.norm(want[0])


def test_lsqr_of_a_zero_right_hand_side(pkg):
    import torch
    x, istop, itn, r1norm = pkg.lsqr(Dense(torch.eye(4, dtype=torch.float64)), torch.zeros(4, dtype=torch.float64))
    assert torch.equal(x, torch.zeros(4, dtype=torch.float64)) and (istop, itn, r1norm) == (0, 0, 0.0)
