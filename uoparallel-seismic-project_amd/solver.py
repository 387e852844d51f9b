"""Python mirror of the C ABI in include/ttsweep.h (thin ctypes layer, no compute).

`TravelTimeSolver` wraps one `ttsweep_ctx`.  Method names follow the C entry
points; array arguments use the reference's FLOATBOX layout ([x][y][z], z fastest,
include/floatbox.h:127-129).  All arithmetic happens in libttsweep.so on the GPU;
if the library or a HIP device is missing every call raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import FS, PullEntry, Start, Stats
from .inputs import FS_DTYPE


class TTSweepError(RuntimeError):
    pass


def _check(rc: int, what: str) -> int:
    if rc < 0:
        raise TTSweepError(f"{what}: {_lib.last_error()}")
    return rc


def _require(cond: bool, what: str):
    """Argument checks that must survive `python -O` (a wrong shape, dtype or device handed
    to the C ABI is an out-of-bounds or cross-device access on the GPU)."""
    if not cond:
        raise TTSweepError(what)


def device_count() -> int:
    return _check(_lib.lib().ttsweep_device_count(), "ttsweep_device_count")


def build_pull_star(fs: np.ndarray, starstart: int = 0, starstop: int | None = None):
    """Host-only: the pull form of the star as a list of (di,dj,dk,flags,h)."""
    fs = np.ascontiguousarray(fs, dtype=FS_DTYPE)
    if starstop is None:
        starstop = len(fs) - 1
    cap = 2 * max(len(fs), 1)
    buf = (PullEntry * cap)()
    n = _check(_lib.lib().ttsweep_build_pull_star(fs.ctypes.data, starstart, starstop, buf, cap),
               "ttsweep_build_pull_star")
    return [(e.di, e.dj, e.dk, e.flags, e.h) for e in buf[:n]]


def relaxations_per_sweep(shape, fs: np.ndarray, starstart: int = 0, starstop: int | None = None) -> int:
    fs = np.ascontiguousarray(fs, dtype=FS_DTYPE)
    if starstop is None:
        starstop = len(fs) - 1
    return _lib.lib().ttsweep_relaxations_per_sweep(*map(int, shape), fs.ctypes.data,
                                                    starstart, starstop)


class TravelTimeSolver:
    """One solver context: a grid size, a star range and a device.

    starstop defaults to len(fs)-1, the (exclusive) bound the reference call site
    passes (serial_new/sweep-tt-multistart.c:160)."""

    def __init__(self, shape, fs: np.ndarray, starstart: int = 0, starstop: int | None = None,
                 device: int = 0):
        self._L = _lib.lib()
        self.shape = tuple(int(n) for n in shape)
        self.fs = np.ascontiguousarray(fs, dtype=FS_DTYPE)
        self.starstart = starstart
        self.starstop = len(self.fs) - 1 if starstop is None else starstop
        self.device = device
        self._ctx = self._L.ttsweep_create(device, *self.shape, self.fs.ctypes.data,
                                           self.starstart, self.starstop)
        if not self._ctx:
            raise TTSweepError(f"ttsweep_create: {_lib.last_error()}")

    # -- lifecycle ----------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._L.ttsweep_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, key: int, value: int):
        _check(self._L.ttsweep_set_option(self._ctx, key, value), "ttsweep_set_option")

    # -- inputs -------------------------------------------------------------
    def set_velocity(self, v):
        """v: numpy float32 [nx,ny,nz] (host) or a CUDA/HIP torch tensor (device)."""
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v, dtype=np.float32)
            _require(v.shape == self.shape, f"velocity shape {v.shape} != {self.shape}")
            _check(self._L.ttsweep_set_velocity(self._ctx, v.ctypes.data), "ttsweep_set_velocity")
        else:
            self._require_device_tensor(v, self.shape, "velocity")
            import torch
            torch.cuda.current_stream(v.device).synchronize()
            _check(self._L.ttsweep_set_velocity_device(self._ctx, v.data_ptr()),
                   "ttsweep_set_velocity_device")

    def _require_device_tensor(self, t, shape, what):
        import torch
        _require(isinstance(t, torch.Tensor) and t.is_cuda, f"{what}: not a device tensor")
        _require(t.dtype == torch.float32 and t.is_contiguous(), f"{what}: must be contiguous float32")
        _require(tuple(t.shape) == tuple(shape), f"{what}: shape {tuple(t.shape)} != {tuple(shape)}")
        _require(t.device.index == self.device,
                 f"{what}: tensor on device {t.device.index}, solver on device {self.device}")

    # -- the hot path -------------------------------------------------------
    @staticmethod
    def _starts_array(starts):
        # one copy of the (n, 3) int32 rows: struct START is three packed ints (receiver lists are long)
        starts = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1, 3))
        return (Start * len(starts)).from_buffer_copy(starts.tobytes())

    def solve(self, starts, tt_boxes) -> int:
        """In-place solve of host boxes (numpy float32 arrays, one per start).
        Returns 1 if anything improved, 0 if all boxes were already converged."""
        arr = self._starts_array(starts)
        _require(len(tt_boxes) == len(arr), "one box per start")
        ptrs = (C.c_void_p * len(arr))()
        for s, box in enumerate(tt_boxes):
            _require(isinstance(box, np.ndarray) and box.dtype == np.float32, f"box {s}: float32 ndarray")
            _require(box.flags["C_CONTIGUOUS"] and box.shape == self.shape, f"box {s}: shape / layout")
            ptrs[s] = box.ctypes.data
        return _check(self._L.ttsweep_solve(self._ctx, len(arr), arr, ptrs), "ttsweep_solve")

    def solve_device(self, starts, tt, init: bool = True) -> int:
        """Solve with the boxes resident in HBM.  tt: torch float32 tensor
        [nstart,nx,ny,nz] on this solver's device, written in place."""
        import torch
        arr = self._starts_array(starts)
        self._require_device_tensor(tt, (len(arr),) + self.shape, "travel-time boxes")
        ptrs = (C.c_void_p * len(arr))()
        stride = tt.stride(0) * 4
        for s in range(len(arr)):
            ptrs[s] = tt.data_ptr() + s * stride
        torch.cuda.current_stream(tt.device).synchronize()
        return _check(self._L.ttsweep_solve_device(self._ctx, len(arr), arr, ptrs, int(init)),
                      "ttsweep_solve_device")

    def changed(self, nstart: int):
        """Per-start outcome of the last solve: 1 where a travel time of that start improved (the
        reference's changed[s], serial_new/sweep-tt-multistart.c:158-164)."""
        out = (C.c_int * nstart)()
        m = _check(self._L.ttsweep_get_changed(self._ctx, out, nstart), "ttsweep_get_changed")
        return [int(out[s]) for s in range(m)]

    def validate_device(self, start, tt):
        """(open_edges, cells_infinite, cells_unsupported) of one box in HBM (torch tensor
        [nx,ny,nz]): the reference's store conditions evaluated on the device, and the cells
        no store can have produced; (0, 0, 0) exactly for the converged box."""
        import torch
        self._require_device_tensor(tt, self.shape, "travel-time box")
        torch.cuda.current_stream(tt.device).synchronize()
        st = Start(int(start[0]), int(start[1]), int(start[2]))
        a, b, c = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _check(self._L.ttsweep_validate_device(self._ctx, C.byref(st), tt.data_ptr(), C.byref(a),
                                               C.byref(b), C.byref(c)), "ttsweep_validate_device")
        return a.value, b.value, c.value

    # -- rays ---------------------------------------------------------------
    def _box_pointers(self, t, n):
        ptrs = (C.c_void_p * max(n, 1))()
        for s in range(n):
            ptrs[s] = t.data_ptr() + s * t.stride(0) * t.element_size()
        return ptrs

    def predecessors(self, starts, tt):
        """ttsweep_predecessors_device: for every cell of every box of tt (torch float32 [nstart,nx,ny,nz]
        on this solver's device) the smallest FLOATBOX index of a neighbour whose candidate is its travel
        time, or PRED_SOURCE / PRED_SEED / PRED_UNREACHED.  Returns a torch.int32 tensor of tt's shape on
        the same device."""
        import torch
        arr = self._starts_array(starts)
        n = len(arr)
        self._require_device_tensor(tt, (n,) + self.shape, "travel-time boxes")
        pred = torch.empty(tt.shape, dtype=torch.int32, device=tt.device)
        torch.cuda.current_stream(tt.device).synchronize()
        _check(self._L.ttsweep_predecessors_device(self._ctx, n, arr, self._box_pointers(tt, n),
                                                   self._box_pointers(pred, n)), "ttsweep_predecessors_device")
        return pred

    def _require_pred(self, starts, tt, pred):
        """pred of the boxes tt: the caller's, checked, or the result of predecessors() when None."""
        import torch
        if pred is None:
            return self.predecessors(starts, tt)
        _require(isinstance(pred, torch.Tensor) and pred.dtype == torch.int32 and pred.is_contiguous()
                 and tuple(pred.shape) == tuple(tt.shape) and pred.device == tt.device,
                 "pred: contiguous int32 tensor of the boxes' shape on their device")
        return pred

    def trace_rays(self, starts, tt, receivers, pred=None) -> "Rays":
        """ttsweep_trace_rays_device: the ray from every start of tt to every receiver ((nrecv, 3) cells),
        ray r = s * nrecv + q.  pred: the result of predecessors() for these boxes (computed when None).
        Two calls of the C ABI: one counts the path cells, the second fills the paths."""
        import torch
        arr = self._starts_array(starts)
        n = len(arr)
        self._require_device_tensor(tt, (n,) + self.shape, "travel-time boxes")
        pred = self._require_pred(starts, tt, pred)
        recv = self._starts_array(receivers)
        nrays = n * len(recv)
        offsets = torch.zeros(nrays + 1, dtype=torch.int64)
        status = torch.empty(nrays, dtype=torch.int32)
        t_recv = torch.empty(nrays, dtype=torch.float32)
        tptr, pptr = self._box_pointers(tt, n), self._box_pointers(pred, n)
        torch.cuda.current_stream(tt.device).synchronize()

        def call(cells, hop_d, cap):
            return _check(self._L.ttsweep_trace_rays_device(
                self._ctx, n, arr, tptr, pptr, len(recv), recv, offsets.data_ptr(), status.data_ptr(),
                t_recv.data_ptr(), cells, hop_d, cap), "ttsweep_trace_rays_device")

        total = call(None, None, 0)
        cells = torch.empty(total, dtype=torch.int32, device=tt.device)
        hop_d = torch.empty(total, dtype=torch.float32, device=tt.device)
        if total:
            _require(call(cells.data_ptr(), hop_d.data_ptr(), total) == total, "ray count changed between calls")
        return Rays(offsets, cells, hop_d, status, t_recv)

    def frechet_operator(self, starts, tt, receivers=None, pred=None, *, pairs=None) -> "FrechetOperator":
        """The Frechet matrix G of the rays from every start of tt to every receiver, as an operator
        (ttsweep_ray_forward_device / ttsweep_ray_adjoint_device): G m and G^T w without storing a path.
        pred: the result of predecessors() for these boxes (computed once here when None).
        pairs = (pair_box [npair], pair_recv [npair, 3]) instead of receivers: row r is the ray of box pair_box[r]
        from the cell pair_recv[r] (ttsweep_ray_pairs_forward_device / ttsweep_ray_pairs_adjoint_device)."""
        _require((receivers is None) != (pairs is None), "frechet_operator: give receivers or pairs")
        return FrechetOperator(self, starts, tt, receivers, pred, pairs=pairs)

    @staticmethod
    def _pair_arrays(pair_box, pair_recv):
        box = np.ascontiguousarray(np.asarray(pair_box, dtype=np.int32).reshape(-1))
        recv = TravelTimeSolver._starts_array(pair_recv)
        _require(len(box) == len(recv), f"pairs: {len(box)} boxes, {len(recv)} receivers")
        return (C.c_int * max(len(box), 1)).from_buffer_copy(box.tobytes() if len(box) else bytes(4)), recv

    def ray_geometry(self, starts, tt, pair_box, pair_recv, pred=None) -> "RayGeometry":
        """ttsweep_ray_pairs_geometry_device: hop count, length, first and last hop and deepest cell of the ray of
        box pair_box[r] from the cell pair_recv[r], for every pair, without storing a path.  pred: the result of
        predecessors() for these boxes (computed when None)."""
        import torch
        arr = self._starts_array(starts)
        n = len(arr)
        self._require_device_tensor(tt, (n,) + self.shape, "travel-time boxes")
        pred = self._require_pred(starts, tt, pred)
        box, recv = self._pair_arrays(pair_box, pair_recv)
        npair = len(recv)
        dev = tt.device
        new = lambda dtype, *shape: torch.empty((npair,) + shape, dtype=dtype, device=dev)
        out = RayGeometry(
            status=torch.empty(npair, dtype=torch.int32), t_recv=new(torch.float32), hops=new(torch.int32),
            length=new(torch.float64), recv_hop=new(torch.int32, 3), recv_d=new(torch.float32),
            recv_dt=new(torch.float32), src_hop=new(torch.int32, 3), src_d=new(torch.float32),
            src_dt=new(torch.float32), deep=new(torch.int32))
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.ttsweep_ray_pairs_geometry_device(
            self._ctx, n, arr, self._box_pointers(tt, n), self._box_pointers(pred, n), npair, box, recv,
            out.status.data_ptr(), out.t_recv.data_ptr(), out.hops.data_ptr(), out.length.data_ptr(),
            out.recv_hop.data_ptr(), out.recv_d.data_ptr(), out.recv_dt.data_ptr(), out.src_hop.data_ptr(),
            out.src_d.data_ptr(), out.src_dt.data_ptr(), out.deep.data_ptr()), "ttsweep_ray_pairs_geometry_device")
        return out

    # -- fat rays ------------------------------------------------------------
    def _fresnel_args(self, starts, tt, pair_a, pair_b, tau, lo, hi):
        """The shared arguments of the three ttsweep_fresnel_*_device calls as a tuple, checked; the arrays it points
        into are kept alive by the tuple's last entry."""
        arr = self._starts_array(starts)
        n = len(arr)
        _require(n >= 1, "fresnel: at least one box")
        self._require_device_tensor(tt, (n,) + self.shape, "travel-time boxes")
        a = np.ascontiguousarray(np.asarray(pair_a, dtype=np.int32).reshape(-1))
        b = np.ascontiguousarray(np.asarray(pair_b, dtype=np.int32).reshape(-1))
        npair = len(a)
        _require(len(b) == npair, f"pairs: {npair} boxes a, {len(b)} boxes b")
        _require(npair == 0 or (min(a.min(), b.min()) >= 0 and max(a.max(), b.max()) < n),
                 f"pairs: box indices in [0, {n})")
        tau = np.asarray(tau if isinstance(tau, (np.ndarray, list, tuple, float, int)) else _host(tau),
                         dtype=np.float64)
        _require(tau.shape in ((), (npair,)), f"tau: a number or [{npair}] values")
        tau = np.ascontiguousarray(np.broadcast_to(tau, (npair,)))
        lo, hi = self._windows(npair, lo, hi)
        keep = (arr, a, b, tau, lo, hi, tt)
        ptr = lambda x: None if x is None else x.ctypes.data
        return (self._ctx, n, arr, self._box_pointers(tt, n), npair, ptr(a), ptr(b), ptr(tau), ptr(lo), ptr(hi), keep)

    def fresnel_volumes(self, starts, tt, pair_a, pair_b, tau, lo=None, hi=None) -> "FresnelVolumes":
        """ttsweep_fresnel_volume_device: the fat ray (first Fresnel volume) of every pair (box pair_a[r], box
        pair_b[r]) of tt (torch float32 [nbox,nx,ny,nz] on this solver's device, box k solved from starts[k] with a
        symmetric star): the cells whose detour T_a[x] + T_b[x] - T_a[start_b] is below tau[r] (a number or [npair]),
        weighted by the linear taper phi (include/ttsweep.h, "fresnel").  lo, hi: inclusive windows, [3] or
        [npair,3]; both None: the whole grid."""
        import torch
        args = self._fresnel_args(starts, tt, pair_a, pair_b, tau, lo, hi)
        npair, dev = args[4], tt.device
        new = lambda dtype, *shape: torch.empty((npair,) + shape, dtype=dtype, device=dev)
        out = FresnelVolumes(status=torch.empty(npair, dtype=torch.int32), t_ab=new(torch.float32),
                             count=new(torch.int64), phi=new(torch.float64), lo=new(torch.int32, 3),
                             hi=new(torch.int32, 3),
                             start_a=np.frombuffer(args[2], dtype=np.int32).reshape(-1, 3)[args[10][1]])
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.ttsweep_fresnel_volume_device(
            *args[:10], out.status.data_ptr(), out.t_ab.data_ptr(), out.count.data_ptr(), out.lo.data_ptr(),
            out.hi.data_ptr(), out.phi.data_ptr()), "ttsweep_fresnel_volume_device")
        return out

    def fresnel_operator(self, starts, tt, pair_a, pair_b, tau, norm=None, windows=True) -> "FresnelOperator":
        """The fat-ray sensitivity matrix of the pairs as an operator for lsqr: row r is coef[r] * phi_r(x), coef =
        norm / Phi (0 where Phi = 0; norm None: 1), so a row sums to norm[r] - with norm = ray_geometry(...).length
        to the thin ray's length, the unit the rows of frechet_operator carry.  Built from one volume call; windows:
        feed the volumes' bounding boxes back as windows (fewer cells visited, the same bits)."""
        return FresnelOperator(self, starts, tt, pair_a, pair_b, tau, norm=norm, windows=windows)

    # -- event location -----------------------------------------------------
    def locate(self, tt, picks, weights=None, misfit_events=None) -> "Locations":
        """ttsweep_locate_device: grid-search location of events over station boxes (include/ttsweep.h, "locate").
        tt: torch float32 [K,nx,ny,nz] on this solver's device, box k solved from station k.  picks, weights:
        [E,K] float64 torch tensors on that device, or numpy arrays (copied over); weights None: every weight 1.0,
        a zero weight: no pick.  misfit_events: event indices whose misfit volume J is returned as well."""
        import torch
        K, E, dev, picks, weights = self._locate_inputs(tt, picks, weights)
        vev = [] if misfit_events is None else [int(e) for e in misfit_events]
        _require(all(0 <= e < E for e in vev), f"misfit_events: indices in [0, {E})")
        cell = torch.empty(E, dtype=torch.int32, device=dev)
        misfit = torch.empty(E, dtype=torch.float64, device=dev)
        t0 = torch.empty(E, dtype=torch.float64, device=dev)
        vols = torch.empty((len(vev),) + self.shape, dtype=torch.float64, device=dev) if vev else None
        varr = (C.c_int * max(len(vev), 1))(*vev)
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.ttsweep_locate_device(
            self._ctx, K, self._box_pointers(tt, K), E, picks.data_ptr(),
            None if weights is None else weights.data_ptr(), cell.data_ptr(), misfit.data_ptr(), t0.data_ptr(),
            len(vev), varr if vev else None, self._box_pointers(vols, len(vev)) if vev else None),
            "ttsweep_locate_device")
        return Locations(cell, self._cell_xyz(cell), misfit, t0, vols)

    def _locate_inputs(self, tt, picks, weights):
        """(K, E, device, picks, weights) of a locate call, checked: tt [K,nx,ny,nz] float32 on this solver's device,
        picks / weights [E,K] float64 contiguous on it (numpy arrays are copied over; weights may be None)."""
        import torch
        _require(isinstance(tt, torch.Tensor) and tt.dim() == 4, "tt: torch float32 [K, nx, ny, nz]")
        K = int(tt.shape[0])
        self._require_device_tensor(tt, (K,) + self.shape, "station boxes")
        dev = tt.device

        def events_by_stations(a, what):
            if isinstance(a, np.ndarray):
                _require(a.dtype == np.float64, f"{what}: float64")
                a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            _require(isinstance(a, torch.Tensor) and a.dtype == torch.float64 and a.device == dev,
                     f"{what}: float64 tensor on {dev} or numpy array")
            _require(a.dim() == 2 and a.shape[1] == K and a.shape[0] >= 1, f"{what}: shape {tuple(a.shape)}, want [E, {K}]")
            return a.contiguous()

        picks = events_by_stations(picks, "picks")
        E = int(picks.shape[0])
        if weights is not None:
            weights = events_by_stations(weights, "weights")
            _require(tuple(weights.shape) == (E, K), f"weights: shape {tuple(weights.shape)}, want {(E, K)}")
        return K, E, dev, picks, weights

    @staticmethod
    def _windows(E, lo, hi):
        """(lo, hi) of a windowed call as contiguous int32 [E,3], or (None, None): each given as [3] (every event) or
        [E,3] integers, numpy or lists."""
        _require((lo is None) == (hi is None), "lo and hi: both or neither")

        def window(a, what):
            if a is None:
                return None
            a = np.asarray(a)
            _require(a.dtype.kind in "iu" and a.shape in ((3,), (E, 3)), f"{what}: integers, [3] or [{E}, 3]")
            _require(a.size == 0 or (a.min() >= -2**31 and a.max() < 2**31), f"{what}: int32 values")
            return np.ascontiguousarray(np.broadcast_to(a, (E, 3)), dtype=np.int32)

        return window(lo, "lo"), window(hi, "hi")

    def _cell_xyz(self, cell):
        """[E,3] int32 on the host: the FLOATBOX indices as (x, y, z), (-1, -1, -1) for -1."""
        import torch
        c = cell.cpu().to(torch.int64)
        nyz = self.shape[1] * self.shape[2]
        xyz = torch.stack([c // nyz, (c // self.shape[2]) % self.shape[1], c % self.shape[2]], dim=1).to(torch.int32)
        xyz[c < 0] = -1
        return xyz

    def locate_window(self, tt, picks, weights=None, lo=None, hi=None, stride=1) -> "Locations":
        """ttsweep_locate_window_device: the search of locate over a window and a lattice per event (include/ttsweep.h,
        "locate window").  tt, picks, weights as for locate.  lo, hi: the inclusive window as [3] (every event) or
        [E,3] integers, numpy or lists; both None: the whole grid.  stride: an int or [3], >= 1; the lattice is
        anchored at the window's lo.  The candidates of event e are the cells lo[e] + i * stride <= hi[e]; cell is
        the smallest index among those of minimal J.  volumes is None in the result."""
        import torch
        K, E, dev, picks, weights = self._locate_inputs(tt, picks, weights)
        lo, hi = self._windows(E, lo, hi)
        stride = np.asarray(stride)
        _require(stride.dtype.kind in "iu" and stride.shape in ((), (3,)), "stride: an int or [3] integers")
        _require(stride.min() >= -2**31 and stride.max() < 2**31, "stride: int32 values")
        stride = np.ascontiguousarray(np.broadcast_to(stride, (3,)), dtype=np.int32)
        cell = torch.empty(E, dtype=torch.int32, device=dev)
        misfit = torch.empty(E, dtype=torch.float64, device=dev)
        t0 = torch.empty(E, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.ttsweep_locate_window_device(
            self._ctx, K, self._box_pointers(tt, K), E, picks.data_ptr(),
            None if weights is None else weights.data_ptr(), None if lo is None else lo.ctypes.data,
            None if hi is None else hi.ctypes.data, stride.ctypes.data, cell.data_ptr(), misfit.data_ptr(),
            t0.data_ptr()), "ttsweep_locate_window_device")
        return Locations(cell, self._cell_xyz(cell), misfit, t0, None)

    def locate_refine(self, tt, picks, weights=None, stride=4, radius=None) -> "Locations":
        """Coarse-to-fine location in two calls of locate_window.  Stage 1 searches the whole grid on the lattice of
        `stride` (an int or [3]) anchored at cell (0, 0, 0).  Stage 2 searches with stride 1, in one call for all
        events: the window xyz +- radius around the stage-1 cell, clipped to the grid, for an event stage 1 placed;
        the whole grid (which is exact) for an event whose lattice nodes are all inadmissible.  radius: an int or
        [3], default the stride per axis, so that the cells past the last lattice node are covered.

        NOT exact: the refined cell is locate's global minimum only where the basin of the misfit's minimum holds
        the window of a lattice node, i.e. where the best lattice node lies within `radius` of the best cell.  By
        construction misfit <= coarse_misfit (the lattice node is inside its window) and misfit >= locate's misfit.
        The result carries the stage-2 outputs, and coarse_cell / coarse_misfit of stage 1."""
        n = np.asarray(self.shape, dtype=np.int64)
        stride = np.broadcast_to(np.asarray(stride), (3,))
        radius = stride if radius is None else np.broadcast_to(np.asarray(radius), (3,))
        _require(radius.dtype.kind in "iu" and radius.min() >= 0, "radius: a non-negative int or [3] integers")
        _, _, _, picks, weights = self._locate_inputs(tt, picks, weights)       # copied to the device once
        coarse = self.locate_window(tt, picks, weights, lo=np.zeros(3, np.int64), hi=n - 1, stride=stride)
        xyz = coarse.xyz.numpy().astype(np.int64)
        placed = (xyz[:, 0] >= 0)[:, None]
        lo = np.where(placed, np.maximum(xyz - radius, 0), 0)
        hi = np.where(placed, np.minimum(xyz + radius, n - 1), n - 1)
        fine = self.locate_window(tt, picks, weights, lo=lo, hi=hi, stride=1)
        fine.coarse_cell, fine.coarse_misfit = coarse.cell, coarse.misfit
        return fine

    def locate_subcell(self, tt, picks, weights=None, lo=None, hi=None, sub=8) -> "SubcellLocations":
        """ttsweep_locate_subcell_device: the search of locate over the nodes of a lattice of `sub` steps per cell edge
        inside a window of cells, the station times interpolated trilinearly (include/ttsweep.h, "locate subcell").
        tt, picks, weights as for locate.  lo, hi: the inclusive window in cells as [3] (every event) or [E,3]
        integers; both None: the whole grid.  sub: 1..64.  Node q stands for the position q / sub in cells."""
        import torch
        K, E, dev, picks, weights = self._locate_inputs(tt, picks, weights)
        lo, hi = self._windows(E, lo, hi)
        _require(isinstance(sub, (int, np.integer)) and -2**31 <= sub < 2**31, "sub: an int")
        node = torch.empty((E, 3), dtype=torch.int32, device=dev)
        misfit = torch.empty(E, dtype=torch.float64, device=dev)
        t0 = torch.empty(E, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.ttsweep_locate_subcell_device(
            self._ctx, K, self._box_pointers(tt, K), E, picks.data_ptr(),
            None if weights is None else weights.data_ptr(), None if lo is None else lo.ctypes.data,
            None if hi is None else hi.ctypes.data, int(sub), node.data_ptr(), misfit.data_ptr(), t0.data_ptr()),
            "ttsweep_locate_subcell_device")
        q = node.cpu().numpy()
        position = np.where(q < 0, np.nan, q.astype(np.float64) / float(sub))
        return SubcellLocations(node, int(sub), position, misfit, t0)

    def locate_fine(self, tt, picks, weights=None, sub=8, radius=1, cells=None) -> "SubcellLocations":
        """Sub-cell location around the best cell: locate_subcell on the window cell +- radius (an int or [3]), clipped
        to the grid.  cells: int32 [E] FLOATBOX indices of an earlier search (locate, locate_window, locate_refine),
        numpy or on the device, -1 for an event it did not place; None: locate is run here.  An event with cell -1
        gets the window of cell (0, 0, 0) alone and stays unplaced, which is exact: no cell is admissible for it, every
        node has its base cell as a corner, so no node is admissible either.  The result carries cell and cell_misfit
        of the first stage (cell_misfit is None when cells was given); the cell is inside its window, so
        misfit <= its misfit."""
        n = np.asarray(self.shape, dtype=np.int64)
        radius = np.broadcast_to(np.asarray(radius), (3,))
        _require(radius.dtype.kind in "iu" and radius.min() >= 0, "radius: a non-negative int or [3] integers")
        _, E, _, picks, weights = self._locate_inputs(tt, picks, weights)       # copied to the device once
        cell_misfit = None
        if cells is None:
            first = self.locate(tt, picks, weights)
            cells, cell_misfit = first.cell, first.misfit
        c = _host(cells)
        _require(c.dtype.kind in "iu" and c.shape == (E,), f"cells: integers [{E}]")
        c = c.astype(np.int64)
        _require(c.min() >= -1 and c.max() < int(np.prod(n)), "cells: FLOATBOX indices of this grid, or -1")
        placed = (c >= 0)[:, None]
        xyz = np.stack(np.unravel_index(np.maximum(c, 0), self.shape), 1).astype(np.int64)
        lo = np.where(placed, np.maximum(xyz - radius, 0), 0)
        hi = np.where(placed, np.minimum(xyz + radius, n - 1), 0)
        fine = self.locate_subcell(tt, picks, weights, lo=lo, hi=hi, sub=sub)
        fine.cell, fine.cell_misfit = cells, cell_misfit
        return fine

    def locate_confidence(self, tt, picks, weights, misfit, delta) -> "ConfidenceRegions":
        """ttsweep_locate_confidence_device: per event and level the region of admissible cells with
        J <= misfit[e] + delta[e, l], summarised without a misfit volume (include/ttsweep.h, "locate confidence").
        tt, picks, weights as for locate (weights None: every weight 1.0).  misfit: float64 [E] on the device or
        numpy, normally Locations.misfit.  delta: a scalar, [L] or [E, L] (1 <= L <= 4), broadcast to [E, L]
        float64; inf is allowed (every admissible cell)."""
        import torch
        _require(isinstance(tt, torch.Tensor) and tt.dim() == 4, "tt: torch float32 [K, nx, ny, nz]")
        K = int(tt.shape[0])
        self._require_device_tensor(tt, (K,) + self.shape, "station boxes")
        dev = tt.device

        def on_device(a, what):
            if isinstance(a, np.ndarray):
                _require(a.dtype == np.float64, f"{what}: float64")
                a = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            _require(isinstance(a, torch.Tensor) and a.dtype == torch.float64 and a.device == dev,
                     f"{what}: float64 tensor on {dev} or numpy array")
            return a.contiguous()

        picks = on_device(picks, "picks")
        _require(picks.dim() == 2 and picks.shape[1] == K and picks.shape[0] >= 1,
                 f"picks: shape {tuple(picks.shape)}, want [E, {K}]")
        E = int(picks.shape[0])
        if weights is not None:
            weights = on_device(weights, "weights")
            _require(tuple(weights.shape) == (E, K), f"weights: shape {tuple(weights.shape)}, want {(E, K)}")
        misfit = on_device(misfit, "misfit")
        _require(tuple(misfit.shape) == (E,), f"misfit: shape {tuple(misfit.shape)}, want {(E,)}")
        if not isinstance(delta, torch.Tensor):
            delta = np.atleast_1d(np.asarray(delta, dtype=np.float64))
        delta = on_device(delta, "delta")
        if delta.dim() < 2:
            delta = delta.reshape(1, -1)
        _require(delta.dim() == 2 and 1 <= delta.shape[1] <= 4 and delta.shape[0] in (1, E),
                 f"delta: shape {tuple(delta.shape)}, want a scalar, [L] or [{E}, L] with 1 <= L <= 4")
        L = int(delta.shape[1])
        delta = delta.expand(E, L).contiguous()

        def out(dtype, *tail):
            return torch.empty((E, L) + tail, dtype=dtype, device=dev)

        r = ConfidenceRegions(out(torch.int64), out(torch.int64, 3), out(torch.int64, 6), out(torch.int32, 3),
                              out(torch.int32, 3), out(torch.float64), out(torch.float64), self.shape)
        torch.cuda.current_stream(dev).synchronize()
        _check(self._L.ttsweep_locate_confidence_device(
            self._ctx, K, self._box_pointers(tt, K), E, picks.data_ptr(),
            None if weights is None else weights.data_ptr(), misfit.data_ptr(), L, delta.data_ptr(),
            r.count.data_ptr(), r.sum.data_ptr(), r.sum2.data_ptr(), r.lo.data_ptr(), r.hi.data_ptr(),
            r.t0_lo.data_ptr(), r.t0_hi.data_ptr()), "ttsweep_locate_confidence_device")
        return r

    def stats(self) -> dict:
        st = Stats()
        _check(self._L.ttsweep_get_stats(self._ctx, C.byref(st)), "ttsweep_get_stats")
        return {name: getattr(st, name) for name, _ in Stats._fields_}


@dataclass
class Rays:
    """Rays of TravelTimeSolver.trace_rays; ray r = s * nrecv + q (start s, receiver q).
      offsets [nrays + 1] int64 (host): ray r's cells are cells[offsets[r]:offsets[r + 1]]
      cells   int32 (device): FLOATBOX indices of the path, source -> receiver
      hop_d   float32 (device), aligned with cells: star length of the hop to the next cell, 0 at a ray's last cell
      status  [nrays] int32 (host): RAY_OK / RAY_SEED / RAY_UNREACHED / RAY_INVALID
      t_recv  [nrays] float32 (host): the travel time at the receiver"""
    offsets: "object"
    cells: "object"
    hop_d: "object"
    status: "object"
    t_recv: "object"

    def __len__(self):
        return len(self.status)


@dataclass
class RayGeometry:
    """Geometry of the rays of TravelTimeSolver.ray_geometry (include/ttsweep.h, "rays: pair lists"), one row per
    (box, receiver) pair; hops run in walk order, receiver -> source.  status is on the host, the rest on the device.
      status   [npair] int32: RAY_OK / RAY_SEED / RAY_UNREACHED / RAY_INVALID
      t_recv   [npair] float32: the travel time at the receiver
      hops     [npair] int32: hops of the path; 0 for an UNREACHED or INVALID ray
      length   [npair] float64: the sum of the hops' star lengths d
      recv_hop [npair,3] int32, recv_d, recv_dt [npair] float32: offset, d and time difference of the hop out of the
               receiver (pointing towards the source)
      src_hop  [npair,3] int32, src_d, src_dt [npair] float32: the same of the hop out of the source
      deep     [npair] int32: FLOATBOX index of the path cell with the greatest z, -1 for an UNREACHED or INVALID ray"""
    status: "object"
    t_recv: "object"
    hops: "object"
    length: "object"
    recv_hop: "object"
    recv_d: "object"
    recv_dt: "object"
    src_hop: "object"
    src_d: "object"
    src_dt: "object"
    deep: "object"

    def __len__(self):
        return len(self.status)

    def receiver_gradient(self):
        """float64 [npair, 3]: (double)recv_dt * recv_hop[a] / (recv_hop . recv_hop), the travel time gained per cell
        moved away from the source along axis a at the receiver (minus the slope of T along the first hop: the
        partials of a hypocentre at the receiver cell); 0 for a ray without a hop."""
        import torch
        h = self.recv_hop.to(torch.float64)
        n2 = (h * h).sum(dim=1, keepdim=True)
        g = self.recv_dt.to(torch.float64)[:, None] * h / n2
        return torch.where(n2 > 0, g, torch.zeros_like(g))

    def takeoff(self):
        """float64 [npair, 3]: the unit vector of src_hop, the direction in which the ray leaves the source, in
        cells; 0 for a ray without a hop."""
        import torch
        h = self.src_hop.to(torch.float64)
        n2 = (h * h).sum(dim=1, keepdim=True)
        u = h / torch.sqrt(n2)
        return torch.where(n2 > 0, u, torch.zeros_like(u))


def pairs_from_locations(cells, weights=None, nstations=None):
    """The (box, receiver) pairs of located events for TravelTimeSolver.frechet_operator(pairs=...) and
    ray_geometry: the pair (k, cell[e]) of every (e, k) with weights[e][k] != 0 and an event cell, in (e, k) order.
    cells: a Locations, or [E, 3] integer cells (x, y, z) with a negative row for an event without a cell.  weights:
    [E, K] numpy or torch, None: every one of nstations stations is picked.  Returns numpy arrays
    (pair_box int32 [npair], pair_recv int32 [npair, 3], event_of_pair int64, station_of_pair int64): with them the
    residuals o[event_of_pair, station_of_pair] - t0[event_of_pair] - t_recv line up with the operator's rows."""
    xyz = np.asarray(_host(cells.xyz if isinstance(cells, Locations) else cells)).reshape(-1, 3)
    if weights is None:
        _require(nstations is not None, "pairs_from_locations: weights or nstations")
        picked = np.ones((len(xyz), int(nstations)), dtype=bool)
    else:
        picked = np.asarray(_host(weights)) != 0
        _require(picked.ndim == 2 and len(picked) == len(xyz), "pairs_from_locations: weights [E, K], cells [E, 3]")
    picked = picked & np.all(xyz >= 0, axis=1)[:, None]
    event, station = np.nonzero(picked)         # row-major: (e, k) order
    return (station.astype(np.int32), np.ascontiguousarray(xyz[event], dtype=np.int32), event.astype(np.int64),
            station.astype(np.int64))


@dataclass
class Locations:
    """Events located by TravelTimeSolver.locate (include/ttsweep.h, "locate"), E events.
      cell    [E] int32 (device): FLOATBOX index of the best cell, -1 when no cell is admissible
      xyz     [E,3] int32 (host): the cell as (x, y, z), (-1, -1, -1) when there is none
      misfit  [E] float64 (device): the weighted L2 misfit J at the cell, +inf when there is none
      t0      [E] float64 (device): the origin time at the cell, NaN when there is none
      volumes [nvol,nx,ny,nz] float64 (device) or None: J of every cell for misfit_events, +inf where inadmissible
    locate_window fills the same fields over its candidates (volumes None); locate_refine adds
      coarse_cell, coarse_misfit [E] int32 / float64 (device): cell and misfit of its stage 1 on the lattice"""
    cell: "object"
    xyz: "object"
    misfit: "object"
    t0: "object"
    volumes: "object"
    coarse_cell: "object" = None
    coarse_misfit: "object" = None

    def __len__(self):
        return len(self.cell)


@dataclass
class SubcellLocations:
    """Events located by TravelTimeSolver.locate_subcell (include/ttsweep.h, "locate subcell"), E events.
      node     [E,3] int32 (device): the best node (qx, qy, qz), (-1, -1, -1) when no node is admissible
      sub      lattice steps per cell edge
      position [E,3] float64 (host): node / sub, the hypocentre in cells; NaN rows where node is -1
      misfit   [E] float64 (device): J at the node, +inf when there is none
      t0       [E] float64 (device): the origin time at the node, NaN when there is none
    locate_fine adds
      cell, cell_misfit: cell ([E] int32) and misfit ([E] float64, device) of the first stage; cell_misfit is None
      when the cells were given by the caller"""
    node: "object"
    sub: int
    position: "object"
    misfit: "object"
    t0: "object"
    cell: "object" = None
    cell_misfit: "object" = None

    def __len__(self):
        return len(self.node)


def _host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


@dataclass
class ConfidenceRegions:
    """Regions of TravelTimeSolver.locate_confidence (include/ttsweep.h, "locate confidence"), E events, L levels:
    the admissible cells with J <= misfit[e] + delta[e, l].  All on the device.
      count        [E,L] int64: cells in the region
      sum          [E,L,3] int64: sum of x, y, z over it
      sum2         [E,L,6] int64: sum of xx, yy, zz, xy, xz, yz
      lo, hi       [E,L,3] int32: its bounding box, inclusive; (nx, ny, nz) and (-1, -1, -1) when empty
      t0_lo, t0_hi [E,L] float64: the range of the origin time over it; +inf and -inf when empty
      shape        (nx, ny, nz) of the grid
    centroid(), covariance() and open() are computed on the host in float64 (numpy)."""
    count: "object"
    sum: "object"
    sum2: "object"
    lo: "object"
    hi: "object"
    t0_lo: "object"
    t0_hi: "object"
    shape: tuple

    def __len__(self):
        return len(self.count)

    def centroid(self):
        """[E,L,3] float64: sum / count in cells, the sub-cell hypocentre estimate; NaN where the region is empty."""
        n = _host(self.count).astype(np.float64)[..., None]
        with np.errstate(invalid="ignore", divide="ignore"):
            return _host(self.sum).astype(np.float64) / n

    def covariance(self):
        """[E,L,3,3] float64 in cells^2: (sum_ab - sum_a * (sum_b / n)) / n, each operation rounded once; symmetric
        (an off-diagonal pair is computed once); NaN where the region is empty."""
        n = _host(self.count).astype(np.float64)
        s = _host(self.sum).astype(np.float64)
        q = _host(self.sum2).astype(np.float64)
        cov = np.empty(n.shape + (3, 3))
        with np.errstate(invalid="ignore", divide="ignore"):
            for i, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
                cov[..., a, b] = cov[..., b, a] = (q[..., i] - s[..., a] * (s[..., b] / n)) / n
        return cov

    def open(self):
        """[E,L] bool: the bounding box touches a face of the grid, so the region is cut off by the model boundary
        and its statistics understate the uncertainty.  False where the region is empty."""
        lo, hi = _host(self.lo), _host(self.hi)
        top = np.asarray(self.shape, dtype=lo.dtype) - 1
        return (_host(self.count) > 0) & np.any((lo == 0) | (hi == top), axis=-1)


class _CellOperator:
    """What FrechetOperator and FresnelOperator share: an operator [nrows, nx*ny*nz] whose adjoint is one call of the
    C ABI that sums in int64 fixed point.  A subclass sets shape, grid, device and last_scale, and supplies
    _adjoint_call(w, g, hits, scale) (the C call on device pointers or None; returns (rc, the call's name)) and, where
    its rows carry coefficients, _row_weights(w)."""

    def _cells(self, t, what):
        import torch
        _require(isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == self.device,
                 f"{what}: float64 tensor on {self.device}")
        _require(t.numel() == self.shape[1] and tuple(t.shape) in ((self.shape[1],), self.grid),
                 f"{what}: shape {tuple(t.shape)}, want {self.grid} or ({self.shape[1]},)")
        return t.contiguous()

    def _row_weights(self, w):
        return w

    def _adjoint(self, w, hits):
        import torch
        scale = C.c_int(0)
        g = None
        if w is not None:
            _require(isinstance(w, torch.Tensor) and w.dtype == torch.float64 and w.device == self.device
                     and tuple(w.shape) == (self.shape[0],), f"w: float64 [{self.shape[0]}] on {self.device}")
            w = self._row_weights(w).contiguous()
            g = torch.empty(self.grid, dtype=torch.float64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        ptr = lambda t: None if t is None else t.data_ptr()
        _check(*self._adjoint_call(ptr(w), ptr(g), ptr(hits), C.byref(scale)))
        if w is not None:
            self.last_scale = scale.value
        return g

    def rmatvec(self, w):
        """A^T w (FresnelOperator: F^T (coef * w)): w float64 [nrows] on the device; float64 [nx,ny,nz], deterministic
        (int64 fixed point)."""
        return self._adjoint(w, None)

    def rmatvec_hits(self, w):
        """(rmatvec(w), hits) of one walk of the rays, or one pass over the pairs."""
        import torch
        hits = torch.empty(self.grid, dtype=torch.int32, device=self.device)
        return self._adjoint(w, hits), hits

    def hits(self):
        """int32 [nx,ny,nz]: the number of OK or SEED rays whose path holds each cell (FresnelOperator: of pairs whose
        volume holds it)."""
        import torch
        hits = torch.empty(self.grid, dtype=torch.int32, device=self.device)
        self._adjoint(None, hits)
        return hits


class FrechetOperator(_CellOperator):
    """G [nrays, nx*ny*nz] of TravelTimeSolver.trace_rays + rays_to_frechet, applied by walking the rays on the
    device instead of storing them (TravelTimeSolver.frechet_operator).  Holds the solver, the boxes, pred and
    the start and receiver lists as C arrays (built once); the boxes and pred must not change while it is used.
      shape      (nrays, ncells); ray r = s * nrecv + q, or pair r of a pair list
      status     [nrays] int32 (host): RAY_OK / RAY_SEED / RAY_UNREACHED / RAY_INVALID
      t_recv     [nrays] float32 (host): the travel time at the receiver
      last_scale S of the last rmatvec: g is summed in units of 2^-S (include/ttsweep.h)"""

    def __init__(self, solver, starts, tt, receivers, pred=None, pairs=None):
        import torch
        self._sol = solver
        self._starts = solver._starts_array(starts)
        n = len(self._starts)
        solver._require_device_tensor(tt, (n,) + solver.shape, "travel-time boxes")
        pred = solver._require_pred(starts, tt, pred)
        self.tt, self.pred = tt, pred
        self._tptr, self._pptr = solver._box_pointers(tt, n), solver._box_pointers(pred, n)
        self.grid = solver.shape
        self.device = tt.device
        self.last_scale = 0
        L = solver._L
        if pairs is None:
            self._recv = solver._starts_array(receivers)
            nrays = n * len(self._recv)
            self._rays = (n, self._starts, self._tptr, self._pptr, len(self._recv), self._recv)
            self._calls = (L.ttsweep_ray_forward_device, "ttsweep_ray_forward_device",
                           L.ttsweep_ray_adjoint_device, "ttsweep_ray_adjoint_device")
        else:
            self._pair_box, self._recv = solver._pair_arrays(*pairs)
            nrays = len(self._recv)
            self._rays = (n, self._starts, self._tptr, self._pptr, nrays, self._pair_box, self._recv)
            self._calls = (L.ttsweep_ray_pairs_forward_device, "ttsweep_ray_pairs_forward_device",
                           L.ttsweep_ray_pairs_adjoint_device, "ttsweep_ray_pairs_adjoint_device")
        self._nstart = n
        self.shape = (nrays, int(np.prod(solver.shape)))
        self.status = torch.empty(nrays, dtype=torch.int32)
        # the first forward call checks the rays (a box index or a receiver outside its range is refused there)
        self._forward(torch.zeros(self.shape[1], dtype=torch.float64, device=self.device), self.status)
        recv = torch.from_numpy(np.frombuffer(self._recv, dtype=np.int32).reshape(-1, 3).astype(np.int64))
        flat = ((recv[:, 0] * self.grid[1] + recv[:, 1]) * self.grid[2] + recv[:, 2]).to(tt.device)
        if pairs is None:
            self.t_recv = tt.reshape(n, -1)[:, flat].reshape(-1).cpu()
        else:
            box = torch.from_numpy(np.frombuffer(self._pair_box, dtype=np.int32)[:nrays].astype(np.int64))
            self.t_recv = tt.reshape(n, -1)[box.to(tt.device), flat].cpu()

    def _forward(self, m, status=None):
        import torch
        y = torch.empty(self.shape[0], dtype=torch.float64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        _check(self._calls[0](self._sol._ctx, *self._rays, m.data_ptr(), y.data_ptr(),
                              None if status is None else status.data_ptr()), self._calls[1])
        return y

    def matvec(self, m):
        """G m: m float64 [nx,ny,nz] or [ncells] on the device; float64 [nrays]."""
        return self._forward(self._cells(m, "m"))

    def _adjoint_call(self, w, g, hits, scale):
        return self._calls[2](self._sol._ctx, *self._rays, w, g, hits, scale), self._calls[3]


@dataclass
class FresnelVolumes:
    """Volumes of TravelTimeSolver.fresnel_volumes (include/ttsweep.h, "fresnel"), one entry per pair.
      status  [npair] int32 (host): FRESNEL_OK / FRESNEL_UNREACHED
      t_ab    [npair] float32 (device): T_a at the start of box b
      count   [npair] int64 (device): cells with phi > 0
      phi     [npair] float64 (device): the sum of phi over them (int64 fixed point, deterministic)
      lo, hi  [npair,3] int32 (device): their bounding box; (nx, ny, nz) and (-1, -1, -1) for an empty pair
      start_a [npair,3] int32 (host): the start cell of box a of every pair"""
    status: "object"
    t_ab: "object"
    count: "object"
    phi: "object"
    lo: "object"
    hi: "object"
    start_a: "object"

    def __len__(self):
        return len(self.status)

    def windows(self):
        """(lo, hi) int32 [npair,3] on the host, valid as windows of the fresnel calls: the bounding boxes, an empty
        pair collapsed to the start cell of its box a."""
        lo, hi = _host(self.lo).copy(), _host(self.hi).copy()
        empty = _host(self.count) == 0
        lo[empty] = hi[empty] = self.start_a[empty]
        return lo, hi


class FresnelOperator(_CellOperator):
    """F [npair, nx*ny*nz] with F[r, x] = coef[r] * phi_r(x), applied by streaming the two boxes of every pair on the
    device (TravelTimeSolver.fresnel_operator); lsqr takes it as it is.  The boxes must not change while it is used.
      shape      (npair, ncells)
      status     [npair] int32 (host): FRESNEL_OK / FRESNEL_UNREACHED
      volumes    the FresnelVolumes of the one volume call it was built from
      coef       [npair] float64 (device): norm / Phi, 0 where Phi = 0
      last_scale S_w of the last rmatvec, last_forward_scale S_m of the last matvec (include/ttsweep.h)"""

    def __init__(self, solver, starts, tt, pair_a, pair_b, tau, norm=None, windows=True):
        import torch
        self._sol = solver
        self.volumes = solver.fresnel_volumes(starts, tt, pair_a, pair_b, tau)
        lo, hi = self.volumes.windows() if windows else (None, None)
        self._args = solver._fresnel_args(starts, tt, pair_a, pair_b, tau, lo, hi)
        npair = self._args[4]
        self.tt, self.grid, self.device = tt, solver.shape, tt.device
        self.shape = (npair, int(np.prod(solver.shape)))
        self.status = self.volumes.status
        phi = self.volumes.phi
        if norm is None:
            norm = torch.ones(npair, dtype=torch.float64, device=self.device)
        elif not isinstance(norm, torch.Tensor):
            norm = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(norm, dtype=np.float64), (npair,))))
        norm = norm.to(device=self.device, dtype=torch.float64)
        _require(tuple(norm.shape) == (npair,), f"norm: [{npair}] values")
        self.coef = torch.where(phi > 0, norm / phi, torch.zeros_like(phi))
        self.last_scale = 0
        self.last_forward_scale = 0

    def forward_raw(self, m):
        """y = F m without the row coefficients: ttsweep_fresnel_forward_device as it is."""
        import torch
        m = self._cells(m, "m")
        y = torch.empty(self.shape[0], dtype=torch.float64, device=self.device)
        scale = C.c_int(0)
        torch.cuda.current_stream(self.device).synchronize()
        _check(self._sol._L.ttsweep_fresnel_forward_device(*self._args[:10], m.data_ptr(), y.data_ptr(), None,
                                                           C.byref(scale)), "ttsweep_fresnel_forward_device")
        self.last_forward_scale = scale.value
        return y

    def matvec(self, m):
        """coef * (F m): m float64 [nx,ny,nz] or [ncells] on the device; float64 [npair]."""
        return self.coef * self.forward_raw(m)

    def _row_weights(self, w):
        return self.coef * w

    def _adjoint_call(self, w, g, hits, scale):
        return (self._sol._L.ttsweep_fresnel_adjoint_device(*self._args[:10], w, g, hits, None, scale),
                "ttsweep_fresnel_adjoint_device")


def lsqr(A, b, damp=0.0, atol=1e-8, btol=1e-8, iter_lim=None):
    """Paige & Saunders' LSQR for min ||A x - b||^2 + damp^2 ||x||^2, in float64 torch on b's device, for any A
    with .shape, .matvec(x) and .rmatvec(y) (a FrechetOperator, or a matrix wrapped on the CPU).  Stops as
    scipy.sparse.linalg.lsqr does (istop 1, 2 on btol / atol; 4, 5 at machine precision; 7 at iter_lim, default
    2 * ncols; no condition-number limit).  Returns
    (x [ncols], istop, itn, r1norm)."""
    import torch
    m, n = A.shape
    dev = b.device
    b = b.to(torch.float64).reshape(-1)
    iter_lim = 2 * n if iter_lim is None else iter_lim
    eps = float(np.finfo(np.float64).eps)
    x = torch.zeros(n, dtype=torch.float64, device=dev)
    u = b.clone()
    beta = float(torch.linalg.vector_norm(u))
    bnorm = beta
    if beta > 0:
        u = u / beta
        v = A.rmatvec(u).reshape(-1)
        alfa = float(torch.linalg.vector_norm(v))
    else:
        v = torch.zeros(n, dtype=torch.float64, device=dev)
        alfa = 0.0
    if alfa > 0:
        v = v / alfa
    wv = v.clone()
    rhobar, phibar = alfa, beta
    anorm, ddnorm, res2, xxnorm, z, cs2, sn2 = 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0
    rnorm, r1norm, arnorm = beta, beta, alfa * beta
    itn, istop = 0, 0
    if arnorm == 0:
        return x, 0, 0, r1norm
    while itn < iter_lim:
        itn += 1
        u = A.matvec(v).reshape(-1) - alfa * u
        beta = float(torch.linalg.vector_norm(u))
        if beta > 0:
            u = u / beta
            anorm = (anorm ** 2 + alfa ** 2 + beta ** 2 + damp ** 2) ** 0.5
            v = A.rmatvec(u).reshape(-1) - beta * v
            alfa = float(torch.linalg.vector_norm(v))
            if alfa > 0:
                v = v / alfa
        rhobar1 = (rhobar ** 2 + damp ** 2) ** 0.5
        cs1, sn1 = rhobar / rhobar1, damp / rhobar1
        psi = sn1 * phibar
        phibar = cs1 * phibar
        rho = (rhobar1 ** 2 + beta ** 2) ** 0.5
        cs, sn = rhobar1 / rho, beta / rho
        theta = sn * alfa
        rhobar = -cs * alfa
        phi = cs * phibar
        phibar = sn * phibar
        tau = sn * phi
        t1, t2 = phi / rho, -theta / rho
        dk = wv / rho
        x = x + t1 * wv
        wv = v + t2 * wv
        ddnorm += float(torch.linalg.vector_norm(dk)) ** 2
        delta = sn2 * rho
        gambar = -cs2 * rho
        rhs = phi - delta * z
        zbar = rhs / gambar
        xnorm = (xxnorm + zbar ** 2) ** 0.5
        gamma = (gambar ** 2 + theta ** 2) ** 0.5
        cs2, sn2 = gambar / gamma, theta / gamma
        z = rhs / gamma
        xxnorm += z ** 2
        res1 = phibar ** 2
        res2 += psi ** 2
        rnorm = (res1 + res2) ** 0.5
        arnorm = alfa * abs(tau)
        r1sq = rnorm ** 2 - damp ** 2 * xxnorm
        r1norm = abs(r1sq) ** 0.5 * (-1 if r1sq < 0 else 1)
        test1 = rnorm / bnorm
        test2 = arnorm / (anorm * rnorm + eps)
        rtol = btol + atol * anorm * xnorm / bnorm
        if 1 + test2 <= 1:
            istop = 5
        if 1 + test1 / (1 + anorm * xnorm / bnorm) <= 1:
            istop = 4
        if test2 <= atol:
            istop = 2
        if test1 <= rtol:
            istop = 1
        if istop:
            break
    if not istop and itn >= iter_lim:
        istop = 7
    return x, istop, itn, r1norm


def rays_to_frechet(rays: Rays, v_shape, dtype=None):
    """Frechet (sensitivity) matrix of the discrete rays: a torch.sparse_coo_tensor [nrays, nx*ny*nz] on the
    rays' device in which every hop of length d between cells a and b adds d / 2 at (ray, a) and at (ray, b):
    the delay d (v[a] + v[b]) / 2 is linear in v, so G @ v is the sum of a ray's delays (t_recv for an OK ray,
    t_recv - T[path[0]] for a SEED ray) and G is dt/dv of the path.  dtype: default torch.float64."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    ncells = int(np.prod([int(n) for n in v_shape]))
    dev = rays.cells.device
    offsets = rays.offsets.to(dev)
    nrays = len(offsets) - 1
    counts = offsets[1:] - offsets[:-1]
    row = torch.repeat_interleave(torch.arange(nrays, device=dev), counts)
    half = rays.hop_d.to(dtype) / 2
    cells = rays.cells.to(torch.int64)
    # hop g -> g + 1 for every position g but a ray's last
    last = torch.zeros(len(cells), dtype=torch.bool, device=dev)
    last[offsets[1:][counts > 0] - 1] = True
    g = torch.nonzero(~last).flatten()
    rows = torch.cat([row[g], row[g]])
    cols = torch.cat([cells[g], cells[g + 1]])
    vals = torch.cat([half[g], half[g]])
    return torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (nrays, ncells)).coalesce()


def solve_multi(devices, v: np.ndarray, fs: np.ndarray, starts, tt_boxes, starstart: int = 0,
                starstop: int | None = None, changed: list | None = None) -> int:
    """ttsweep_solve_multi[_changed]: shard the starts, balanced by cost, over `devices` (host boxes).
    changed: a list that receives the per-start outcome (serial_new/...:158-164: changed[s])."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    fs = np.ascontiguousarray(fs, dtype=FS_DTYPE)
    if starstop is None:
        starstop = len(fs) - 1
    arr = TravelTimeSolver._starts_array(starts)
    _require(len(tt_boxes) == len(arr), "one box per start")
    ptrs = (C.c_void_p * len(arr))()
    for s, box in enumerate(tt_boxes):
        _require(box.dtype == np.float32 and box.flags["C_CONTIGUOUS"] and box.shape == v.shape,
                 f"box {s}: float32, C order, shape of the velocity volume")
        ptrs[s] = box.ctypes.data
    dev = (C.c_int * len(devices))(*devices)
    nx, ny, nz = v.shape
    if changed is not None:
        out = (C.c_int * len(arr))()
        rc = _check(_lib.lib().ttsweep_solve_multi_changed(len(devices), dev, nx, ny, nz, fs.ctypes.data,
                                                           starstart, starstop, v.ctypes.data, len(arr), arr,
                                                           ptrs, out), "ttsweep_solve_multi_changed")
        changed[:] = list(out)
        return rc
    return _check(_lib.lib().ttsweep_solve_multi(len(devices), dev, nx, ny, nz, fs.ctypes.data,
                                                 starstart, starstop, v.ctypes.data, len(arr), arr,
                                                 ptrs), "ttsweep_solve_multi")


def sweepXYZ(v: np.ndarray, tt: np.ndarray, fs: np.ndarray, start, starstart: int = 0,
             starstop: int | None = None) -> int:
    """The one-call drop-in (ttsweep_sweepXYZ): converge `tt` in place on device 0."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    fs = np.ascontiguousarray(fs, dtype=FS_DTYPE)
    _require(tt.dtype == np.float32 and tt.flags["C_CONTIGUOUS"] and tt.shape == v.shape,
             "tt: float32, C order, shape of the velocity volume")
    if starstop is None:
        starstop = len(fs) - 1
    nx, ny, nz = v.shape
    return _check(_lib.lib().ttsweep_sweepXYZ(v.ctypes.data, tt.ctypes.data, nx, ny, nz,
                                              fs.ctypes.data, starstart, starstop,
                                              int(start[0]), int(start[1]), int(start[2])),
                  "ttsweep_sweepXYZ")


MULTI_LOOPBACK, MULTI_NO_RCCL = 1, 2
GATHER_NONE, GATHER_RCCL, GATHER_PEER = 0, 1, 2


def solve_multi_device(devices, v: np.ndarray, fs: np.ndarray, starts, tt_root, starstart: int = 0,
                       starstop: int | None = None, flags: int = 0):
    """ttsweep_solve_multi_device: shard the starts over `devices`, solve in HBM, gather the boxes on
    devices[0] into tt_root (torch float32 tensor [nstart, nx, ny, nz] on that device).  Returns
    (rc, changed per start, gather path)."""
    import torch
    v = np.ascontiguousarray(v, dtype=np.float32)
    fs = np.ascontiguousarray(fs, dtype=FS_DTYPE)
    if starstop is None:
        starstop = len(fs) - 1
    arr = TravelTimeSolver._starts_array(starts)
    n = len(arr)
    _require(tt_root.is_cuda and tt_root.dtype == torch.float32 and tt_root.is_contiguous()
             and tuple(tt_root.shape) == (n,) + tuple(v.shape) and tt_root.device.index == devices[0],
             "tt_root: contiguous float32 [nstart, nx, ny, nz] on devices[0]")
    ptrs = (C.c_void_p * n)()
    for s in range(n):
        ptrs[s] = tt_root.data_ptr() + s * tt_root.stride(0) * 4
    dev = (C.c_int * len(devices))(*devices)
    changed = (C.c_int * max(n, 1))()
    path = C.c_int(0)
    nx, ny, nz = v.shape
    torch.cuda.synchronize(tt_root.device)
    rc = _check(_lib.lib().ttsweep_solve_multi_device(len(devices), dev, nx, ny, nz, fs.ctypes.data, starstart, starstop,
                                                      v.ctypes.data, n, arr, ptrs, flags, changed, C.byref(path)),
                "ttsweep_solve_multi_device")
    return rc, [int(changed[s]) for s in range(n)], path.value
