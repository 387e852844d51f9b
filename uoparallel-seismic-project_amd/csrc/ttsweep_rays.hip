// ttsweep_rays.hip - shortest-path rays of converged travel-time boxes (include/ttsweep.h, "rays").
//
// The relaxation is Moser's network ray method: every finite travel time of a converged box is the
// candidate delay + T[o] of some live pull edge (o -> c) whose T[o] is smaller.  These kernels read that
// back without changing any box:
//   predecessor_kernel  pred[s][c] = the smallest FLOATBOX index o of such a neighbour, for every cell of
//                       every box, in one launch (a thread owns one cell of up to RAY_SB boxes: the delay
//                       of an entry does not depend on the start, so v[o] and the delay are computed once
//                       and compared against every box of the batch);
//   trace_rays_kernel   one lane per ray: follows pred from a receiver back to the start, checking every
//                       hop against the box (0 <= p < N, T[p] < T[c], a live edge whose candidate is T[c]),
//                       so a wrong pred buffer ends a walk as TTSWEEP_RAY_INVALID instead of running on.
// The liveness rule and the delay are those of sweep_cell_kernel / support_kernel (ttsweep_kernels.hip),
// bit for bit: the same edge_delay<EXACT> under the same ctx->exact_half choice, and - the Makefile's
// -ffp-contract=off - the add is rounded on its own, so `delay + T[o] == T[c]` is the solve's own store.
// Boxes and pred are in the caller's FLOATBOX layout (x * ny * nz + y * nz + z), int32 indices
// (ttsweep_rays.cpp refuses grids of more than INT32_MAX cells); velocity is read from the library's
// padded copy through RayGeom, only for neighbours inside the grid.
#include "ttsweep_kernels.h"

#include "../../include/ttsweep.h"

namespace ttsweep {

constexpr int RAY_BLOCK = 256;
constexpr int RAY_SB = 8;       // boxes per thread of the predecessor kernel, at most

// not below +INFINITY: +INFINITY or NaN (on the bits: the library is built with -fno-honor-nans)
__device__ __forceinline__ bool ray_unreached(float t)
{
    const unsigned u = __float_as_uint(t);
    return u == 0x7f800000u || (u & 0x7fffffffu) > 0x7f800000u;
}

template <bool EXACT, int SB>
__global__ void __launch_bounds__(RAY_BLOCK)
predecessor_kernel(RayGeom G, const float *__restrict__ v, const RayBox *__restrict__ boxes, int nstart,
                   const RayEntry *__restrict__ entries, int nentries)
{
    const long long N = (long long)G.n[0] * G.n[1] * G.n[2];
    const long long cl = (long long)blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (cl >= N) return;
    const int c = (int)cl;
    const int nyz = G.n[1] * G.n[2];
    const int x = c / nyz, y = (c - x * nyz) / G.n[2], z = c - x * nyz - y * G.n[2];
    const int s0 = blockIdx.y * SB;
    const int nb = min(SB, nstart - s0);

    const float *T[SB];
    float tc[SB];
    int sf[SB], best[SB];
    bool any = false;
#pragma unroll
    for (int k = 0; k < SB; k++) {
        const RayBox B = boxes[s0 + (k < nb ? k : 0)];
        T[k] = B.T;
        sf[k] = B.sflat;
        best[k] = 0x7fffffff;
        const float t = B.T[c];
        // a start cell, an unreached cell and a padding slot look for nothing: nothing is below -INFINITY
        const bool look = k < nb && c != B.sflat && !ray_unreached(t);
        tc[k] = look ? t : -__builtin_inff();
        any |= look;
    }
    if (any) {
        const long long vci = G.vbase + x * G.vs[0] + y * G.vs[1] + z * G.vs[2];
        const float vc = v[vci];
        for (int e = 0; e < nentries; e++) {
            const RayEntry en = entries[e];
            if ((unsigned)(x + en.di) >= (unsigned)G.n[0] || (unsigned)(y + en.dj) >= (unsigned)G.n[1]
                || (unsigned)(z + en.dk) >= (unsigned)G.n[2])
                continue;
            const int o = c + en.udelta;
            const float delay = edge_delay<EXACT>(en.h, en.d, vc + v[vci + en.vdelta]);
            const bool fwd = (en.flags & PULL_FWD) != 0, rev = (en.flags & PULL_REV) != 0;
#pragma unroll
            for (int k = 0; k < SB; k++) {
                const float to = T[k][o];
                const bool live = (fwd && c != sf[k]) || (rev && o != sf[k]);
                if (live && to < tc[k] && delay + to == tc[k] && o < best[k]) best[k] = o;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < SB; k++) {
        if (k >= nb) break;
        int p;
        if (c == sf[k]) p = TTSWEEP_PRED_SOURCE;
        else if (ray_unreached(T[k][c])) p = TTSWEEP_PRED_UNREACHED;
        else p = best[k] == 0x7fffffff ? TTSWEEP_PRED_SEED : best[k];
        boxes[s0 + k].pred[c] = p;
    }
}

template <int SB>
static void launch_pred_sb(dim3 grid, const RayGeom &G, const float *v, const RayBox *boxes, int nstart,
                           const RayEntry *entries, int nentries, bool exact, hipStream_t st)
{
    auto kernel = exact ? predecessor_kernel<true, SB> : predecessor_kernel<false, SB>;
    hipLaunchKernelGGL(kernel, grid, dim3(RAY_BLOCK), 0, st, G, v, boxes, nstart, entries, nentries);
}

hipError_t launch_predecessors(const RayGeom &G, const float *v, const RayBox *boxes, int nstart,
                               const RayEntry *entries, int nentries, bool exact, hipStream_t st)
{
    const long long N = (long long)G.n[0] * G.n[1] * G.n[2];
    if (N <= 0 || nstart <= 0) return hipSuccess;
    const long long nblocks = (N + RAY_BLOCK - 1) / RAY_BLOCK;
    if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
    // boxes per thread: 8 where there are as many, else the smallest power of two that holds them
    int sb = 1;
    while (sb < RAY_SB && sb < nstart) sb *= 2;
    const dim3 grid((unsigned)nblocks, (unsigned)((nstart + sb - 1) / sb));
    switch (sb) {
    case 1: launch_pred_sb<1>(grid, G, v, boxes, nstart, entries, nentries, exact, st); break;
    case 2: launch_pred_sb<2>(grid, G, v, boxes, nstart, entries, nentries, exact, st); break;
    case 4: launch_pred_sb<4>(grid, G, v, boxes, nstart, entries, nentries, exact, st); break;
    default: launch_pred_sb<RAY_SB>(grid, G, v, boxes, nstart, entries, nentries, exact, st); break;
    }
    return hipGetLastError();
}

// The length d of the hop p -> c (c the later cell, p = c + (di, dj, dk) inside the grid, T[p] = tp): the
// smallest d of a live entry with that offset whose candidate is T[c] = tc, in *d; false when there is none.  Entries
// are sorted by (di, dj, dk, d): a binary search finds the offset's first entry.
template <bool EXACT>
__device__ bool hop_length(const RayGeom &G, const float *__restrict__ v, const RayEntry *__restrict__ entries,
                            int nentries, int c, int p, int sflat, float tc, float tp, float *d)
{
    const int nyz = G.n[1] * G.n[2];
    const int cx = c / nyz, cy = (c - cx * nyz) / G.n[2], cz = c - cx * nyz - cy * G.n[2];
    const int px = p / nyz, py = (p - px * nyz) / G.n[2], pz = p - px * nyz - py * G.n[2];
    const int di = px - cx, dj = py - cy, dk = pz - cz;
    int lo = 0, hi = nentries;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const RayEntry &m = entries[mid];
        const bool less = m.di < di || (m.di == di && (m.dj < dj || (m.dj == dj && m.dk < dk)));
        if (less) lo = mid + 1;
        else hi = mid;
    }
    const float sum = v[G.vbase + cx * G.vs[0] + cy * G.vs[1] + cz * G.vs[2]]
                    + v[G.vbase + px * G.vs[0] + py * G.vs[1] + pz * G.vs[2]];
    for (int e = lo; e < nentries; e++) {
        const RayEntry en = entries[e];
        if (en.di != di || en.dj != dj || en.dk != dk) break;
        const bool live = ((en.flags & PULL_FWD) && c != sflat) || ((en.flags & PULL_REV) && p != sflat);
        if (live && edge_delay<EXACT>(en.h, en.d, sum) + tp == tc) {
            *d = en.d;
            return true;
        }
    }
    return false;
}

// One lane per ray r = s * nrecv + q.  FILL = false: count[r] (cells of the path; 0 unless OK / SEED),
// status[r], t_recv[r].  FILL = true: the same walk again, storing the path backwards into
// [offsets[r], offsets[r + 1]) so that it reads source -> receiver.
template <bool EXACT, bool FILL>
__global__ void __launch_bounds__(RAY_BLOCK)
trace_rays_kernel(RayGeom G, const float *__restrict__ v, const RayBox *__restrict__ boxes, int nstart,
                  const int *__restrict__ recv, int nrecv, const RayEntry *__restrict__ entries, int nentries,
                  int *__restrict__ count, int *__restrict__ status, float *__restrict__ t_recv,
                  const long long *__restrict__ offsets, int *__restrict__ cells, float *__restrict__ hop_d)
{
    const long long r = (long long)blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (r >= (long long)nstart * nrecv) return;
    const int s = (int)(r / nrecv);
    const int q = recv[r - (long long)s * nrecv];
    const RayBox B = boxes[s];
    const int N = G.n[0] * G.n[1] * G.n[2];
    long long lo = 0, pos = 0;
    if (FILL) {
        lo = offsets[r];
        pos = offsets[r + 1];
        if (pos <= lo) return;
        pos--;
        cells[pos] = q;
        hop_d[pos] = 0.0f;
    }
    float tc = B.T[q];
    int st, n = 0;
    if (ray_unreached(tc)) {
        st = TTSWEEP_RAY_UNREACHED;
    } else {
        int c = q;
        n = 1;
        for (;;) {
            const int p = B.pred[c];
            if (p == TTSWEEP_PRED_SOURCE) { st = c == B.sflat ? TTSWEEP_RAY_OK : TTSWEEP_RAY_INVALID; break; }
            if (p == TTSWEEP_PRED_SEED) { st = TTSWEEP_RAY_SEED; break; }
            if (p < 0 || p >= N) { st = TTSWEEP_RAY_INVALID; break; }
            const float tp = B.T[p];
            // strictly decreasing travel times: a walk visits a cell at most once and ends
            if (!(tp < tc)) { st = TTSWEEP_RAY_INVALID; break; }
            float d = 0.0f;
            if (!hop_length<EXACT>(G, v, entries, nentries, c, p, B.sflat, tc, tp, &d)) {
                st = TTSWEEP_RAY_INVALID;
                break;
            }
            n++;
            if (FILL) {
                if (pos <= lo) break;       // (the count pass saw this box: it cannot happen)
                pos--;
                cells[pos] = p;
                hop_d[pos] = d;
            }
            c = p;
            tc = tp;
        }
    }
    if (!FILL) {
        count[r] = (st == TTSWEEP_RAY_OK || st == TTSWEEP_RAY_SEED) ? n : 0;
        status[r] = st;
        t_recv[r] = B.T[q];
    }
}

hipError_t launch_trace_rays(const RayGeom &G, const float *v, const RayBox *boxes, int nstart, const int *recv,
                             int nrecv, const RayEntry *entries, int nentries, bool exact, int *count, int *status,
                             float *t_recv, const long long *offsets, int *cells, float *hop_d, bool fill,
                             hipStream_t st)
{
    const long long nrays = (long long)nstart * nrecv;
    if (nrays <= 0) return hipSuccess;
    const long long nblocks = (nrays + RAY_BLOCK - 1) / RAY_BLOCK;
    if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
    auto kernel = fill ? (exact ? trace_rays_kernel<true, true> : trace_rays_kernel<false, true>)
                       : (exact ? trace_rays_kernel<true, false> : trace_rays_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(RAY_BLOCK), 0, st, G, v, boxes, nstart, recv, nrecv,
                       entries, nentries, count, status, t_recv, offsets, cells, hop_d);
    return hipGetLastError();
}

} // namespace ttsweep
