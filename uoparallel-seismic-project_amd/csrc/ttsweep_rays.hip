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
static void launch_pred_sb(dim3 grid, const RayArgs &A, int nstart, bool exact, hipStream_t st)
{
    auto kernel = exact ? predecessor_kernel<true, SB> : predecessor_kernel<false, SB>;
    hipLaunchKernelGGL(kernel, grid, dim3(RAY_BLOCK), 0, st, A.G, A.v, A.boxes, nstart, A.entries, A.nentries);
}

hipError_t launch_predecessors(const RayArgs &A, int nstart, bool exact, hipStream_t st)
{
    const long long N = (long long)A.G.n[0] * A.G.n[1] * A.G.n[2];
    if (N <= 0 || nstart <= 0) return hipSuccess;
    const long long nblocks = (N + RAY_BLOCK - 1) / RAY_BLOCK;
    if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
    // boxes per thread: 8 where there are as many, else the smallest power of two that holds them
    int sb = 1;
    while (sb < RAY_SB && sb < nstart) sb *= 2;
    const dim3 grid((unsigned)nblocks, (unsigned)((nstart + sb - 1) / sb));
    switch (sb) {
    case 1: launch_pred_sb<1>(grid, A, nstart, exact, st); break;
    case 2: launch_pred_sb<2>(grid, A, nstart, exact, st); break;
    case 4: launch_pred_sb<4>(grid, A, nstart, exact, st); break;
    default: launch_pred_sb<RAY_SB>(grid, A, nstart, exact, st); break;
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

// The walk from receiver q of box B along pred back to the start, checking every hop: hop(c, p, d) for every hop
// p -> c of length d, in walk order (receiver -> source).  Returns the ray's status; *end is the cell the walk
// ended at.
template <bool EXACT, class Hop>
__device__ __forceinline__ int ray_walk(const RayArgs &A, const RayBox &B, int q, int *end, Hop hop)
{
    const int N = A.G.n[0] * A.G.n[1] * A.G.n[2];
    float tc = B.T[q];
    int c = q;
    *end = q;
    if (ray_unreached(tc)) return TTSWEEP_RAY_UNREACHED;
    for (;;) {
        const int p = B.pred[c];
        *end = c;
        if (p == TTSWEEP_PRED_SOURCE) return c == B.sflat ? TTSWEEP_RAY_OK : TTSWEEP_RAY_INVALID;
        if (p == TTSWEEP_PRED_SEED) return TTSWEEP_RAY_SEED;
        if (p < 0 || p >= N) return TTSWEEP_RAY_INVALID;
        const float tp = B.T[p];
        // strictly decreasing travel times: a walk visits a cell at most once and ends
        if (!(tp < tc)) return TTSWEEP_RAY_INVALID;
        float d = 0.0f;
        if (!hop_length<EXACT>(A.G, A.v, A.entries, A.nentries, c, p, B.sflat, tc, tp, &d))
            return TTSWEEP_RAY_INVALID;
        hop(c, p, d);
        c = p;
        tc = tp;
    }
}

// box s and flat receiver q of ray r of the list: r = s * nrecv + q' with q = recv[q'] in a cross product, the
// record of a pair list in one 8-byte load.  I: the type of a ray index (int but for the trace)
template <bool PAIRS, class I>
__device__ __forceinline__ void ray_of(const RayList &L, I r, int &s, int &q)
{
    if (PAIRS) {
        const RayPair pr = L.pairs[r];
        s = pr.box;
        q = pr.recv;
    } else {
        s = (int)(r / L.nrecv);
        q = L.recv[r - (I)s * L.nrecv];
    }
}

// One lane per ray of a cross product.  FILL = false: count[r] (cells of the path; 0 unless OK / SEED), status[r],
// t_recv[r].  FILL = true: the same walk again, storing the path backwards into [offsets[r], offsets[r + 1]) so
// that it reads source -> receiver.
template <bool EXACT, bool FILL>
__global__ void __launch_bounds__(RAY_BLOCK)
trace_rays_kernel(RayArgs A, RayList L, int *__restrict__ count, int *__restrict__ status,
                  float *__restrict__ t_recv, const long long *__restrict__ offsets, int *__restrict__ cells,
                  float *__restrict__ hop_d)
{
    const long long r = (long long)blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (r >= L.n) return;
    int s, q, end;
    ray_of<false>(L, r, s, q);
    const RayBox B = A.boxes[s];
    if (FILL) {
        const long long lo = offsets[r];
        long long pos = offsets[r + 1];
        if (pos <= lo) return;
        pos--;
        cells[pos] = q;
        hop_d[pos] = 0.0f;
        ray_walk<EXACT>(A, B, q, &end, [&](int, int p, float d) {
            if (pos <= lo) return;          // (the count pass saw this box: it cannot happen)
            pos--;
            cells[pos] = p;
            hop_d[pos] = d;
        });
    } else {
        int n = 1;
        const int st = ray_walk<EXACT>(A, B, q, &end, [&](int, int, float) { n++; });
        count[r] = (st == TTSWEEP_RAY_OK || st == TTSWEEP_RAY_SEED) ? n : 0;
        status[r] = st;
        t_recv[r] = B.T[q];
    }
}

// ---- the Frechet operators of the rays: G m and G^T w without storing a path ----
// G is rays_to_frechet(trace_rays(...)): every hop p -> c of length d of an OK or SEED ray adds d / 2 at
// (ray, p) and at (ray, c).  Both kernels walk one lane per ray like trace_rays_kernel (the same ray_walk, so the
// same checks per hop, the same statuses, the same hop_length<EXACT> choice of d) and read or scatter along the walk
// instead of storing it.  UNREACHED and INVALID rays contribute nothing.  PAIRS: the rays are the records of a pair
// list instead of the cross product (ray_of), and ray_geometry_kernel reads the geometry of each ray off the same
// walk (include/ttsweep.h, "rays: pair lists").

// y[r] = (G m)[r]: y = y + (0.5 * (double)d) * (m[c] + m[p]) per hop p -> c in walk order from y = 0.0;
// 0 for UNREACHED and INVALID rays.  One store per ray.
template <bool EXACT, bool PAIRS>
__global__ void __launch_bounds__(RAY_BLOCK)
ray_forward_kernel(RayArgs A, RayList L, const double *__restrict__ m, double *__restrict__ y,
                   int *__restrict__ status)
{
    const int r = blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (r >= (int)L.n) return;
    int s, q, end;
    ray_of<PAIRS>(L, r, s, q);
    const RayBox B = A.boxes[s];
    double acc = 0.0;
    const int st = ray_walk<EXACT>(A, B, q, &end,
                                   [&](int c, int p, float d) { acc = acc + (0.5 * (double)d) * (m[c] + m[p]); });
    y[r] = (st == TTSWEEP_RAY_OK || st == TTSWEEP_RAY_SEED) ? acc : 0.0;
    status[r] = st;
}

// The fixed-point term of one visit: llrint(ldexp(w * (0.5 * ((double)d_in + (double)d_out)), S))
__device__ __forceinline__ long long ray_term(double w, float d_in, float d_out, int S)
{
    return __builtin_llrint(__builtin_ldexp(w * (0.5 * ((double)d_in + (double)d_out)), S));
}

// acc (the caller's g, as int64) += the terms of every OK / SEED ray, hits[x] += 1 per such ray through x (hits
// may be NULL; w NULL: hits only).  A cell's term is added once it has both its hops: at the hop out of it in
// walk order, and at the end of the walk for the last cell.  An INVALID ray's terms are already added when its
// walk fails: the same walk again takes them back out (integer adds: exact in any order).  Every OK ray of box
// s ends at its start cell: those terms and hits are summed across the wave first, one atomic per wave and box.
// Every lane of a wave reaches the wave sum (no early return).  The wave sum is keyed on the end cell, not on the
// box: the lanes of one wave may belong to any boxes (a pair list), each distinct start cell gets its own round.
template <bool EXACT, bool PAIRS>
__global__ void __launch_bounds__(RAY_BLOCK)
ray_adjoint_kernel(RayArgs A, RayList L, const double *__restrict__ w, int S, unsigned long long *__restrict__ acc,
                   int *__restrict__ hits)
{
    const int r = blockIdx.x * RAY_BLOCK + threadIdx.x;
    const bool lane = r < (int)L.n;
    const double wr = (lane && w) ? w[r] : 0.0;
    const bool weighted = wr != 0.0;
    int st = TTSWEEP_RAY_UNREACHED, end = -1;
    float dlast = 0.0f;
    if (lane && (weighted || hits)) {
        int s, q;
        ray_of<PAIRS>(L, r, s, q);
        const RayBox B = A.boxes[s];
        auto visit = [&](long long sign) {
            float dout = 0.0f;      // the hop out of the cell in the path's direction: none at the receiver
            return [&, sign, dout](int c, int, float d) mutable {
                if (weighted) {
                    const long long t = ray_term(wr, d, dout, S);
                    if (t) atomicAdd(acc + c, (unsigned long long)(sign * t));
                }
                if (hits) atomicAdd(hits + c, (int)sign);
                dout = d;
                dlast = d;
            };
        };
        st = ray_walk<EXACT>(A, B, q, &end, visit(1));
        if (st == TTSWEEP_RAY_INVALID) {
            int e2;
            ray_walk<EXACT>(A, B, q, &e2, visit(-1));
        }
        if (st == TTSWEEP_RAY_SEED) {           // the last cell of a SEED ray: not shared, one atomic of its own
            if (weighted) {
                const long long t = ray_term(wr, 0.0f, dlast, S);
                if (t) atomicAdd(acc + end, (unsigned long long)t);
            }
            if (hits) atomicAdd(hits + end, 1);
        }
    }
    // the start cells of the OK rays: one wave sum per distinct cell (in the dense call a wave spans one box
    // unless nrecv < 64 or it straddles a box boundary; in a pair list it spans whatever boxes its pairs name)
    bool pend = st == TTSWEEP_RAY_OK;
    const long long mine = (pend && weighted) ? ray_term(wr, 0.0f, dlast, S) : 0;
    unsigned long long live = __ballot(pend);
    while (live) {
        const int leader = __ffsll((long long)live) - 1;
        const int key = __shfl(end, leader);
        const bool take = pend && end == key;
        long long sum = take ? mine : 0;
        int n = take ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sum += __shfl_xor(sum, off);
            n += __shfl_xor(n, off);
        }
        if ((int)__lane_id() == leader) {
            if (sum) atomicAdd(acc + key, (unsigned long long)sum);
            if (hits) atomicAdd(hits + key, n);
        }
        pend = pend && !take;
        live = __ballot(pend);
    }
}

// The geometry of the ray of every pair, from the same walk.  Everything is kept in registers while the walk runs
// and stored once it has returned its status: an INVALID ray is only known to be one when its walk fails.  Of the
// first and the last hop the cells and d are kept; their offsets are decoded and their times read after the walk.
template <bool EXACT, bool PAIRS>
__global__ void __launch_bounds__(RAY_BLOCK)
ray_geometry_kernel(RayArgs A, RayList L, int *__restrict__ status, RayGeometryOut O)
{
    const int r = blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (r >= (int)L.n) return;
    int s, q;
    ray_of<PAIRS>(L, r, s, q);
    const RayBox B = A.boxes[s];
    const int nz = A.G.n[2], nyz = A.G.n[1] * A.G.n[2];
    int hops = 0, first_p = q, last_c = q, deep = q, deepz = q % nz, end;
    float d_first = 0.0f, d_last = 0.0f;
    double length = 0.0;
    const int st = ray_walk<EXACT>(A, B, q, &end, [&](int c, int p, float d) {
        if (hops == 0) {
            first_p = p;
            d_first = d;
        }
        hops++;
        length = length + (double)d;
        last_c = c;
        d_last = d;
        const int z = p % nz;       // FLOATBOX index (x * ny + y) * nz + z
        if (z > deepz) {
            deepz = z;
            deep = p;
        }
    });
    const bool ok = st == TTSWEEP_RAY_OK || st == TTSWEEP_RAY_SEED;
    const bool hop = ok && hops > 0;
    status[r] = st;
    if (O.t_recv) O.t_recv[r] = B.T[q];
    if (O.hops) O.hops[r] = ok ? hops : 0;
    if (O.length) O.length[r] = ok ? length : 0.0;
    if (O.deep) O.deep[r] = ok ? deep : -1;
    // the hop out of the receiver, c = q -> p = first_p, and the hop into the end cell, c = last_c -> p = end
    auto store = [&](int from, int to, float d, float dt, int *o3, float *od, float *odt) {
        if (o3) {
            const int fx = from / nyz, fy = (from - fx * nyz) / nz, fz = from - fx * nyz - fy * nz;
            const int tx = to / nyz, ty = (to - tx * nyz) / nz, tz = to - tx * nyz - ty * nz;
            o3[3 * (long long)r + 0] = hop ? tx - fx : 0;
            o3[3 * (long long)r + 1] = hop ? ty - fy : 0;
            o3[3 * (long long)r + 2] = hop ? tz - fz : 0;
        }
        if (od) od[r] = hop ? d : 0.0f;
        if (odt) odt[r] = hop ? dt : 0.0f;
    };
    float dt_first = 0.0f, dt_last = 0.0f;
    if (hop) {
        dt_first = B.T[q] - B.T[first_p];
        dt_last = B.T[last_c] - B.T[end];
    }
    store(q, first_p, d_first, dt_first, O.recv_hop, O.recv_d, O.recv_dt);
    store(end, last_c, d_last, dt_last, O.src_hop, O.src_d, O.src_dt);
}

// The weights' scan: out[0] = max over nonzero w of (frexp exponent + 2048) (0: every weight is zero), out[1] =
// 1 if any weight is NaN or infinite.  Tested on the bits (the library is built with -fno-honor-nans); integer
// max and or: the same result whatever the order.
__global__ void __launch_bounds__(RAY_BLOCK)
ray_weight_scan_kernel(const double *__restrict__ w, int n, int *__restrict__ out)
{
    int e = 0, bad = 0;
    for (int i = blockIdx.x * RAY_BLOCK + threadIdx.x; i < n; i += gridDim.x * RAY_BLOCK) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(w[i]) & 0x7fffffffffffffffULL;
        if (u == 0) continue;
        const int eb = (int)(u >> 52);
        if (eb == 2047) bad = 1;
        else e = max(e, 2048 + (eb ? eb - 1022 : -1010 - __clzll((long long)u)));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        e = max(e, __shfl_xor(e, off));
        bad |= __shfl_xor(bad, off);
    }
    if (__lane_id() == 0) {
        if (e) atomicMax(out, e);
        if (bad) atomicOr(out + 1, 1);
    }
}

// g[x] = ldexp((double)acc[x], -S), in place
__global__ void __launch_bounds__(RAY_BLOCK)
ray_fixed_to_double_kernel(long long *__restrict__ g, long long n, int S)
{
    const long long x = (long long)blockIdx.x * RAY_BLOCK + threadIdx.x;
    if (x >= n) return;
    const double t = __builtin_ldexp((double)g[x], -S);
    reinterpret_cast<double *>(g)[x] = t;
}

// One lane per ray: the blocks of nrays rays, the kernel of the `exact` choice, the launch's error.  limit: the rays
// the kernel's index type holds.
template <class Kernel, class... Args>
static hipError_t launch_per_ray(bool exact, Kernel exact_kernel, Kernel kernel, long long nrays, long long limit,
                                 hipStream_t st, const Args &...args)
{
    if (nrays <= 0) return hipSuccess;
    const long long nblocks = (nrays + RAY_BLOCK - 1) / RAY_BLOCK;
    if (nrays > limit || nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(exact ? exact_kernel : kernel, dim3((unsigned)nblocks), dim3(RAY_BLOCK), 0, st, args...);
    return hipGetLastError();
}

constexpr long long RAY_INT32 = 0x7fffffffLL, RAY_INT64 = 0x7fffffffffffffffLL;

hipError_t launch_trace_rays(const RayArgs &A, const RayList &L, bool exact, int *count, int *status, float *t_recv,
                             const long long *offsets, int *cells, float *hop_d, bool fill, hipStream_t st)
{
    if (fill)
        return launch_per_ray(exact, trace_rays_kernel<true, true>, trace_rays_kernel<false, true>, L.n, RAY_INT64,
                              st, A, L, count, status, t_recv, offsets, cells, hop_d);
    return launch_per_ray(exact, trace_rays_kernel<true, false>, trace_rays_kernel<false, false>, L.n, RAY_INT64, st,
                          A, L, count, status, t_recv, offsets, cells, hop_d);
}

hipError_t launch_ray_forward(const RayArgs &A, const RayList &L, bool exact, const double *m, double *y, int *status,
                              hipStream_t st)
{
    if (L.pairs)
        return launch_per_ray(exact, ray_forward_kernel<true, true>, ray_forward_kernel<false, true>, L.n, RAY_INT32,
                              st, A, L, m, y, status);
    return launch_per_ray(exact, ray_forward_kernel<true, false>, ray_forward_kernel<false, false>, L.n, RAY_INT32,
                          st, A, L, m, y, status);
}

hipError_t launch_ray_adjoint(const RayArgs &A, const RayList &L, bool exact, const double *w, int S, long long *acc,
                              int *hits, hipStream_t st)
{
    unsigned long long *const sums = (unsigned long long *)acc;
    if (L.pairs)
        return launch_per_ray(exact, ray_adjoint_kernel<true, true>, ray_adjoint_kernel<false, true>, L.n, RAY_INT32,
                              st, A, L, w, S, sums, hits);
    return launch_per_ray(exact, ray_adjoint_kernel<true, false>, ray_adjoint_kernel<false, false>, L.n, RAY_INT32,
                          st, A, L, w, S, sums, hits);
}

hipError_t launch_ray_pairs_geometry(const RayArgs &A, const RayList &L, bool exact, int *status,
                                     const RayGeometryOut &out, hipStream_t st)
{
    return launch_per_ray(exact, ray_geometry_kernel<true, true>, ray_geometry_kernel<false, true>, L.n, RAY_INT32,
                          st, A, L, status, out);
}

hipError_t launch_ray_weight_scan(const double *w, int n, int *out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int want = (n + RAY_BLOCK - 1) / RAY_BLOCK;
    const unsigned nblocks = (unsigned)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(ray_weight_scan_kernel, dim3(nblocks), dim3(RAY_BLOCK), 0, st, w, n, out);
    return hipGetLastError();
}

hipError_t launch_ray_fixed_to_double(long long *g, long long n, int S, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const long long nblocks = (n + RAY_BLOCK - 1) / RAY_BLOCK;
    if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ray_fixed_to_double_kernel, dim3((unsigned)nblocks), dim3(RAY_BLOCK), 0, st, g, n, S);
    return hipGetLastError();
}

} // namespace ttsweep
