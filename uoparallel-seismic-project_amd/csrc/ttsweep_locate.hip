// ttsweep_locate.hip - grid-search event location over station travel-time boxes (include/ttsweep.h, "locate").
//
// By reciprocity T_k[x] is the travel time between station k and a candidate hypocentre x.  For every event e
// and cell x the weighted L2 misfit of the picks with the origin time eliminated is, in double, stations in
// ascending k, zero weights skipped (-ffp-contract=off: every operation rounded on its own):
//   S1 = S1 + w * (o - (double)T)        t0 = S1 * invW        J = J + (w * r) * r,  r = (o - (double)T) - t0
// These kernels:
//   locate_check_kernel     one lane per event: refuses non-finite picks, negative / non-finite weights and
//                           events without a weight (flag per event, on the bits: the library is built with
//                           -fno-honor-nans) and computes invW = 1.0 / W
//   locate_search_kernel    one lane per cell of a tile of LOC_C * LOC_BLOCK cells, LOC_ET events per block; the
//                           lane keeps its best (J, x) per event in LDS across its cells, then one wave
//                           reduction per event and tile gives a per-tile partial (J bits, x)
//   locate_final_kernel     one block per event: the smallest (J bits, x) over the tiles, then t0 at that cell
//   locate_volume_kernel    J (+INF where inadmissible) of every cell for a list of events
//   locate_window_*_kernel  the same search over a window and lattice per event ("locate window", further down)
//   locate_subcell_*_kernel the search over the nodes of a finer lattice inside a window of cells, the station times
//                           interpolated trilinearly ("locate subcell", further down)
// A cell is inadmissible when a picked station has T >= +INFINITY or J is not below +INFINITY.  The first implies
// the second in IEEE arithmetic (o - INF = -INF enters S1, so t0 is -INF or NaN and r of that station is NaN), so
// one test on the bits of J covers both: J >= 0 always, and +INF and every NaN compare above it as unsigned
// integers.  The argmin is the lexicographic minimum of (bits of J, x): the same whatever order the tiles, lanes
// and waves are combined in, so results do not depend on the launch or on which events share a batch.  No float
// atomics.  T is read through (double) of the float: exact.
#include "ttsweep_kernels.h"

#include "../../include/ttsweep.h"

namespace ttsweep {

constexpr int LOC_BLOCK = 256;
constexpr int LOC_ET = 8;       // events per search block (mirrored: tests/test_locate_cpu.py::test_case_constants_mirror_the_sources)
constexpr int LOC_C = 16;       // cells per lane per search block: a tile is LOC_C * LOC_BLOCK cells
constexpr unsigned long long LOC_INF = 0x7ff0000000000000ULL;

__device__ __forceinline__ unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }

// the station k of an event with weights w (nullptr: every weight 1.0) is picked
__device__ __forceinline__ bool loc_picked(const double *__restrict__ w, int k)
{
    return !w || (dbits(w[k]) << 1) != 0;
}

__device__ __forceinline__ double loc_w(const double *__restrict__ w, int k) { return w ? w[k] : 1.0; }

// J and t0 of one event at the cell whose travel times are t(k), the semantics of include/ttsweep.h
template <int KR, typename TF>
__device__ __forceinline__ double loc_misfit(TF t, int K, const double *__restrict__ o, const double *__restrict__ w,
                                             double invw, double &t0)
{
    double s1 = 0.0, J = 0.0;
    if constexpr (KR > 0) {
#pragma unroll
        for (int k = 0; k < KR; k++)
            if (k < K && loc_picked(w, k)) {
                const double d = o[k] - t(k);
                s1 = s1 + loc_w(w, k) * d;
            }
        t0 = s1 * invw;
#pragma unroll
        for (int k = 0; k < KR; k++)
            if (k < K && loc_picked(w, k)) {
                const double r = (o[k] - t(k)) - t0;
                J = J + (loc_w(w, k) * r) * r;
            }
    } else {
        for (int k = 0; k < K; k++)
            if (loc_picked(w, k)) {
                const double d = o[k] - t(k);
                s1 = s1 + loc_w(w, k) * d;
            }
        t0 = s1 * invw;
        for (int k = 0; k < K; k++)
            if (loc_picked(w, k)) {
                const double r = (o[k] - t(k)) - t0;
                J = J + (loc_w(w, k) * r) * r;
            }
    }
    return J;
}

__device__ __forceinline__ bool loc_less(unsigned long long ka, int xa, unsigned long long kb, int xb)
{
    return ka < kb || (ka == kb && xa < xb);
}

// the lexicographic minimum of (key, x) over the 64 lanes of the wave, in every lane
__device__ __forceinline__ void loc_wave_min(unsigned long long &key, int &x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long k2 = __shfl_xor(key, off);
        const int x2 = __shfl_xor(x, off);
        if (loc_less(k2, x2, key, x)) {
            key = k2;
            x = x2;
        }
    }
}

// flag[e]: bit 0 a non-finite pick, bit 1 a negative or non-finite weight, bit 2 no weight above zero
__global__ void __launch_bounds__(LOC_BLOCK)
locate_check_kernel(int K, int nevent, const double *__restrict__ picks, const double *__restrict__ weights,
                    double *__restrict__ invw, int *__restrict__ flag)
{
    const int e = blockIdx.x * LOC_BLOCK + threadIdx.x;
    if (e >= nevent) return;
    const double *o = picks + (long long)e * K;
    const double *w = weights ? weights + (long long)e * K : nullptr;
    int f = 0;
    double W = 0.0;
    for (int k = 0; k < K; k++) {
        if (((dbits(o[k]) >> 52) & 0x7ff) == 0x7ff) f |= 1;
        if (w) {
            const unsigned long long u = dbits(w[k]);
            if (((u >> 52) & 0x7ff) == 0x7ff || (u >> 63 && (u << 1) != 0)) {
                f |= 2;
                continue;
            }
        }
        if (loc_picked(w, k)) W = W + loc_w(w, k);
    }
    if ((dbits(W) << 1) == 0) f |= 4;
    invw[e] = f ? 0.0 : 1.0 / W;
    flag[e] = f;
}

// blockIdx.x: a tile of LOC_C * LOC_BLOCK cells; blockIdx.y: LOC_ET events from e0.  Writes part_key / part_x
// [(e - e0) * ntiles + tile] (J bits, x) of the best admissible cell of the tile, (+INF bits, INT_MAX) when none.
template <int KR>
__global__ void __launch_bounds__(LOC_BLOCK)
locate_search_kernel(const float *const *__restrict__ boxes, int K, int N, const double *__restrict__ picks,
                     const double *__restrict__ weights, const double *__restrict__ invw, int e0, int ne, int ntiles,
                     unsigned long long *__restrict__ part_key, int *__restrict__ part_x)
{
    __shared__ unsigned long long s_key[LOC_ET][LOC_BLOCK];
    __shared__ int s_x[LOC_ET][LOC_BLOCK];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int eb = blockIdx.y * LOC_ET;                 // first event of the block, relative to e0
    const int net = min(LOC_ET, ne - eb);
#pragma unroll
    for (int i = 0; i < LOC_ET; i++) {
        s_key[i][tid] = LOC_INF;
        s_x[i][tid] = 0x7fffffff;
    }
    // the cell loop and the event loop are uniform (lanes past the grid compute the last cell and keep nothing), so
    // the picks and weights are uniform loads and a zero weight is a uniform branch
    const long long base = (long long)tile * (LOC_C * LOC_BLOCK);
    const int nj = (int)min((long long)LOC_C, (N - base + LOC_BLOCK - 1) / LOC_BLOCK);
    for (int j = 0; j < nj; j++) {
        const long long xl = base + (long long)j * LOC_BLOCK + tid;
        const bool in = xl < N;
        const int x = in ? (int)xl : N - 1;
        double tr[KR > 0 ? KR : 1];
        if constexpr (KR > 0) {
#pragma unroll
            for (int k = 0; k < KR; k++) tr[k] = k < K ? (double)boxes[k][x] : 0.0;
        }
        for (int i = 0; i < net; i++) {
            const int e = __builtin_amdgcn_readfirstlane(e0 + eb + i);
            const double *o = picks + (long long)e * K;
            const double *w = weights ? weights + (long long)e * K : nullptr;
            double t0;
            const double J = KR > 0 ? loc_misfit<KR>([&](int k) { return tr[k]; }, K, o, w, invw[e], t0)
                                    : loc_misfit<0>([&](int k) { return (double)boxes[k][x]; }, K, o, w, invw[e], t0);
            const unsigned long long key = dbits(J);
            if (in && key < s_key[i][tid]) {     // cells of a lane ascend: strict keeps the smallest x
                s_key[i][tid] = key;
                s_x[i][tid] = x;
            }
        }
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int i = wave; i < net; i += LOC_BLOCK / 64) {
        unsigned long long key = s_key[i][lane];
        int x = s_x[i][lane];
#pragma unroll
        for (int q = 1; q < LOC_BLOCK / 64; q++) {
            const unsigned long long k2 = s_key[i][lane + 64 * q];
            const int x2 = s_x[i][lane + 64 * q];
            if (loc_less(k2, x2, key, x)) {
                key = k2;
                x = x2;
            }
        }
        loc_wave_min(key, x);
        if (lane == 0) {
            const long long p = (long long)(eb + i) * ntiles + tile;
            part_key[p] = key;
            part_x[p] = x;
        }
    }
}

// one block per event e0 + blockIdx.x: the smallest (J bits, x) over the tiles; cell, misfit and t0 (bits) of it,
// or (-1, +INF, nan_bits) when no cell is admissible (the NaN comes from the host)
template <int KR>
__global__ void __launch_bounds__(LOC_BLOCK)
locate_final_kernel(const float *const *__restrict__ boxes, int K, const double *__restrict__ picks,
                    const double *__restrict__ weights, const double *__restrict__ invw, int e0, int ntiles,
                    const unsigned long long *__restrict__ part_key, const int *__restrict__ part_x,
                    int *__restrict__ cell, unsigned long long *__restrict__ misfit, unsigned long long *__restrict__ t0out,
                    unsigned long long nan_bits)
{
    __shared__ unsigned long long s_key[LOC_BLOCK / 64];
    __shared__ int s_x[LOC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int eo = blockIdx.x;
    const int e = e0 + eo;
    unsigned long long key = LOC_INF;
    int x = 0x7fffffff;
    for (int t = tid; t < ntiles; t += LOC_BLOCK) {
        const long long p = (long long)eo * ntiles + t;
        if (loc_less(part_key[p], part_x[p], key, x)) {
            key = part_key[p];
            x = part_x[p];
        }
    }
    loc_wave_min(key, x);
    if (lane == 0) {
        s_key[wave] = key;
        s_x[wave] = x;
    }
    __syncthreads();
    if (tid) return;
    key = s_key[0];
    x = s_x[0];
    for (int q = 1; q < LOC_BLOCK / 64; q++)
        if (loc_less(s_key[q], s_x[q], key, x)) {
            key = s_key[q];
            x = s_x[q];
        }
    const bool found = key < LOC_INF;
    unsigned long long tb = nan_bits;
    if (found) {
        const double *o = picks + (long long)e * K;
        const double *w = weights ? weights + (long long)e * K : nullptr;
        double t0;
        loc_misfit<0>([&](int k) { return (double)boxes[k][x]; }, K, o, w, invw[e], t0);
        tb = dbits(t0);
    }
    if (cell) cell[e] = found ? x : -1;
    if (misfit) misfit[e] = found ? key : LOC_INF;
    if (t0out) t0out[e] = tb;
}

// blockIdx.y: entry v of the volume list; vol[v][x] = J of event vev[v] at x, +INF where inadmissible
template <int KR>
__global__ void __launch_bounds__(LOC_BLOCK)
locate_volume_kernel(const float *const *__restrict__ boxes, int K, int N, const double *__restrict__ picks,
                     const double *__restrict__ weights, const double *__restrict__ invw, const int *__restrict__ vev,
                     unsigned long long *const *__restrict__ vol)
{
    const long long xl = (long long)blockIdx.x * LOC_BLOCK + threadIdx.x;
    if (xl >= N) return;
    const int x = (int)xl;
    const int e = vev[blockIdx.y];
    const double *o = picks + (long long)e * K;
    const double *w = weights ? weights + (long long)e * K : nullptr;
    double t0;
    double J;
    if constexpr (KR > 0) {
        double tr[KR];
#pragma unroll
        for (int k = 0; k < KR; k++) tr[k] = k < K ? (double)boxes[k][x] : 0.0;
        J = loc_misfit<KR>([&](int k) { return tr[k]; }, K, o, w, invw[e], t0);
    } else {
        J = loc_misfit<0>([&](int k) { return (double)boxes[k][x]; }, K, o, w, invw[e], t0);
    }
    const unsigned long long key = dbits(J);
    vol[blockIdx.y][x] = key < LOC_INF ? key : LOC_INF;
}

// ---- windowed, strided search (include/ttsweep.h, "locate window") ----
// The candidates of an event are the nodes of a lattice inside its window.  The host cuts the events into groups of at
// most LOC_ET consecutive events with one window (WinGroup) and lists every (group, tile of LOC_WC * LOC_BLOCK
// candidates) as a block (WinBlock).  A lane decodes its candidate number q (z fastest) to a cell once per step, with
// two divisions, loads the K travel times of that cell once and scores the events of the group on them: the cell
// loop, event loop, loc_misfit and the per-lane minimum in LDS of locate_search_kernel.  The cell index ascends with
// q, so the strict compare of a lane and the lexicographic minimum of (bits of J, cell) give the smallest index among
// the candidates of minimal J whatever the grouping.
//   locate_window_search_kernel  one block per WinBlock; the partial of event i of the group at
//                                [group.part + i * group.ntiles + tile]
//   locate_window_final_kernel   one block per event: the smallest of its partials, then t0 at that cell
constexpr int LOC_WC = 16;      // candidates per lane per window block
static_assert(LOC_WIN_ET <= LOC_ET, "a group's events share the per-lane minima of one block");

template <int KR>
__global__ void __launch_bounds__(LOC_BLOCK)
locate_window_search_kernel(const float *const *__restrict__ boxes, int K, int mx, int my, int mz,
                            const double *__restrict__ picks, const double *__restrict__ weights,
                            const double *__restrict__ invw, const WinGroup *__restrict__ groups,
                            const WinBlock *__restrict__ blocks, unsigned long long *__restrict__ part_key,
                            int *__restrict__ part_x)
{
    __shared__ unsigned long long s_key[LOC_ET][LOC_BLOCK];
    __shared__ int s_x[LOC_ET][LOC_BLOCK];
    const int tid = threadIdx.x;
    const WinBlock B = blocks[blockIdx.x];              // uniform: scalar loads
    const WinGroup G = groups[B.group];
    const int net = G.ne;
#pragma unroll
    for (int i = 0; i < LOC_ET; i++) {
        s_key[i][tid] = LOC_INF;
        s_x[i][tid] = 0x7fffffff;
    }
    // uniform loops as in locate_search_kernel: lanes past the last candidate compute it again and keep nothing
    const long long base = (long long)B.tile * (LOC_WC * LOC_BLOCK);
    const int nj = (int)min((long long)LOC_WC, (G.ncand - base + LOC_BLOCK - 1) / LOC_BLOCK);
    for (int j = 0; j < nj; j++) {
        const long long ql = base + (long long)j * LOC_BLOCK + tid;
        const bool in = ql < G.ncand;
        const unsigned q = in ? (unsigned)ql : (unsigned)(G.ncand - 1);
        const unsigned qxy = q / (unsigned)G.cz, cz = q - qxy * (unsigned)G.cz;
        const unsigned cx = qxy / (unsigned)G.cy, cy = qxy - cx * (unsigned)G.cy;
        const int x = G.x0 + (int)cx * mx + (int)cy * my + (int)cz * mz;
        double tr[KR > 0 ? KR : 1];
        if constexpr (KR > 0) {
#pragma unroll
            for (int k = 0; k < KR; k++) tr[k] = k < K ? (double)boxes[k][x] : 0.0;
        }
        for (int i = 0; i < net; i++) {
            const int e = __builtin_amdgcn_readfirstlane(G.e0 + i);
            const double *o = picks + (long long)e * K;
            const double *w = weights ? weights + (long long)e * K : nullptr;
            double t0;
            const double J = KR > 0 ? loc_misfit<KR>([&](int k) { return tr[k]; }, K, o, w, invw[e], t0)
                                    : loc_misfit<0>([&](int k) { return (double)boxes[k][x]; }, K, o, w, invw[e], t0);
            const unsigned long long key = dbits(J);
            if (in && key < s_key[i][tid]) {     // cells of a lane ascend: strict keeps the smallest x
                s_key[i][tid] = key;
                s_x[i][tid] = x;
            }
        }
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int i = wave; i < net; i += LOC_BLOCK / 64) {
        unsigned long long key = s_key[i][lane];
        int x = s_x[i][lane];
#pragma unroll
        for (int q = 1; q < LOC_BLOCK / 64; q++) {
            const unsigned long long k2 = s_key[i][lane + 64 * q];
            const int x2 = s_x[i][lane + 64 * q];
            if (loc_less(k2, x2, key, x)) {
                key = k2;
                x = x2;
            }
        }
        loc_wave_min(key, x);
        if (lane == 0) {
            const long long p = G.part + (long long)i * G.ntiles + B.tile;
            part_key[p] = key;
            part_x[p] = x;
        }
    }
}

// one block per event e0 + blockIdx.x: the smallest (J bits, x) of its ev_ntiles partials from ev_part; the outputs
// of locate_final_kernel
__global__ void __launch_bounds__(LOC_BLOCK)
locate_window_final_kernel(const float *const *__restrict__ boxes, int K, const double *__restrict__ picks,
                           const double *__restrict__ weights, const double *__restrict__ invw, int e0,
                           const long long *__restrict__ ev_part, const int *__restrict__ ev_ntiles,
                           const unsigned long long *__restrict__ part_key, const int *__restrict__ part_x,
                           int *__restrict__ cell, unsigned long long *__restrict__ misfit,
                           unsigned long long *__restrict__ t0out, unsigned long long nan_bits)
{
    __shared__ unsigned long long s_key[LOC_BLOCK / 64];
    __shared__ int s_x[LOC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = e0 + blockIdx.x;
    const long long p0 = ev_part[blockIdx.x];
    const int ntiles = ev_ntiles[blockIdx.x];
    unsigned long long key = LOC_INF;
    int x = 0x7fffffff;
    for (int t = tid; t < ntiles; t += LOC_BLOCK)
        if (loc_less(part_key[p0 + t], part_x[p0 + t], key, x)) {
            key = part_key[p0 + t];
            x = part_x[p0 + t];
        }
    loc_wave_min(key, x);
    if (lane == 0) {
        s_key[wave] = key;
        s_x[wave] = x;
    }
    __syncthreads();
    if (tid) return;
    key = s_key[0];
    x = s_x[0];
    for (int q = 1; q < LOC_BLOCK / 64; q++)
        if (loc_less(s_key[q], s_x[q], key, x)) {
            key = s_key[q];
            x = s_x[q];
        }
    const bool found = key < LOC_INF;
    unsigned long long tb = nan_bits;
    if (found) {
        const double *o = picks + (long long)e * K;
        const double *w = weights ? weights + (long long)e * K : nullptr;
        double t0;
        loc_misfit<0>([&](int k) { return (double)boxes[k][x]; }, K, o, w, invw[e], t0);
        tb = dbits(t0);
    }
    if (cell) cell[e] = found ? x : -1;
    if (misfit) misfit[e] = found ? key : LOC_INF;
    if (t0out) t0out[e] = tb;
}

// ---- sub-cell search (include/ttsweep.h, "locate subcell") ----
// The candidates of an event are the nodes of a lattice of `sub` steps per cell edge inside its window of cells; the
// travel time of a station at a node is the trilinear interpolation of the eight cells around it, in double, seven
// lerps a + u * (b - a) with every operation rounded on its own.  Groups (SubGroup), the block table and the partials
// are those of the windowed search.  A lane decodes its node number q (z fastest, relative to the window) once per
// step, with five divisions: the base cell, which of its three upper neighbours differ from it (f != 0) and ux, uy,
// uz.  It interpolates the K station times once into the register instance and scores the events of the group on
// them with loc_misfit.  q ascends with (qx, qy, qz), so the strict compare of a lane and the lexicographic minimum of
// (bits of J, q) give the smallest node among those of minimal J whatever the grouping.
//   locate_subcell_search_kernel<KR, STAGED>  one block per WinBlock.  STAGED: the block first copies the window's
//                                cells of every station to LDS (K * wn <= LOC_SUB_STAGE floats, decided by the host per
//                                group) and the eight corners are LDS reads; neighbouring nodes share them.  Otherwise
//                                the corners are read from the boxes.  Both write the partial of event i of the
//                                group at [group.part + i * group.ntiles + tile]
//   locate_subcell_final_kernel  one block per event: the smallest of its partials, the node and t0 at it
// (mirrored: tests/test_gpu_locate_subcell.py::test_node_counts_around_the_tile and ::test_both_corner_paths)
constexpr int LOC_SC = 8;               // nodes per lane per sub-cell block: a tile is LOC_SC * LOC_BLOCK nodes
constexpr int LOC_SUB_STAGE = 4096;     // floats of a window (stations x cells) a block stages in LDS, at most

__device__ __forceinline__ double loc_lerp(double a, double b, double u) { return a + u * (b - a); }

// a node as its base cell b (an offset from the window's lo corner in the layout the corners are read from), the
// offsets dx, dy, dz to the upper neighbour along each axis (0 where f == 0: the upper corner is the base cell and
// nothing past the window is read) and the three weights
struct SubNode {
    int b, dx, dy, dz;
    double ux, uy, uz;
};

// node q of a window of ny x nz nodes along y and z; sx, sy: the offset steps of a cell along x and y
__device__ __forceinline__ SubNode sub_decode(unsigned q, unsigned ny, unsigned nz, unsigned sub, int sx, int sy,
                                              unsigned &qx, unsigned &qy, unsigned &qz)
{
    const unsigned qxy = q / nz;
    qz = q - qxy * nz;
    qx = qxy / ny;
    qy = qxy - qx * ny;
    const unsigned ix = qx / sub, iy = qy / sub, iz = qz / sub;
    const unsigned fx = qx - ix * sub, fy = qy - iy * sub, fz = qz - iz * sub;
    SubNode n;
    n.b = (int)ix * sx + (int)iy * sy + (int)iz;
    n.dx = fx ? sx : 0;
    n.dy = fy ? sy : 0;
    n.dz = fz ? 1 : 0;
    n.ux = (double)fx / (double)sub;
    n.uy = (double)fy / (double)sub;
    n.uz = (double)fz / (double)sub;
    return n;
}

// That of the contract: rd(off) is the station's float at offset off
template <typename RD>
__device__ __forceinline__ double sub_time(RD rd, const SubNode &n)
{
    const double c00 = loc_lerp((double)rd(n.b), (double)rd(n.b + n.dz), n.uz);
    const double c01 = loc_lerp((double)rd(n.b + n.dy), (double)rd(n.b + n.dy + n.dz), n.uz);
    const double c10 = loc_lerp((double)rd(n.b + n.dx), (double)rd(n.b + n.dx + n.dz), n.uz);
    const double c11 = loc_lerp((double)rd(n.b + n.dx + n.dy), (double)rd(n.b + n.dx + n.dy + n.dz), n.uz);
    return loc_lerp(loc_lerp(c00, c01, n.uy), loc_lerp(c10, c11, n.uy), n.ux);
}

template <int KR, bool STAGED>
__global__ void __launch_bounds__(LOC_BLOCK)
locate_subcell_search_kernel(const float *const *__restrict__ boxes, int K, int gnyz, int gnz, int sub,
                             const double *__restrict__ picks, const double *__restrict__ weights,
                             const double *__restrict__ invw, const SubGroup *__restrict__ groups,
                             const WinBlock *__restrict__ blocks, unsigned long long *__restrict__ part_key,
                             int *__restrict__ part_x)
{
    __shared__ unsigned long long s_key[LOC_ET][LOC_BLOCK];
    __shared__ int s_x[LOC_ET][LOC_BLOCK];
    __shared__ float s_t[STAGED ? LOC_SUB_STAGE : 1];
    const int tid = threadIdx.x;
    const WinBlock B = blocks[blockIdx.x];              // uniform: scalar loads
    const SubGroup G = groups[B.group];
    const int net = G.ne;
#pragma unroll
    for (int i = 0; i < LOC_ET; i++) {
        s_key[i][tid] = LOC_INF;
        s_x[i][tid] = 0x7fffffff;
    }
    if constexpr (STAGED) {                             // s_t[k * wn + c]: cell c of the window (z fastest), station k
        for (int p = tid; p < K * G.wn; p += LOC_BLOCK) {
            const int k = p / G.wn, c = p - k * G.wn;
            const int cxy = c / G.wz, cz = c - cxy * G.wz;
            const int cx = cxy / G.wy, cy = cxy - cx * G.wy;
            s_t[p] = boxes[k][G.x0 + cx * gnyz + cy * gnz + cz];
        }
        __syncthreads();
    }
    const int sx = STAGED ? G.wy * G.wz : gnyz, sy = STAGED ? G.wz : gnz;
    auto that = [&](int k, const SubNode &n) {
        if constexpr (STAGED) {
            const float *t = s_t + k * G.wn;
            return sub_time([&](int off) { return t[off]; }, n);
        } else {
            const float *t = boxes[k] + G.x0;
            return sub_time([&](int off) { return t[off]; }, n);
        }
    };
    // uniform loops as in locate_search_kernel: lanes past the last node compute it again and keep nothing
    const long long base = (long long)B.tile * (LOC_SC * LOC_BLOCK);
    const int nj = (int)min((long long)LOC_SC, (G.nnode - base + LOC_BLOCK - 1) / LOC_BLOCK);
    for (int j = 0; j < nj; j++) {
        const long long ql = base + (long long)j * LOC_BLOCK + tid;
        const bool in = ql < G.nnode;
        const int q = in ? (int)ql : G.nnode - 1;
        unsigned qx, qy, qz;
        const SubNode n = sub_decode((unsigned)q, (unsigned)G.ny, (unsigned)G.nz, (unsigned)sub, sx, sy, qx, qy, qz);
        double tr[KR > 0 ? KR : 1];
        if constexpr (KR > 0) {
#pragma unroll
            for (int k = 0; k < KR; k++) tr[k] = k < K ? that(k, n) : 0.0;
        }
        for (int i = 0; i < net; i++) {
            const int e = __builtin_amdgcn_readfirstlane(G.e0 + i);
            const double *o = picks + (long long)e * K;
            const double *w = weights ? weights + (long long)e * K : nullptr;
            double t0;
            const double J = KR > 0 ? loc_misfit<KR>([&](int k) { return tr[k]; }, K, o, w, invw[e], t0)
                                    : loc_misfit<0>([&](int k) { return that(k, n); }, K, o, w, invw[e], t0);
            const unsigned long long key = dbits(J);
            if (in && key < s_key[i][tid]) {     // nodes of a lane ascend: strict keeps the smallest q
                s_key[i][tid] = key;
                s_x[i][tid] = q;
            }
        }
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int i = wave; i < net; i += LOC_BLOCK / 64) {
        unsigned long long key = s_key[i][lane];
        int x = s_x[i][lane];
#pragma unroll
        for (int q = 1; q < LOC_BLOCK / 64; q++) {
            const unsigned long long k2 = s_key[i][lane + 64 * q];
            const int x2 = s_x[i][lane + 64 * q];
            if (loc_less(k2, x2, key, x)) {
                key = k2;
                x = x2;
            }
        }
        loc_wave_min(key, x);
        if (lane == 0) {
            const long long p = G.part + (long long)i * G.ntiles + B.tile;
            part_key[p] = key;
            part_x[p] = x;
        }
    }
}

// one block per event e0 + blockIdx.x, of group ev_group[blockIdx.x]: the smallest (J bits, q) of its partials;
// node, misfit and t0 (bits) of it, or ((-1, -1, -1), +INF, nan_bits) when no node is admissible
__global__ void __launch_bounds__(LOC_BLOCK)
locate_subcell_final_kernel(const float *const *__restrict__ boxes, int K, int gnyz, int gnz, int sub,
                            const double *__restrict__ picks, const double *__restrict__ weights,
                            const double *__restrict__ invw, int e0, const int *__restrict__ ev_group,
                            const SubGroup *__restrict__ groups, const unsigned long long *__restrict__ part_key,
                            const int *__restrict__ part_x, int *__restrict__ node,
                            unsigned long long *__restrict__ misfit, unsigned long long *__restrict__ t0out,
                            unsigned long long nan_bits)
{
    __shared__ unsigned long long s_key[LOC_BLOCK / 64];
    __shared__ int s_x[LOC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = e0 + blockIdx.x;
    const SubGroup G = groups[ev_group[blockIdx.x]];
    const long long p0 = G.part + (long long)(e - G.e0) * G.ntiles;
    unsigned long long key = LOC_INF;
    int x = 0x7fffffff;
    for (int t = tid; t < G.ntiles; t += LOC_BLOCK)
        if (loc_less(part_key[p0 + t], part_x[p0 + t], key, x)) {
            key = part_key[p0 + t];
            x = part_x[p0 + t];
        }
    loc_wave_min(key, x);
    if (lane == 0) {
        s_key[wave] = key;
        s_x[wave] = x;
    }
    __syncthreads();
    if (tid) return;
    key = s_key[0];
    x = s_x[0];
    for (int q = 1; q < LOC_BLOCK / 64; q++)
        if (loc_less(s_key[q], s_x[q], key, x)) {
            key = s_key[q];
            x = s_x[q];
        }
    const bool found = key < LOC_INF;
    unsigned long long tb = nan_bits;
    int qn[3] = {-1, -1, -1};
    if (found) {
        unsigned qx, qy, qz;
        const SubNode n = sub_decode((unsigned)x, (unsigned)G.ny, (unsigned)G.nz, (unsigned)sub, gnyz, gnz, qx, qy, qz);
        qn[0] = G.lo[0] * sub + (int)qx;
        qn[1] = G.lo[1] * sub + (int)qy;
        qn[2] = G.lo[2] * sub + (int)qz;
        const double *o = picks + (long long)e * K;
        const double *w = weights ? weights + (long long)e * K : nullptr;
        double t0;
        loc_misfit<0>([&](int k) {
            const float *t = boxes[k] + G.x0;
            return sub_time([&](int off) { return t[off]; }, n);
        }, K, o, w, invw[e], t0);
        tb = dbits(t0);
    }
    if (node)
        for (int a = 0; a < 3; a++) node[3LL * e + a] = qn[a];
    if (misfit) misfit[e] = found ? key : LOC_INF;
    if (t0out) t0out[e] = tb;
}

// ---- confidence regions (include/ttsweep.h, "locate confidence") ----
// R(e, l) = { x admissible and J(x) <= m[e] + delta[e][l] }, summarised without a volume.  J >= +0 on every cell, so
// "admissible and J <= thr" is one unsigned compare of the bits of J with an exclusive limit:
//   lim[e][l] = min(bits(thr) + 1, bits(+INF)), 0 for the empty region (m[e] = +INF); limmax[e] the greatest of them
//   confidence_check_kernel   one lane per event: refuses a NaN or negative m / delta on the bits, forms the limits
//   confidence_init_kernel    the accumulators of every (e, l) at their empty-region values
//   confidence_search_kernel  the cell and event loops of locate_search_kernel with loc_misfit, the same J bits.  Per
//                             (cell step, event) one wave vote on key < limmax[e]; only when a lane is inside do the
//                             lanes inside level l add to the block's accumulators in LDS.  Those atomics have a
//                             wave-uniform address, which the compiler (its atomic optimizer, -S) turns into a
//                             scalar pass over the lanes inside (v_readlane per lane) and one atomic of one lane:
//                             the cost follows the number of cells inside, not the wave width.  At the end of the
//                             block the (event, level) pairs that met a cell add their 18 values to the global
//                             accumulators.
//   confidence_final_kernel   one lane per (e, l): the accumulators to the caller's arrays, t0 keys back to doubles
// Every accumulator is an integer sum, minimum or maximum (t0 through its totalOrder key), so the result does not
// depend on the order of the atomics: no float atomics, no partials, no fixed final order.
constexpr int CONF_LMAX = 4;
constexpr int CONF_NSUM = 10;      // count, x, y, z, xx, yy, zz, xy, xz, yz

// IEEE totalOrder of doubles as an unsigned order of keys, and back
__device__ __forceinline__ unsigned long long conf_t0_key(double t)
{
    const unsigned long long u = dbits(t);
    return u >> 63 ? ~u : u | 0x8000000000000000ULL;
}

__device__ __forceinline__ unsigned long long conf_t0_bits(unsigned long long k)
{
    return k >> 63 ? k & 0x7fffffffffffffffULL : ~k;
}

// flag[e]: bit 0 a NaN or negative m, bit 1 a NaN or negative delta
__global__ void __launch_bounds__(LOC_BLOCK)
confidence_check_kernel(int nevent, int L, const double *__restrict__ m, const double *__restrict__ delta,
                        unsigned long long *__restrict__ lim, unsigned long long *__restrict__ limmax,
                        int *__restrict__ flag)
{
    const int e = blockIdx.x * LOC_BLOCK + threadIdx.x;
    if (e >= nevent) return;
    auto bad = [](unsigned long long u) {      // NaN, or below zero (-0.0 is zero)
        return (u & 0x7fffffffffffffffULL) > LOC_INF || (u >> 63 && (u << 1) != 0);
    };
    const unsigned long long mb = dbits(m[e]);
    int f = bad(mb) ? 1 : 0;
    for (int l = 0; l < L; l++)
        if (bad(dbits(delta[(long long)e * L + l]))) f |= 2;
    unsigned long long top = 0;
    for (int l = 0; l < L; l++) {               // a refused or never located event: the empty region at every level
        unsigned long long t = 0;
        if (!f && mb != LOC_INF) {
            unsigned long long tb = dbits(m[e] + delta[(long long)e * L + l]);
            if ((tb << 1) == 0) tb = 0;
            t = tb >= LOC_INF ? LOC_INF : tb + 1;
        }
        lim[(long long)e * L + l] = t;
        top = t > top ? t : top;
    }
    limmax[e] = top;
    flag[e] = f;
}

__global__ void __launch_bounds__(LOC_BLOCK)
confidence_init_kernel(long long n, int nx, int ny, int nz, unsigned long long *__restrict__ g_sum,
                       unsigned long long *__restrict__ g_t0, int *__restrict__ g_box)
{
    const long long p = (long long)blockIdx.x * LOC_BLOCK + threadIdx.x;
    if (p >= n) return;
    for (int q = 0; q < CONF_NSUM; q++) g_sum[p * CONF_NSUM + q] = 0;
    g_t0[p * 2] = ~0ULL;
    g_t0[p * 2 + 1] = 0;
    g_box[p * 6] = nx;
    g_box[p * 6 + 1] = ny;
    g_box[p * 6 + 2] = nz;
    g_box[p * 6 + 3] = g_box[p * 6 + 4] = g_box[p * 6 + 5] = -1;
}

// blockIdx.x: a tile of LOC_C * LOC_BLOCK cells; blockIdx.y: LOC_ET events from e0
template <int KR>
__global__ void __launch_bounds__(LOC_BLOCK)
confidence_search_kernel(const float *const *__restrict__ boxes, int K, int N, int ny, int nz,
                         const double *__restrict__ picks, const double *__restrict__ weights,
                         const double *__restrict__ invw, int e0, int ne, int L,
                         const unsigned long long *__restrict__ lim, const unsigned long long *__restrict__ limmax,
                         unsigned long long *__restrict__ g_sum, unsigned long long *__restrict__ g_t0,
                         int *__restrict__ g_box)
{
    __shared__ unsigned long long s_sum[LOC_ET * CONF_LMAX][CONF_NSUM];
    __shared__ unsigned long long s_t0[LOC_ET * CONF_LMAX][2];
    __shared__ int s_box[LOC_ET * CONF_LMAX][6];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int eb = blockIdx.y * LOC_ET;                 // first event of the block, relative to e0
    const int net = min(LOC_ET, ne - eb);
    if (tid < LOC_ET * CONF_LMAX) {
        for (int q = 0; q < CONF_NSUM; q++) s_sum[tid][q] = 0;
        s_t0[tid][0] = ~0ULL;
        s_t0[tid][1] = 0;
        s_box[tid][0] = s_box[tid][1] = s_box[tid][2] = 0x7fffffff;
        s_box[tid][3] = s_box[tid][4] = s_box[tid][5] = -1;
    }
    __syncthreads();
    const long long base = (long long)tile * (LOC_C * LOC_BLOCK);
    const int nj = (int)min((long long)LOC_C, (N - base + LOC_BLOCK - 1) / LOC_BLOCK);
    const int nyz = ny * nz;
    for (int j = 0; j < nj; j++) {
        const long long xl = base + (long long)j * LOC_BLOCK + tid;
        const bool in = xl < N;
        const int x = in ? (int)xl : N - 1;
        double tr[KR > 0 ? KR : 1];
        if constexpr (KR > 0) {
#pragma unroll
            for (int k = 0; k < KR; k++) tr[k] = k < K ? (double)boxes[k][x] : 0.0;
        }
        for (int i = 0; i < net; i++) {
            const int e = __builtin_amdgcn_readfirstlane(e0 + eb + i);
            const double *o = picks + (long long)e * K;
            const double *w = weights ? weights + (long long)e * K : nullptr;
            double t0;
            const double J = KR > 0 ? loc_misfit<KR>([&](int k) { return tr[k]; }, K, o, w, invw[e], t0)
                                    : loc_misfit<0>([&](int k) { return (double)boxes[k][x]; }, K, o, w, invw[e], t0);
            const unsigned long long key = dbits(J);
            if (!__any(in && key < limmax[e])) continue;        // the common case: no lane of the wave is inside
            const unsigned long long cx = (unsigned)(x / nyz), cy = (unsigned)(x % nyz / nz), cz = (unsigned)(x % nz);
            const unsigned long long tk = conf_t0_key(t0);
            for (int l = 0; l < L; l++) {
                if (!(in && key < lim[(long long)e * L + l])) continue;
                const int a = i * CONF_LMAX + l;                // wave-uniform: one atomic of one lane per value
                atomicAdd(&s_sum[a][0], 1ULL);
                atomicAdd(&s_sum[a][1], cx);
                atomicAdd(&s_sum[a][2], cy);
                atomicAdd(&s_sum[a][3], cz);
                atomicAdd(&s_sum[a][4], cx * cx);
                atomicAdd(&s_sum[a][5], cy * cy);
                atomicAdd(&s_sum[a][6], cz * cz);
                atomicAdd(&s_sum[a][7], cx * cy);
                atomicAdd(&s_sum[a][8], cx * cz);
                atomicAdd(&s_sum[a][9], cy * cz);
                atomicMin(&s_t0[a][0], tk);
                atomicMax(&s_t0[a][1], tk);
                atomicMin(&s_box[a][0], (int)cx);
                atomicMin(&s_box[a][1], (int)cy);
                atomicMin(&s_box[a][2], (int)cz);
                atomicMax(&s_box[a][3], (int)cx);
                atomicMax(&s_box[a][4], (int)cy);
                atomicMax(&s_box[a][5], (int)cz);
            }
        }
    }
    __syncthreads();
    if (tid >= net * CONF_LMAX || (tid & (CONF_LMAX - 1)) >= L || s_sum[tid][0] == 0) return;
    const long long p = (long long)(e0 + eb + tid / CONF_LMAX) * L + (tid & (CONF_LMAX - 1));
    for (int q = 0; q < CONF_NSUM; q++) atomicAdd(&g_sum[p * CONF_NSUM + q], s_sum[tid][q]);
    atomicMin(&g_t0[p * 2], s_t0[tid][0]);
    atomicMax(&g_t0[p * 2 + 1], s_t0[tid][1]);
    for (int q = 0; q < 3; q++) {
        atomicMin(&g_box[p * 6 + q], s_box[tid][q]);
        atomicMax(&g_box[p * 6 + 3 + q], s_box[tid][3 + q]);
    }
}

// one lane per (e, l); every output may be nullptr
__global__ void __launch_bounds__(LOC_BLOCK)
confidence_final_kernel(long long n, const unsigned long long *__restrict__ g_sum,
                        const unsigned long long *__restrict__ g_t0, const int *__restrict__ g_box,
                        long long *__restrict__ count, long long *__restrict__ sum, long long *__restrict__ sum2,
                        int *__restrict__ lo, int *__restrict__ hi, unsigned long long *__restrict__ t0_lo,
                        unsigned long long *__restrict__ t0_hi)
{
    const long long p = (long long)blockIdx.x * LOC_BLOCK + threadIdx.x;
    if (p >= n) return;
    const unsigned long long *s = g_sum + p * CONF_NSUM;
    const bool any = s[0] != 0;
    if (count) count[p] = (long long)s[0];
    for (int q = 0; q < 3; q++) {
        if (sum) sum[p * 3 + q] = (long long)s[1 + q];
        if (lo) lo[p * 3 + q] = g_box[p * 6 + q];
        if (hi) hi[p * 3 + q] = g_box[p * 6 + 3 + q];
    }
    if (sum2)
        for (int q = 0; q < 6; q++) sum2[p * 6 + q] = (long long)s[4 + q];
    if (t0_lo) t0_lo[p] = any ? conf_t0_bits(g_t0[p * 2]) : LOC_INF;
    if (t0_hi) t0_hi[p] = any ? conf_t0_bits(g_t0[p * 2 + 1]) : LOC_INF | 0x8000000000000000ULL;
}

int locate_tile_cells() { return LOC_C * LOC_BLOCK; }

hipError_t launch_confidence_check(int nevent, int L, const double *m, const double *delta, unsigned long long *lim,
                                   unsigned long long *limmax, int *flag, hipStream_t st)
{
    hipLaunchKernelGGL(confidence_check_kernel, dim3((nevent + LOC_BLOCK - 1) / LOC_BLOCK), dim3(LOC_BLOCK), 0, st,
                       nevent, L, m, delta, lim, limmax, flag);
    return hipGetLastError();
}

hipError_t launch_confidence_init(long long n, int nx, int ny, int nz, unsigned long long *g_sum,
                                  unsigned long long *g_t0, int *g_box, hipStream_t st)
{
    hipLaunchKernelGGL(confidence_init_kernel, dim3((unsigned)((n + LOC_BLOCK - 1) / LOC_BLOCK)), dim3(LOC_BLOCK), 0,
                       st, n, nx, ny, nz, g_sum, g_t0, g_box);
    return hipGetLastError();
}

hipError_t launch_confidence_final(long long n, const unsigned long long *g_sum, const unsigned long long *g_t0,
                                   const int *g_box, long long *count, long long *sum, long long *sum2, int *lo,
                                   int *hi, double *t0_lo, double *t0_hi, hipStream_t st)
{
    hipLaunchKernelGGL(confidence_final_kernel, dim3((unsigned)((n + LOC_BLOCK - 1) / LOC_BLOCK)), dim3(LOC_BLOCK), 0,
                       st, n, g_sum, g_t0, g_box, count, sum, sum2, lo, hi, (unsigned long long *)t0_lo,
                       (unsigned long long *)t0_hi);
    return hipGetLastError();
}

hipError_t launch_locate_check(int K, int nevent, const double *picks, const double *weights, double *invw, int *flag,
                               hipStream_t st)
{
    if (nevent <= 0) return hipSuccess;
    hipLaunchKernelGGL(locate_check_kernel, dim3((nevent + LOC_BLOCK - 1) / LOC_BLOCK), dim3(LOC_BLOCK), 0, st, K,
                       nevent, picks, weights, invw, flag);
    return hipGetLastError();
}

// the register width of the stations: the smallest of 8 / 16 / 24 / 32 that holds K, 0 (read T on use) above 32
static int loc_kr(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : K <= 24 ? 24 : K <= 32 ? 32 : 0; }

hipError_t launch_locate_search(const float *const *boxes, int K, int N, const double *picks, const double *weights,
                                const double *invw, int e0, int ne, int ntiles, unsigned long long *part_key,
                                int *part_x, hipStream_t st)
{
    if (ne <= 0 || ntiles <= 0) return hipSuccess;
    const dim3 grid(ntiles, (ne + LOC_ET - 1) / LOC_ET);
    if (grid.y > 65535) return hipErrorInvalidValue;
    switch (loc_kr(K)) {
    case 8: hipLaunchKernelGGL(locate_search_kernel<8>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                               invw, e0, ne, ntiles, part_key, part_x); break;
    case 16: hipLaunchKernelGGL(locate_search_kernel<16>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                                invw, e0, ne, ntiles, part_key, part_x); break;
    case 24: hipLaunchKernelGGL(locate_search_kernel<24>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                                invw, e0, ne, ntiles, part_key, part_x); break;
    case 32: hipLaunchKernelGGL(locate_search_kernel<32>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                                invw, e0, ne, ntiles, part_key, part_x); break;
    default: hipLaunchKernelGGL(locate_search_kernel<0>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                                invw, e0, ne, ntiles, part_key, part_x); break;
    }
    return hipGetLastError();
}

hipError_t launch_locate_final(const float *const *boxes, int K, const double *picks, const double *weights,
                               const double *invw, int e0, int ne, int ntiles, const unsigned long long *part_key,
                               const int *part_x, int *cell, double *misfit, double *t0, unsigned long long nan_bits,
                               hipStream_t st)
{
    if (ne <= 0) return hipSuccess;
    hipLaunchKernelGGL(locate_final_kernel<0>, dim3(ne), dim3(LOC_BLOCK), 0, st, boxes, K, picks, weights, invw, e0,
                       ntiles, part_key, part_x, cell, (unsigned long long *)misfit, (unsigned long long *)t0,
                       nan_bits);
    return hipGetLastError();
}

hipError_t launch_locate_volume(const float *const *boxes, int K, int N, const double *picks, const double *weights,
                                const double *invw, const int *vev, double *const *vol, int nvol, hipStream_t st)
{
    if (nvol <= 0 || N <= 0) return hipSuccess;
    const dim3 grid((N + LOC_BLOCK - 1) / LOC_BLOCK, nvol);
    if (grid.y > 65535) return hipErrorInvalidValue;
    auto v = (unsigned long long *const *)vol;
    switch (loc_kr(K)) {
    case 8: hipLaunchKernelGGL(locate_volume_kernel<8>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                               invw, vev, v); break;
    case 16: hipLaunchKernelGGL(locate_volume_kernel<16>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                                invw, vev, v); break;
    case 24: hipLaunchKernelGGL(locate_volume_kernel<24>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                                invw, vev, v); break;
    case 32: hipLaunchKernelGGL(locate_volume_kernel<32>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                                invw, vev, v); break;
    default: hipLaunchKernelGGL(locate_volume_kernel<0>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks, weights,
                                invw, vev, v); break;
    }
    return hipGetLastError();
}

int locate_window_tile_cells() { return LOC_WC * LOC_BLOCK; }

hipError_t launch_locate_window_search(const float *const *boxes, int K, int mx, int my, int mz,
                                       const double *picks, const double *weights, const double *invw,
                                       const WinGroup *groups, const WinBlock *blocks, int nblocks,
                                       unsigned long long *part_key, int *part_x, hipStream_t st)
{
    if (nblocks <= 0) return hipSuccess;
    const dim3 grid(nblocks);
    switch (loc_kr(K)) {
    case 8: hipLaunchKernelGGL(locate_window_search_kernel<8>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, mx, my, mz,
                                picks, weights, invw, groups, blocks, part_key, part_x); break;
    case 16: hipLaunchKernelGGL(locate_window_search_kernel<16>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, mx, my, mz,
                                picks, weights, invw, groups, blocks, part_key, part_x); break;
    case 24: hipLaunchKernelGGL(locate_window_search_kernel<24>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, mx, my, mz,
                                picks, weights, invw, groups, blocks, part_key, part_x); break;
    case 32: hipLaunchKernelGGL(locate_window_search_kernel<32>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, mx, my, mz,
                                picks, weights, invw, groups, blocks, part_key, part_x); break;
    default: hipLaunchKernelGGL(locate_window_search_kernel<0>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, mx, my, mz,
                                picks, weights, invw, groups, blocks, part_key, part_x); break;
    }
    return hipGetLastError();
}

hipError_t launch_locate_window_final(const float *const *boxes, int K, const double *picks, const double *weights,
                                      const double *invw, int e0, int ne, const long long *ev_part,
                                      const int *ev_ntiles, const unsigned long long *part_key, const int *part_x,
                                      int *cell, double *misfit, double *t0, unsigned long long nan_bits,
                                      hipStream_t st)
{
    if (ne <= 0) return hipSuccess;
    hipLaunchKernelGGL(locate_window_final_kernel, dim3(ne), dim3(LOC_BLOCK), 0, st, boxes, K, picks, weights, invw, e0,
                       ev_part, ev_ntiles, part_key, part_x, cell, (unsigned long long *)misfit,
                       (unsigned long long *)t0, nan_bits);
    return hipGetLastError();
}

int locate_subcell_tile_nodes() { return LOC_SC * LOC_BLOCK; }
int locate_subcell_stage_floats() { return LOC_SUB_STAGE; }

template <bool STAGED>
static void launch_subcell_search_kr(dim3 grid, hipStream_t st, const float *const *boxes, int K, int gnyz, int gnz,
                                     int sub, const double *picks, const double *weights, const double *invw,
                                     const SubGroup *groups, const WinBlock *blocks, unsigned long long *part_key,
                                     int *part_x)
{
    switch (loc_kr(K)) {
    case 8: hipLaunchKernelGGL((locate_subcell_search_kernel<8, STAGED>), grid, dim3(LOC_BLOCK), 0, st, boxes, K, gnyz,
                               gnz, sub, picks, weights, invw, groups, blocks, part_key, part_x); break;
    case 16: hipLaunchKernelGGL((locate_subcell_search_kernel<16, STAGED>), grid, dim3(LOC_BLOCK), 0, st, boxes, K, gnyz,
                                gnz, sub, picks, weights, invw, groups, blocks, part_key, part_x); break;
    case 24: hipLaunchKernelGGL((locate_subcell_search_kernel<24, STAGED>), grid, dim3(LOC_BLOCK), 0, st, boxes, K, gnyz,
                                gnz, sub, picks, weights, invw, groups, blocks, part_key, part_x); break;
    case 32: hipLaunchKernelGGL((locate_subcell_search_kernel<32, STAGED>), grid, dim3(LOC_BLOCK), 0, st, boxes, K, gnyz,
                                gnz, sub, picks, weights, invw, groups, blocks, part_key, part_x); break;
    default: hipLaunchKernelGGL((locate_subcell_search_kernel<0, STAGED>), grid, dim3(LOC_BLOCK), 0, st, boxes, K, gnyz,
                                gnz, sub, picks, weights, invw, groups, blocks, part_key, part_x); break;
    }
}

hipError_t launch_locate_subcell_search(const float *const *boxes, int K, int gnyz, int gnz, int sub,
                                        const double *picks, const double *weights, const double *invw,
                                        const SubGroup *groups, const WinBlock *blocks, int nblocks, bool staged,
                                        unsigned long long *part_key, int *part_x, hipStream_t st)
{
    if (nblocks <= 0) return hipSuccess;
    if (staged)
        launch_subcell_search_kr<true>(dim3(nblocks), st, boxes, K, gnyz, gnz, sub, picks, weights, invw, groups,
                                       blocks, part_key, part_x);
    else
        launch_subcell_search_kr<false>(dim3(nblocks), st, boxes, K, gnyz, gnz, sub, picks, weights, invw, groups,
                                        blocks, part_key, part_x);
    return hipGetLastError();
}

hipError_t launch_locate_subcell_final(const float *const *boxes, int K, int gnyz, int gnz, int sub,
                                       const double *picks, const double *weights, const double *invw, int e0, int ne,
                                       const int *ev_group, const SubGroup *groups,
                                       const unsigned long long *part_key, const int *part_x, int *node,
                                       double *misfit, double *t0, unsigned long long nan_bits, hipStream_t st)
{
    if (ne <= 0) return hipSuccess;
    hipLaunchKernelGGL(locate_subcell_final_kernel, dim3(ne), dim3(LOC_BLOCK), 0, st, boxes, K, gnyz, gnz, sub, picks,
                       weights, invw, e0, ev_group, groups, part_key, part_x, node, (unsigned long long *)misfit,
                       (unsigned long long *)t0, nan_bits);
    return hipGetLastError();
}

hipError_t launch_confidence_search(const float *const *boxes, int K, int N, int ny, int nz, const double *picks,
                                    const double *weights, const double *invw, int e0, int ne, int L,
                                    const unsigned long long *lim, const unsigned long long *limmax,
                                    unsigned long long *g_sum, unsigned long long *g_t0, int *g_box, hipStream_t st)
{
    if (ne <= 0 || N <= 0) return hipSuccess;
    const int ntiles = (int)(((long long)N + LOC_C * LOC_BLOCK - 1) / (LOC_C * LOC_BLOCK));
    const dim3 grid(ntiles, (ne + LOC_ET - 1) / LOC_ET);
    if (grid.y > 65535 || L < 1 || L > CONF_LMAX) return hipErrorInvalidValue;
    switch (loc_kr(K)) {
    case 8: hipLaunchKernelGGL(confidence_search_kernel<8>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, ny, nz, picks,
                               weights, invw, e0, ne, L, lim, limmax, g_sum, g_t0, g_box); break;
    case 16: hipLaunchKernelGGL(confidence_search_kernel<16>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, ny, nz, picks,
                                weights, invw, e0, ne, L, lim, limmax, g_sum, g_t0, g_box); break;
    case 24: hipLaunchKernelGGL(confidence_search_kernel<24>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, ny, nz, picks,
                                weights, invw, e0, ne, L, lim, limmax, g_sum, g_t0, g_box); break;
    case 32: hipLaunchKernelGGL(confidence_search_kernel<32>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, ny, nz, picks,
                                weights, invw, e0, ne, L, lim, limmax, g_sum, g_t0, g_box); break;
    default: hipLaunchKernelGGL(confidence_search_kernel<0>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, ny, nz, picks,
                                weights, invw, e0, ne, L, lim, limmax, g_sum, g_t0, g_box); break;
    }
    return hipGetLastError();
}

} // namespace ttsweep
