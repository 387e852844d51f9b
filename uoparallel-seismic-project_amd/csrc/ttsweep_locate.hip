// ttsweep_locate.hip - grid-search event location over station travel-time boxes (include/ttsweep.h, "locate").
//
// By reciprocity T_k[x] is the travel time between station k and a candidate hypocentre x.  For every event e
// and candidate x the weighted L2 misfit of the picks with the origin time eliminated is, in double, stations in
// ascending k, zero weights skipped (-ffp-contract=off: every operation rounded on its own):
//   S1 = S1 + w * (o - (double)T)        t0 = S1 * invW        J = J + (w * r) * r,  r = (o - (double)T) - t0
// Every search is one scan with two parameters:
//   loc_scan<KR, PER>   the step loop of a block over its tile of PER * LOC_BLOCK candidates: cand(q) turns candidate
//                       number q into an id and the travel times of the K stations, which the lane loads once and
//                       scores the block's events on (loc_misfit); sink(...) takes every (event, candidate) score
//   loc_search_min      the scan with the sink all three argmin searches share: the lane keeps its best (J bits, id)
//                       per event in LDS across its candidates, then one wave reduction per event gives the tile's
//                       partial
//   loc_partial_min, loc_store   the final of an event: the smallest of its partials, then its place, misfit and t0
// The kernels only say what a candidate is and where the partials lie:
//   locate_check_kernel     one lane per event: refuses non-finite picks, negative / non-finite weights and
//                           events without a weight (flag per event, on the bits: the library is built with
//                           -fno-honor-nans) and computes invW = 1.0 / W
//   locate_search_kernel, locate_final_kernel   candidate q is cell q of the grid; LOC_ET events per block
//   locate_volume_kernel    J (+INF where inadmissible) of every cell for a list of events, one cell per lane
//   locate_window_*_kernel  the candidates are a lattice inside a window per group of events ("locate window")
//   locate_subcell_*_kernel the candidates are the nodes of a finer lattice inside a window of cells, the station
//                           times interpolated trilinearly ("locate subcell")
//   confidence_*_kernel     the scan over the grid with a sink that accumulates regions ("locate confidence")
// A candidate is inadmissible when a picked station has T >= +INFINITY or J is not below +INFINITY.  The first
// implies the second in IEEE arithmetic (o - INF = -INF enters S1, so t0 is -INF or NaN and r of that station is
// NaN), so one test on the bits of J covers both: J >= 0 always, and +INF and every NaN compare above it as unsigned
// integers.  The argmin is the lexicographic minimum of (bits of J, id): the same whatever order the tiles, lanes
// and waves are combined in, so results do not depend on the launch or on which events share a batch.  No float
// atomics.  T is read through (double) of the float: exact.
#include "ttsweep_kernels.h"

#include "../../include/ttsweep.h"

#include <type_traits>

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

// f(k) of the picked stations k < K of an event with weights w, in ascending order: unrolled over a register width
// KR >= K, or a loop when KR == 0
template <int KR, typename F>
__device__ __forceinline__ void loc_stations(int K, const double *__restrict__ w, F f)
{
    if constexpr (KR > 0) {
#pragma unroll
        for (int k = 0; k < KR; k++)
            if (k < K && loc_picked(w, k)) f(k);
    } else {
        for (int k = 0; k < K; k++)
            if (loc_picked(w, k)) f(k);
    }
}

// J and t0 of event e at the candidate whose travel times are t(k), the semantics of include/ttsweep.h
template <int KR, typename TF>
__device__ __forceinline__ double loc_misfit(TF t, int e, int K, const double *__restrict__ picks,
                                             const double *__restrict__ weights, const double *__restrict__ invw,
                                             double &t0)
{
    const double *o = picks + (long long)e * K;
    const double *w = weights ? weights + (long long)e * K : nullptr;
    double s1 = 0.0, J = 0.0;
    loc_stations<KR>(K, w, [&](int k) {
        const double d = o[k] - t(k);
        s1 = s1 + loc_w(w, k) * d;
    });
    t0 = s1 * invw[e];
    loc_stations<KR>(K, w, [&](int k) {
        const double r = (o[k] - t(k)) - t0;
        J = J + (loc_w(w, k) * r) * r;
    });
    return J;
}

// A candidate: the id its score is kept under and time(k), the travel time of station k there
template <typename Time>
struct LocCand {
    int id;
    Time time;
};
template <typename Time>
__device__ __forceinline__ LocCand<Time> loc_cand(int id, Time time) { return {id, time}; }

// cell x of the grid
__device__ __forceinline__ auto loc_cell(const float *const *__restrict__ boxes, int x)
{
    return loc_cand(x, [=](int k) { return (double)boxes[k][x]; });
}

// The K travel times of a candidate, loaded once into tr (KR > 0) for all the events scored on it; with more than 32
// stations (KR == 0) they are read on use
template <int KR, typename Time>
__device__ __forceinline__ void loc_load(Time time, int K, double (&tr)[KR > 0 ? KR : 1])
{
    if constexpr (KR > 0) {
#pragma unroll
        for (int k = 0; k < KR; k++) tr[k] = k < K ? time(k) : 0.0;
    }
}

template <int KR, typename Time>
__device__ __forceinline__ double loc_score(const double (&tr)[KR > 0 ? KR : 1], Time time, int e, int K,
                                            const double *__restrict__ picks, const double *__restrict__ weights,
                                            const double *__restrict__ invw, double &t0)
{
    return KR > 0 ? loc_misfit<KR>([&](int k) { return tr[k]; }, e, K, picks, weights, invw, t0)
                  : loc_misfit<0>(time, e, K, picks, weights, invw, t0);
}

// The step loop of a search block: its tile of PER * LOC_BLOCK of the ncand candidates, one per lane and step, scored
// for the net events from first_event.  sink(i, e, in, id, key, t0) takes the score of event e = first_event + i at
// the lane's candidate: key the bits of J, in false for the lanes past the last candidate.  The step loop and the event
// loop are uniform (those lanes compute the last candidate again and must keep nothing), so the picks and weights are
// uniform loads and a zero weight is a uniform branch.
template <int KR, int PER, typename Cand, typename Sink>
__device__ __forceinline__ void loc_scan(int ncand, int tile, int net, int first_event, int K,
                                         const double *__restrict__ picks, const double *__restrict__ weights,
                                         const double *__restrict__ invw, Cand cand, Sink sink)
{
    const long long base = (long long)tile * (PER * LOC_BLOCK);
    const int nj = (int)min((long long)PER, (ncand - base + LOC_BLOCK - 1) / LOC_BLOCK);
    for (int j = 0; j < nj; j++) {
        const long long ql = base + (long long)j * LOC_BLOCK + threadIdx.x;
        const bool in = ql < ncand;
        const auto c = cand(in ? (int)ql : ncand - 1);
        double tr[KR > 0 ? KR : 1];
        loc_load<KR>(c.time, K, tr);
        for (int i = 0; i < net; i++) {
            const int e = __builtin_amdgcn_readfirstlane(first_event + i);
            double t0;
            const double J = loc_score<KR>(tr, c.time, e, K, picks, weights, invw, t0);
            sink(i, e, in, c.id, dbits(J), t0);
        }
    }
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

// The scan of an argmin search.  Writes part_key / part_x [part + (row + i) * ntiles + tile] (J bits, id) of the best
// admissible candidate of the tile for event i of the block, (+INF bits, INT_MAX) when none.  The ids of a lane must
// ascend with q: then the lexicographic minimum of (bits of J, id) is the smallest id among the candidates of minimal
// J whatever the tiling and the grouping.
template <int KR, int PER, typename Cand>
__device__ __forceinline__ void loc_search_min(int ncand, int tile, int net, int first_event, int K,
                                               const double *__restrict__ picks, const double *__restrict__ weights,
                                               const double *__restrict__ invw, Cand cand, long long part, int row,
                                               int ntiles, unsigned long long *__restrict__ part_key,
                                               int *__restrict__ part_x)
{
    __shared__ unsigned long long s_key[LOC_ET][LOC_BLOCK];
    __shared__ int s_x[LOC_ET][LOC_BLOCK];
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < LOC_ET; i++) {
        s_key[i][tid] = LOC_INF;
        s_x[i][tid] = 0x7fffffff;
    }
    loc_scan<KR, PER>(ncand, tile, net, first_event, K, picks, weights, invw, cand,
                      [&](int i, int, bool in, int id, unsigned long long key, double) {
                          if (in && key < s_key[i][tid]) {     // ids of a lane ascend: strict keeps the smallest id
                              s_key[i][tid] = key;
                              s_x[i][tid] = id;
                          }
                      });
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
            const long long p = part + (long long)(row + i) * ntiles + tile;
            part_key[p] = key;
            part_x[p] = x;
        }
    }
}

// The smallest (J bits, id) of the ntiles partials from p0, by a block; the result is in thread 0 only
__device__ __forceinline__ void loc_partial_min(const unsigned long long *__restrict__ part_key,
                                                const int *__restrict__ part_x, long long p0, int ntiles,
                                                unsigned long long &key, int &x)
{
    __shared__ unsigned long long s_key[LOC_BLOCK / 64];
    __shared__ int s_x[LOC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    key = LOC_INF;
    x = 0x7fffffff;
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
}

// The outputs of event e from its smallest partial (key, x), by one thread: misfit and t0 (bits) of it, or (+INF,
// nan_bits) when no candidate is admissible (the NaN comes from the host).  place(found, x) writes where the
// candidate is (its "nowhere" unless found) and returns its time(k), which is used only when found.
template <typename Place>
__device__ __forceinline__ void loc_store(int e, unsigned long long key, int x, int K, const double *__restrict__ picks,
                                          const double *__restrict__ weights, const double *__restrict__ invw,
                                          unsigned long long *__restrict__ misfit,
                                          unsigned long long *__restrict__ t0out, unsigned long long nan_bits,
                                          Place place)
{
    const bool found = key < LOC_INF;
    const auto time = place(found, x);
    unsigned long long tb = nan_bits;
    if (found) {
        double t0;
        loc_misfit<0>(time, e, K, picks, weights, invw, t0);
        tb = dbits(t0);
    }
    if (misfit) misfit[e] = found ? key : LOC_INF;
    if (t0out) t0out[e] = tb;
}

// place of loc_store for the searches over cells: cell[e] = x, or -1
__device__ __forceinline__ auto loc_place_cell(const float *const *__restrict__ boxes, int *__restrict__ cell, int e)
{
    return [=](bool found, int x) {
        if (cell) cell[e] = found ? x : -1;
        return loc_cell(boxes, x).time;
    };
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

// blockIdx.x: a tile of LOC_C * LOC_BLOCK cells; blockIdx.y: LOC_ET events from e0.  The partials of event e are
// [(e - e0) * ntiles + tile]
template <int KR>
__global__ void __launch_bounds__(LOC_BLOCK)
locate_search_kernel(const float *const *__restrict__ boxes, int K, int N, const double *__restrict__ picks,
                     const double *__restrict__ weights, const double *__restrict__ invw, int e0, int ne, int ntiles,
                     unsigned long long *__restrict__ part_key, int *__restrict__ part_x)
{
    const int tile = blockIdx.x;
    const int eb = blockIdx.y * LOC_ET;                 // first event of the block, relative to e0
    loc_search_min<KR, LOC_C>(N, tile, min(LOC_ET, ne - eb), e0 + eb, K, picks, weights, invw,
                              [&](int x) { return loc_cell(boxes, x); }, 0, eb, ntiles, part_key,
                              part_x);
}

// one block per event e0 + blockIdx.x: cell, misfit and t0 of the smallest (J bits, x) over the tiles, cell -1 when
// no cell is admissible
__global__ void __launch_bounds__(LOC_BLOCK)
locate_final_kernel(const float *const *__restrict__ boxes, int K, const double *__restrict__ picks,
                    const double *__restrict__ weights, const double *__restrict__ invw, int e0, int ntiles,
                    const unsigned long long *__restrict__ part_key, const int *__restrict__ part_x,
                    int *__restrict__ cell, unsigned long long *__restrict__ misfit, unsigned long long *__restrict__ t0out,
                    unsigned long long nan_bits)
{
    const int e = e0 + blockIdx.x;
    unsigned long long key;
    int x;
    loc_partial_min(part_key, part_x, (long long)blockIdx.x * ntiles, ntiles, key, x);
    if (threadIdx.x) return;
    loc_store(e, key, x, K, picks, weights, invw, misfit, t0out, nan_bits, loc_place_cell(boxes, cell, e));
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
    const auto time = loc_cell(boxes, x).time;
    double tr[KR > 0 ? KR : 1], t0;
    loc_load<KR>(time, K, tr);
    const unsigned long long key = dbits(loc_score<KR>(tr, time, e, K, picks, weights, invw, t0));
    vol[blockIdx.y][x] = key < LOC_INF ? key : LOC_INF;
}

// ---- windowed, strided search (include/ttsweep.h, "locate window") ----
// The candidates of an event are the nodes of a lattice inside its window.  The host cuts the events into groups of at
// most LOC_ET consecutive events with one window (WinGroup) and lists every (group, tile of LOC_WC * LOC_BLOCK
// candidates) as a block (WinBlock).  A lane decodes its candidate number q (z fastest) to a cell once per step, with
// two divisions; the id is the cell index, which ascends with q.
//   locate_window_search_kernel  one block per WinBlock; the partial of event i of the group at
//                                [group.part + i * group.ntiles + tile]
//   locate_window_final_kernel   one block per event, of group ev_group[e - e0]: the outputs of locate_final_kernel
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
    const WinBlock B = blocks[blockIdx.x];              // uniform: scalar loads
    const WinGroup G = groups[B.group];
    auto cand = [&](int qi) {
        const unsigned q = (unsigned)qi;
        const unsigned qxy = q / (unsigned)G.cz, cz = q - qxy * (unsigned)G.cz;
        const unsigned cx = qxy / (unsigned)G.cy, cy = qxy - cx * (unsigned)G.cy;
        return loc_cell(boxes, G.x0 + (int)cx * mx + (int)cy * my + (int)cz * mz);
    };
    loc_search_min<KR, LOC_WC>(G.ncand, B.tile, G.ne, G.e0, K, picks, weights, invw, cand, G.part, 0, G.ntiles,
                               part_key, part_x);
}

__global__ void __launch_bounds__(LOC_BLOCK)
locate_window_final_kernel(const float *const *__restrict__ boxes, int K, const double *__restrict__ picks,
                           const double *__restrict__ weights, const double *__restrict__ invw, int e0,
                           const int *__restrict__ ev_group, const WinGroup *__restrict__ groups,
                           const unsigned long long *__restrict__ part_key, const int *__restrict__ part_x,
                           int *__restrict__ cell, unsigned long long *__restrict__ misfit,
                           unsigned long long *__restrict__ t0out, unsigned long long nan_bits)
{
    const int e = e0 + blockIdx.x;
    const WinGroup G = groups[ev_group[blockIdx.x]];
    unsigned long long key;
    int x;
    loc_partial_min(part_key, part_x, G.part + (long long)(e - G.e0) * G.ntiles, G.ntiles, key, x);
    if (threadIdx.x) return;
    loc_store(e, key, x, K, picks, weights, invw, misfit, t0out, nan_bits, loc_place_cell(boxes, cell, e));
}

// ---- sub-cell search (include/ttsweep.h, "locate subcell") ----
// The candidates of an event are the nodes of a lattice of `sub` steps per cell edge inside its window of cells; the
// travel time of a station at a node is the trilinear interpolation of the eight cells around it, in double, seven
// lerps a + u * (b - a) with every operation rounded on its own.  Groups (SubGroup), the block table and the partials
// are those of the windowed search.  A lane decodes its node number q (z fastest, relative to the window) once per
// step, with five divisions: the base cell, which of its three upper neighbours differ from it (f != 0) and ux, uy,
// uz.  The id is q, which ascends with (qx, qy, qz).
//   locate_subcell_search_kernel<KR, STAGED>  one block per WinBlock.  STAGED: the block first copies the window's
//                                cells of every station to LDS (K * wn <= LOC_SUB_STAGE floats, decided by the host per
//                                group) and the eight corners are LDS reads; neighbouring nodes share them.  Otherwise
//                                the corners are read from the boxes.  Both write the partial of event i of the
//                                group at [group.part + i * group.ntiles + tile]
//   locate_subcell_final_kernel  one block per event, of group ev_group[e - e0]: the smallest of its partials, the
//                                node (-1, -1, -1 when no node is admissible), misfit and t0 at it
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

// That of the contract: t[off] is the station's float at offset off from the window's lo corner
__device__ __forceinline__ double sub_time(const float *t, const SubNode &n)
{
    const double c00 = loc_lerp((double)t[n.b], (double)t[n.b + n.dz], n.uz);
    const double c01 = loc_lerp((double)t[n.b + n.dy], (double)t[n.b + n.dy + n.dz], n.uz);
    const double c10 = loc_lerp((double)t[n.b + n.dx], (double)t[n.b + n.dx + n.dz], n.uz);
    const double c11 = loc_lerp((double)t[n.b + n.dx + n.dy], (double)t[n.b + n.dx + n.dy + n.dz], n.uz);
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
    __shared__ float s_t[STAGED ? LOC_SUB_STAGE : 1];
    const WinBlock B = blocks[blockIdx.x];              // uniform: scalar loads
    const SubGroup G = groups[B.group];
    if constexpr (STAGED) {                             // s_t[k * wn + c]: cell c of the window (z fastest), station k
        for (int p = threadIdx.x; p < K * G.wn; p += LOC_BLOCK) {
            const int k = p / G.wn, c = p - k * G.wn;
            const int cxy = c / G.wz, cz = c - cxy * G.wz;
            const int cx = cxy / G.wy, cy = cxy - cx * G.wy;
            s_t[p] = boxes[k][G.x0 + cx * gnyz + cy * gnz + cz];
        }
        __syncthreads();
    }
    const int sx = STAGED ? G.wy * G.wz : gnyz, sy = STAGED ? G.wz : gnz, wn = G.wn, x0 = G.x0;
    auto cand = [&](int q) {
        unsigned qx, qy, qz;
        const SubNode n = sub_decode((unsigned)q, (unsigned)G.ny, (unsigned)G.nz, (unsigned)sub, sx, sy, qx, qy, qz);
        return loc_cand(q, [=](int k) {
            if constexpr (STAGED) {             // station k by offset: a pointer per station would stay in VGPRs
                SubNode m = n;
                m.b += k * wn;
                return sub_time(s_t, m);
            } else {
                return sub_time(boxes[k] + x0, n);
            }
        });
    };
    loc_search_min<KR, LOC_SC>(G.nnode, B.tile, G.ne, G.e0, K, picks, weights, invw, cand, G.part, 0, G.ntiles,
                               part_key, part_x);
}

__global__ void __launch_bounds__(LOC_BLOCK)
locate_subcell_final_kernel(const float *const *__restrict__ boxes, int K, int gnyz, int gnz, int sub,
                            const double *__restrict__ picks, const double *__restrict__ weights,
                            const double *__restrict__ invw, int e0, const int *__restrict__ ev_group,
                            const SubGroup *__restrict__ groups, const unsigned long long *__restrict__ part_key,
                            const int *__restrict__ part_x, int *__restrict__ node,
                            unsigned long long *__restrict__ misfit, unsigned long long *__restrict__ t0out,
                            unsigned long long nan_bits)
{
    const int e = e0 + blockIdx.x;
    const SubGroup G = groups[ev_group[blockIdx.x]];
    unsigned long long key;
    int x;
    loc_partial_min(part_key, part_x, G.part + (long long)(e - G.e0) * G.ntiles, G.ntiles, key, x);
    if (threadIdx.x) return;
    loc_store(e, key, x, K, picks, weights, invw, misfit, t0out, nan_bits, [&](bool found, int q) {
        unsigned qn[3];
        const SubNode n = sub_decode(found ? (unsigned)q : 0u, (unsigned)G.ny, (unsigned)G.nz, (unsigned)sub, gnyz, gnz,
                                     qn[0], qn[1], qn[2]);
        if (node)
            for (int a = 0; a < 3; a++) node[3LL * e + a] = found ? G.lo[a] * sub + (int)qn[a] : -1;
        const int x0 = G.x0;
        return [=](int k) { return sub_time(boxes[k] + x0, n); };
    });
}

// ---- confidence regions (include/ttsweep.h, "locate confidence") ----
// R(e, l) = { x admissible and J(x) <= m[e] + delta[e][l] }, summarised without a volume.  J >= +0 on every cell, so
// "admissible and J <= thr" is one unsigned compare of the bits of J with an exclusive limit:
//   lim[e][l] = min(bits(thr) + 1, bits(+INF)), 0 for the empty region (m[e] = +INF); limmax[e] the greatest of them
//   confidence_check_kernel   one lane per event: refuses a NaN or negative m / delta on the bits, forms the limits
//   confidence_init_kernel    the accumulators of every (e, l) at their empty-region values
//   confidence_search_kernel  loc_scan over the cells of the grid, as locate_search_kernel: the same J bits.  Its
//                             sink: per (cell step, event) one wave vote on key < limmax[e]; only when a lane is inside do the
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
    const int nyz = ny * nz;
    loc_scan<KR, LOC_C>(N, blockIdx.x, net, e0 + eb, K, picks, weights, invw, [&](int x) { return loc_cell(boxes, x); },
                        [&](int i, int e, bool in, int x, unsigned long long key, double t0) {
        if (!__any(in && key < limmax[e])) return;              // the common case: no lane of the wave is inside
        const unsigned long long cx = (unsigned)(x / nyz), cy = (unsigned)(x % nyz / nz), cz = (unsigned)(x % nz);
        const unsigned long long tk = conf_t0_key(t0);
        for (int l = 0; l < L; l++) {
            if (!(in && key < lim[(long long)e * L + l])) continue;
            const int a = i * CONF_LMAX + l;                    // wave-uniform: one atomic of one lane per value
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
    });
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

// f(std::integral_constant<int, KR>) for the register width of the stations: the smallest of 8 / 16 / 24 / 32 that
// holds K, 0 (read T on use) above 32
template <typename F>
static void loc_with_kr(int K, F f)
{
    switch (K <= 8 ? 8 : K <= 16 ? 16 : K <= 24 ? 24 : K <= 32 ? 32 : 0) {
    case 8: f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 24: f(std::integral_constant<int, 24>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    default: f(std::integral_constant<int, 0>()); break;
    }
}

hipError_t launch_locate_search(const float *const *boxes, int K, int N, const double *picks, const double *weights,
                                const double *invw, int e0, int ne, int ntiles, unsigned long long *part_key,
                                int *part_x, hipStream_t st)
{
    if (ne <= 0 || ntiles <= 0) return hipSuccess;
    const dim3 grid(ntiles, (ne + LOC_ET - 1) / LOC_ET);
    if (grid.y > 65535) return hipErrorInvalidValue;
    loc_with_kr(K, [&](auto kr) {
        hipLaunchKernelGGL(locate_search_kernel<decltype(kr)::value>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks,
                           weights, invw, e0, ne, ntiles, part_key, part_x);
    });
    return hipGetLastError();
}

hipError_t launch_locate_final(const float *const *boxes, int K, const double *picks, const double *weights,
                               const double *invw, int e0, int ne, int ntiles, const unsigned long long *part_key,
                               const int *part_x, int *cell, double *misfit, double *t0, unsigned long long nan_bits,
                               hipStream_t st)
{
    if (ne <= 0) return hipSuccess;
    hipLaunchKernelGGL(locate_final_kernel, dim3(ne), dim3(LOC_BLOCK), 0, st, boxes, K, picks, weights, invw, e0,
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
    loc_with_kr(K, [&](auto kr) {
        hipLaunchKernelGGL(locate_volume_kernel<decltype(kr)::value>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, picks,
                           weights, invw, vev, (unsigned long long *const *)vol);
    });
    return hipGetLastError();
}

int locate_window_tile_cells() { return LOC_WC * LOC_BLOCK; }

hipError_t launch_locate_window_search(const float *const *boxes, int K, int mx, int my, int mz,
                                       const double *picks, const double *weights, const double *invw,
                                       const WinGroup *groups, const WinBlock *blocks, int nblocks,
                                       unsigned long long *part_key, int *part_x, hipStream_t st)
{
    if (nblocks <= 0) return hipSuccess;
    loc_with_kr(K, [&](auto kr) {
        hipLaunchKernelGGL(locate_window_search_kernel<decltype(kr)::value>, dim3(nblocks), dim3(LOC_BLOCK), 0, st,
                           boxes, K, mx, my, mz, picks, weights, invw, groups, blocks, part_key, part_x);
    });
    return hipGetLastError();
}

hipError_t launch_locate_window_final(const float *const *boxes, int K, const double *picks, const double *weights,
                                      const double *invw, int e0, int ne, const int *ev_group, const WinGroup *groups,
                                      const unsigned long long *part_key, const int *part_x, int *cell, double *misfit,
                                      double *t0, unsigned long long nan_bits, hipStream_t st)
{
    if (ne <= 0) return hipSuccess;
    hipLaunchKernelGGL(locate_window_final_kernel, dim3(ne), dim3(LOC_BLOCK), 0, st, boxes, K, picks, weights, invw, e0,
                       ev_group, groups, part_key, part_x, cell, (unsigned long long *)misfit,
                       (unsigned long long *)t0, nan_bits);
    return hipGetLastError();
}

int locate_subcell_tile_nodes() { return LOC_SC * LOC_BLOCK; }
int locate_subcell_stage_floats() { return LOC_SUB_STAGE; }

hipError_t launch_locate_subcell_search(const float *const *boxes, int K, int gnyz, int gnz, int sub,
                                        const double *picks, const double *weights, const double *invw,
                                        const SubGroup *groups, const WinBlock *blocks, int nblocks, bool staged,
                                        unsigned long long *part_key, int *part_x, hipStream_t st)
{
    if (nblocks <= 0) return hipSuccess;
    loc_with_kr(K, [&](auto kr) {
        auto kernel = staged ? locate_subcell_search_kernel<decltype(kr)::value, true>
                             : locate_subcell_search_kernel<decltype(kr)::value, false>;
        hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(LOC_BLOCK), 0, st, boxes, K, gnyz, gnz, sub, picks, weights,
                           invw, groups, blocks, part_key, part_x);
    });
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
    loc_with_kr(K, [&](auto kr) {
        hipLaunchKernelGGL(confidence_search_kernel<decltype(kr)::value>, grid, dim3(LOC_BLOCK), 0, st, boxes, K, N, ny,
                           nz, picks, weights, invw, e0, ne, L, lim, limmax, g_sum, g_t0, g_box);
    });
    return hipGetLastError();
}

} // namespace ttsweep
