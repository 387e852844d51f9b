// ttsweep_fresnel.hip - the kernels of the Fresnel-volume calls (host side: ttsweep_fresnel.cpp; semantics:
// include/ttsweep.h, "fresnel").  One kernel body streams the (pair, window cell) visits of all three calls: a block
// is one tile of one pair's window, a thread takes quads of 4 consecutive z of a window row (one 16-byte load per box
// where the quad is whole and aligned), so consecutive lanes read consecutive z and the coordinates are decoded once
// per quad.  Every output is an integer sum, minimum or maximum: the bits do not depend on the launch.
//
// The library is built with -fno-honor-nans, and the boxes may hold any float: every test that a NaN can reach is
// made on the bits, and the one operation that could produce a NaN (-INF - -INF) is not evaluated.
#include "ttsweep_kernels.h"

#include "../../include/ttsweep.h"

namespace ttsweep {

namespace {

constexpr int FRES_BLOCK = 256;
// quads of a thread: a block first finds its pair (a binary search of dependent loads), and at 2 quads per thread that
// fixed cost, not the stream, set the time of a whole-grid call (measured at 2, 4 and 8: DESIGN.md 4.10)
constexpr int FRES_QPT = 8;
constexpr int FRES_TILE_QUADS = FRES_BLOCK * FRES_QPT;  // up to 8192 cells of a block

constexpr unsigned F32_INF = 0x7f800000u, F32_NEG_INF = 0xff800000u;
constexpr long long F64_INF = 0x7ff0000000000000LL, F64_ONE = 0x3ff0000000000000LL;

// !(f < +INFINITY): +INFINITY or a NaN
__device__ inline bool not_below_inf(float f)
{
    const unsigned u = __float_as_uint(f);
    return u == F32_INF || (u & 0x7fffffffu) > F32_INF;
}

// The weight of a cell: a, b its travel times in the two boxes, tab = (double)t_ab (below +INFINITY), tab_neg_inf:
// t_ab is -INFINITY.  0.0 for a cell outside the volume.
__device__ inline double fresnel_phi(float a, float b, double tab, bool tab_neg_inf, double tau)
{
    if (not_below_inf(a) || not_below_inf(b)) return 0.0;
    // -INF - -INF would be the NaN of the definition, which gives phi = 0
    if (tab_neg_inf && (__float_as_uint(a) == F32_NEG_INF || __float_as_uint(b) == F32_NEG_INF)) return 0.0;
    const double delta = ((double)a + (double)b) - tab;
    const double phi = 1.0 - delta / tau;
    const long long bits = __double_as_longlong(phi);
    if (bits <= 0 || bits > F64_INF) return 0.0;        // negative, a zero, a NaN: !(phi > 0.0)
    return bits > F64_ONE ? 1.0 : phi;
}

enum { FRES_VOLUME = 0, FRES_FORWARD = 1, FRES_ADJOINT = 2 };

template <int MODE>
__global__ void __launch_bounds__(FRES_BLOCK)
fresnel_kernel(const FresPair *__restrict__ pairs, const long long *__restrict__ first, int npair, long long block0,
               const float *__restrict__ t_ab, int gnyz, int gnz, int S, const double *__restrict__ mw,
               unsigned long long *__restrict__ g_cnt, unsigned long long *__restrict__ g_sum, int *__restrict__ g_box,
               unsigned long long *__restrict__ acc, int *__restrict__ hits)
{
    // the pair of this block: the last r with first[r] <= b (uniform over the block)
    const long long b = block0 + blockIdx.x;
    int r = 0, top = npair - 1;
    while (r < top) {
        const int mid = (int)(((long long)r + top + 1) >> 1);
        if (first[mid] <= b) r = mid;
        else top = mid - 1;
    }
    const float tabf = t_ab[r];
    if (not_below_inf(tabf)) return;                    // UNREACHED: no cells
    const int tile = (int)(b - first[r]);
    const FresPair P = pairs[r];
    const double tab = (double)tabf, tau = P.tau;
    const bool tab_neg_inf = __float_as_uint(tabf) == F32_NEG_INF;
    const int qz = (P.wz + 3) >> 2;
    const double wr = MODE == FRES_ADJOINT && mw ? mw[r] : 0.0;

    long long sum = 0;
    int cnt = 0;
    int lo0 = 0x7fffffff, lo1 = 0x7fffffff, lo2 = 0x7fffffff, hi0 = -1, hi1 = -1, hi2 = -1;
#pragma unroll
    for (int k = 0; k < FRES_QPT; k++) {
        const long long ql = (long long)tile * FRES_TILE_QUADS + k * FRES_BLOCK + threadIdx.x;
        if (ql >= P.nquad) continue;
        const int q = (int)ql;
        const int row = q / qz, z0 = (q - row * qz) * 4;
        const int cx = row / P.wy, cy = row - cx * P.wy;
        const int n = min(4, P.wz - z0);
        const int x = P.x0 + cx * gnyz + cy * gnz + z0;   // inside the grid: the window is
        const float *pa = P.Ta + x, *pb = P.Tb + x;
        float a[4], c[4];
        if (n == 4 && (((unsigned long long)pa | (unsigned long long)pb) & 15) == 0) {
            const float4 va = *reinterpret_cast<const float4 *>(pa), vb = *reinterpret_cast<const float4 *>(pb);
            a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
            c[0] = vb.x; c[1] = vb.y; c[2] = vb.z; c[3] = vb.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                a[j] = j < n ? pa[j] : __uint_as_float(F32_INF);
                c[j] = j < n ? pb[j] : __uint_as_float(F32_INF);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double phi = fresnel_phi(a[j], c[j], tab, tab_neg_inf, tau);
            if (phi == 0.0) continue;                   // (phi is 0.0 or in (0, 1]: never a NaN)
            if (MODE == FRES_VOLUME) {
                sum += __builtin_llrint(__builtin_ldexp(phi, S));
                cnt++;
                lo0 = min(lo0, P.lo[0] + cx); hi0 = max(hi0, P.lo[0] + cx);
                lo1 = min(lo1, P.lo[1] + cy); hi1 = max(hi1, P.lo[1] + cy);
                lo2 = min(lo2, P.lo[2] + z0 + j); hi2 = max(hi2, P.lo[2] + z0 + j);
            } else if (MODE == FRES_FORWARD) {
                sum += __builtin_llrint(__builtin_ldexp(phi * mw[x + j], S));
                cnt = 1;
            } else {
                if (acc) {
                    const long long t = __builtin_llrint(__builtin_ldexp(wr * phi, S));
                    if (t) atomicAdd(acc + x + j, (unsigned long long)t);
                }
                if (hits) atomicAdd(hits + x + j, 1);
            }
        }
    }
    if (MODE == FRES_ADJOINT) return;

    // one set of atomics per wave and pair
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        cnt += __shfl_xor(cnt, off);
        if (MODE == FRES_VOLUME) {
            lo0 = min(lo0, __shfl_xor(lo0, off)); hi0 = max(hi0, __shfl_xor(hi0, off));
            lo1 = min(lo1, __shfl_xor(lo1, off)); hi1 = max(hi1, __shfl_xor(hi1, off));
            lo2 = min(lo2, __shfl_xor(lo2, off)); hi2 = max(hi2, __shfl_xor(hi2, off));
        }
    }
    if (__lane_id() != 0 || cnt == 0) return;
    if (sum) atomicAdd(g_sum + r, (unsigned long long)sum);
    if (MODE == FRES_VOLUME) {
        atomicAdd(g_cnt + r, (unsigned long long)cnt);
        int *box = g_box + 6LL * r;
        atomicMin(box + 0, lo0); atomicMin(box + 1, lo1); atomicMin(box + 2, lo2);
        atomicMax(box + 3, hi0); atomicMax(box + 4, hi1); atomicMax(box + 5, hi2);
    }
}

__global__ void __launch_bounds__(FRES_BLOCK)
fresnel_pairs_kernel(const FresPair *__restrict__ pairs, int npair, float *__restrict__ t_ab, int *__restrict__ status)
{
    const int r = blockIdx.x * FRES_BLOCK + threadIdx.x;
    if (r >= npair) return;
    const float t = pairs[r].Ta[pairs[r].sb];
    t_ab[r] = t;
    status[r] = not_below_inf(t) ? TTSWEEP_FRESNEL_UNREACHED : TTSWEEP_FRESNEL_OK;
}

__global__ void __launch_bounds__(FRES_BLOCK)
fresnel_init_kernel(int npair, int nx, int ny, int nz, unsigned long long *__restrict__ cnt,
                    unsigned long long *__restrict__ sum, int *__restrict__ box)
{
    const int r = blockIdx.x * FRES_BLOCK + threadIdx.x;
    if (r >= npair) return;
    cnt[r] = 0;
    sum[r] = 0;
    int *b = box + 6LL * r;
    b[0] = nx; b[1] = ny; b[2] = nz;
    b[3] = b[4] = b[5] = -1;
}

__global__ void __launch_bounds__(FRES_BLOCK)
fresnel_final_kernel(int npair, int S, const unsigned long long *__restrict__ cnt,
                     const unsigned long long *__restrict__ sum, const int *__restrict__ box,
                     const float *__restrict__ t_ab, long long *__restrict__ count, int *__restrict__ lo,
                     int *__restrict__ hi, double *__restrict__ out, float *__restrict__ t_ab_out)
{
    const int r = blockIdx.x * FRES_BLOCK + threadIdx.x;
    if (r >= npair) return;
    if (count) count[r] = (long long)cnt[r];
    if (out) out[r] = __builtin_ldexp((double)(long long)sum[r], -S);
    if (t_ab_out) t_ab_out[r] = t_ab[r];
    for (int a = 0; a < 3; a++) {
        if (lo) lo[3LL * r + a] = box[6LL * r + a];
        if (hi) hi[3LL * r + a] = box[6LL * r + 3 + a];
    }
}

unsigned per_pair_blocks(int npair) { return (unsigned)(((long long)npair + FRES_BLOCK - 1) / FRES_BLOCK); }

} // namespace

int fresnel_tile_quads() { return FRES_TILE_QUADS; }

hipError_t launch_fresnel_pairs(const FresPair *pairs, int npair, float *t_ab, int *status, hipStream_t st)
{
    if (npair <= 0) return hipSuccess;
    hipLaunchKernelGGL(fresnel_pairs_kernel, dim3(per_pair_blocks(npair)), dim3(FRES_BLOCK), 0, st, pairs, npair, t_ab,
                       status);
    return hipGetLastError();
}

hipError_t launch_fresnel_init(int npair, int nx, int ny, int nz, unsigned long long *cnt, unsigned long long *sum,
                               int *box, hipStream_t st)
{
    if (npair <= 0) return hipSuccess;
    hipLaunchKernelGGL(fresnel_init_kernel, dim3(per_pair_blocks(npair)), dim3(FRES_BLOCK), 0, st, npair, nx, ny, nz,
                       cnt, sum, box);
    return hipGetLastError();
}

hipError_t launch_fresnel_volume(const FresPair *pairs, const long long *first, int npair, long long block0,
                                 int nblocks, const float *t_ab, int gnyz, int gnz, int S, unsigned long long *cnt,
                                 unsigned long long *sum, int *box, hipStream_t st)
{
    if (npair <= 0 || nblocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(fresnel_kernel<FRES_VOLUME>, dim3((unsigned)nblocks), dim3(FRES_BLOCK), 0, st, pairs, first,
                       npair, block0, t_ab, gnyz, gnz, S, (const double *)nullptr, cnt, sum, box,
                       (unsigned long long *)nullptr, (int *)nullptr);
    return hipGetLastError();
}

hipError_t launch_fresnel_forward(const FresPair *pairs, const long long *first, int npair, long long block0,
                                  int nblocks, const float *t_ab, int gnyz, int gnz, int S, const double *m,
                                  unsigned long long *sum, hipStream_t st)
{
    if (npair <= 0 || nblocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(fresnel_kernel<FRES_FORWARD>, dim3((unsigned)nblocks), dim3(FRES_BLOCK), 0, st, pairs, first,
                       npair, block0, t_ab, gnyz, gnz, S, m, (unsigned long long *)nullptr, sum, (int *)nullptr,
                       (unsigned long long *)nullptr, (int *)nullptr);
    return hipGetLastError();
}

hipError_t launch_fresnel_adjoint(const FresPair *pairs, const long long *first, int npair, long long block0,
                                  int nblocks, const float *t_ab, int gnyz, int gnz, int S, const double *w,
                                  long long *acc, int *hits, hipStream_t st)
{
    if (npair <= 0 || nblocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(fresnel_kernel<FRES_ADJOINT>, dim3((unsigned)nblocks), dim3(FRES_BLOCK), 0, st, pairs, first,
                       npair, block0, t_ab, gnyz, gnz, S, w, (unsigned long long *)nullptr,
                       (unsigned long long *)nullptr, (int *)nullptr, (unsigned long long *)acc, hits);
    return hipGetLastError();
}

hipError_t launch_fresnel_final(int npair, int S, const unsigned long long *cnt, const unsigned long long *sum,
                                const int *box, const float *t_ab, long long *count, int *lo, int *hi, double *out,
                                float *t_ab_out, hipStream_t st)
{
    if (npair <= 0) return hipSuccess;
    hipLaunchKernelGGL(fresnel_final_kernel, dim3(per_pair_blocks(npair)), dim3(FRES_BLOCK), 0, st, npair, S, cnt, sum,
                       box, t_ab, count, lo, hi, out, t_ab_out);
    return hipGetLastError();
}

} // namespace ttsweep
