// ttsweep_fresnel.cpp - ttsweep_fresnel_volume_device, ttsweep_fresnel_forward_device and
// ttsweep_fresnel_adjoint_device of include/ttsweep.h (kernels: ttsweep_fresnel.hip).  The three entry points share
// one preparation: every refusal that concerns host arguments (before the device is touched), the pair records and
// the prefix of their tile counts, the scratch, and the pairs' t_ab and status.  The blocks of a call are launched
// FRES_LAUNCH_BLOCKS at a time.  The scratch is allocated per call and grows with the pair list only (72 bytes per
// pair, plus 40 of accumulators in the volume and forward calls): nothing of the context changes, so the boxes the
// confirming-pass shortcut of ttsweep_solve remembers, its pools and its options stay as they are.
#include "ttsweep_ctx.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <vector>

using namespace ttsweep;

namespace {

// blocks of one launch, at most: 2^16 tiles of up to 8192 cells keep a launch within a few milliseconds at the HBM rate
// (mirrored: tests/test_gpu_fresnel.py::test_a_launch_edge)
constexpr long long FRES_LAUNCH_BLOCKS = 1LL << 16;

// tau > 0 and finite, on the bits (the library is built with -fno-honor-nans)
bool tau_ok(double tau)
{
    unsigned long long u;
    memcpy(&u, &tau, sizeof(u));
    return u > 0 && u < 0x7ff0000000000000ULL;
}

// what a call holds on the device once prepare() has run
struct Prepared {
    Scratch S;
    int npair = 0;
    long long nblocks = 0;
    FresPair *d_pairs = nullptr;
    long long *d_first = nullptr;
    float *d_tab = nullptr;
    int *d_status = nullptr, *d_scan = nullptr, *d_box = nullptr;
    unsigned long long *d_cnt = nullptr, *d_sum = nullptr;
};

// The refusals of the shared arguments in the order of include/ttsweep.h, then the pair records, the scratch (with
// the per-pair accumulators when `sums`), t_ab and status of every pair on the device.  pointers: the call's own
// pointer checks.
int prepare(const char *what, ttsweep_ctx *ctx, int nbox, const ttsweep_start *starts, const float *const *tt_dev,
            long long npair, const int *pair_a, const int *pair_b, const double *tau, const int *lo, const int *hi,
            bool pointers, bool sums, Prepared &P)
{
    if (!ctx || nbox < 1 || npair < 0 || !starts || !tt_dev || !pointers ||
        (npair > 0 && (!pair_a || !pair_b || !tau)))
        return set_error("%s: null or bad argument", what);
    if (npair > INT_MAX) return set_error("%s: %lld pairs do not fit int32 indices", what, npair);
    if (!lo != !hi) return set_error("%s: lo and hi must both be given or both be NULL", what);
    const int n[3] = {ctx->nx, ctx->ny, ctx->nz};
    if ((long long)n[0] * n[1] * n[2] > INT_MAX)
        return set_error("%s: %d x %d x %d cells do not fit int32 indices", what, n[0], n[1], n[2]);
    for (int k = 0; k < nbox; k++) {
        const ttsweep_start &s = starts[k];
        if (s.i < 0 || s.i >= n[0] || s.j < 0 || s.j >= n[1] || s.k < 0 || s.k >= n[2])
            return set_error("%s: start %d (%d, %d, %d) outside the grid", what, k, s.i, s.j, s.k);
        if (!tt_dev[k]) return set_error("%s: null box pointer %d", what, k);
    }
    // (up to INT32_MAX pairs at 64 bytes each: a failed allocation is a refusal, not an exception through the C ABI)
    std::vector<FresPair> pairs;
    std::vector<long long> first;
    try {
        pairs.resize(npair);
        first.resize(npair + 1);
    } catch (const std::bad_alloc &) {
        return set_error("%s: no host memory for the records of %lld pairs", what, npair);
    }
    const int tile = fresnel_tile_quads();
    long long nblocks = 0;
    for (long long r = 0; r < npair; r++) {
        const int a = pair_a[r], b = pair_b[r];
        if (a < 0 || a >= nbox || b < 0 || b >= nbox)
            return set_error("%s: pair %lld names boxes %d and %d, not both in [0, %d)", what, r, a, b, nbox);
        if (!tau_ok(tau[r]))
            return set_error("%s: pair %lld has a tau that is NaN, infinite or not above zero", what, r);
        int l[3] = {0, 0, 0}, h[3] = {n[0] - 1, n[1] - 1, n[2] - 1};
        for (int d = 0; lo && d < 3; d++) {
            l[d] = lo[3 * r + d];
            h[d] = hi[3 * r + d];
            if (l[d] < 0 || l[d] > h[d] || h[d] >= n[d])
                return set_error("%s: pair %lld has a bad window [%d, %d] along axis %d (%d cells)", what, r, l[d],
                                 h[d], d, n[d]);
        }
        FresPair &p = pairs[r];
        p.Ta = tt_dev[a];
        p.Tb = tt_dev[b];
        p.tau = tau[r];
        p.sb = (starts[b].i * n[1] + starts[b].j) * n[2] + starts[b].k;
        p.x0 = (l[0] * n[1] + l[1]) * n[2] + l[2];
        for (int d = 0; d < 3; d++) p.lo[d] = l[d];
        p.wy = h[1] - l[1] + 1;
        p.wz = h[2] - l[2] + 1;
        // quads of 4 z per row: at most the cells of the window, so within int32
        p.nquad = (int)((long long)(h[0] - l[0] + 1) * p.wy * ((p.wz + 3) / 4));
        first[r] = nblocks;
        nblocks += (p.nquad + tile - 1) / tile;
    }
    first[npair] = nblocks;
    if (ctx_bind(ctx)) return -1;

    P.npair = (int)npair;
    P.nblocks = nblocks;
    const size_t np = std::max<long long>(npair, 1);
    P.S.add(P.d_pairs, np);
    P.S.add(P.d_first, np + 1);
    P.S.add(P.d_tab, np);
    P.S.add(P.d_status, np);
    P.S.add(P.d_scan, 2);
    if (sums) {
        P.S.add(P.d_cnt, np);
        P.S.add(P.d_sum, np);
        P.S.add(P.d_box, 6 * np);
    }
    HIPCHK(P.S.alloc());
    if (npair == 0) return 0;
    HIPCHK(hipMemcpyAsync(P.d_pairs, pairs.data(), npair * sizeof(FresPair), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(P.d_first, first.data(), (npair + 1) * sizeof(long long), hipMemcpyHostToDevice,
                          ctx->stream));
    HIPCHK(launch_fresnel_pairs(P.d_pairs, P.npair, P.d_tab, P.d_status, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));          // (the host tables end with this function)
    return 0;
}

// the end of a call that was not refused: the statuses to the host, and the stream drained
int finish(ttsweep_ctx *ctx, const Prepared &P, int *status)
{
    if (status && P.npair)
        HIPCHK(hipMemcpyAsync(status, P.d_status, P.npair * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// the blocks of a call, FRES_LAUNCH_BLOCKS per launch: launch(first block, blocks)
template <class Launch>
int run_blocks(const Prepared &P, Launch launch)
{
    for (long long b0 = 0; b0 < P.nblocks; b0 += FRES_LAUNCH_BLOCKS)
        HIPCHK(launch(b0, (int)std::min(FRES_LAUNCH_BLOCKS, P.nblocks - b0)));
    return 0;
}

// e - 2048 = the largest frexp exponent of the n values at v (e = 0: all zero); a NaN or infinite one is refused
int scan_values(const char *what, const char *name, ttsweep_ctx *ctx, const double *v, long long n, int *d_scan,
                int &e)
{
    bool bad = false;
    if (fixed_point_scan(ctx, v, n, d_scan, &e, &bad)) return -1;
    return bad ? set_error("%s: %s holds a NaN or infinite value", what, name) : 0;
}

} // namespace

extern "C" {

int ttsweep_fresnel_volume_device(ttsweep_ctx *ctx, int nbox, const ttsweep_start *starts, const float *const *tt_dev,
                                  long long npair, const int *pair_a, const int *pair_b, const double *tau,
                                  const int *lo, const int *hi, int *status, float *t_ab_dev, long long *count_dev,
                                  int *lo_dev, int *hi_dev, double *phi_dev)
{
    const char *what = "ttsweep_fresnel_volume_device";
    Prepared P;
    if (prepare(what, ctx, nbox, starts, tt_dev, npair, pair_a, pair_b, tau, lo, hi, true, true, P)) return -1;
    if (npair == 0) return 0;
    const int S = 60 - ceil_log2((long long)ctx->nx * ctx->ny * ctx->nz);
    const int gnyz = ctx->ny * ctx->nz, gnz = ctx->nz;
    HIPCHK(launch_fresnel_init(P.npair, ctx->nx, ctx->ny, ctx->nz, P.d_cnt, P.d_sum, P.d_box, ctx->stream));
    if (count_dev || lo_dev || hi_dev || phi_dev)
        if (run_blocks(P, [&](long long b0, int nb) {
                return launch_fresnel_volume(P.d_pairs, P.d_first, P.npair, b0, nb, P.d_tab, gnyz, gnz, S, P.d_cnt,
                                             P.d_sum, P.d_box, ctx->stream);
            }))
            return -1;
    HIPCHK(launch_fresnel_final(P.npair, S, P.d_cnt, P.d_sum, P.d_box, P.d_tab, count_dev, lo_dev, hi_dev, phi_dev,
                                t_ab_dev, ctx->stream));
    return finish(ctx, P, status);
}

int ttsweep_fresnel_forward_device(ttsweep_ctx *ctx, int nbox, const ttsweep_start *starts, const float *const *tt_dev,
                                   long long npair, const int *pair_a, const int *pair_b, const double *tau,
                                   const int *lo, const int *hi, const double *m_dev, double *y_dev, int *status,
                                   int *scale)
{
    const char *what = "ttsweep_fresnel_forward_device";
    Prepared P;
    if (prepare(what, ctx, nbox, starts, tt_dev, npair, pair_a, pair_b, tau, lo, hi, m_dev && (y_dev || npair == 0),
                true, P))
        return -1;
    const long long ncells = (long long)ctx->nx * ctx->ny * ctx->nz;
    int e = 0;
    if (scan_values(what, "m", ctx, m_dev, ncells, P.d_scan, e)) return -1;
    const int S = e ? 61 - (e - 2048) - ceil_log2(ncells) : 0;
    if (scale) *scale = S;
    if (npair == 0) return 0;
    HIPCHK(hipMemsetAsync(P.d_sum, 0, npair * sizeof(unsigned long long), ctx->stream));
    if (e)
        if (run_blocks(P, [&](long long b0, int nb) {
                return launch_fresnel_forward(P.d_pairs, P.d_first, P.npair, b0, nb, P.d_tab, ctx->ny * ctx->nz,
                                              ctx->nz, S, m_dev, P.d_sum, ctx->stream);
            }))
            return -1;
    HIPCHK(launch_fresnel_final(P.npair, S, nullptr, P.d_sum, nullptr, P.d_tab, nullptr, nullptr, nullptr, y_dev,
                                nullptr, ctx->stream));
    return finish(ctx, P, status);
}

int ttsweep_fresnel_adjoint_device(ttsweep_ctx *ctx, int nbox, const ttsweep_start *starts, const float *const *tt_dev,
                                   long long npair, const int *pair_a, const int *pair_b, const double *tau,
                                   const int *lo, const int *hi, const double *w_dev, double *g_dev, int *hits_dev,
                                   int *status, int *scale)
{
    const char *what = "ttsweep_fresnel_adjoint_device";
    // (an empty list has no weights to point at: g is zeroed all the same)
    if (npair > 0 && !w_dev != !g_dev) return set_error("%s: w and g must both be given or both be NULL", what);
    Prepared P;
    if (prepare(what, ctx, nbox, starts, tt_dev, npair, pair_a, pair_b, tau, lo, hi, true, false, P)) return -1;
    // S = 61 - E_w - K: a visit adds less than 2^(E_w + S) = 2^(61 - K) in magnitude (phi <= 1) and a cell is visited
    // by at most 2^K pairs, so |acc[x]| < 2^61
    int e = 0;
    if (w_dev && npair > 0 && scan_values(what, "w", ctx, w_dev, npair, P.d_scan, e)) return -1;
    const int S = e ? 61 - (e - 2048) - ceil_log2(npair) : 0;
    const auto blocks = [&] {
        return run_blocks(P, [&](long long b0, int nb) {
            return launch_fresnel_adjoint(P.d_pairs, P.d_first, P.npair, b0, nb, P.d_tab, ctx->ny * ctx->nz, ctx->nz,
                                          S, e ? w_dev : nullptr, e ? (long long *)g_dev : nullptr, hits_dev,
                                          ctx->stream);
        });
    };
    if (finish(ctx, P, status)) return -1;          // (the statuses are prepare()'s)
    return fixed_point_adjoint(ctx, e != 0, S, g_dev, hits_dev, scale, blocks);
}

} // extern "C"
