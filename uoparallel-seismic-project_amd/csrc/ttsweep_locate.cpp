// ttsweep_locate.cpp - ttsweep_locate_device and ttsweep_locate_confidence_device of include/ttsweep.h (kernels:
// ttsweep_locate.hip).  For locate: argument
// checks, the check scan of picks and weights (refused before any output is touched), event batches sized so that
// the per-tile partials stay within a fixed scratch budget, the misfit volumes.  The scratch is allocated per call:
// nothing of the context changes, so the boxes the confirming-pass shortcut of ttsweep_solve remembers, its pools
// and its options stay as they are.
#include "ttsweep_ctx.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

using namespace ttsweep;

namespace {

size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

// per-tile partials of one batch of events, at most (12 bytes each)
// (mirrored: tests/test_locate_cpu.py::test_case_constants_mirror_the_sources)
constexpr long long LOC_PARTIALS = 1LL << 24;

struct DevScratch {
    char *p = nullptr;
    ~DevScratch()
    {
        if (p) (void)hipFree(p);
    }
};

} // namespace

extern "C" {

int ttsweep_locate_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev, int nevent, const double *picks_dev,
                          const double *weights_dev, int *cell_dev, double *misfit_dev, double *t0_dev, int nvol,
                          const int *vol_events, double *const *vol_dev)
{
    const char *what = "ttsweep_locate_device";
    if (nbox < 1 || nevent < 1 || !tt_dev || !picks_dev || nvol < 0 || (nvol > 0 && (!vol_events || !vol_dev)))
        return set_error("%s: null or bad argument", what);
    if ((long long)nbox * nevent > INT_MAX)
        return set_error("%s: %d boxes x %d events do not fit int32 pick indices", what, nbox, nevent);
    if (!ctx) return set_error("%s: null or bad argument", what);
    const long long ncells = (long long)ctx->nx * ctx->ny * ctx->nz;
    if (ncells > INT_MAX)
        return set_error("%s: %d x %d x %d cells do not fit int32 indices", what, ctx->nx, ctx->ny, ctx->nz);
    for (int k = 0; k < nbox; k++)
        if (!tt_dev[k]) return set_error("%s: null box pointer %d", what, k);
    for (int v = 0; v < nvol; v++) {
        if (vol_events[v] < 0 || vol_events[v] >= nevent)
            return set_error("%s: volume event %d (%d) outside [0, %d)", what, v, vol_events[v], nevent);
        if (!vol_dev[v]) return set_error("%s: null volume pointer %d", what, v);
    }
    if (nvol > 65535) return set_error("%s: %d volumes in one call (at most 65535)", what, nvol);
    if (ctx_bind(ctx)) return -1;

    const int N = (int)ncells;
    const int ntiles = (int)((ncells + locate_tile_cells() - 1) / locate_tile_cells());
    const int eb = (int)std::max(1LL, std::min<long long>({(long long)nevent, LOC_PARTIALS / ntiles, 65535LL * 8}));
    const size_t bb = align_up(nbox * sizeof(float *)), bi = align_up(nevent * sizeof(double));
    const size_t bf = align_up(nevent * sizeof(int)), bv = align_up(std::max(nvol, 1) * (sizeof(int) + sizeof(void *)));
    const size_t bk = align_up((size_t)eb * ntiles * sizeof(unsigned long long)), bx = align_up((size_t)eb * ntiles * sizeof(int));
    DevScratch S;
    HIPCHK(hipMalloc((void **)&S.p, bb + bi + bf + bv + bk + bx));
    const float **d_boxes = (const float **)S.p;
    double *d_invw = (double *)(S.p + bb);
    int *d_flag = (int *)(S.p + bb + bi);
    int *d_vev = (int *)(S.p + bb + bi + bf);
    double **d_vol = (double **)(S.p + bb + bi + bf + align_up(std::max(nvol, 1) * sizeof(int)));
    unsigned long long *d_key = (unsigned long long *)(S.p + bb + bi + bf + bv);
    int *d_x = (int *)(S.p + bb + bi + bf + bv + bk);

    HIPCHK(hipMemcpyAsync(d_boxes, tt_dev, nbox * sizeof(float *), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_locate_check(nbox, nevent, picks_dev, weights_dev, d_invw, d_flag, ctx->stream));
    std::vector<int> flag(nevent);
    HIPCHK(hipMemcpyAsync(flag.data(), d_flag, nevent * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int e = 0; e < nevent; e++) {
        if (flag[e] & 1) return set_error("%s: event %d has a NaN or infinite pick", what, e);
        if (flag[e] & 2) return set_error("%s: event %d has a negative, NaN or infinite weight", what, e);
        if (flag[e] & 4) return set_error("%s: event %d has no weight above zero", what, e);
    }

    const unsigned long long nan_bits = 0x7ff8000000000000ULL;     // the quiet NaN of t0 when no cell is admissible
    if (cell_dev || misfit_dev || t0_dev)
        for (int e0 = 0; e0 < nevent; e0 += eb) {
            const int ne = std::min(eb, nevent - e0);
            HIPCHK(launch_locate_search(d_boxes, nbox, N, picks_dev, weights_dev, d_invw, e0, ne, ntiles, d_key, d_x,
                                        ctx->stream));
            HIPCHK(launch_locate_final(d_boxes, nbox, picks_dev, weights_dev, d_invw, e0, ne, ntiles, d_key, d_x,
                                       cell_dev, misfit_dev, t0_dev, nan_bits, ctx->stream));
        }
    if (nvol) {
        HIPCHK(hipMemcpyAsync(d_vev, vol_events, nvol * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(d_vol, vol_dev, nvol * sizeof(double *), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(launch_locate_volume(d_boxes, nbox, N, picks_dev, weights_dev, d_invw, d_vev, d_vol, nvol, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The scratch is 24 bytes per event (invW, two flags, the greatest limit) and 128 per (event, level): the limits and
// the accumulators.  Nothing grows with the grid.  The accumulators need no partials, so events are batched only by
// the launch limit on grid.y.
int ttsweep_locate_confidence_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev, int nevent,
                                     const double *picks_dev, const double *weights_dev, const double *misfit_dev,
                                     int nlevel, const double *delta_dev, long long *count_dev, long long *sum_dev,
                                     long long *sum2_dev, int *lo_dev, int *hi_dev, double *t0_lo_dev,
                                     double *t0_hi_dev)
{
    const char *what = "ttsweep_locate_confidence_device";
    if (nbox < 1 || nevent < 1 || !tt_dev || !picks_dev || !misfit_dev || !delta_dev || nlevel < 1 || nlevel > 4)
        return set_error("%s: null or bad argument", what);
    if ((long long)nbox * nevent > INT_MAX)
        return set_error("%s: %d boxes x %d events do not fit int32 pick indices", what, nbox, nevent);
    if (!ctx) return set_error("%s: null or bad argument", what);
    const long long ncells = (long long)ctx->nx * ctx->ny * ctx->nz;
    if (ncells > INT_MAX)
        return set_error("%s: %d x %d x %d cells do not fit int32 indices", what, ctx->nx, ctx->ny, ctx->nz);
    const unsigned long long side = (unsigned long long)std::max({ctx->nx, ctx->ny, ctx->nz});
    if ((unsigned __int128)ncells * side * side >= (unsigned __int128)1 << 63)
        return set_error("%s: the second moments of %d x %d x %d cells could overflow int64", what, ctx->nx, ctx->ny,
                         ctx->nz);
    for (int k = 0; k < nbox; k++)
        if (!tt_dev[k]) return set_error("%s: null box pointer %d", what, k);
    if (ctx_bind(ctx)) return -1;

    const int N = (int)ncells;
    const long long n = (long long)nevent * nlevel;
    const size_t bb = align_up(nbox * sizeof(float *)), bi = align_up(nevent * sizeof(double));
    const size_t bf = align_up(2 * (size_t)nevent * sizeof(int)), bm = align_up(nevent * sizeof(unsigned long long));
    const size_t bl = align_up(n * sizeof(unsigned long long)), bs = align_up(n * 10 * sizeof(unsigned long long));
    const size_t bt = align_up(n * 2 * sizeof(unsigned long long)), bx = align_up(n * 6 * sizeof(int));
    DevScratch S;
    HIPCHK(hipMalloc((void **)&S.p, bb + bi + bf + bm + bl + bs + bt + bx));
    char *p = S.p;
    auto take = [&p](size_t bytes) {
        char *q = p;
        p += bytes;
        return q;
    };
    const float **d_boxes = (const float **)take(bb);
    double *d_invw = (double *)take(bi);
    int *d_flag = (int *)take(bf);
    unsigned long long *d_limmax = (unsigned long long *)take(bm);
    unsigned long long *d_lim = (unsigned long long *)take(bl);
    unsigned long long *d_sum = (unsigned long long *)take(bs);
    unsigned long long *d_t0 = (unsigned long long *)take(bt);
    int *d_box = (int *)take(bx);

    HIPCHK(hipMemcpyAsync(d_boxes, tt_dev, nbox * sizeof(float *), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_locate_check(nbox, nevent, picks_dev, weights_dev, d_invw, d_flag, ctx->stream));
    HIPCHK(launch_confidence_check(nevent, nlevel, misfit_dev, delta_dev, d_lim, d_limmax, d_flag + nevent,
                                   ctx->stream));
    std::vector<int> flag(2 * (size_t)nevent);
    HIPCHK(hipMemcpyAsync(flag.data(), d_flag, flag.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int e = 0; e < nevent; e++) {
        if (flag[e] & 1) return set_error("%s: event %d has a NaN or infinite pick", what, e);
        if (flag[e] & 2) return set_error("%s: event %d has a negative, NaN or infinite weight", what, e);
        if (flag[e] & 4) return set_error("%s: event %d has no weight above zero", what, e);
        if (flag[nevent + e] & 1) return set_error("%s: event %d has a NaN or negative misfit level", what, e);
        if (flag[nevent + e] & 2) return set_error("%s: event %d has a NaN or negative delta", what, e);
    }

    HIPCHK(launch_confidence_init(n, ctx->nx, ctx->ny, ctx->nz, d_sum, d_t0, d_box, ctx->stream));
    const int eb = 65535 * 8;
    for (int e0 = 0; e0 < nevent; e0 += eb)
        HIPCHK(launch_confidence_search(d_boxes, nbox, N, ctx->ny, ctx->nz, picks_dev, weights_dev, d_invw, e0,
                                        std::min(eb, nevent - e0), nlevel, d_lim, d_limmax, d_sum, d_t0, d_box,
                                        ctx->stream));
    HIPCHK(launch_confidence_final(n, d_sum, d_t0, d_box, count_dev, sum_dev, sum2_dev, lo_dev, hi_dev, t0_lo_dev,
                                   t0_hi_dev, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

} // extern "C"
