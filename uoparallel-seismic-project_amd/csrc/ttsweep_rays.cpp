// ttsweep_rays.cpp - the ray calls of include/ttsweep.h: ttsweep_predecessors_device,
// ttsweep_trace_rays_device, the Frechet operators ttsweep_ray_forward_device / ttsweep_ray_adjoint_device and
// their pair-list forms ttsweep_ray_pairs_{forward,adjoint,geometry}_device (kernels: ttsweep_rays.hip).
// Argument checks, the star's ray entries, the host-side scan of the per-ray cell counts.  Nothing here touches the solve's state: the boxes the
// confirming-pass shortcut of ttsweep_solve remembers, its pools and its options stay as they are.
#include "ttsweep_ctx.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

using namespace ttsweep;

namespace {

size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

bool inside(const ttsweep_ctx *ctx, const ttsweep_start &p)
{
    return p.i >= 0 && p.i < ctx->nx && p.j >= 0 && p.j < ctx->ny && p.k >= 0 && p.k < ctx->nz;
}

int flat(const ttsweep_ctx *ctx, const ttsweep_start &p) { return (p.i * ctx->ny + p.j) * ctx->nz + p.k; }

// what both calls check before any device work
int check_boxes(const ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts, const float *const *tt_dev,
                const void *const *pred_dev, const char *what)
{
    if (!ctx || nstart < 0 || (nstart > 0 && (!starts || !tt_dev || !pred_dev)))
        return set_error("%s: null or bad argument", what);
    if ((long long)ctx->nx * ctx->ny * ctx->nz > INT_MAX)
        return set_error("%s: %d x %d x %d cells do not fit int32 indices", what, ctx->nx, ctx->ny, ctx->nz);
    if (!ctx->have_v) return set_error("%s: velocity not set", what);
    for (int s = 0; s < nstart; s++) {
        if (!tt_dev[s] || !pred_dev[s]) return set_error("%s: null box pointer %d", what, s);
        if (!inside(ctx, starts[s]))
            return set_error("%s: start %d (%d, %d, %d) outside the grid", what, s, starts[s].i, starts[s].j,
                             starts[s].k);
    }
    return 0;
}

// the receivers as FLOATBOX indices; each must lie inside the grid
int flat_receivers(const ttsweep_ctx *ctx, int nrecv, const ttsweep_start *receivers, const char *what,
                   std::vector<int> &recv)
{
    recv.resize(nrecv);
    for (int q = 0; q < nrecv; q++) {
        if (!inside(ctx, receivers[q]))
            return set_error("%s: receiver %d (%d, %d, %d) outside the grid", what, q, receivers[q].i,
                             receivers[q].j, receivers[q].k);
        recv[q] = flat(ctx, receivers[q]);
    }
    return 0;
}

// the checks of the two operator calls before any device work: the ray counts (one int32 index per ray), the
// boxes, the receivers
int check_operator(const ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts, const float *const *tt_dev,
                   const int *const *pred_dev, int nrecv, const ttsweep_start *receivers, const char *what,
                   std::vector<int> &recv)
{
    if (nstart < 0 || nrecv < 0 || (nrecv > 0 && !receivers)) return set_error("%s: null or bad argument", what);
    if ((long long)nstart * nrecv > INT_MAX)
        return set_error("%s: %d starts x %d receivers do not fit int32 ray indices", what, nstart, nrecv);
    if (check_boxes(ctx, nstart, starts, tt_dev, (const void *const *)pred_dev, what)) return -1;
    return flat_receivers(ctx, nrecv, receivers, what, recv);
}

// the grid in the caller's axes over the padded velocity volume of the current layout
RayGeom ray_geom(const ttsweep_ctx *ctx)
{
    const DevLayout &L = ctx->L;
    RayGeom G{};
    G.n[0] = ctx->nx; G.n[1] = ctx->ny; G.n[2] = ctx->nz;
    const long long stride[3] = {L.s0, L.s1, 1};
    for (int d = 0; d < 3; d++) G.vs[L.perm[d]] = stride[d];
    G.vbase = dev_index(L, 0, 0, 0);
    return G;
}

// the pull star as ray entries: offsets that fit the grid, sorted by (di, dj, dk, d)
std::vector<RayEntry> ray_entries(const ttsweep_ctx *ctx, const RayGeom &G)
{
    std::vector<RayEntry> out;
    for (size_t e = 0; e < ctx->pull.size(); e++) {
        const ttsweep_pull_entry &p = ctx->pull[e];
        if (std::abs(p.di) >= ctx->nx || std::abs(p.dj) >= ctx->ny || std::abs(p.dk) >= ctx->nz) continue;
        RayEntry r{};
        r.di = p.di; r.dj = p.dj; r.dk = p.dk;
        r.flags = p.flags;
        r.udelta = (int)(((long long)p.di * ctx->ny + p.dj) * ctx->nz + p.dk);
        r.h = p.h;
        r.d = ctx->pull_d[e];
        r.vdelta = p.di * G.vs[0] + p.dj * G.vs[1] + p.dk * G.vs[2];
        out.push_back(r);
    }
    std::sort(out.begin(), out.end(), [](const RayEntry &a, const RayEntry &b) {
        if (a.di != b.di) return a.di < b.di;
        if (a.dj != b.dj) return a.dj < b.dj;
        if (a.dk != b.dk) return a.dk < b.dk;
        return a.d < b.d;
    });
    return out;
}

// ctx->d_rays holds at least `bytes`
int ensure_ray_buffer(ttsweep_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->rays_cap) return 0;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipFree(ctx->d_rays));
    ctx->d_rays = nullptr;
    ctx->rays_cap = 0;
    HIPCHK(hipMalloc((void **)&ctx->d_rays, bytes));
    ctx->rays_cap = bytes;
    return 0;
}

// entries and box records on the device, at the front of ctx->d_rays (extra: bytes the caller needs behind them)
struct RayStage {
    RayGeom G;
    std::vector<RayEntry> ent;
    std::vector<RayBox> boxes;
    RayEntry *d_ent = nullptr;
    RayBox *d_boxes = nullptr;
    char *rest = nullptr;
};

int stage(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts, const float *const *tt_dev,
          int *const *pred_dev, size_t extra, RayStage &S)
{
    S.G = ray_geom(ctx);
    S.ent = ray_entries(ctx, S.G);
    S.boxes.resize(nstart);
    for (int s = 0; s < nstart; s++) S.boxes[s] = RayBox{tt_dev[s], pred_dev[s], flat(ctx, starts[s]), 0};
    const size_t be = align_up(std::max<size_t>(S.ent.size(), 1) * sizeof(RayEntry));
    const size_t bb = align_up(std::max(nstart, 1) * sizeof(RayBox));
    if (ensure_ray_buffer(ctx, be + bb + extra)) return -1;
    S.d_ent = (RayEntry *)ctx->d_rays;
    S.d_boxes = (RayBox *)(ctx->d_rays + be);
    S.rest = ctx->d_rays + be + bb;
    if (!S.ent.empty())
        HIPCHK(hipMemcpyAsync(S.d_ent, S.ent.data(), S.ent.size() * sizeof(RayEntry), hipMemcpyHostToDevice,
                              ctx->stream));
    if (nstart)
        HIPCHK(hipMemcpyAsync(S.d_boxes, S.boxes.data(), nstart * sizeof(RayBox), hipMemcpyHostToDevice,
                              ctx->stream));
    return 0;
}

// the checks of the three pair-list calls before any device work: the pair count (one int32 index per ray), the
// boxes, every pair; the pairs as device records
int check_pairs(const ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts, const float *const *tt_dev,
                const int *const *pred_dev, long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                const char *what, std::vector<RayPair> &pairs)
{
    if (nstart < 0 || npair < 0) return set_error("%s: null or bad argument", what);
    if (npair > INT_MAX) return set_error("%s: %lld pairs do not fit int32 ray indices", what, npair);
    if (npair > 0 && (!pair_box || !pair_recv)) return set_error("%s: null or bad argument", what);
    if (check_boxes(ctx, nstart, starts, tt_dev, (const void *const *)pred_dev, what)) return -1;
    pairs.resize(npair);
    for (long long r = 0; r < npair; r++) {
        if (pair_box[r] < 0 || pair_box[r] >= nstart)
            return set_error("%s: pair %lld names box %d, not in [0, %d)", what, r, pair_box[r], nstart);
        if (!inside(ctx, pair_recv[r]))
            return set_error("%s: receiver of pair %lld (%d, %d, %d) outside the grid", what, r, pair_recv[r].i,
                             pair_recv[r].j, pair_recv[r].k);
        pairs[r] = RayPair{pair_box[r], flat(ctx, pair_recv[r])};
    }
    return 0;
}

// The adjoint of nrays rays once the boxes and the rays' records are staged: the weights' scan (a NaN or infinite
// weight is refused before g is touched), S = 61 - E_w - E_d - K, the zeroed accumulators, launch(w, S) and the
// conversion of g.  d_scan: two ints of the ray buffer.
template <class Launch>
int run_adjoint(ttsweep_ctx *ctx, const char *what, const RayStage &S, long long nrays, int *d_scan,
                const double *w_dev, double *g_dev, int *hits_dev, int *scale, Launch launch)
{
    const long long ncells = (long long)ctx->nx * ctx->ny * ctx->nz;
    // S = 61 - E_w - E_d - K: a visit adds less than 2^(E_w + E_d + S) = 2^(61 - K) in magnitude, a ray visits a
    // cell at most once (T strictly decreases along it) and there are at most 2^K rays, so |acc[x]| < 2^61
    int shift = 0;
    bool weighted = false;
    if (w_dev && nrays > 0) {
        int scan[2] = {0, 0};
        HIPCHK(hipMemsetAsync(d_scan, 0, 2 * sizeof(int), ctx->stream));
        HIPCHK(launch_ray_weight_scan(w_dev, (int)nrays, d_scan, ctx->stream));
        HIPCHK(hipMemcpyAsync(scan, d_scan, sizeof(scan), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (scan[1]) return set_error("%s: a weight is NaN or infinite", what);
        if (scan[0]) {
            float dmax = 0.0f;
            for (const RayEntry &e : S.ent) dmax = std::max(dmax, e.d);
            int e_d = 0;
            std::frexp((double)dmax, &e_d);
            int k = 0;
            while ((1LL << k) < nrays) k++;
            shift = 61 - (scan[0] - 2048) - e_d - k;
            weighted = true;
        }
    }
    if (g_dev) HIPCHK(hipMemsetAsync(g_dev, 0, ncells * sizeof(double), ctx->stream));
    if (hits_dev) HIPCHK(hipMemsetAsync(hits_dev, 0, ncells * sizeof(int), ctx->stream));
    if (weighted || hits_dev) HIPCHK(launch(weighted ? w_dev : nullptr, shift));
    if (weighted) HIPCHK(launch_ray_fixed_to_double((long long *)g_dev, ncells, shift, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (scale) *scale = shift;
    return 0;
}

} // namespace

extern "C" {

int ttsweep_predecessors_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                const float *const *tt_dev, int *const *pred_dev)
{
    if (check_boxes(ctx, nstart, starts, tt_dev, (const void *const *)pred_dev, "ttsweep_predecessors_device"))
        return -1;
    if (nstart == 0) return 0;
    if (ctx_bind(ctx)) return -1;
    RayStage S;
    if (stage(ctx, nstart, starts, tt_dev, pred_dev, 0, S)) return -1;
    HIPCHK(launch_predecessors(S.G, ctx->d_v, S.d_boxes, nstart, S.d_ent, (int)S.ent.size(), ctx->exact_half,
                               ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));      // (also keeps S's host vectors alive past the copies)
    return 0;
}

long long ttsweep_trace_rays_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                    const float *const *tt_dev, const int *const *pred_dev,
                                    int nrecv, const ttsweep_start *receivers,
                                    long long *offsets, int *status, float *t_recv,
                                    int *cells_dev, float *hop_d_dev, long long capacity)
{
    const char *what = "ttsweep_trace_rays_device";
    if (check_boxes(ctx, nstart, starts, tt_dev, (const void *const *)pred_dev, what)) return -1;
    if (nrecv < 0 || (nrecv > 0 && !receivers) || !offsets) return set_error("%s: null or bad argument", what);
    std::vector<int> recv;
    if (flat_receivers(ctx, nrecv, receivers, what, recv)) return -1;
    const long long nrays = (long long)nstart * nrecv;
    offsets[0] = 0;
    if (nrays == 0) return 0;
    if (ctx_bind(ctx)) return -1;
    const size_t br = align_up(nrecv * sizeof(int)), bn = align_up(nrays * sizeof(int));
    const size_t bo = align_up((nrays + 1) * sizeof(long long));
    RayStage S;
    if (stage(ctx, nstart, starts, tt_dev, (int *const *)pred_dev, br + 3 * bn + bo, S)) return -1;
    int *d_recv = (int *)S.rest;
    int *d_count = (int *)(S.rest + br);
    int *d_status = (int *)(S.rest + br + bn);
    float *d_trecv = (float *)(S.rest + br + 2 * bn);
    long long *d_offsets = (long long *)(S.rest + br + 3 * bn);
    HIPCHK(hipMemcpyAsync(d_recv, recv.data(), nrecv * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const int nent = (int)S.ent.size();
    HIPCHK(launch_trace_rays(S.G, ctx->d_v, S.d_boxes, nstart, d_recv, nrecv, S.d_ent, nent, ctx->exact_half,
                             d_count, d_status, d_trecv, nullptr, nullptr, nullptr, false, ctx->stream));
    std::vector<int> count(nrays);
    HIPCHK(hipMemcpyAsync(count.data(), d_count, nrays * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d_status, nrays * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (t_recv) HIPCHK(hipMemcpyAsync(t_recv, d_trecv, nrays * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    long long total = 0;
    for (long long r = 0; r < nrays; r++) {
        total += count[r];
        offsets[r + 1] = total;
    }
    if (cells_dev && hop_d_dev && capacity >= total && total > 0) {
        HIPCHK(hipMemcpyAsync(d_offsets, offsets, (nrays + 1) * sizeof(long long), hipMemcpyHostToDevice,
                              ctx->stream));
        HIPCHK(launch_trace_rays(S.G, ctx->d_v, S.d_boxes, nstart, d_recv, nrecv, S.d_ent, nent, ctx->exact_half,
                                 d_count, d_status, d_trecv, d_offsets, cells_dev, hop_d_dev, true, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return total;
}

int ttsweep_ray_forward_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                               const float *const *tt_dev, const int *const *pred_dev,
                               int nrecv, const ttsweep_start *receivers,
                               const double *m_dev, double *y_dev, int *status)
{
    const char *what = "ttsweep_ray_forward_device";
    std::vector<int> recv;
    if (check_operator(ctx, nstart, starts, tt_dev, pred_dev, nrecv, receivers, what, recv)) return -1;
    const long long nrays = (long long)nstart * nrecv;
    if (nrays == 0) return 0;
    if (!m_dev || !y_dev) return set_error("%s: null or bad argument", what);
    if (ctx_bind(ctx)) return -1;
    const size_t br = align_up(nrecv * sizeof(int)), bn = align_up(nrays * sizeof(int));
    RayStage S;
    if (stage(ctx, nstart, starts, tt_dev, (int *const *)pred_dev, br + bn, S)) return -1;
    int *d_recv = (int *)S.rest;
    int *d_status = (int *)(S.rest + br);
    HIPCHK(hipMemcpyAsync(d_recv, recv.data(), nrecv * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_ray_forward(S.G, ctx->d_v, S.d_boxes, nstart, d_recv, nrecv, S.d_ent, (int)S.ent.size(),
                              ctx->exact_half, m_dev, y_dev, d_status, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d_status, nrays * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int ttsweep_ray_adjoint_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                               const float *const *tt_dev, const int *const *pred_dev,
                               int nrecv, const ttsweep_start *receivers,
                               const double *w_dev, double *g_dev, int *hits_dev, int *scale)
{
    const char *what = "ttsweep_ray_adjoint_device";
    std::vector<int> recv;
    if (check_operator(ctx, nstart, starts, tt_dev, pred_dev, nrecv, receivers, what, recv)) return -1;
    if (!w_dev != !g_dev) return set_error("%s: w and g must both be given or both be NULL", what);
    const long long nrays = (long long)nstart * nrecv;
    if (!g_dev && !hits_dev) {
        if (scale) *scale = 0;
        return 0;
    }
    if (ctx_bind(ctx)) return -1;
    const size_t br = align_up(std::max(nrecv, 1) * sizeof(int));
    RayStage S;
    if (stage(ctx, nstart, starts, tt_dev, (int *const *)pred_dev, br + 256, S)) return -1;
    int *d_recv = (int *)S.rest;
    int *d_scan = (int *)(S.rest + br);
    if (nrecv)
        HIPCHK(hipMemcpyAsync(d_recv, recv.data(), nrecv * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    return run_adjoint(ctx, what, S, nrays, d_scan, w_dev, g_dev, hits_dev, scale, [&](const double *w, int shift) {
        return launch_ray_adjoint(S.G, ctx->d_v, S.d_boxes, nstart, d_recv, nrecv, S.d_ent, (int)S.ent.size(),
                                  ctx->exact_half, w, shift, (long long *)g_dev, hits_dev, ctx->stream);
    });
}

int ttsweep_ray_pairs_forward_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                     const float *const *tt_dev, const int *const *pred_dev,
                                     long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                     const double *m_dev, double *y_dev, int *status)
{
    const char *what = "ttsweep_ray_pairs_forward_device";
    std::vector<RayPair> pairs;
    if (check_pairs(ctx, nstart, starts, tt_dev, pred_dev, npair, pair_box, pair_recv, what, pairs)) return -1;
    if (npair == 0) return 0;
    if (!m_dev || !y_dev) return set_error("%s: null or bad argument", what);
    if (ctx_bind(ctx)) return -1;
    const size_t bp = align_up(npair * sizeof(RayPair)), bn = align_up(npair * sizeof(int));
    RayStage S;
    if (stage(ctx, nstart, starts, tt_dev, (int *const *)pred_dev, bp + bn, S)) return -1;
    RayPair *d_pairs = (RayPair *)S.rest;
    int *d_status = (int *)(S.rest + bp);
    HIPCHK(hipMemcpyAsync(d_pairs, pairs.data(), npair * sizeof(RayPair), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_ray_pairs_forward(S.G, ctx->d_v, S.d_boxes, d_pairs, (int)npair, S.d_ent, (int)S.ent.size(),
                                    ctx->exact_half, m_dev, y_dev, d_status, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d_status, npair * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int ttsweep_ray_pairs_adjoint_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                     const float *const *tt_dev, const int *const *pred_dev,
                                     long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                     const double *w_dev, double *g_dev, int *hits_dev, int *scale)
{
    const char *what = "ttsweep_ray_pairs_adjoint_device";
    std::vector<RayPair> pairs;
    if (check_pairs(ctx, nstart, starts, tt_dev, pred_dev, npair, pair_box, pair_recv, what, pairs)) return -1;
    if (!w_dev != !g_dev) return set_error("%s: w and g must both be given or both be NULL", what);
    if (!g_dev && !hits_dev) {
        if (scale) *scale = 0;
        return 0;
    }
    if (ctx_bind(ctx)) return -1;
    const size_t bp = align_up(std::max<long long>(npair, 1) * sizeof(RayPair));
    RayStage S;
    if (stage(ctx, nstart, starts, tt_dev, (int *const *)pred_dev, bp + 256, S)) return -1;
    RayPair *d_pairs = (RayPair *)S.rest;
    int *d_scan = (int *)(S.rest + bp);
    if (npair)
        HIPCHK(hipMemcpyAsync(d_pairs, pairs.data(), npair * sizeof(RayPair), hipMemcpyHostToDevice, ctx->stream));
    return run_adjoint(ctx, what, S, npair, d_scan, w_dev, g_dev, hits_dev, scale, [&](const double *w, int shift) {
        return launch_ray_pairs_adjoint(S.G, ctx->d_v, S.d_boxes, d_pairs, (int)npair, S.d_ent, (int)S.ent.size(),
                                        ctx->exact_half, w, shift, (long long *)g_dev, hits_dev, ctx->stream);
    });
}

int ttsweep_ray_pairs_geometry_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                      const float *const *tt_dev, const int *const *pred_dev,
                                      long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                      int *status, float *t_recv_dev, int *hops_dev, double *length_dev,
                                      int *recv_hop_dev, float *recv_d_dev, float *recv_dt_dev,
                                      int *src_hop_dev, float *src_d_dev, float *src_dt_dev, int *deep_dev)
{
    const char *what = "ttsweep_ray_pairs_geometry_device";
    std::vector<RayPair> pairs;
    if (check_pairs(ctx, nstart, starts, tt_dev, pred_dev, npair, pair_box, pair_recv, what, pairs)) return -1;
    if (npair == 0) return 0;
    if (ctx_bind(ctx)) return -1;
    const size_t bp = align_up(npair * sizeof(RayPair)), bn = align_up(npair * sizeof(int));
    RayStage S;
    if (stage(ctx, nstart, starts, tt_dev, (int *const *)pred_dev, bp + bn, S)) return -1;
    RayPair *d_pairs = (RayPair *)S.rest;
    int *d_status = (int *)(S.rest + bp);
    HIPCHK(hipMemcpyAsync(d_pairs, pairs.data(), npair * sizeof(RayPair), hipMemcpyHostToDevice, ctx->stream));
    const RayGeometryOut out{t_recv_dev, hops_dev, length_dev, recv_hop_dev, recv_d_dev, recv_dt_dev,
                             src_hop_dev, src_d_dev, src_dt_dev, deep_dev};
    HIPCHK(launch_ray_pairs_geometry(S.G, ctx->d_v, S.d_boxes, d_pairs, (int)npair, S.d_ent, (int)S.ent.size(),
                                     ctx->exact_half, d_status, out, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d_status, npair * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

} // extern "C"
