// ttsweep_rays.cpp - the ray calls of include/ttsweep.h: ttsweep_predecessors_device,
// ttsweep_trace_rays_device, the Frechet operators ttsweep_ray_forward_device / ttsweep_ray_adjoint_device and
// their pair-list forms ttsweep_ray_pairs_{forward,adjoint,geometry}_device (kernels: ttsweep_rays.hip).
// Argument checks, the star's ray entries, one staging of the device arrays for all seven calls, the host-side scan of
// the per-ray cell counts, the fixed-point helpers the Fresnel calls share.  Nothing here touches the solve's state: the boxes the
// confirming-pass shortcut of ttsweep_solve remembers, its pools and its options stay as they are.
#include "ttsweep_ctx.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

using namespace ttsweep;

namespace {

bool inside(const ttsweep_ctx *ctx, const ttsweep_start &p)
{
    return p.i >= 0 && p.i < ctx->nx && p.j >= 0 && p.j < ctx->ny && p.k >= 0 && p.k < ctx->nz;
}

int flat(const ttsweep_ctx *ctx, const ttsweep_start &p) { return (p.i * ctx->ny + p.j) * ctx->nz + p.k; }

// what both calls check before any device work
int check_boxes(const ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts, const float *const *tt_dev,
                const int *const *pred_dev, const char *what)
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

// the boxes and the rays of a call once its checks have passed: the cross product of the boxes with recv (FLOATBOX
// indices), or the records of a pair list
struct RayInput {
    int nstart = 0;
    const ttsweep_start *starts = nullptr;
    const float *const *tt_dev = nullptr;
    const int *const *pred_dev = nullptr;
    bool by_pairs = false;
    std::vector<int> recv;
    std::vector<RayPair> pairs;
    long long nrays() const { return by_pairs ? (long long)pairs.size() : (long long)nstart * (long long)recv.size(); }
};

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
                   RayInput &in)
{
    if (nstart < 0 || nrecv < 0 || (nrecv > 0 && !receivers)) return set_error("%s: null or bad argument", what);
    if ((long long)nstart * nrecv > INT_MAX)
        return set_error("%s: %d starts x %d receivers do not fit int32 ray indices", what, nstart, nrecv);
    if (check_boxes(ctx, nstart, starts, tt_dev, pred_dev, what)) return -1;
    in = RayInput{nstart, starts, tt_dev, pred_dev};
    return flat_receivers(ctx, nrecv, receivers, what, in.recv);
}

// the checks of the three pair-list calls before any device work: the pair count (one int32 index per ray), the
// boxes, every pair; the pairs as device records
int check_pairs(const ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts, const float *const *tt_dev,
                const int *const *pred_dev, long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                const char *what, RayInput &in)
{
    if (nstart < 0 || npair < 0) return set_error("%s: null or bad argument", what);
    if (npair > INT_MAX) return set_error("%s: %lld pairs do not fit int32 ray indices", what, npair);
    if (npair > 0 && (!pair_box || !pair_recv)) return set_error("%s: null or bad argument", what);
    if (check_boxes(ctx, nstart, starts, tt_dev, pred_dev, what)) return -1;
    in = RayInput{nstart, starts, tt_dev, pred_dev, true};
    in.pairs.resize(npair);
    for (long long r = 0; r < npair; r++) {
        if (pair_box[r] < 0 || pair_box[r] >= nstart)
            return set_error("%s: pair %lld names box %d, not in [0, %d)", what, r, pair_box[r], nstart);
        if (!inside(ctx, pair_recv[r]))
            return set_error("%s: receiver of pair %lld (%d, %d, %d) outside the grid", what, r, pair_recv[r].i,
                             pair_recv[r].j, pair_recv[r].k);
        in.pairs[r] = RayPair{pair_box[r], flat(ctx, pair_recv[r])};
    }
    return 0;
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

// What a ray call holds once stage() has run: the arguments of its kernels (A, L: the entries, the box records and
// the receivers or pair records, uploaded) and the per-ray arrays it copies back, all of them in ctx->d_rays
struct Staged {
    std::vector<RayEntry> ent;
    std::vector<RayBox> boxes;
    RayArgs A{};
    RayList L{};
    int *d_status = nullptr, *d_scan = nullptr;
    int *d_count = nullptr;             // trace only: cells per ray, t_recv and the offsets of the fill pass
    float *d_trecv = nullptr;
    long long *d_offsets = nullptr;
};

// The preparation every ray call shares once it is not refused: the device, the layout of its arrays in ctx->d_rays
// (grown when it does not hold them), the upload of the entries, the boxes and the list of rays.  The host arrays
// behind the copies (S, in) live until the caller has synchronised.
int stage(ttsweep_ctx *ctx, const RayInput &in, bool trace, Staged &S)
{
    if (ctx_bind(ctx)) return -1;
    S.A.G = ray_geom(ctx);
    S.A.v = ctx->d_v;
    S.ent = ray_entries(ctx, S.A.G);
    S.A.nentries = (int)S.ent.size();
    S.boxes.resize(in.nstart);
    for (int s = 0; s < in.nstart; s++)
        S.boxes[s] = RayBox{in.tt_dev[s], (int *)in.pred_dev[s], flat(ctx, in.starts[s]), 0};
    S.L.nrecv = (int)in.recv.size();
    S.L.n = in.nrays();
    ScratchLayout lay;
    lay.add(S.A.entries, S.ent.size());
    lay.add(S.A.boxes, S.boxes.size());
    if (in.by_pairs) lay.add(S.L.pairs, in.pairs.size());
    else lay.add(S.L.recv, in.recv.size());
    lay.add(S.d_status, S.L.n);
    if (trace) {
        lay.add(S.d_count, S.L.n);
        lay.add(S.d_trecv, S.L.n);
        lay.add(S.d_offsets, S.L.n + 1);
    }
    lay.add(S.d_scan, 2);
    if (ensure_ray_buffer(ctx, lay.size())) return -1;
    lay.place(ctx->d_rays);
    auto upload = [&](const void *dst, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(const_cast<void *>(dst), src, bytes, hipMemcpyHostToDevice, ctx->stream)
                     : hipSuccess;
    };
    HIPCHK(upload(S.A.entries, S.ent.data(), S.ent.size() * sizeof(RayEntry)));
    HIPCHK(upload(S.A.boxes, S.boxes.data(), S.boxes.size() * sizeof(RayBox)));
    HIPCHK(upload(S.L.recv, in.recv.data(), in.recv.size() * sizeof(int)));
    HIPCHK(upload(S.L.pairs, in.pairs.data(), in.pairs.size() * sizeof(RayPair)));
    return 0;
}

// the end of a call that was not refused: the statuses to the host, and the stream drained
int finish(ttsweep_ctx *ctx, const Staged &S, int *status)
{
    if (status && S.L.n)
        HIPCHK(hipMemcpyAsync(status, S.d_status, S.L.n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// G m of the rays of either kind of list, after the list's own checks
int run_forward(ttsweep_ctx *ctx, const char *what, const RayInput &in, const double *m_dev, double *y_dev,
                int *status)
{
    if (in.nrays() == 0) return 0;
    if (!m_dev || !y_dev) return set_error("%s: null or bad argument", what);
    Staged S;
    if (stage(ctx, in, false, S)) return -1;
    HIPCHK(launch_ray_forward(S.A, S.L, ctx->exact_half, m_dev, y_dev, S.d_status, ctx->stream));
    return finish(ctx, S, status);
}

// G^T w and the hits of the rays of either kind of list, after the list's own checks: the weights' scan (a NaN or
// infinite weight is refused before g is touched), the shift, the zeroed accumulators, the walk and the conversion
// of g
int run_adjoint(ttsweep_ctx *ctx, const char *what, const RayInput &in, const double *w_dev, double *g_dev,
                int *hits_dev, int *scale)
{
    if (!w_dev != !g_dev) return set_error("%s: w and g must both be given or both be NULL", what);
    if (!g_dev && !hits_dev) {
        if (scale) *scale = 0;
        return 0;
    }
    Staged S;
    if (stage(ctx, in, false, S)) return -1;
    // S = 61 - E_w - E_d - K: a visit adds less than 2^(E_w + E_d + S) = 2^(61 - K) in magnitude, a ray visits a
    // cell at most once (T strictly decreases along it) and there are at most 2^K rays, so |acc[x]| < 2^61
    const long long nrays = in.nrays();
    int e_w = 0, shift = 0;
    bool bad = false;
    if (w_dev && nrays > 0 && fixed_point_scan(ctx, w_dev, nrays, S.d_scan, &e_w, &bad)) return -1;
    if (bad) return set_error("%s: a weight is NaN or infinite", what);
    if (e_w) {
        float dmax = 0.0f;
        for (const RayEntry &e : S.ent) dmax = std::max(dmax, e.d);
        int e_d = 0;
        std::frexp((double)dmax, &e_d);
        shift = 61 - (e_w - 2048) - e_d - ceil_log2(nrays);
    }
    return fixed_point_adjoint(ctx, e_w != 0, shift, g_dev, hits_dev, scale, [&] {
        HIPCHK(launch_ray_adjoint(S.A, S.L, ctx->exact_half, e_w ? w_dev : nullptr, shift, (long long *)g_dev,
                                  hits_dev, ctx->stream));
        return 0;
    });
}

} // namespace

int ttsweep::fixed_point_scan(ttsweep_ctx *ctx, const double *v, long long n, int *d_scan, int *e, bool *bad)
{
    int scan[2] = {0, 0};
    HIPCHK(hipMemsetAsync(d_scan, 0, 2 * sizeof(int), ctx->stream));
    HIPCHK(launch_ray_weight_scan(v, (int)n, d_scan, ctx->stream));
    HIPCHK(hipMemcpyAsync(scan, d_scan, sizeof(scan), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *e = scan[0];
    *bad = scan[1] != 0;
    return 0;
}

extern "C" {

int ttsweep_predecessors_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                const float *const *tt_dev, int *const *pred_dev)
{
    if (check_boxes(ctx, nstart, starts, tt_dev, pred_dev, "ttsweep_predecessors_device"))
        return -1;
    if (nstart == 0) return 0;
    Staged S;
    if (stage(ctx, RayInput{nstart, starts, tt_dev, pred_dev}, false, S)) return -1;
    HIPCHK(launch_predecessors(S.A, nstart, ctx->exact_half, ctx->stream));
    return finish(ctx, S, nullptr);
}

long long ttsweep_trace_rays_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                    const float *const *tt_dev, const int *const *pred_dev,
                                    int nrecv, const ttsweep_start *receivers,
                                    long long *offsets, int *status, float *t_recv,
                                    int *cells_dev, float *hop_d_dev, long long capacity)
{
    const char *what = "ttsweep_trace_rays_device";
    if (check_boxes(ctx, nstart, starts, tt_dev, pred_dev, what)) return -1;
    if (nrecv < 0 || (nrecv > 0 && !receivers) || !offsets) return set_error("%s: null or bad argument", what);
    RayInput in{nstart, starts, tt_dev, pred_dev};
    if (flat_receivers(ctx, nrecv, receivers, what, in.recv)) return -1;
    const long long nrays = in.nrays();
    offsets[0] = 0;
    if (nrays == 0) return 0;
    Staged S;
    if (stage(ctx, in, true, S)) return -1;
    HIPCHK(launch_trace_rays(S.A, S.L, ctx->exact_half, S.d_count, S.d_status, S.d_trecv, nullptr, nullptr, nullptr,
                             false, ctx->stream));
    std::vector<int> count(nrays);
    HIPCHK(hipMemcpyAsync(count.data(), S.d_count, nrays * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (t_recv) HIPCHK(hipMemcpyAsync(t_recv, S.d_trecv, nrays * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (finish(ctx, S, status)) return -1;
    long long total = 0;
    for (long long r = 0; r < nrays; r++) {
        total += count[r];
        offsets[r + 1] = total;
    }
    if (cells_dev && hop_d_dev && capacity >= total && total > 0) {
        HIPCHK(hipMemcpyAsync(S.d_offsets, offsets, (nrays + 1) * sizeof(long long), hipMemcpyHostToDevice,
                              ctx->stream));
        HIPCHK(launch_trace_rays(S.A, S.L, ctx->exact_half, S.d_count, S.d_status, S.d_trecv, S.d_offsets, cells_dev,
                                 hop_d_dev, true, ctx->stream));
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
    RayInput in;
    if (check_operator(ctx, nstart, starts, tt_dev, pred_dev, nrecv, receivers, what, in)) return -1;
    return run_forward(ctx, what, in, m_dev, y_dev, status);
}

int ttsweep_ray_adjoint_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                               const float *const *tt_dev, const int *const *pred_dev,
                               int nrecv, const ttsweep_start *receivers,
                               const double *w_dev, double *g_dev, int *hits_dev, int *scale)
{
    const char *what = "ttsweep_ray_adjoint_device";
    RayInput in;
    if (check_operator(ctx, nstart, starts, tt_dev, pred_dev, nrecv, receivers, what, in)) return -1;
    return run_adjoint(ctx, what, in, w_dev, g_dev, hits_dev, scale);
}

int ttsweep_ray_pairs_forward_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                     const float *const *tt_dev, const int *const *pred_dev,
                                     long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                     const double *m_dev, double *y_dev, int *status)
{
    const char *what = "ttsweep_ray_pairs_forward_device";
    RayInput in;
    if (check_pairs(ctx, nstart, starts, tt_dev, pred_dev, npair, pair_box, pair_recv, what, in)) return -1;
    return run_forward(ctx, what, in, m_dev, y_dev, status);
}

int ttsweep_ray_pairs_adjoint_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                     const float *const *tt_dev, const int *const *pred_dev,
                                     long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                     const double *w_dev, double *g_dev, int *hits_dev, int *scale)
{
    const char *what = "ttsweep_ray_pairs_adjoint_device";
    RayInput in;
    if (check_pairs(ctx, nstart, starts, tt_dev, pred_dev, npair, pair_box, pair_recv, what, in)) return -1;
    return run_adjoint(ctx, what, in, w_dev, g_dev, hits_dev, scale);
}

int ttsweep_ray_pairs_geometry_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                      const float *const *tt_dev, const int *const *pred_dev,
                                      long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                      int *status, float *t_recv_dev, int *hops_dev, double *length_dev,
                                      int *recv_hop_dev, float *recv_d_dev, float *recv_dt_dev,
                                      int *src_hop_dev, float *src_d_dev, float *src_dt_dev, int *deep_dev)
{
    const char *what = "ttsweep_ray_pairs_geometry_device";
    RayInput in;
    if (check_pairs(ctx, nstart, starts, tt_dev, pred_dev, npair, pair_box, pair_recv, what, in)) return -1;
    if (npair == 0) return 0;
    Staged S;
    if (stage(ctx, in, false, S)) return -1;
    const RayGeometryOut out{t_recv_dev, hops_dev, length_dev, recv_hop_dev, recv_d_dev, recv_dt_dev,
                             src_hop_dev, src_d_dev, src_dt_dev, deep_dev};
    HIPCHK(launch_ray_pairs_geometry(S.A, S.L, ctx->exact_half, S.d_status, out, ctx->stream));
    return finish(ctx, S, status);
}

} // extern "C"
