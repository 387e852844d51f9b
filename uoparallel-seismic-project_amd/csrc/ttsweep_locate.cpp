// ttsweep_locate.cpp - ttsweep_locate_device, ttsweep_locate_window_device, ttsweep_locate_subcell_device and
// ttsweep_locate_confidence_device of include/ttsweep.h (kernels: ttsweep_locate.hip).  The four entry points are built
// from the same pieces: the argument, window, grid and box-pointer checks (each refusal once; an entry point calls them
// in the order in which its refusals take precedence, those that need no device first), one scratch carver (Scratch,
// ttsweep_ctx.h), the check scan of picks and weights (refused before any output is touched) and, for the searches over
// windows, one cut of the groups into batches whose per-tile partials stay within a fixed budget and one driver of
// those batches.  The scratch is allocated per call: nothing of the context changes, so the boxes the confirming-pass
// shortcut of ttsweep_solve remembers, its pools and its options stay as they are.
#include "ttsweep_ctx.h"

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

using namespace ttsweep;

namespace {

// per-tile partials of one batch of events, at most (12 bytes each)
// (mirrored: tests/test_locate_cpu.py::test_case_constants_mirror_the_sources)
constexpr long long LOC_PARTIALS = 1LL << 24;

// blocks (group, tile) of one batch of ttsweep_locate_window_device / ttsweep_locate_subcell_device, at most (8 bytes
// each) (both mirrored: tests/test_gpu_locate_subcell.py::test_a_batch_edge)
constexpr long long LOC_WIN_BLOCKS = 1LL << 22;

int check_counts(const char *what, int nbox, int nevent, bool pointers)
{
    if (nbox < 1 || nevent < 1 || !pointers) return set_error("%s: null or bad argument", what);
    if ((long long)nbox * nevent > INT_MAX)
        return set_error("%s: %d boxes x %d events do not fit int32 pick indices", what, nbox, nevent);
    return 0;
}

int check_window_pair(const char *what, const int *lo, const int *hi)
{
    if (!lo != !hi) return set_error("%s: lo and hi must both be given or both be NULL", what);
    return 0;
}

int check_window_order(const char *what, int nevent, const int *lo, const int *hi)
{
    for (long long i = 0; lo && i < 3LL * nevent; i++)
        if (lo[i] < 0 || lo[i] > hi[i])
            return set_error("%s: event %d has a bad window [%d, %d] along axis %d", what, (int)(i / 3), lo[i], hi[i],
                             (int)(i % 3));
    return 0;
}

// n: the cells of the grid per axis
int check_window_inside(const char *what, int nevent, const int *lo, const int *hi, const int *n)
{
    for (long long i = 0; hi && i < 3LL * nevent; i++)
        if (hi[i] >= n[i % 3])
            return set_error("%s: event %d has a window [%d, %d] along axis %d that leaves the grid (%d cells)", what,
                             (int)(i / 3), lo[i], hi[i], (int)(i % 3), n[i % 3]);
    return 0;
}

int check_grid(const char *what, const ttsweep_ctx *ctx)
{
    if (!ctx) return set_error("%s: null or bad argument", what);
    if ((long long)ctx->nx * ctx->ny * ctx->nz > INT_MAX)
        return set_error("%s: %d x %d x %d cells do not fit int32 indices", what, ctx->nx, ctx->ny, ctx->nz);
    return 0;
}

int check_boxes(const char *what, int nbox, const float *const *tt_dev)
{
    for (int k = 0; k < nbox; k++)
        if (!tt_dev[k]) return set_error("%s: null box pointer %d", what, k);
    return 0;
}

// The box pointers to d_boxes, then the check scan: invW of every event to d_invw, and the first event that is
// refused, by its first reason.  d_flag holds nflag words per event, [nflag][nevent]: the first is written here, the
// others by check kernels the caller has enqueued; more(flag, e) refuses event e on those, after the reasons here.
template <typename More>
int check_events(const char *what, ttsweep_ctx *ctx, int nbox, const float *const *tt_dev, int nevent,
                 const double *picks_dev, const double *weights_dev, const float **d_boxes, double *d_invw, int *d_flag,
                 int nflag, More more)
{
    HIPCHK(hipMemcpyAsync(d_boxes, tt_dev, nbox * sizeof(float *), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(launch_locate_check(nbox, nevent, picks_dev, weights_dev, d_invw, d_flag, ctx->stream));
    std::vector<int> flag((size_t)nflag * nevent);
    HIPCHK(hipMemcpyAsync(flag.data(), d_flag, flag.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int e = 0; e < nevent; e++) {
        if (flag[e] & 1) return set_error("%s: event %d has a NaN or infinite pick", what, e);
        if (flag[e] & 2) return set_error("%s: event %d has a negative, NaN or infinite weight", what, e);
        if (flag[e] & 4) return set_error("%s: event %d has no weight above zero", what, e);
        if (more(flag.data(), e)) return -1;
    }
    return 0;
}

// the same with one flag word per event and no further reasons
int check_events(const char *what, ttsweep_ctx *ctx, int nbox, const float *const *tt_dev, int nevent,
                 const double *picks_dev, const double *weights_dev, const float **d_boxes, double *d_invw, int *d_flag)
{
    return check_events(what, ctx, nbox, tt_dev, nevent, picks_dev, weights_dev, d_boxes, d_invw, d_flag, 1,
                        [](const int *, int) { return 0; });
}

const unsigned long long NAN_BITS = 0x7ff8000000000000ULL;     // the quiet NaN of t0 when no candidate is admissible

// the windows of the events: lo / hi [nevent][3], or the whole grid of n cells per axis for every event
struct Windows {
    const int *lo, *hi;
    int whole_lo[3], whole_hi[3];
    Windows(const int *lo, const int *hi, const int *n) : lo(lo), hi(hi), whole_lo{0, 0, 0}, whole_hi{n[0] - 1, n[1] - 1, n[2] - 1} {}
    const int *lo_of(int e) const { return lo ? lo + 3LL * e : whole_lo; }
    const int *hi_of(int e) const { return hi ? hi + 3LL * e : whole_hi; }
    // the events from e on that share its window, at most LOC_WIN_ET: one group
    int run(int e, int nevent) const
    {
        int ne = 1;
        while (ne < LOC_WIN_ET && e + ne < nevent && !memcmp(lo_of(e + ne), lo_of(e), 3 * sizeof(int)) &&
               !memcmp(hi_of(e + ne), hi_of(e), 3 * sizeof(int)))
            ne++;
        return ne;
    }
};

// groups [g0, g1) of one batch, with its partials, blocks and events
struct Batch {
    size_t g0, g1;
    long long parts, blocks;
    int ne;
};

// The groups (WinGroup or SubGroup) cut into batches whose partials stay within LOC_PARTIALS and whose block table
// within LOC_WIN_BLOCKS entries; a group beyond either on its own is a batch.  With the most partials, blocks, groups
// and events of a batch (at least 1 each): what the scratch is sized by.
struct Batches {
    std::vector<Batch> list;
    long long maxp = 1, maxb = 1;
    size_t maxg = 1;
    int maxe = 1;
};

template <typename Group>
Batches cut_batches(const std::vector<Group> &groups)
{
    Batches B;
    for (size_t g = 0; g < groups.size();) {
        Batch b{g, g, 0, 0, 0};
        while (b.g1 < groups.size()) {
            const Group &G = groups[b.g1];
            if (b.g1 > b.g0 && (b.parts + (long long)G.ne * G.ntiles > LOC_PARTIALS || b.blocks + G.ntiles > LOC_WIN_BLOCKS))
                break;
            b.parts += (long long)G.ne * G.ntiles;
            b.blocks += G.ntiles;
            b.g1++;
        }
        b.ne = groups[b.g1 - 1].e0 + groups[b.g1 - 1].ne - groups[b.g0].e0;
        B.list.push_back(b);
        B.maxp = std::max(B.maxp, b.parts);
        B.maxb = std::max(B.maxb, b.blocks);
        B.maxg = std::max(B.maxg, b.g1 - b.g0);
        B.maxe = std::max(B.maxe, b.ne);
        g = b.g1;
    }
    return B;
}

// The batches one after the other: the partials of the batch's groups laid out from 0, its events' groups (d_evgroup)
// and its blocks listed, both uploaded with the groups, then launch(first event, events, blocks listed first, blocks
// in all).  later(G): the blocks of group G are listed after those of the groups it is false for.  A batch is awaited
// before the next one: the host tables are rebuilt.
template <typename Group, typename Later, typename Launch>
int run_batches(ttsweep_ctx *ctx, std::vector<Group> &groups, const Batches &B, Group *d_groups, WinBlock *d_blocks,
                int *d_evgroup, Later later, Launch launch)
{
    std::vector<WinBlock> blocks;
    std::vector<int> evgroup;
    for (const Batch &b : B.list) {
        blocks.clear();
        evgroup.clear();
        long long part = 0;
        for (size_t g = b.g0; g < b.g1; g++) {
            groups[g].part = part;
            part += (long long)groups[g].ne * groups[g].ntiles;
            evgroup.insert(evgroup.end(), groups[g].ne, (int)(g - b.g0));
        }
        int nfirst = 0;
        for (int pass = 0; pass < 2; pass++) {
            for (size_t g = b.g0; g < b.g1; g++)
                for (int t = 0; later(groups[g]) == (pass == 1) && t < groups[g].ntiles; t++)
                    blocks.push_back(WinBlock{(int)(g - b.g0), t});
            if (pass == 0) nfirst = (int)blocks.size();
        }
        HIPCHK(hipMemcpyAsync(d_groups, groups.data() + b.g0, (b.g1 - b.g0) * sizeof(Group), hipMemcpyHostToDevice,
                              ctx->stream));
        HIPCHK(hipMemcpyAsync(d_blocks, blocks.data(), blocks.size() * sizeof(WinBlock), hipMemcpyHostToDevice,
                              ctx->stream));
        HIPCHK(hipMemcpyAsync(d_evgroup, evgroup.data(), b.ne * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        if (launch(groups[b.g0].e0, b.ne, nfirst, (int)blocks.size())) return -1;
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

} // namespace

extern "C" {

// Event batches sized so that the per-tile partials stay within LOC_PARTIALS, then the misfit volumes.
int ttsweep_locate_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev, int nevent, const double *picks_dev,
                          const double *weights_dev, int *cell_dev, double *misfit_dev, double *t0_dev, int nvol,
                          const int *vol_events, double *const *vol_dev)
{
    const char *what = "ttsweep_locate_device";
    if (check_counts(what, nbox, nevent, tt_dev && picks_dev && nvol >= 0 && (nvol == 0 || (vol_events && vol_dev))))
        return -1;
    if (check_grid(what, ctx) || check_boxes(what, nbox, tt_dev)) return -1;
    for (int v = 0; v < nvol; v++) {
        if (vol_events[v] < 0 || vol_events[v] >= nevent)
            return set_error("%s: volume event %d (%d) outside [0, %d)", what, v, vol_events[v], nevent);
        if (!vol_dev[v]) return set_error("%s: null volume pointer %d", what, v);
    }
    if (nvol > 65535) return set_error("%s: %d volumes in one call (at most 65535)", what, nvol);
    if (ctx_bind(ctx)) return -1;

    const int N = ctx->nx * ctx->ny * ctx->nz;
    const int ntiles = (N + locate_tile_cells() - 1) / locate_tile_cells();
    const int eb = (int)std::max(1LL, std::min<long long>({(long long)nevent, LOC_PARTIALS / ntiles, 65535LL * 8}));
    const float **d_boxes;
    double *d_invw, **d_vol;
    int *d_flag, *d_vev, *d_x;
    unsigned long long *d_key;
    Scratch S;
    S.add(d_boxes, nbox);
    S.add(d_invw, nevent);
    S.add(d_flag, nevent);
    S.add(d_vev, std::max(nvol, 1));
    S.add(d_vol, std::max(nvol, 1));                   // a piece of its own: sharing d_vev's let its end reach d_key
    S.add(d_key, (size_t)eb * ntiles);
    S.add(d_x, (size_t)eb * ntiles);
    HIPCHK(S.alloc());
    if (check_events(what, ctx, nbox, tt_dev, nevent, picks_dev, weights_dev, d_boxes, d_invw, d_flag)) return -1;

    if (cell_dev || misfit_dev || t0_dev)
        for (int e0 = 0; e0 < nevent; e0 += eb) {
            const int ne = std::min(eb, nevent - e0);
            HIPCHK(launch_locate_search(d_boxes, nbox, N, picks_dev, weights_dev, d_invw, e0, ne, ntiles, d_key, d_x,
                                        ctx->stream));
            HIPCHK(launch_locate_final(d_boxes, nbox, picks_dev, weights_dev, d_invw, e0, ne, ntiles, d_key, d_x,
                                       cell_dev, misfit_dev, t0_dev, NAN_BITS, ctx->stream));
        }
    if (nvol) {
        HIPCHK(hipMemcpyAsync(d_vev, vol_events, nvol * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(d_vol, vol_dev, nvol * sizeof(double *), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(launch_locate_volume(d_boxes, nbox, N, picks_dev, weights_dev, d_invw, d_vev, d_vol, nvol, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// Windows and strides are host arrays, so every refusal that concerns them comes before the device is touched.  The
// events are cut into groups of at most 8 consecutive events with one window (the kernel loads a candidate's travel
// times once per group), the groups into batches (cut_batches).  The scratch is 16 bytes per event, 40 per group, 8 per
// block and 12 per partial of the largest batch: nothing grows with the grid.
int ttsweep_locate_window_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev, int nevent,
                                 const double *picks_dev, const double *weights_dev, const int *lo, const int *hi,
                                 const int *stride, int *cell_dev, double *misfit_dev, double *t0_dev)
{
    const char *what = "ttsweep_locate_window_device";
    if (check_counts(what, nbox, nevent, tt_dev && picks_dev) || check_window_pair(what, lo, hi)) return -1;
    int st[3] = {1, 1, 1};
    for (int a = 0; stride && a < 3; a++) {
        if (stride[a] < 1) return set_error("%s: stride %d along axis %d is below 1", what, stride[a], a);
        st[a] = stride[a];
    }
    if (check_window_order(what, nevent, lo, hi) || check_grid(what, ctx)) return -1;
    const int n[3] = {ctx->nx, ctx->ny, ctx->nz};
    if (check_window_inside(what, nevent, lo, hi, n) || check_boxes(what, nbox, tt_dev)) return -1;

    // groups, and batches of groups
    const Windows win(lo, hi, n);
    const int tile = locate_window_tile_cells();
    // the index steps of the lattice; a stride beyond the grid is never stepped (one node along that axis)
    const int mx = (int)std::min<long long>(st[0], n[0]) * n[1] * n[2], my = (int)std::min<long long>(st[1], n[1]) * n[2];
    const int mz = std::min(st[2], n[2]);
    std::vector<WinGroup> groups;
    for (int e = 0; e < nevent;) {
        const int *l = win.lo_of(e), *h = win.hi_of(e);
        WinGroup g;
        g.e0 = e;
        g.ne = win.run(e, nevent);
        long long c[3];
        for (int a = 0; a < 3; a++) c[a] = (h[a] - l[a]) / st[a] + 1;
        g.x0 = (l[0] * n[1] + l[1]) * n[2] + l[2];
        g.cy = (int)c[1];
        g.cz = (int)c[2];
        g.ncand = (int)(c[0] * c[1] * c[2]);            // at most ncells
        g.ntiles = (g.ncand + tile - 1) / tile;
        g.part = 0;
        groups.push_back(g);
        e += g.ne;
    }
    const Batches batches = cut_batches(groups);
    if (ctx_bind(ctx)) return -1;

    const float **d_boxes;
    double *d_invw;
    int *d_flag, *d_evgroup, *d_x;
    WinGroup *d_groups;
    WinBlock *d_blocks;
    unsigned long long *d_key;
    Scratch S;
    S.add(d_boxes, nbox);
    S.add(d_invw, nevent);
    S.add(d_flag, nevent);
    S.add(d_groups, batches.maxg);
    S.add(d_blocks, (size_t)batches.maxb);
    S.add(d_evgroup, batches.maxe);
    S.add(d_key, (size_t)batches.maxp);
    S.add(d_x, (size_t)batches.maxp);
    HIPCHK(S.alloc());
    if (check_events(what, ctx, nbox, tt_dev, nevent, picks_dev, weights_dev, d_boxes, d_invw, d_flag)) return -1;
    if (!cell_dev && !misfit_dev && !t0_dev) return 0;

    return run_batches(ctx, groups, batches, d_groups, d_blocks, d_evgroup, [](const WinGroup &) { return false; },
                       [&](int e0, int ne, int, int nblocks) {
        HIPCHK(launch_locate_window_search(d_boxes, nbox, mx, my, mz, picks_dev, weights_dev, d_invw, d_groups,
                                           d_blocks, nblocks, d_key, d_x, ctx->stream));
        HIPCHK(launch_locate_window_final(d_boxes, nbox, picks_dev, weights_dev, d_invw, e0, ne, d_evgroup, d_groups,
                                          d_key, d_x, cell_dev, misfit_dev, t0_dev, NAN_BITS, ctx->stream));
        return 0;
    });
}

// Windows and sub are host values, so every refusal that concerns them comes before the device is touched.  Groups
// and batches as in ttsweep_locate_window_device, over nodes instead of cells.  A group whose window holds at most
// locate_subcell_stage_floats() floats over all stations is searched by the blocks that stage it in LDS; the two kinds
// of blocks are listed apart and launched one after the other.  The scratch is 16 bytes per event, 64 per group, 8
// per block and 12 per partial of the largest batch: nothing grows with the grid.
int ttsweep_locate_subcell_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev, int nevent,
                                  const double *picks_dev, const double *weights_dev, const int *lo, const int *hi,
                                  int sub, int *node_dev, double *misfit_dev, double *t0_dev)
{
    const char *what = "ttsweep_locate_subcell_device";
    if (check_counts(what, nbox, nevent, tt_dev && picks_dev) || check_window_pair(what, lo, hi)) return -1;
    if (sub < 1 || sub > 64) return set_error("%s: sub %d is outside 1..64", what, sub);
    if (check_window_order(what, nevent, lo, hi) || check_grid(what, ctx)) return -1;
    const int n[3] = {ctx->nx, ctx->ny, ctx->nz};
    if (check_window_inside(what, nevent, lo, hi, n)) return -1;
    for (int a = 0; a < 3; a++)
        if ((long long)(n[a] - 1) * sub > INT_MAX)
            return set_error("%s: the nodes of %d cells at sub %d along axis %d do not fit int32", what, n[a], sub, a);
    if (check_boxes(what, nbox, tt_dev)) return -1;

    const Windows win(lo, hi, n);
    const int tile = locate_subcell_tile_nodes();
    std::vector<SubGroup> groups;
    for (int e = 0; e < nevent;) {
        const int *l = win.lo_of(e), *h = win.hi_of(e);
        SubGroup g;
        g.e0 = e;
        g.ne = win.run(e, nevent);
        long long c[3], w[3];
        for (int a = 0; a < 3; a++) {
            w[a] = h[a] - l[a] + 1;
            c[a] = (w[a] - 1) * sub + 1;                // at most INT_MAX each
            g.lo[a] = l[a];
        }
        if (c[0] * c[1] > INT_MAX || c[0] * c[1] * c[2] > INT_MAX)
            return set_error("%s: event %d has %lld x %lld x %lld nodes, more than fit int32 indices", what, e, c[0],
                             c[1], c[2]);
        g.x0 = (l[0] * n[1] + l[1]) * n[2] + l[2];
        g.wy = (int)w[1];
        g.wz = (int)w[2];
        g.wn = (int)(w[0] * w[1] * w[2]);               // at most ncells
        g.ny = (int)c[1];
        g.nz = (int)c[2];
        g.nnode = (int)(c[0] * c[1] * c[2]);
        g.ntiles = (g.nnode + tile - 1) / tile;
        g.staged = (long long)nbox * g.wn <= locate_subcell_stage_floats();
        g.part = 0;
        groups.push_back(g);
        e += g.ne;
    }
    const Batches batches = cut_batches(groups);
    if (ctx_bind(ctx)) return -1;

    const float **d_boxes;
    double *d_invw;
    int *d_flag, *d_evgroup, *d_x;
    SubGroup *d_groups;
    WinBlock *d_blocks;
    unsigned long long *d_key;
    Scratch S;
    S.add(d_boxes, nbox);
    S.add(d_invw, nevent);
    S.add(d_flag, nevent);
    S.add(d_groups, batches.maxg);
    S.add(d_blocks, (size_t)batches.maxb);
    S.add(d_evgroup, batches.maxe);
    S.add(d_key, (size_t)batches.maxp);
    S.add(d_x, (size_t)batches.maxp);
    HIPCHK(S.alloc());
    if (check_events(what, ctx, nbox, tt_dev, nevent, picks_dev, weights_dev, d_boxes, d_invw, d_flag)) return -1;
    if (!node_dev && !misfit_dev && !t0_dev) return 0;

    const int gnyz = n[1] * n[2], gnz = n[2];
    return run_batches(ctx, groups, batches, d_groups, d_blocks, d_evgroup, [](const SubGroup &G) { return !G.staged; },
                       [&](int e0, int ne, int nstaged, int nblocks) {
        HIPCHK(launch_locate_subcell_search(d_boxes, nbox, gnyz, gnz, sub, picks_dev, weights_dev, d_invw, d_groups,
                                            d_blocks, nstaged, true, d_key, d_x, ctx->stream));
        HIPCHK(launch_locate_subcell_search(d_boxes, nbox, gnyz, gnz, sub, picks_dev, weights_dev, d_invw, d_groups,
                                            d_blocks + nstaged, nblocks - nstaged, false, d_key, d_x, ctx->stream));
        HIPCHK(launch_locate_subcell_final(d_boxes, nbox, gnyz, gnz, sub, picks_dev, weights_dev, d_invw, e0, ne,
                                           d_evgroup, d_groups, d_key, d_x, node_dev, misfit_dev, t0_dev, NAN_BITS,
                                           ctx->stream));
        return 0;
    });
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
    if (check_counts(what, nbox, nevent, tt_dev && picks_dev && misfit_dev && delta_dev && nlevel >= 1 && nlevel <= 4))
        return -1;
    if (check_grid(what, ctx)) return -1;
    const long long ncells = (long long)ctx->nx * ctx->ny * ctx->nz;
    const unsigned long long side = (unsigned long long)std::max({ctx->nx, ctx->ny, ctx->nz});
    if ((unsigned __int128)ncells * side * side >= (unsigned __int128)1 << 63)
        return set_error("%s: the second moments of %d x %d x %d cells could overflow int64", what, ctx->nx, ctx->ny,
                         ctx->nz);
    if (check_boxes(what, nbox, tt_dev) || ctx_bind(ctx)) return -1;

    const int N = (int)ncells;
    const long long n = (long long)nevent * nlevel;
    const float **d_boxes;
    double *d_invw;
    int *d_flag, *d_box;
    unsigned long long *d_limmax, *d_lim, *d_sum, *d_t0;
    Scratch S;
    S.add(d_boxes, nbox);
    S.add(d_invw, nevent);
    S.add(d_flag, 2 * (size_t)nevent);
    S.add(d_limmax, nevent);
    S.add(d_lim, n);
    S.add(d_sum, n * 10);
    S.add(d_t0, n * 2);
    S.add(d_box, n * 6);
    HIPCHK(S.alloc());
    HIPCHK(launch_confidence_check(nevent, nlevel, misfit_dev, delta_dev, d_lim, d_limmax, d_flag + nevent,
                                   ctx->stream));
    auto levels = [&](const int *flag, int e) {
        if (flag[nevent + e] & 1) return set_error("%s: event %d has a NaN or negative misfit level", what, e);
        if (flag[nevent + e] & 2) return set_error("%s: event %d has a NaN or negative delta", what, e);
        return 0;
    };
    if (check_events(what, ctx, nbox, tt_dev, nevent, picks_dev, weights_dev, d_boxes, d_invw, d_flag, 2, levels))
        return -1;

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
