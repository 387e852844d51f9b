// ttsweep_driver.cpp - the driver loop of serial_new/sweep-tt-multistart.c:151-170 without the
// break (:168-169), i.e. old/sweep-serial/sweep-tt-multistart.c:189-211, on device-resident
// boxes.  A solve is four phases (solve_device_body): set up, the one-launch form where there is one, passes of the
// kernel variant in use (enqueued one ahead of the convergence test) for whatever is not at rest by then, finish.
// What the drivers decide from numbers alone is in driver_rules.h and strip_rules.h; here are the HIP calls and the context's bookkeeping.
#include "ttsweep_ctx.h"
#include "driver_rules.h"
#include "strip_rules.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ttsweep {

static int timed_event(ttsweep_ctx *ctx, hipEvent_t *out)
{
    if (ctx->ev_used == ctx->ev_pool.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        ctx->ev_pool.push_back(e);
    }
    *out = ctx->ev_pool[ctx->ev_used++];
    HIPCHK(hipEventRecord(*out, ctx->stream));
    return 0;
}

// Squared radius (cells) of the distance gate for the pass about to be launched.
static float gate_r2(const ttsweep_ctx *ctx)
{
    if (ctx->gate_speed <= 0) return 3.0e38f;       // gate disabled
    const double r = ctx->gate_r0 + ctx->gate_speed * (double)ctx->pass_index;
    return (float)(r * r);
}

// ---- one pass of each kernel variant -----------------------------------------------------

// STRIP: plan_pass_kernel + sweep_units_kernel.  The pass's "changed" words arrive in
// h_changed_slot without a copy command, and d_changed_next is cleared for the pass after this
// one (UnitPassTail).
static int launch_pass_strip(ttsweep_ctx *ctx, int nactive, int nstart, int *d_changed, int *h_changed_slot,
                             int *d_changed_next)
{
    const StripPlan &plan = ctx->plans[ctx->np - 1];
    HIPCHK(launch_plan_pass(ctx->L, ctx->d_starts, ctx->d_worklist, ctx->worklist_len, d_changed,
                            ctx->d_unitq, (int)ctx->unitq_cap, ctx->nlists, ctx->d_unitq_ctrl,
                            plan, gate_r2(ctx), ctx->d_tile_flags, (long long)flag_words(ctx->L, ctx->kernel), ctx->stream));
    UnitPassTail tail;
    tail.active = ctx->d_active;
    tail.nactive = nactive;
    tail.entries = ctx->d_cell_entries;
    tail.nentries = ctx->n_cell_entries;
    tail.max_box_cells = (int)ctx->max_box_cells;
    tail.nstart = nstart;
    tail.changed_host = h_changed_slot;
    tail.changed_next = d_changed_next;
    tail.defer_margin = ctx->defer_suspended ? -3.0e38f : ctx->defer_margin;
    HIPCHK(launch_sweep_units(ctx->L, ctx->d_v, ctx->d_starts, ctx->d_unitq, (int)ctx->unitq_cap,
                              ctx->nlists, ctx->d_unitq_ctrl, ctx->unitq_blocks, d_changed,
                              ctx->d_strip_items[ctx->np - 1], plan, tail, ctx->stream));
    return 0;
}

// The private work sums of the TILE workgroups / the column waves: room for `need` words, zero for the solve to come.
static int zeroed_wgwork(ttsweep_ctx *ctx, size_t need)
{
    if (need > ctx->tile_wgwork_cap) {
        if (ctx->d_tile_wgwork) HIPCHK(hipFree(ctx->d_tile_wgwork));
        ctx->d_tile_wgwork = nullptr;
        ctx->tile_wgwork_cap = 0;
        HIPCHK(hipMalloc((void **)&ctx->d_tile_wgwork, need * sizeof(unsigned long long)));
        ctx->tile_wgwork_cap = need;
    }
    HIPCHK(hipMemsetAsync(ctx->d_tile_wgwork, 0, need * sizeof(unsigned long long), ctx->stream));
    return 0;
}

// TILE: what stays the same for every launch of a solve (filled once per solve).
static int prepare_tile_sweep(ttsweep_ctx *ctx)
{
    TileSweep &P = ctx->tile_sweep;
    P = TileSweep{};
    P.L = ctx->L;
    P.v = ctx->d_v;
    P.starts = ctx->d_starts;
    P.active = ctx->d_active;
    P.NI = tile_count(ctx->L.n[0], TILE_X);
    P.NJ = tile_count(ctx->L.n[1], TILE_Y);
    P.NK = tile_count(ctx->L.n[2], TILE_Z);
    P.R = ctx->tile_R;
    P.nent = ctx->tile_nent;
    P.T0 = ctx->d_T;
    P.state0 = ctx->d_tile_flags;
    P.state_stride = (long long)flag_words(ctx->L, ctx->kernel);
    P.work0 = ctx->d_work;
    P.fz = ctx->tile_fz;
    P.vface = ctx->d_vface;
    P.tface = ctx->d_tface;
    P.face_cells = tile_face_cells(ctx->L, ctx->tile_fz);
    P.sx = P.sy = P.sz = 1;
    P.nblocks = 1;
    for (int e = 0; e < TILE_MAX_ENT; e++) P.ent[e] = ctx->tile_ent[e];
    if (ctx->tile_blocks == 0) {
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, ctx->device));
        // as many single-wavefront workgroups as the device holds at once
#ifdef TTSWEEP_TILE_WGS_PER_CU
        int per_cu = TTSWEEP_TILE_WGS_PER_CU;
#else
        int per_cu = 1;
        HIPCHK(tile_sweep_wgs_per_cu(P, &per_cu));
#endif
        ctx->tile_blocks = per_cu * std::max(prop.multiProcessorCount, 1);
    }
    // the workgroups' private work sums: [tile_blocks][nstart][2], zero between solves
    P.nblocks = ctx->tile_blocks;
    P.nxcd = std::max(ctx->nlists, 1);
    if (ctx->tile_blocks % P.nxcd) P.nxcd = 1;
    P.nstart = ctx->stats.nstart;
    if (zeroed_wgwork(ctx, (size_t)ctx->tile_blocks * (size_t)P.nstart * 2)) return -1;
    P.wgwork = ctx->d_tile_wgwork;
    if (!ctx->d_tile_dmin) HIPCHK(hipMalloc((void **)&ctx->d_tile_dmin, 2 * sizeof(int)));
    if (!ctx->h_tile_dmin) HIPCHK(hipHostMalloc((void **)&ctx->h_tile_dmin, 2 * sizeof(int)));
    ctx->h_tile_dmin[0] = ctx->h_tile_dmin[1] = 0;
    return 0;
}

// TILE: one ordering sweep = the tile hyperplanes in stream order, one launch each (the
// launch finds its due tiles itself: ttsweep_tile.hip, tile_candidate).
static int launch_pass_tile(ttsweep_ctx *ctx, int nactive, int *d_changed)
{
    TileSweep &P = ctx->tile_sweep;
    P.changed = d_changed;
    P.nactive = nactive;
    // the resident grid (no more workgroups than candidates; whole XCD rounds) and the workgroups per XCD that take
    // candidates
    P.nblocks = (int)resident_grid(ctx->tile_blocks, (long long)P.NJ * P.NK * nactive, P.nxcd);
    P.wstride = tile_wstride(P.nblocks / P.nxcd, nactive);
    const int o = ctx->pass_index & 7, on = (ctx->pass_index + 1) & 7;     // the eight orderings in turn
    P.sx = (o & 1) ? -1 : 1;
    P.sy = (o & 2) ? -1 : 1;
    P.sz = (o & 4) ? -1 : 1;
    P.nsx = (on & 1) ? -1 : 1;
    P.nsy = (on & 2) ? -1 : 1;
    P.nsz = (on & 4) ? -1 : 1;
    // Hyperplanes in front of the first one that can hold a due tile are not launched: the
    // previous sweep recorded, for THIS ordering, the earliest hyperplane next to a tile it
    // improved (tile_next_plane; its word is on the host: TILE sweeps are enqueued one at a
    // time, each after the previous one's words have arrived).  The first sweep of a solve
    // starts at 0; a sweep that finds the word untouched has nothing to do at all.
    const int nsteps = P.NI + P.NJ + P.NK - 2;
    const int slot = ctx->pass_index & 1;
    const int first = ctx->pass_index == 0 ? 0 : std::min(ctx->h_tile_dmin[slot ^ 1], nsteps);
    P.dmin_next = ctx->d_tile_dmin + slot;
    HIPCHK(hipMemsetAsync(P.dmin_next, 0x7f, sizeof(int), ctx->stream));
    for (int D = first; D < nsteps; D++) {
        P.D = D;
        P.epoch = ++ctx->tile_epoch;
        HIPCHK(launch_tile_sweep(P, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(ctx->h_tile_dmin + slot, P.dmin_next, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->stats.launches += nsteps - first - 1;
    return 0;
}

// One full-grid pass for the active starts.
static int launch_pass(ttsweep_ctx *ctx, int nactive, int nstart, int *d_changed, int *h_changed_slot,
                       int *d_changed_next)
{
    hipEvent_t e0, e1;
    if (ctx->timing && timed_event(ctx, &e0)) return -1;
    if (ctx->kernel == TTSWEEP_KERNEL_STRIP) {
        if (launch_pass_strip(ctx, nactive, nstart, d_changed, h_changed_slot, d_changed_next)) return -1;
    } else if (ctx->kernel == TTSWEEP_KERNEL_TILE) {
        if (launch_pass_tile(ctx, nactive, d_changed)) return -1;
    } else {
        HIPCHK(launch_sweep_cell(ctx->L, ctx->d_v, ctx->d_starts, ctx->d_active, nactive,
                                 d_changed, ctx->d_cell_entries, ctx->n_cell_entries, ctx->exact_half,
                                 ctx->stream));
    }
    if (ctx->timing && timed_event(ctx, &e1)) return -1;
    ctx->stats.launches++;
    ctx->pass_index++;
    return 0;
}

// STRIP, one launch per solve (AsyncSolve, ttsweep_dev.h): can this solve run that way, and should it?
static bool use_async(ttsweep_ctx *ctx, int nstart)
{
    if (ctx->kernel != TTSWEEP_KERNEL_STRIP || ctx->async_mode == 0) return false;
    if (nstart > ASYNC_MAX_STARTS || strip_units(ctx->L, ctx->np) >= (int)ASYNC_UNIT_SPECIAL) return false;
    // (planners take up to ASYNC_MAX_RINGS workgroups of the resident grid: a device that holds only a handful
    // keeps the pass driver)
    if (ensure_unit_grid(ctx) || ctx->unitq_blocks < 4 * ASYNC_MAX_RINGS) return false;
    // (a ring serves at most ASYNC_RING_STARTS starts, and there are as many rings as XCDs: a device or a partition
    // with fewer XCDs holds fewer starts per launch - the pass driver takes what does not fit)
    const int nrings = std::max(ring_count(nstart, ctx->nlists, ASYNC_MAX_RINGS), 1);
    if (starts_per_ring(nstart, nrings) > ASYNC_RING_STARTS) return false;
    return true;        // (-1: wherever it can run; 1: the same)
}


#ifdef TTSWEEP_DEBUG_ENV
// What the rings and the activity words looked like when the one-launch STRIP solve gave up.
static void dump_async_state(ttsweep_ctx *ctx, const AsyncSolve &as, int nstart, int nunits)
{
    std::vector<unsigned long long> ctl((size_t)ASYNC_MAX_RINGS * ASYNC_CTL_STRIDE);
    (void)hipMemcpy(ctl.data(), ctx->d_async_ctl, ctl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    for (int r = 0; r < as.nrings; r++) {
        const unsigned long long x = ctl[(size_t)r * ASYNC_CTL_STRIDE];
        float g;
        const unsigned gb = (unsigned)ctl[(size_t)r * ASYNC_CTL_STRIDE + 8];
        memcpy(&g, &gb, sizeof g);
        fprintf(stderr, "  ring %d: head %u tail %u done %d completed %u gate_r2 %g | stored by the planner %llu, handed off %llu (reserved %llu), consumed %llu, reserved by the planner %llu (negative %llu)\n", r, (unsigned)x,
                (unsigned)(x >> 32) & 0x7fffffffu, (int)(x >> 63), (unsigned)ctl[(size_t)r * ASYNC_CTL_STRIDE + 16], g,
                ctl[(size_t)r * ASYNC_CTL_STRIDE + 24], ctl[(size_t)r * ASYNC_CTL_STRIDE + 25], ctl[(size_t)r * ASYNC_CTL_STRIDE + 27],
                ctl[(size_t)r * ASYNC_CTL_STRIDE + 26], ctl[(size_t)r * ASYNC_CTL_STRIDE + 28], ctl[(size_t)r * ASYNC_CTL_STRIDE + 29]);
    }
    const size_t fw = flag_words(ctx->L, ctx->kernel);
    const int nflag = ctx->L.n[0] * strip_btiles(ctx->L) * strip_cstrips(ctx->L);
    std::vector<int> fl(fw);
    for (int s = 0; s < nstart; s++) {
        (void)hipMemcpy(fl.data(), ctx->d_tile_flags + (size_t)s * fw, fw * sizeof(int), hipMemcpyDeviceToHost);
        int busy = 0, bits = 0, defer = 0, first_busy = -1, first_bits = -1;
        for (int u = 0; u < nunits; u++) {
            const unsigned w = (unsigned)fl[2 * nflag + u];
            if (w & ASYNC_BUSY) { busy++; if (first_busy < 0) first_busy = u; }
            if (w & ~ASYNC_BUSY) { bits++; if (first_bits < 0) first_bits = u; }
            if (fl[u]) defer++;
        }
        fprintf(stderr, "  start %d: %d units busy (first %d), %d with plane bits (first %d, word %08x), %d with deferred bits\n",
                s, busy, first_busy, bits, first_bits, first_bits >= 0 ? (unsigned)fl[2 * nflag + first_bits] : 0u, defer);
    }
    std::vector<unsigned long long> ent((size_t)(as.cap_mask + 1));
    for (int r = 0; r < as.nrings; r++) {
        (void)hipMemcpy(ent.data(), ctx->d_async_entries + (size_t)r * (as.cap_mask + 1), ent.size() * 8, hipMemcpyDeviceToHost);
        int full = 0;
        for (size_t i = 0; i < ent.size(); i++) {
            const unsigned long long e = ent[i];
            if (e == 0ull) continue;
            full++;
            fprintf(stderr, "  ring %d slot %zu: planes %04x unit %u start %u tag %u valid %d nodefer %d\n", r, i,
                    (unsigned)(e & 0xffffu), (unsigned)((e >> 16) & 0xfffffu), (unsigned)((e >> 36) & 0xffu),
                    (unsigned)((e >> 44) & ASYNC_TAG_MASK), (int)((e >> 62) & 1), (int)(e >> 63));
        }
        fprintf(stderr, "  ring %d: %d slots hold an entry\n", r, full);
    }
}
#endif

static_assert(sizeof(RingListEntry) == sizeof(int4), "a ring list entry is the int4 the kernel reads");

// The whole driver loop as one launch: the rings' lists (driver_rules.h), the ring memory, the launch, its verdict.
// sweeps[s]: whole-grid equivalents of units relaxed for start s (what a pass count is for the
// pass driver).  Returns 1 / 0 (something improved / nothing did), -2 (the launch gave up: the boxes hold valid upper
// bounds, the caller goes on with the pass driver) or < 0.
static int solve_async_strip(ttsweep_ctx *ctx, int nstart, std::vector<int> &sweeps)
{
    const int nunits = strip_units(ctx->L, ctx->np), units1 = strip_units(ctx->L, 1);
    if (ensure_unit_grid(ctx)) return -1;
    const bool lat = use_latency_instance(ctx->np == 1 && ctx->unitq_blocks_lat >= 4 * ASYNC_MAX_RINGS, ctx->async_waves,
                                          STRIP_NS_LAT, ctx->lat_max_units, nstart, units1);
    const StripPlan &plan = lat ? ctx->plan_lat : ctx->plans[ctx->np - 1];
    const StripItem *const d_items = lat ? ctx->d_strip_items_lat : ctx->d_strip_items[ctx->np - 1];
    const int nblocks = lat ? ctx->unitq_blocks_lat : ctx->unitq_blocks;
    AsyncSolve as{};
    as.nrings = ring_count(nstart, ctx->nlists, ASYNC_MAX_RINGS);
    const int cap = 1 << 14;
    as.cap_mask = cap - 1;
    const RingMarks marks = ring_marks(nstart, nunits, as.nrings, nblocks, cap, ctx->async_low, ctx->async_high);
    as.low = marks.low;
    as.high = marks.high;
    as.special_every = ctx->async_special_every;
    as.policy = ctx->async_policy;
    as.gate_r0 = (float)ctx->gate_r0;
    as.gate_speed = ctx->gate_speed > 0 ? ctx->async_gate_speed : 0.f;     // (per start: only for boxes that grow from one unit)
    as.gate_fast = std::max(ctx->async_gate_fast, as.gate_speed);
    as.window = ctx->async_window;
    // (the lists depend on the start cells and the unit grid only: a solve of the same starts keeps them)
    std::vector<long long> key;
    key.reserve(nstart + 2);
    key.push_back(ctx->np);
    key.push_back(as.nrings);
    for (int s = 0; s < nstart; s++) key.push_back(ctx->h_starts[s].sidx);
    const bool cached = key == ctx->async_list_key && ctx->d_async_list;
    RingLists lists;
    if (cached) {
        for (int r = 0; r < ASYNC_MAX_RINGS; r++) { as.ring_off[r] = ctx->async_rings.ring_off[r]; as.ring_len[r] = ctx->async_rings.ring_len[r]; }
        for (int r = 0; r <= ASYNC_MAX_RINGS; r++) as.ring_start_off[r] = ctx->async_rings.ring_start_off[r];
    } else {
        const UnitGrid grid{ctx->np, ctx->L.n[1], strip_btiles(ctx->L), strip_cstrips(ctx->L), STRIP_TB, STRIP_K};
        std::vector<StartCell> at(nstart);
        for (int s = 0; s < nstart; s++) at[s] = {ctx->h_starts[s].sa, ctx->h_starts[s].sb, ctx->h_starts[s].sc};
        if (const char *why = build_ring_lists(nstart, as.nrings, ASYNC_RING_STARTS, nunits, grid, at, ctx->unit_order, lists))
            return set_error("%s", why);
        for (int r = 0; r < as.nrings; r++) { as.ring_off[r] = lists.ring_off[r]; as.ring_len[r] = lists.ring_len[r]; }
        for (int r = 0; r <= as.nrings; r++) as.ring_start_off[r] = lists.ring_start_off[r];
    }
    long long longest = 0;
    for (int r = 0; r < as.nrings; r++) longest = std::max<long long>(longest, as.ring_len[r]);
    as.scan_slack = ring_scan_slack(nstart, as.nrings);
    as.inunit = inunit_passes(ctx->async_inunit, lat, nstart);
    as.handoff = handoff_bits(as.policy, longest, ASYNC_RING_STARTS, cap, ctx->async_handoff, ctx->handoff_max_units,
                              ctx->handoff_default, nstart, units1);
    if (!cached && lists.flat.size() > ctx->async_list_cap) {
        if (ctx->d_async_list) HIPCHK(hipFree(ctx->d_async_list));
        ctx->d_async_list = nullptr;
        ctx->async_list_cap = 0;
        HIPCHK(hipMalloc((void **)&ctx->d_async_list, lists.flat.size() * sizeof(int4)));
        ctx->async_list_cap = lists.flat.size();
    }
    if (!ctx->d_async_ring_starts) HIPCHK(hipMalloc((void **)&ctx->d_async_ring_starts, ASYNC_MAX_STARTS * sizeof(int)));
    if (!ctx->d_async_entries) HIPCHK(hipMalloc((void **)&ctx->d_async_entries, (size_t)ASYNC_MAX_RINGS * cap * sizeof(unsigned long long)));
    if (!ctx->d_async_ctl) HIPCHK(hipMalloc((void **)&ctx->d_async_ctl, (size_t)ASYNC_MAX_RINGS * ASYNC_CTL_STRIDE * sizeof(unsigned long long)));
    if (!ctx->d_async_status) HIPCHK(hipMalloc((void **)&ctx->d_async_status, 8 * sizeof(unsigned)));
    if (!ctx->h_async_status) HIPCHK(hipHostMalloc((void **)&ctx->h_async_status, 8 * sizeof(unsigned)));
    if (!cached) {
        ctx->async_list_key.clear();        // (until the upload below has completed)
        HIPCHK(hipMemcpyAsync(ctx->d_async_list, lists.flat.data(), lists.flat.size() * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->d_async_ring_starts, lists.ring_starts.data(), lists.ring_starts.size() * sizeof(int),
                              hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(hipMemsetAsync(ctx->d_async_entries, 0, (size_t)ASYNC_MAX_RINGS * cap * sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_async_ctl, 0, (size_t)ASYNC_MAX_RINGS * ASYNC_CTL_STRIDE * sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_async_status, 0, 8 * sizeof(unsigned), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_changed, 0, (size_t)nstart * sizeof(int), ctx->stream));
    if (!cached) {
        HIPCHK(hipStreamSynchronize(ctx->stream));  // (`lists` is a stack-lifetime buffer)
        ctx->async_list_key = key;
        ctx->async_rings = as;
    }
    as.list = ctx->d_async_list;
    as.ring_starts = ctx->d_async_ring_starts;
    as.entries = ctx->d_async_entries;
    as.ctl = ctx->d_async_ctl;
    as.status = ctx->d_async_status;
    // (what the solve should take at a tenth of the machine's rate; 1024x1024x512 x 14 with the 818-offset star: 5.6 s
    // measured, limit about 130 s)
    as.timeout_ticks = wait_limit_ticks((double)ctx->relax_per_sweep * (double)nstart * 8.0 / 1.0e12, ctx->async_timeout_ms);
    as.max_entries = ring_max_entries(ctx->max_sweeps, longest);

    UnitPassTail tail{};
    tail.entries = ctx->d_cell_entries;
    tail.nentries = ctx->n_cell_entries;
    tail.max_box_cells = (int)ctx->max_box_cells;
    tail.nstart = nstart;
    tail.defer_margin = ctx->defer_margin;
    hipEvent_t e0, e1;
    if (ctx->timing && timed_event(ctx, &e0)) return -1;
    HIPCHK(launch_solve_units(ctx->L, ctx->d_v, ctx->d_starts, nblocks, ctx->d_changed,
                              d_items, plan, lat ? STRIP_NS_LAT : STRIP_NS, tail, as, ctx->d_tile_flags,
                              (long long)flag_words(ctx->L, ctx->kernel), ctx->stream));
    if (ctx->timing && timed_event(ctx, &e1)) return -1;
    ctx->stats.launches++;
    HIPCHK(hipMemcpyAsync(ctx->h_async_status, ctx->d_async_status, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->h_changed, ctx->d_changed, (size_t)nstart * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->h_work, ctx->d_work, 3 * nstart * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
#ifdef TTSWEEP_ASYNC_STATS
    fprintf(stderr, "one-launch solve: %u units (%u staged planes) relaxed, %u units (%u planes) improved nothing\n",
            ctx->h_async_status[4], ctx->h_async_status[5], ctx->h_async_status[6], ctx->h_async_status[7]);
#endif
    if (ctx->h_async_status[0] == ASYNC_ERR_CAP)
        return set_error("a start did not converge in %lld sweeps", ctx->max_sweeps);
    if (ctx->h_async_status[0] != ASYNC_OK) {
#ifdef TTSWEEP_DEBUG_ENV
        dump_async_state(ctx, as, nstart, nunits);
#endif
        set_error("the one-launch solve gave up (code %u)", ctx->h_async_status[0]);
        return -2;
    }
    bool any = false;
    for (int s = 0; s < nstart; s++) {
        any |= (ctx->h_changed[s] & CHANGED_IMPROVED) != 0;
        sweeps[s] = (int)((ctx->h_work[3 * s + 2] + (unsigned long long)nunits - 1) / (unsigned long long)nunits);
    }
    return any ? 1 : 0;
}

// the caller's FLOATBOX array as a layout without halo (include/floatbox.h:127-129: x * ny * nz + y * nz + z)
static DevLayout user_layout(const DevLayout &L)
{
    DevLayout U = L;
    for (int d = 0; d < 3; d++) { U.lo[d] = 0; U.n[d] = U.p[d] = L.un[d]; U.perm[d] = d; }
    U.s1 = U.p[2];
    U.s0 = (long long)U.p[1] * U.p[2];
    U.cells = U.s0 * U.p[0];
    return U;
}

// TILE, plain 6-neighbour star: can the solve run as ONE launch of column pipelines (ColumnSolve, ttsweep_dev.h)?
static bool use_column(ttsweep_ctx *ctx, int nstart)
{
    if (ctx->kernel != TTSWEEP_KERNEL_TILE || ctx->async_mode == 0) return false;
    if (!tile_star_is_six(ctx->tile_ent, ctx->tile_nent, ctx->tile_R)) return false;
    // (the two z entries have one length - both stand for the same two star entries -: the column kernel carries the
    // z edge of a cell to the next step, where it is the edge back)
    if (ctx->tile_ent[2].h != ctx->tile_ent[3].h) return false;
    const DevLayout &L = ctx->L;
    const int NI = tile_count(L.n[0], TILE_X), NJ = tile_count(L.n[1], TILE_Y), NK = tile_count(L.n[2], TILE_Z);
    if (NK > COL_MAX_NK || NI > 32767 || NJ > 32767 || nstart > 32767) return false;
    if (!column_offsets_fit(L.s0, L.s1)) return false;
    if (ctx->col_blocks == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return false;
        int per_cu = 0;
        if (column_solve_wgs_per_cu(&per_cu) != hipSuccess) return false;
        ctx->col_blocks = per_cu * std::max(prop.multiProcessorCount, 1);
    }
    return ctx->col_blocks >= COL_SEQS;
}

// The whole driver loop as one launch: claim sequences, first state, the launch, its verdict.  sweeps[s]: ordering
// sweeps start s took part in.  Returns 1 / 0 (something improved / nothing did), -2 (a wait inside the launch ran
// into its wall-clock limit: the boxes hold valid upper bounds, the caller goes on with the hyperplane launches) or < 0.
static int solve_column(ttsweep_ctx *ctx, int nstart, bool from_box, float *const *tt_dev, bool in_place, std::vector<int> &sweeps)
{
    const DevLayout &L = ctx->L;
    ColumnSolve &C = ctx->col;
    C = ColumnSolve{};
    C.L = L;
    C.v = ctx->d_v;
    C.nstart = nstart;
    C.NI = tile_count(L.n[0], TILE_X);
    C.NJ = tile_count(L.n[1], TILE_Y);
    C.NK = tile_count(L.n[2], TILE_Z);
    const int ncol = C.NI * C.NJ;
    C.nseq = column_sequences(C.NI, ctx->nlists, COL_SEQS);
    std::vector<int> tab;
    column_sequence_table(C.NI, C.NJ, C.nseq, tab, C.seq_off, C.seq_len);
    if (ctx->col_seq_key[0] != C.NI || ctx->col_seq_key[1] != C.NJ || ctx->col_seq_key[2] != C.nseq || !ctx->d_col_seqtab) {
        if (ctx->d_col_seqtab) HIPCHK(hipFree(ctx->d_col_seqtab));
        ctx->d_col_seqtab = nullptr;
        HIPCHK(hipMalloc((void **)&ctx->d_col_seqtab, tab.size() * sizeof(int)));
        HIPCHK(hipMemcpy(ctx->d_col_seqtab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
        ctx->col_seq_key[0] = C.NI; ctx->col_seq_key[1] = C.NJ; ctx->col_seq_key[2] = C.nseq;
    }
    if (nstart > ctx->col_cap_starts) {
        if (ctx->d_col_prog) HIPCHK(hipFree(ctx->d_col_prog));
        if (ctx->d_col_due) HIPCHK(hipFree(ctx->d_col_due));
        if (ctx->d_col_done) HIPCHK(hipFree(ctx->d_col_done));
        if (ctx->h_col_done) HIPCHK(hipHostFree(ctx->h_col_done));
        ctx->d_col_prog = nullptr; ctx->d_col_due = nullptr; ctx->d_col_done = nullptr;
        ctx->h_col_done = nullptr;
        ctx->col_cap_starts = 0;
        HIPCHK(hipMalloc((void **)&ctx->d_col_prog, (size_t)2 * nstart * ncol * sizeof(unsigned long long)));    // (two buffers, by sweep parity)
        HIPCHK(hipMalloc((void **)&ctx->d_col_due, (size_t)nstart * ncol * sizeof(unsigned)));
        HIPCHK(hipMalloc((void **)&ctx->d_col_done, (size_t)nstart * sizeof(int)));
        HIPCHK(hipHostMalloc((void **)&ctx->h_col_done, (size_t)nstart * sizeof(int)));
        ctx->col_cap_starts = nstart;
    }
    if (nstart > ctx->col_cap_tptr) {
        if (ctx->d_col_tptr) HIPCHK(hipFree(ctx->d_col_tptr));
        if (ctx->h_col_tptr) HIPCHK(hipHostFree(ctx->h_col_tptr));
        if (ctx->d_col_ordseq) HIPCHK(hipFree(ctx->d_col_ordseq));
        if (ctx->h_col_ordseq) HIPCHK(hipHostFree(ctx->h_col_ordseq));
        if (ctx->d_col_line) HIPCHK(hipFree(ctx->d_col_line));
        if (ctx->h_col_line) HIPCHK(hipHostFree(ctx->h_col_line));
        ctx->d_col_line = nullptr; ctx->h_col_line = nullptr;
        ctx->d_col_tptr = nullptr; ctx->h_col_tptr = nullptr;
        ctx->d_col_ordseq = nullptr; ctx->h_col_ordseq = nullptr;
        ctx->col_cap_tptr = 0;
        HIPCHK(hipMalloc((void **)&ctx->d_col_tptr, (size_t)nstart * sizeof(float *)));
        HIPCHK(hipHostMalloc((void **)&ctx->h_col_tptr, (size_t)nstart * sizeof(float *)));
        HIPCHK(hipMalloc((void **)&ctx->d_col_ordseq, (size_t)nstart * sizeof(unsigned long long)));
        HIPCHK(hipHostMalloc((void **)&ctx->h_col_ordseq, (size_t)nstart * sizeof(unsigned long long)));
        HIPCHK(hipMalloc((void **)&ctx->d_col_line, (size_t)nstart * 3 * sizeof(float)));
        HIPCHK(hipHostMalloc((void **)&ctx->h_col_line, (size_t)nstart * 3 * sizeof(float)));
        ctx->col_cap_tptr = nstart;
    }
    for (int s = 0; s < nstart; s++) ctx->h_col_tptr[s] = in_place ? tt_dev[s] : ctx->d_T + (size_t)s * L.cells;
    HIPCHK(hipMemcpyAsync(ctx->d_col_tptr, ctx->h_col_tptr, (size_t)nstart * sizeof(float *), hipMemcpyHostToDevice, ctx->stream));
    C.tptr = ctx->d_col_tptr;
    C.ts0 = in_place ? (long long)L.n[1] * L.n[2] : L.s0;
    C.ts1 = in_place ? (long long)L.n[2] : L.s1;
    C.tpad = in_place ? 0 : 1;
    C.tlo = in_place ? 0 : L.lo[2];
    if (!ctx->d_col_claim) HIPCHK(hipMalloc((void **)&ctx->d_col_claim, COL_SEQS * 16 * sizeof(unsigned long long)));
    if (!ctx->d_col_status) HIPCHK(hipMalloc((void **)&ctx->d_col_status, 8 * sizeof(unsigned)));
    if (!ctx->h_col_status) HIPCHK(hipHostMalloc((void **)&ctx->h_col_status, 8 * sizeof(unsigned)));
    // the resident grid: no more workgroups than a sweep has columns (a workgroup that finds nothing to do waits
    // inside a later sweep), whole rounds of the sequences
    const int wgw = column_solve_wg_waves();
    const long long blocks = resident_grid(ctx->col_blocks, ((long long)ncol * nstart + wgw - 1) / wgw, C.nseq);
    if (zeroed_wgwork(ctx, (size_t)blocks * wgw * (size_t)nstart * 2)) return -1;
    C.seqtab = ctx->d_col_seqtab;
    C.prog = ctx->d_col_prog;
    C.due = ctx->d_col_due;
    C.done = ctx->d_col_done;
    C.claim = ctx->d_col_claim;
    C.status = ctx->d_col_status;
    C.wgwork = ctx->d_tile_wgwork;
    C.changed = ctx->d_changed;
    for (int e = 0; e < 6; e++) C.h[e] = ctx->tile_ent[e].h;        // (tile_star_is_six: x-, y-, z-, z+, y+, x+)
    C.max_sweeps = (int)std::min<long long>(ctx->max_sweeps, COL_MAX_SWEEPS - 2);
    if (ctx->col_order < 0) {       // the default: chosen per start from the velocity profile of its vertical line
        HIPCHK(launch_column_line(ctx->d_v, L, ctx->d_starts, nstart, ctx->d_col_line, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->h_col_line, ctx->d_col_line, (size_t)nstart * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    for (int s = 0; s < nstart; s++) {
        const StartDesc &sd = ctx->h_starts[s];
        const int at[3] = {sd.sa, sd.sb, sd.sc}, nn[3] = {L.n[0], L.n[1], L.n[2]};
        const int which = ctx->col_order >= 0 ? ctx->col_order
                        : column_order_default(nn, ctx->h_col_line[3 * s], ctx->h_col_line[3 * s + 1], ctx->h_col_line[3 * s + 2]);
        column_order_sequence(which, nn, at, &ctx->h_col_ordseq[s]);
#ifdef TTSWEEP_DEBUG_ENV
        if (const char *q = getenv("TTSWEEP_COL_ORDSEQ")) ctx->h_col_ordseq[s] = strtoull(q, nullptr, 16);   // (sweep 1: the lowest nibble)
#endif
    }
    HIPCHK(hipMemcpyAsync(ctx->d_col_ordseq, ctx->h_col_ordseq, (size_t)nstart * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    C.ordseq = ctx->d_col_ordseq;
    // (what forty sweep equivalents should take at a quarter of the memory rate)
    C.timeout_ticks = wait_limit_ticks((double)L.n[0] * L.n[1] * L.n[2] * (double)nstart * 12.0 * 40.0 / 2.0e12, ctx->async_timeout_ms);

    HIPCHK(launch_column_init(C, ctx->d_starts, from_box, ctx->stream));
    hipEvent_t e0, e1;
    if (ctx->timing && timed_event(ctx, &e0)) return -1;
    {   // (a launch that the device refuses - e.g. the LDS opt-in - leaves the boxes untouched: the hyperplane driver runs)
        const hipError_t le = launch_column_solve(C, (int)blocks, ctx->stream);
        if (le != hipSuccess) {
            (void)hipGetLastError();
            set_error("the column launch failed (%s)", hipGetErrorString(le));
            return -2;
        }
    }
    if (ctx->timing && timed_event(ctx, &e1)) return -1;
    ctx->stats.launches++;
    HIPCHK(hipMemcpyAsync(ctx->h_col_status, ctx->d_col_status, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->h_col_done, ctx->d_col_done, (size_t)nstart * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->h_changed, ctx->d_changed, (size_t)nstart * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->h_col_status[0] == COL_ERR_CAP) {
        // (the launch counts sweeps in COL_MAX_SWEEPS slots: a caller's cap beyond that is the hyperplane driver's to
        // honour - it takes over from the boxes as they are)
        if (ctx->max_sweeps > (long long)C.max_sweeps) {
            set_error("the one-launch solve ran out of sweep slots (%d)", C.max_sweeps);
            return -2;
        }
        return set_error("a start did not converge in %lld sweeps", ctx->max_sweeps);
    }
    if (ctx->h_col_status[0] != COL_DONE) {
        set_error("the one-launch solve gave up (code %u)", ctx->h_col_status[0]);
        return -2;
    }
    bool any = false;
    for (int s = 0; s < nstart; s++) {
        any |= (ctx->h_changed[s] & CHANGED_IMPROVED) != 0;
        sweeps[s] = ctx->h_col_done[s];
    }
    ctx->tile_blocks_used = (int)blocks * wgw;
    return any ? 1 : 0;
}

// ---- a solve, phase by phase ---------------------------------------------------------------------------------------

// The solve in progress: what set_up chose, what the drivers found, and the pass driver's pipeline.
struct Solve {
    int nstart;
    const ttsweep_start *starts;
    float *const *tt_dev;
    bool init;                  // fresh boxes (else: boxes that arrive with values in them)
    // chosen by set_up, fixed from there on
    bool column = false;        // TILE: the column launch runs first
    bool async = false;         // STRIP: the one-launch solve runs first
    bool in_place = false;      // column driver: the caller's arrays ARE the volumes (until it falls back)
    bool batched = false;       // STRIP: fresh boxes are initialised in one launch for all starts
    bool in_step = false;       // STRIP: the caller's boxes equal the padded volumes at the launch (StartDesc::U)
    // found on the way
    bool one_launch_at_rest = false;    // the one-launch STRIP solve ran to rest
    bool fell_back = false;             // the one-launch form gave up: the other driver finishes the solve
    bool anychange_ever = false;
    std::vector<int> sweeps;
    // the pass driver
    std::vector<char> done;                 // converged: the pass launched one ahead for it is not counted
    std::vector<int> snapshot[PASS_SLOTS];  // active starts of each pass in flight
    int nactive = 0, launched = 0, processed = 0;
    int depth = 2;                          // passes in flight, at most
    bool trace = false;
    unsigned long long trace_prev = 0, trace_prev_un = 0;
    std::chrono::steady_clock::time_point t_pass;
};

// Set up: unit size, driver and copy strategy; the starts' descriptors; the boxes initialised (batched or start by
// start, in the caller's arrays or in the padded volumes) or packed; unit orders; uploads.
static int set_up(ttsweep_ctx *ctx, Solve &S)
{
    const DevLayout &L = ctx->L;
    const int nstart = S.nstart;
    const bool strip = ctx->kernel == TTSWEEP_KERNEL_STRIP;
    const int np = use_plane_pairs(ctx->pair_min_starts, ctx->pair_min_units, ctx->async_mode != 0, nstart, strip_units(L, 1))
        ? STRIP_PLANES : 1;
    if (np != ctx->np) ctx->unit_order_key.assign(ctx->unit_order_key.size(), -1);     // orders belong to the other unit grid
    ctx->np = np;
    S.column = use_column(ctx, nstart);
    S.in_place = S.column && !ctx->col_in_place_off && column_rows_in_place(L.n[1], L.n[2], TILE_Z, S.tt_dev, nstart);
    S.batched = S.init && strip && L.cells % 4 == 0 && nstart <= 65535;
    S.in_step = user_boxes_in_step(strip, L.perm[1] == 2, S.init, S.batched, S.tt_dev, nstart);

    for (int s = 0; s < nstart; s++) {
        const int u[3] = {S.starts[s].i, S.starts[s].j, S.starts[s].k};
        StartDesc &sd = ctx->h_starts[s];
        sd.T = ctx->d_T + (size_t)s * L.cells;
        sd.U = S.in_step ? S.tt_dev[s] : nullptr;
        sd.sa = u[L.perm[0]];
        sd.sb = u[L.perm[1]];
        sd.sc = u[L.perm[2]];
        sd.sidx = dev_index(L, sd.sa, sd.sb, sd.sc);
        sd.pad_ = 0;
        fill_special_box(ctx, sd);
        {
            long long vol = 1;
            for (int d = 0; d < 3; d++) vol *= std::max(sd.box_hi[d] - sd.box_lo[d] + 1, 0);
            ctx->max_box_cells = std::max<long long>(s == 0 ? 0 : ctx->max_box_cells, vol);
        }
        sd.tile_flags = ctx->d_tile_flags + (size_t)s * flag_words(L, ctx->kernel);
        sd.work = ctx->d_work + 3 * s;
        ctx->h_active[s] = s;
        if (S.batched) continue;        // (initialised further down, all starts in one launch)
        if (S.in_place) {
            // (a fresh box is initialised where it lies: the reference's state, serial_new/...:139-144)
            if (S.init) HIPCHK(launch_init_tt(user_layout(L), S.tt_dev[s],
                                              ((long long)S.starts[s].i * L.un[1] + S.starts[s].j) * L.un[2] + S.starts[s].k, ctx->stream));
        } else if (S.init) HIPCHK(launch_init_tt(L, sd.T, sd.sidx, ctx->stream));
        else HIPCHK(launch_pack(L, S.tt_dev[s], sd.T, INFINITY, ctx->stream));
        if (strip) HIPCHK(launch_init_tile_flags(L, sd, /*from_box=*/!S.init, ctx->plans[np - 1].ra, np, ctx->stream));
        if (ctx->kernel == TTSWEEP_KERNEL_TILE && !S.column) {
            HIPCHK(launch_init_tile_state(L, sd, /*from_box=*/!S.init, ctx->stream));
            float *const faces = ctx->d_tface + (size_t)s * tile_face_cells(L, ctx->tile_fz);
            if (S.init) HIPCHK(launch_init_tile_faces(L, faces, ctx->tile_fz, sd.sa, sd.sb, sd.sc, ctx->stream));
            else HIPCHK(launch_build_tile_faces(L, sd.T, faces, ctx->tile_fz, ctx->stream));
        }
    }
    if (strip) {
        // host work while the device initialises the boxes: every start's units, nearest
        // first (kept from the previous solve when the start point is the same)
        if ((int)ctx->unit_order.size() < nstart) {
            ctx->unit_order.resize(nstart);
            ctx->unit_order_key.resize(nstart, -1);
        }
        for (int s = 0; s < nstart; s++) {
            const StartDesc &sd = ctx->h_starts[s];
            if (ctx->unit_order_key[s] == sd.sidx && !ctx->unit_order[s].empty()) continue;
            order_units(ctx, sd, ctx->unit_order[s]);
            ctx->unit_order_key[s] = sd.sidx;
        }
    }
    HIPCHK(hipMemcpyAsync(ctx->d_starts, ctx->h_starts, nstart * sizeof(StartDesc),
                          hipMemcpyHostToDevice, ctx->stream));
    if (S.batched) {    // (the padded volumes and, where StartDesc::U is set, the caller's boxes)
        HIPCHK(launch_init_tt_batch(L, ctx->d_T, ctx->d_starts, nstart, ctx->stream));
        HIPCHK(launch_init_tile_flags_batch(L, ctx->d_tile_flags, (long long)flag_words(L, ctx->kernel), ctx->d_starts, nstart,
                                            ctx->plans[np - 1].ra, np, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(ctx->d_active, ctx->h_active, nstart * sizeof(int),
                          hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_work, 0, 3 * nstart * sizeof(unsigned long long), ctx->stream));
    ctx->pass_index = 0;
    ctx->defer_suspended = false;
    ctx->tile_epoch = 1;
    if (ctx->kernel == TTSWEEP_KERNEL_TILE && !S.column && prepare_tile_sweep(ctx)) return -1;
    S.async = use_async(ctx, nstart);
    if (strip && !S.async) {
        if (build_worklist(ctx, nstart)) return -1;
        // the passes keep these cleared themselves from here on
        HIPCHK(hipMemsetAsync(ctx->d_changed, 0, (size_t)PASS_SLOTS * nstart * sizeof(int), ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->d_unitq_ctrl, 0, (UNITQ_CTRL_WORDS + 1) * sizeof(int), ctx->stream));
    }
    S.sweeps.assign(nstart, 0);
    S.done.assign(nstart, 0);
    ctx->batch_changed.assign(nstart, 0);
    S.nactive = nstart;
    // (TILE: a sweep is milliseconds long and the host decides where the next one starts from
    // what this one recorded, so sweeps are enqueued one at a time; STRIP / CELL: one ahead)
    S.depth = ctx->kernel == TTSWEEP_KERNEL_TILE ? 1 : 2;
#ifdef TTSWEEP_DEBUG_ENV
    S.trace = getenv("TTSWEEP_TRACE") != nullptr;
#endif
    S.t_pass = std::chrono::steady_clock::now();
    ctx->tile_blocks_used = ctx->tile_blocks;
    return 0;
}

// A one-launch form gave up (rc -2), mostly because a wait inside the launch ran into its wall-clock limit.  Every
// travel time in the boxes is the length of a real path, so the other driver takes over from there.
// STRIP, the pass driver: activity words as for boxes that arrive with values in them, then passes until nothing changes.
// TILE, the hyperplane launches: the padded volumes (packed now, if the columns ran in the caller's arrays - the boxes
// go back there at the end), every tile due.
static int hand_over(ttsweep_ctx *ctx, Solve &S)
{
    const DevLayout &L = ctx->L;
    for (int s = 0; s < S.nstart; s++) {
        const StartDesc &sd = ctx->h_starts[s];
        if (S.async) {
            HIPCHK(launch_init_tile_flags(L, sd, /*from_box=*/true, ctx->plans[ctx->np - 1].ra, ctx->np, ctx->stream));
        } else {
            if (S.in_place) HIPCHK(launch_pack(L, S.tt_dev[s], sd.T, INFINITY, ctx->stream));
            HIPCHK(launch_init_tile_state(L, sd, /*from_box=*/true, ctx->stream));
            HIPCHK(launch_build_tile_faces(L, sd.T, ctx->d_tface + (size_t)s * tile_face_cells(L, ctx->tile_fz),
                                           ctx->tile_fz, ctx->stream));
        }
    }
    if (S.async) {
        if (build_worklist(ctx, S.nstart)) return -1;
        HIPCHK(hipMemsetAsync(ctx->d_changed, 0, (size_t)PASS_SLOTS * S.nstart * sizeof(int), ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->d_unitq_ctrl, 0, (UNITQ_CTRL_WORDS + 1) * sizeof(int), ctx->stream));
    } else {
        if (prepare_tile_sweep(ctx)) return -1;
        ctx->tile_blocks_used = ctx->tile_blocks;
    }
    S.sweeps.assign(S.nstart, 0);
    S.anychange_ever = true;
    S.fell_back = true;
    return 0;
}

// One launch: the column pipelines (TILE) or the rings (STRIP), where set_up chose one.  At rest afterwards, there is
// nothing left for the passes; after a give-up, everything.
static int one_launch(ttsweep_ctx *ctx, Solve &S)
{
    if (!S.column && !S.async) return 0;
    if (S.column) HIPCHK(hipMemsetAsync(ctx->d_changed, 0, (size_t)S.nstart * sizeof(int), ctx->stream));
    const int rc = S.column ? solve_column(ctx, S.nstart, /*from_box=*/!S.init, S.tt_dev, S.in_place, S.sweeps)
                            : solve_async_strip(ctx, S.nstart, S.sweeps);
    if (rc == -2) {
        if (hand_over(ctx, S)) return -1;
    } else {
        if (rc < 0) return rc;
        S.anychange_ever = rc > 0;
        S.nactive = 0;
        S.one_launch_at_rest = S.async;
    }
    // (also when the launch gave up: what it had improved by then stays improved)
    for (int s = 0; s < S.nstart; s++) ctx->batch_changed[s] |= (ctx->h_changed[s] & CHANGED_IMPROVED) != 0;
    return 0;
}

// Passes, enqueue: the next pass for the active starts, and the event that says its "changed" words are on the host.
static int enqueue_pass(ttsweep_ctx *ctx, Solve &S)
{
    const int nstart = S.nstart, slot = S.launched % PASS_SLOTS;
    int *dch = ctx->d_changed + (size_t)slot * nstart;
    int *hch_slot = ctx->h_changed + (size_t)slot * nstart;
    const bool strip = ctx->kernel == TTSWEEP_KERNEL_STRIP;
    if (!strip) HIPCHK(hipMemsetAsync(dch, 0, nstart * sizeof(int), ctx->stream));
    const auto t_enq = std::chrono::steady_clock::now();
    if (launch_pass(ctx, S.nactive, nstart, dch, hch_slot,
                    ctx->d_changed + (size_t)((S.launched + 1) % PASS_SLOTS) * nstart))
        return -1;
    if (S.trace)
        fprintf(stderr, "   (host: %.0f us to enqueue pass %d)\n",
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enq).count(),
                S.launched + 1);
    if (!strip)
        HIPCHK(hipMemcpyAsync(hch_slot, dch, nstart * sizeof(int), hipMemcpyDeviceToHost,
                              ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev_flags[slot], ctx->stream));
    S.snapshot[slot].assign(ctx->h_active, ctx->h_active + S.nactive);
    S.launched++;
    return 0;
}

// TTSWEEP_TRACE=1: per-pass activity on stderr (serialises the passes)
static int trace_pass(ttsweep_ctx *ctx, Solve &S, int slot)
{
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(ctx->h_work, ctx->d_work, 3 * S.nstart * sizeof(unsigned long long),
                     hipMemcpyDeviceToHost));
    unsigned long long tot = 0, un = 0;
    for (int s = 0; s < S.nstart; s++) { tot += ctx->h_work[3 * s]; un += ctx->h_work[3 * s + 2]; }
    const double us = std::chrono::duration<double, std::micro>(
                          std::chrono::steady_clock::now() - S.t_pass).count();
    S.t_pass = std::chrono::steady_clock::now();
    fprintf(stderr, "ttsweep pass %d: %d active starts, %.3f full-sweep equivalents relaxed, "
            "%llu units, %.0f us\n", S.processed + 1, (int)S.snapshot[slot].size(),
            (double)(tot - S.trace_prev) / (double)ctx->stats.cells
                / (double)std::max<size_t>(ctx->pull.size(), 1),
            un - S.trace_prev_un, us);
    S.trace_prev = tot;
    S.trace_prev_un = un;
    return 0;
}

// Passes, examine: wait for the words of the oldest pass in flight; a start whose words show no change is converged
// and leaves the active list.
static int examine_oldest_pass(ttsweep_ctx *ctx, Solve &S)
{
    const int slot = S.processed % PASS_SLOTS;
    HIPCHK(hipEventSynchronize(ctx->ev_flags[slot]));
    const int *hch = ctx->h_changed + (size_t)slot * S.nstart;
    if (S.trace && trace_pass(ctx, S, slot)) return -1;
    bool dropped = false;
    for (int s : S.snapshot[slot]) {
        if (S.done[s]) continue;
        S.sweeps[s]++;
        if (hch[s]) {           // improved, or units still held back by the gate
            if (hch[s] & CHANGED_IMPROVED) { S.anychange_ever = true; ctx->batch_changed[s] = 1; }
            if (S.sweeps[s] >= ctx->max_sweeps)
                return set_error("start %d did not converge in %lld sweeps", s, ctx->max_sweeps);
        } else {
            // converged: remove it from the active list
            S.done[s] = 1;
            int *end = std::remove(ctx->h_active, ctx->h_active + S.nactive, s);
            if (end != ctx->h_active + S.nactive) dropped = true;
            S.nactive = (int)(end - ctx->h_active);
        }
    }
    S.processed++;
    if (dropped && S.nactive > 0) {
        // (the uploads are stream-ordered behind the pass in flight; the stream is
        // synchronised before h_active is touched again)
        HIPCHK(hipMemcpyAsync(ctx->d_active, ctx->h_active, S.nactive * sizeof(int),
                              hipMemcpyHostToDevice, ctx->stream));
        if (ctx->kernel == TTSWEEP_KERNEL_STRIP) {
            if (build_worklist(ctx, S.nactive)) return -1;
        } else {
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
    }
    return 0;
}

// STRIP pass driver, every start at rest: the bits that were deferred (push_improved: units behind the front) become
// due now, and the starts that had any are active again (S.nactive; 0: the solve is over).
static int flush_deferred(ttsweep_ctx *ctx, Solve &S)
{
    if (ctx->kernel != TTSWEEP_KERNEL_STRIP || S.one_launch_at_rest || ctx->defer_margin < -1.0e30f) return 0;
    const int nstart = S.nstart;
    for (int s = 0; s < nstart; s++) ctx->h_active[s] = s;
    int *const dfl = ctx->d_changed + (size_t)PASS_SLOTS * nstart, *const hfl = ctx->h_changed + (size_t)PASS_SLOTS * nstart;
    HIPCHK(hipMemcpyAsync(ctx->d_active, ctx->h_active, nstart * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(dfl, 0, nstart * sizeof(int), ctx->stream));
    HIPCHK(launch_flush_deferred(ctx->L, ctx->np, ctx->d_tile_flags, (long long)flag_words(ctx->L, ctx->kernel), ctx->d_active,
                                 nstart, dfl, ctx->stream));
    HIPCHK(hipMemcpyAsync(hfl, dfl, nstart * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < nstart; s++)
        if (hfl[s]) { ctx->h_active[S.nactive++] = s; S.done[s] = 0; }
    if (S.nactive == 0) return 0;
    ctx->defer_suspended = true;        // (one flush per solve: from here on every unit is told at once)
    HIPCHK(hipMemcpyAsync(ctx->d_active, ctx->h_active, S.nactive * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (build_worklist(ctx, S.nactive)) return -1;
    return 0;
}

// Passes: serial_new/...:151-170 without the break (:168-169).  Passes are enqueued ONE AHEAD of the convergence
// test: pass k+1 is already running while the host waits for the "changed" words of pass k, so the GPU never idles
// between passes.  A start whose pass-k words show no change is converged; the pass k+1 that was launched
// speculatively for it finds all its units inactive.
static int run_passes(ttsweep_ctx *ctx, Solve &S)
{
    for (;;) {
        if (S.processed == S.launched && S.nactive == 0) {      // everything is at rest
            if (flush_deferred(ctx, S)) return -1;
            if (S.nactive == 0) return 0;
        }
        if (S.nactive > 0 && S.launched - S.processed < S.depth) {
            if (enqueue_pass(ctx, S)) return -1;
            if (S.launched - S.processed < S.depth && S.nactive > 0 && S.launched == 1) continue;   // prime the pipeline
        }
        if (examine_oldest_pass(ctx, S)) return -1;
    }
}

// Finish: the boxes back in the caller's arrays (nothing to do / the dead-edge cells only / all boxes in one launch /
// box by box), the work sums, the events, the statistics.
static int finish(ttsweep_ctx *ctx, Solve &S)
{
    const DevLayout &L = ctx->L;
    const int nstart = S.nstart;
    if (S.in_place && !S.fell_back) {
        // (the travel times were relaxed in the caller's arrays)
    } else if (unpack_can_be_skipped(S.in_step, S.one_launch_at_rest, S.fell_back)) {
        // (STRIP, one launch per solve: every store of a unit went into the caller's boxes as well; the few dead-edge
        // cells are copied)
        if (ctx->max_box_cells > 0) HIPCHK(launch_unpack_boxes(L, ctx->d_starts, nstart, ctx->stream));
    } else if (ctx->kernel == TTSWEEP_KERNEL_STRIP && nstart <= 65535 && nstart > 1) {
        // (all boxes in one launch; the boxes' addresses go through the pinned copy of the "changed" words,
        // which the driver loop is done with: PASS_SLOTS + 1 ints per start hold a pointer per start)
        float **const hp = reinterpret_cast<float **>(ctx->h_changed);
        float **const dp = reinterpret_cast<float **>(ctx->d_changed);
        for (int s = 0; s < nstart; s++) hp[s] = S.tt_dev[s];
        HIPCHK(hipMemcpyAsync(dp, hp, nstart * sizeof(float *), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(launch_unpack_batch(L, ctx->d_T, dp, nstart, ctx->stream));
    } else {
        for (int s = 0; s < nstart; s++)
            HIPCHK(launch_unpack(L, ctx->h_starts[s].T, S.tt_dev[s], ctx->stream));
    }
    if (ctx->kernel == TTSWEEP_KERNEL_TILE)
        HIPCHK(launch_tile_reduce_work(ctx->d_tile_wgwork, ctx->tile_blocks_used, nstart, ctx->d_work, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->h_work, ctx->d_work, 3 * nstart * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev_solve1, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));

#ifdef TTSWEEP_PROFILE
    prof_dump();
#endif
#ifdef TTSWEEP_TILE_PROFILE
    if (ctx->kernel == TTSWEEP_KERNEL_TILE) tile_prof_dump();
#endif
#ifdef TTSWEEP_COL_TRACE
    if (ctx->kernel == TTSWEEP_KERNEL_TILE) column_trace_dump();
#endif
#ifdef TTSWEEP_COL_PROFILE
    if (ctx->kernel == TTSWEEP_KERNEL_TILE) column_prof_dump();
#endif
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_solve0, ctx->ev_solve1));
    ctx->stats.solve_ms = ms;
    for (size_t e = 0; e + 1 < ctx->ev_used; e += 2) {
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev_pool[e], ctx->ev_pool[e + 1]));
        ctx->stats.sweep_kernel_ms += ms;
    }
    for (int s = 0; s < nstart; s++) {
        ctx->stats.sweeps_total += S.sweeps[s];
        ctx->stats.sweeps_max = std::max(ctx->stats.sweeps_max, S.sweeps[s]);
        // CELL kernel relaxes every cell in every pass; STRIP counts its active tiles
        // (STRIP counts cells x offsets actually relaxed; convert to whole-star cell relaxations)
        ctx->stats.cells_relaxed += ctx->kernel != TTSWEEP_KERNEL_CELL
            ? (long long)(ctx->h_work[3 * s] / std::max<size_t>(ctx->pull.size(), 1))
            : (long long)S.sweeps[s] * ctx->stats.cells;
    }
    if (S.fell_back) {
        ctx->stats.fallbacks++;
        set_error("%s", "");    // (the solve succeeded: the one-launch form's complaint is not an error of this call)
    }
    return 0;
}

int solve_device_body(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                             float *const *tt_dev, int init)
{
    HIPCHK(hipEventRecord(ctx->ev_solve0, ctx->stream));
    Solve S{nstart, starts, tt_dev, init != 0};
    if (set_up(ctx, S)) return -1;
    if (const int rc = one_launch(ctx, S)) return rc;
    if (run_passes(ctx, S)) return -1;
    if (finish(ctx, S)) return -1;
    return S.anychange_ever ? 1 : 0;
}

} // namespace ttsweep
