// ttsweep_kernels.h - launchers of the HIP kernels (ttsweep_kernels.hip).
#pragma once

#include "ttsweep_dev.h"

namespace ttsweep {

// ---- layout conversion / initialisation -----------------------------------
// user FLOATBOX array -> padded device volume; halo cells get `halo_value`.
hipError_t launch_pack(const DevLayout &L, const float *user, float *padded,
                       float halo_value, hipStream_t st);
// padded device volume -> user FLOATBOX array (interior only).
hipError_t launch_unpack(const DevLayout &L, const float *padded, float *user,
                         hipStream_t st);
// reference initial state: everything +INFINITY, the start cell 0
// (serial_new/sweep-tt-multistart.c:139-144).
hipError_t launch_init_tt(const DevLayout &L, float *padded, long long sidx,
                          hipStream_t st);

// the same for all starts of a solve in one launch each: volume s at T0 + s * L.cells (L.cells % 4 == 0), start
// cell starts[s].sidx; users[s] = device address of box s (a device array)
hipError_t launch_init_tt_batch(const DevLayout &L, float *T0, const StartDesc *starts, int nstart, hipStream_t st);
hipError_t launch_unpack_batch(const DevLayout &L, const float *padded0, float *const *users, int nstart, hipStream_t st);
// the cells of every start's dead-edge box, padded volume -> the caller's box starts[s].U (where it is set)
hipError_t launch_unpack_boxes(const DevLayout &L, const StartDesc *starts, int nstart, hipStream_t st);

// ---- device census / input check -------------------------------------------
// *seen |= 1 << (XCD id) for every workgroup of an `nblocks`-workgroup launch
hipError_t launch_xcc_census(unsigned *seen, int nblocks, hipStream_t st);
// *bad += cells of the caller's n-cell velocity volume that are negative, not finite, or
// positive but below `tiny` or finite and >= `huge` (bad[1]; bad[0]: negative, infinite, NaN)
hipError_t launch_count_bad_velocity(const float *v, long long n, float tiny, float huge, unsigned long long *bad,
                                     hipStream_t st);

// ---- sweep, variant CELL ---------------------------------------------------
// One chaotic in-place pull pass over the whole grid for the `nactive` starts
// listed in `active`; changed[s] is OR-ed with 1 when any cell of start s
// improved.  exact: delays rounded as the reference rounds them - product first, then halved - for velocity
// volumes whose products can be denormal numbers or overflow, and for stars with a length whose half is not a
// float (ttsweep_set_velocity decides).
hipError_t launch_sweep_cell(const DevLayout &L, const float *v, const StartDesc *starts,
                             const int *active, int nactive, int *changed,
                             const CellEntry *entries, int nentries, bool exact, hipStream_t st);

// ---- validator: counts[0] += (cell, forward entry) pairs a reference sweep would still
// store through, counts[1] += cells still at +INFINITY, counts[2] += cells whose travel
// time no live edge can have produced (T is one padded volume)
hipError_t launch_validate(const DevLayout &L, const float *v, const float *T, long long sidx,
                           const FwdEntry *entries, int nentries, const CellEntry *cell_entries,
                           int ncell_entries, unsigned long long *counts, bool exact, hipStream_t st);

// ---- sweep, variant STRIP --------------------------------------------------
// Same contract as launch_sweep_cell, but cells inside a start's dead-edge box
// (StartDesc::box_*) are left untouched by the unit relaxation; the same kernel relaxes
// exactly those cells with the full liveness rule (one wave per cell).
//
// A pass = launch_plan_pass + launch_sweep_units, nothing else: the last workgroup of
// sweep_units hands the "changed" words to the host and clears the counters (ctrl: the
// UNITQ_CTRL_WORDS queue words + one "workgroups done" word, all zero before the first
// pass) and the next pass's "changed" words.
// plan_pass: one thread per entry of the static work list `work`: work[i] = (start index,
// unit id = (A*btiles + bt)*cstrips + cs) or unit id < 0 for padding; entry i belongs to
// XCD i % nlists.  A unit is due when its pend word holds staged-plane bits (pushed by the
// units that improved those planes: push_improved) and the distance gate has reached it; due
// units are appended as (start, unit, planes) to the queue of their XCD, their word cleared.
// sweep_units: a persistent grid (`nblocks` workgroups) drains the queues, own XCD first.
size_t units_lds_bytes(int waves);
int units_wgs_per_cu();     // persistent workgroups per CU the unit kernel is built for
hipError_t launch_plan_pass(const DevLayout &L, const StartDesc *starts, const int2 *work,
                            long long nwork, int *changed, int4 *lists, int list_cap, int nlists,
                            int *ctrl, const StripPlan &plan, float gate_r2, int *flags0, long long flags_stride,
                            hipStream_t st);      // (flags0 + s * flags_stride = starts[s].tile_flags)
hipError_t launch_sweep_units(const DevLayout &L, const float *v, const StartDesc *starts,
                              const int4 *lists, int list_cap, int nlists, int *ctrl, int nblocks,
                              int *changed, const StripItem *items, const StripPlan &plan,
                              const UnitPassTail &tail, hipStream_t st);
// One launch per solve (AsyncSolve, ttsweep_dev.h): the first as.nrings workgroups plan, the others
// relax; returns when every ring is at rest.  tail: only entries / nentries / max_box_cells are used.
// waves: STRIP_NS (two workgroups per CU) or - units of one plane - STRIP_NS_LAT (the latency instance)
hipError_t launch_solve_units(const DevLayout &L, const float *v, const StartDesc *starts, int nblocks,
                              int *changed, const StripItem *items, const StripPlan &plan, int waves,
                              const UnitPassTail &tail, const AsyncSolve &as, int *flags0, long long flags_stride,
                              hipStream_t st);
// pend |= defer, defer = 0 for the units of the listed starts (np planes per unit); changed[s] |=
// CHANGED_PENDING where a bit moved (push_improved: bits for units nearer to the start are deferred)
hipError_t launch_flush_deferred(const DevLayout &L, int np, int *flags0, long long flags_stride,
                                 const int *active, int nactive, int *changed, hipStream_t st);
// First activity words of a start: from_box = false: only the start's patch is a source;
// from_box = true: every patch that holds a finite travel time is one.  (ra, np: the reach of
// the star along the plane axis and the planes per unit of the solve.)
hipError_t launch_init_tile_flags(const DevLayout &L, const StartDesc &sd, bool from_box, int ra, int np,
                                  hipStream_t st);

// ... for all starts of a solve at once (fresh boxes: the start's patch is the only source); start s's words at
// flags0 + s * stride
hipError_t launch_init_tile_flags_batch(const DevLayout &L, int *flags0, long long stride, const StartDesc *starts,
                                        int nstart, int ra, int np, hipStream_t st);

// ---- sweep, variant TILE ---------------------------------------------------
// One call = the tiles of one hyperplane of an ordering sweep (TileSweep), ONE kernel: a grid of
// P.nblocks single-wavefront workgroups (what tile_sweep_wgs_per_cu says the device holds at
// once); workgroup b evaluates the candidates (active start, J', K') number b, b + nblocks, ...
// - a tile is relaxed only if one of its 27 neighbours improved since it was last relaxed
// (StartDesc::tile_flags holds two words per tile) - and relaxes the due ones; its work sums go
// to private slots (P.wgwork) that launch_tile_reduce_work adds to the starts' counters.  A sweep = the calls D = 0 .. NI + NJ + NK - 3
// in stream order.  changed[s] |= 1 when a tile of start s improved: a whole sweep without a
// change proves convergence.
size_t tile_lds_bytes(int R);
// faces[...] = the z faces (ttsweep_dev.h: tile_face_index) of a padded volume
hipError_t launch_build_tile_faces(const DevLayout &L, const float *padded, float *faces, int fz, hipStream_t st);
// the faces of an initialised box (+INFINITY everywhere, 0 at the start cell (sa, sb, sc))
hipError_t launch_init_tile_faces(const DevLayout &L, float *faces, int fz, int sa, int sb, int sc, hipStream_t st);
hipError_t tile_sweep_wgs_per_cu(const TileSweep &P, int *wgs);
hipError_t launch_tile_sweep(const TileSweep &P, hipStream_t st);
// work0[3 s], work0[3 s + 2] += the workgroups' private sums wgwork[block][s][0 / 1]; slots cleared
hipError_t launch_tile_reduce_work(unsigned long long *wgwork, int nblocks, int nstart, unsigned long long *work0, hipStream_t st);
// from_box = false: only the start's tile counts as changed; true: every tile does.
hipError_t launch_init_tile_state(const DevLayout &L, const StartDesc &sd, bool from_box, hipStream_t st);

// ---- sweep, variant TILE, plain 6-neighbour star: one launch per solve (ttsweep_column.hip) ----
// is this the plain 6-neighbour star (pull entries x-, y-, z-, z+, y+, x+, every edge live in both directions)?
bool tile_star_is_six(const TileEntry *ent, int nent, int R);
// first state: every column sealed in "sweep 0", the tiles around a start due (from_box: every tile)
hipError_t launch_column_init(const ColumnSolve &P, const StartDesc *starts, bool from_box, hipStream_t st);
hipError_t column_solve_wgs_per_cu(int *wgs);   // workgroups a CU holds (and the LDS opt-in)
int column_solve_wg_waves();                    // wavefronts (columns in flight) of one workgroup
// the sequence of orderings the sweeps of a start follow (TTSWEEP_OPT_TILE_ORDER; n: the grid, at: the start, device axes)
constexpr int COL_ORDER_SEQUENCES = 10;
hipError_t launch_column_line(const float *v, const DevLayout &L, const StartDesc *starts, int nstart, float *out, hipStream_t st);
int column_order_default(const int (&n)[3], float at_start, float least, float largest);   // the choice for one start (-1: by the model)
bool column_order_valid(int which);        // table + 10 x first corner + 100 x axis roles
void column_order_sequence(int which, const int (&n)[3], const int (&at)[3], unsigned long long *seq);
// the whole solve: the wavefronts of `nblocks` resident workgroups claim columns until every start is at rest
hipError_t launch_column_solve(const ColumnSolve &P, int nblocks, hipStream_t st);

// ---- rays (ttsweep_rays.hip): predecessors and shortest-path rays of converged boxes ----
// One pull entry of the ray kernels, in the caller's axes: neighbour o = c + (di, dj, dk) of cell c, at
// flat FLOATBOX index c + udelta when it is inside the grid; its velocity vdelta after the cell's own in the
// padded volume (RayGeom).  Entries whose offset does not fit the grid are left out; the rest are sorted by (di, dj, dk, d).
struct RayEntry {
    int di, dj, dk, flags;  // flags: PULL_FWD / PULL_REV
    int udelta;
    float h, d;
    int pad_;
    long long vdelta;
};
// box s of a ray call: travel times and predecessors in the caller's FLOATBOX layout, its start cell
struct RayBox {
    const float *T;
    int *pred;
    int sflat;
    int pad_;
};
// the grid in the caller's axes and where its cells lie in the padded velocity volume:
// cell (x, y, z) at vbase + x * vs[0] + y * vs[1] + z * vs[2]
struct RayGeom {
    int n[3];
    int pad_;
    long long vbase, vs[3];
};
// pair lists: ray r is the ray of box pairs[r].box from the cell of FLOATBOX index pairs[r].recv
struct alignas(8) RayPair {
    int box, recv;
};
// what every ray kernel reads, passed by value: the grid, the padded velocity, the box records and the star's entries
struct RayArgs {
    RayGeom G;
    const float *v;
    const RayBox *boxes;
    const RayEntry *entries;
    int nentries;
};
// the n rays of a call: the cross product r = s * nrecv + q of the boxes with the receivers recv[q] (FLOATBOX
// indices; pairs == nullptr), or the records of a pair list (recv == nullptr)
struct RayList {
    const int *recv;
    int nrecv;
    const RayPair *pairs;
    long long n;
};
// the outputs of the geometry kernel, each [npair] (recv_hop, src_hop: [npair][3]) on the device or nullptr
struct RayGeometryOut {
    float *t_recv;
    int *hops;
    double *length;
    int *recv_hop;
    float *recv_d, *recv_dt;
    int *src_hop;
    float *src_d, *src_dt;
    int *deep;
};
// pred[s][c] for every cell of every box (TTSWEEP_PRED_* or the smallest flat index of a predecessor)
hipError_t launch_predecessors(const RayArgs &A, int nstart, bool exact, hipStream_t st);
// fill = false: count[r], status[r], t_recv[r] of every ray r of a cross product (of any size: 64-bit ray indices);
// fill = true: also the cells and hop lengths of the OK / SEED rays at [offsets[r], offsets[r + 1]) of cells / hop_d
// (written backwards, so a path reads source -> receiver; hop_d[offsets[r + 1] - 1] = 0)
hipError_t launch_trace_rays(const RayArgs &A, const RayList &L, bool exact, int *count, int *status, float *t_recv,
                             const long long *offsets, int *cells, float *hop_d, bool fill, hipStream_t st);
// the Frechet operators of the rays of either kind of list, at most INT32_MAX of them (status[r] of every ray; acc:
// the caller's g read as int64, zeroed first), and the geometry of the rays of a pair list
hipError_t launch_ray_forward(const RayArgs &A, const RayList &L, bool exact, const double *m, double *y, int *status,
                              hipStream_t st);
hipError_t launch_ray_adjoint(const RayArgs &A, const RayList &L, bool exact, const double *w, int S, long long *acc,
                              int *hits, hipStream_t st);
hipError_t launch_ray_pairs_geometry(const RayArgs &A, const RayList &L, bool exact, int *status,
                                     const RayGeometryOut &out, hipStream_t st);
// out[0] = max (frexp exponent + 2048) of the nonzero w (0: none), out[1] = 1 if a w is NaN or infinite; zeroed first
hipError_t launch_ray_weight_scan(const double *w, int n, int *out, hipStream_t st);
// g[x] = ldexp((double)acc[x], -S) in place
hipError_t launch_ray_fixed_to_double(long long *g, long long n, int S, hipStream_t st);

// event location (ttsweep_locate.hip; every search there is one scan, loc_scan, over its own kind of candidate, and
// the three argmin searches share the per-lane minima and the final).  check: invw[e] = 1.0 / W and flag[e] (bit 0 a
// non-finite pick, bit 1 a negative or non-finite weight, bit 2 no weight above zero) of every event; search: the
// per-tile partials [(e - e0) * ntiles + tile] of events e0 .. e0 + ne - 1; final: cell / misfit / t0 (each may be
// nullptr) of those events from the partials; volume: vol[v][x] = J of event vev[v]
int locate_tile_cells();
hipError_t launch_locate_check(int K, int nevent, const double *picks, const double *weights, double *invw, int *flag,
                               hipStream_t st);
hipError_t launch_locate_search(const float *const *boxes, int K, int N, const double *picks, const double *weights,
                                const double *invw, int e0, int ne, int ntiles, unsigned long long *part_key,
                                int *part_x, hipStream_t st);
hipError_t launch_locate_final(const float *const *boxes, int K, const double *picks, const double *weights,
                               const double *invw, int e0, int ne, int ntiles, const unsigned long long *part_key,
                               const int *part_x, int *cell, double *misfit, double *t0, unsigned long long nan_bits,
                               hipStream_t st);
hipError_t launch_locate_volume(const float *const *boxes, int K, int N, const double *picks, const double *weights,
                                const double *invw, const int *vev, double *const *vol, int nvol, hipStream_t st);

// windowed, strided event location (ttsweep_locate.hip).  A group is up to 8 consecutive events that share one
// window: its candidates q = (cx * cy_n + cy) * cz_n + cz (z fastest, ncand of them) are the cells of FLOATBOX
// index x0 + cx * mx + cy * my + cz * mz (x0 the window's lo corner; mx, my, mz = sx * ny * nz, sy * nz, sz the index
// steps of the lattice), cut into ntiles tiles of locate_window_tile_cells().  The
// partials of its event i are [part + i * ntiles + tile].  search: one block per entry of the block table; final: cell
// / misfit / t0 (each may be nullptr) of events e0 .. e0 + ne - 1, event e of group ev_group[e - e0]
constexpr int LOC_WIN_ET = 8;       // events of a group, at most
struct WinGroup {
    int e0, ne;             // first event and number of events
    int x0;                 // FLOATBOX index of the window's lo corner
    int cy, cz;             // lattice nodes along y and z
    int ncand, ntiles;
    long long part;
};
struct WinBlock {
    int group, tile;
};
int locate_window_tile_cells();
hipError_t launch_locate_window_search(const float *const *boxes, int K, int mx, int my, int mz,
                                       const double *picks, const double *weights, const double *invw,
                                       const WinGroup *groups, const WinBlock *blocks, int nblocks,
                                       unsigned long long *part_key, int *part_x, hipStream_t st);
hipError_t launch_locate_window_final(const float *const *boxes, int K, const double *picks, const double *weights,
                                      const double *invw, int e0, int ne, const int *ev_group, const WinGroup *groups,
                                      const unsigned long long *part_key, const int *part_x, int *cell, double *misfit,
                                      double *t0, unsigned long long nan_bits, hipStream_t st);

// sub-cell event location (ttsweep_locate.hip).  A group is up to 8 consecutive events that share one window of
// wx * wy * wz = wn cells from the FLOATBOX index x0 (cell lo).  Its candidates are the nodes q = (qx * ny + qy) * nz
// + qz (z fastest, relative to the window; nx, ny, nz = (w - 1) * sub + 1 nodes per axis, nnode of them), cut into
// ntiles tiles of locate_subcell_tile_nodes().  staged: the K * wn floats of the window are at most
// locate_subcell_stage_floats() and the blocks of the group copy them to LDS; such blocks and the others are listed
// and launched apart.  The partials of its event i are [part + i * ntiles + tile].  search: one block per entry of the
// block table; final: node [.][3] / misfit / t0 (each may be nullptr) of events e0 .. e0 + ne - 1, event e of group
// ev_group[e - e0]
struct SubGroup {
    int e0, ne;             // first event and number of events
    int x0;                 // FLOATBOX index of the window's lo corner
    int lo[3];              // the window's lo corner, in cells
    int wy, wz, wn;         // cells of the window along y and z, and in all
    int ny, nz;             // nodes along y and z
    int nnode, ntiles;
    int staged;
    long long part;
};
int locate_subcell_tile_nodes();
int locate_subcell_stage_floats();
hipError_t launch_locate_subcell_search(const float *const *boxes, int K, int gnyz, int gnz, int sub,
                                        const double *picks, const double *weights, const double *invw,
                                        const SubGroup *groups, const WinBlock *blocks, int nblocks, bool staged,
                                        unsigned long long *part_key, int *part_x, hipStream_t st);
hipError_t launch_locate_subcell_final(const float *const *boxes, int K, int gnyz, int gnz, int sub,
                                       const double *picks, const double *weights, const double *invw, int e0, int ne,
                                       const int *ev_group, const SubGroup *groups,
                                       const unsigned long long *part_key, const int *part_x, int *node,
                                       double *misfit, double *t0, unsigned long long nan_bits, hipStream_t st);

// confidence regions of located events (ttsweep_locate.hip).  check: lim[e * L + l], the exclusive limit on the bits
// of J of level l (0: the empty region), limmax[e] their greatest, flag[e] (bit 0 a NaN or negative m, bit 1 a NaN or
// negative delta); init: the n = nevent * L accumulators (g_sum [n][10], g_t0 [n][2] keys, g_box [n][6]) at their
// empty-region values; search: events e0 .. e0 + ne - 1 (at most 65535 * 8) added to them; final: the accumulators
// to the caller's arrays (each may be nullptr)
hipError_t launch_confidence_check(int nevent, int L, const double *m, const double *delta, unsigned long long *lim,
                                   unsigned long long *limmax, int *flag, hipStream_t st);
hipError_t launch_confidence_init(long long n, int nx, int ny, int nz, unsigned long long *g_sum,
                                  unsigned long long *g_t0, int *g_box, hipStream_t st);
hipError_t launch_confidence_search(const float *const *boxes, int K, int N, int ny, int nz, const double *picks,
                                    const double *weights, const double *invw, int e0, int ne, int L,
                                    const unsigned long long *lim, const unsigned long long *limmax,
                                    unsigned long long *g_sum, unsigned long long *g_t0, int *g_box, hipStream_t st);
hipError_t launch_confidence_final(long long n, const unsigned long long *g_sum, const unsigned long long *g_t0,
                                   const int *g_box, long long *count, long long *sum, long long *sum2, int *lo,
                                   int *hi, double *t0_lo, double *t0_hi, hipStream_t st);

// Fresnel volumes over box pairs (ttsweep_fresnel.hip).  Pair r reads box a (Ta) against box b (Tb) over its window
// of wx * wy * wz cells from the FLOATBOX index x0 (cell lo).  A row of the window is cut into quads of 4 consecutive
// z (the last one ragged): quad q = (cx * wy + cy) * ceil(wz / 4) + zq, nquad of them, cut into tiles of
// fresnel_tile_quads().  first[r] is the number of tiles of the pairs before r (first[npair]: of all), so block b of
// the call belongs to the pair r with first[r] <= b < first[r + 1] and is tile b - first[r] of it.
struct FresPair {
    const float *Ta, *Tb;
    double tau;
    int sb;                 // FLOATBOX index of box b's start cell
    int x0;                 // FLOATBOX index of the window's lo corner
    int lo[3];              // the window's lo corner, in cells
    int wy, wz;             // cells of the window along y and z
    int nquad;
};
int fresnel_tile_quads();
// t_ab[r] = Ta[sb] and status[r] (TTSWEEP_FRESNEL_*) of every pair
hipError_t launch_fresnel_pairs(const FresPair *pairs, int npair, float *t_ab, int *status, hipStream_t st);
// the accumulators of the volume call at their empty-pair values: cnt, sum = 0, box [npair][6] = (nx, ny, nz, -1, -1, -1)
hipError_t launch_fresnel_init(int npair, int nx, int ny, int nz, unsigned long long *cnt, unsigned long long *sum,
                               int *box, hipStream_t st);
// blocks [block0, block0 + nblocks) of the call.  volume: cnt[r] += cells with phi > 0, sum[r] += llrint(ldexp(phi,
// S)), box[r] their bounding box; forward: sum[r] += llrint(ldexp(phi * m[x], S)); adjoint: acc[x] += llrint(ldexp(w[r]
// * phi, S)) (w, acc both nullptr: none) and hits[x] += 1 (nullptr: none).  gnyz, gnz: ny * nz and nz of the grid.
hipError_t launch_fresnel_volume(const FresPair *pairs, const long long *first, int npair, long long block0,
                                 int nblocks, const float *t_ab, int gnyz, int gnz, int S, unsigned long long *cnt,
                                 unsigned long long *sum, int *box, hipStream_t st);
hipError_t launch_fresnel_forward(const FresPair *pairs, const long long *first, int npair, long long block0,
                                  int nblocks, const float *t_ab, int gnyz, int gnz, int S, const double *m,
                                  unsigned long long *sum, hipStream_t st);
hipError_t launch_fresnel_adjoint(const FresPair *pairs, const long long *first, int npair, long long block0,
                                  int nblocks, const float *t_ab, int gnyz, int gnz, int S, const double *w,
                                  long long *acc, int *hits, hipStream_t st);
// the accumulators to the caller's arrays (each may be nullptr): count / lo / hi as they are, out[r] = ldexp((double)
// sum[r], -S) (phi of the volume call, y of the forward call)
hipError_t launch_fresnel_final(int npair, int S, const unsigned long long *cnt, const unsigned long long *sum,
                                const int *box, const float *t_ab, long long *count, int *lo, int *hi, double *out,
                                float *t_ab_out, hipStream_t st);

#ifdef TTSWEEP_TILE_PROFILE
void tile_prof_dump();   // prints and clears the phase counters of tile_sweep_kernel
#endif
#ifdef TTSWEEP_COL_TRACE
void column_trace_dump(); // writes the event log of column_solve_kernel to $TTSWEEP_COL_TRACE_FILE and clears it
#endif
#ifdef TTSWEEP_COL_PROFILE
void column_prof_dump(); // prints and clears the phase counters of column_solve_kernel
#endif
#ifdef TTSWEEP_PROFILE
void prof_dump();        // prints and clears the phase counters of sweep_units_kernel
#endif

} // namespace ttsweep
