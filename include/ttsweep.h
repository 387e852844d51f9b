/* ttsweep.h - C ABI of the MI355X travel-time sweep library (libttsweep.so).
 *
 * This is the drop-in boundary for the hot path of the reference program
 * serial_new/sweep-tt-multistart.c: the file-local call
 *     changed[s] += sweepXYZ(nx, ny, nz, s, 0, starsize-1);        (:160)
 * inside the `while (anychange)` driver loop (:151-170), which reads the
 * file-scope globals fs[], start[], vbox and ttboxes[] (:62-66).  Nothing but
 * plain pointers, ints and the two small POD structs below crosses this
 * boundary; no FLOATBOX/VELOCITYBOX struct and no torch type does.
 *
 * Data layout at the boundary is the reference's FLOATBOX layout
 * (include/floatbox.h:127-129,160): a contiguous float32 array indexed
 * x*ny*nz + y*nz + z.  The library keeps its own padded/permuted device
 * copies; caller buffers are never re-allocated or freed by the library.
 *
 * Semantics.  One library "solve" is the reference's driver loop run to its
 * end: it relaxes every live edge of the forward star until no travel time
 * can improve (the `while (anychange)` loop without the temporary `break` of
 * :168-169; see old/sweep-serial/sweep-tt-multistart.c:189-211).  The
 * converged box does not depend on the order of relaxation, so the GPU is free
 * to use its own schedule and reproduces the serial fixed point bit for bit,
 * including the reference's two quirks (exclusive upper star bound at :160/:206
 * and the skipped edges centred on the start point, :219-221).
 *
 * Error convention: functions returning int return a negative value on a
 * HIP/argument error (text via ttsweep_last_error()); the reference's own
 * "0 = failure" convention stays on the header surface (floatbox.h etc.).
 * There is NO CPU fallback: without a usable HIP device every solve fails.
 */
#ifndef TTSWEEP_H
#define TTSWEEP_H

#ifdef __cplusplus
extern "C" {
#endif

#define TTSWEEP_ABI_VERSION 6      /* 6 (round 5): + ttsweep_solve_multi_changed, options 22-23; 5 (round 4): + ttsweep_get_changed,
                                      ttsweep_solve_multi_device, stats.fallbacks (in the struct's former padding),
                                      options 19-21; every version-4 caller runs unchanged */

/* Forward-star entry: same layout as `struct FS`
 * (serial_new/sweep-tt-multistart.c:46-49).  d must already hold
 * delta * |offset| exactly as the reference main() prepares it (:122,:127). */
typedef struct ttsweep_fs {
    int i, j, k;
    float d;
} ttsweep_fs;

/* Start point: same layout as `struct START` (serial_new/...:56-58). */
typedef struct ttsweep_start {
    int i, j, k;
} ttsweep_start;

/* Counters of the most recent solve on a context. */
typedef struct ttsweep_stats {
    int nstart;                 /* starts in the solve */
    int sweeps_max;             /* passes executed for the slowest start */
    long long sweeps_total;     /* sum over starts of passes launched (a pass relaxes only
                                   the units that are due: whose inputs changed and that the
                                   distance gate has reached; TILE kernel: a pass is one
                                   ordering sweep over the tiles that are due) */
    long long cells_relaxed;    /* cells actually relaxed against the whole star, summed
                                   over passes and starts (= sweeps_total * cells when
                                   nothing is skipped) */
    long long cells;            /* nx*ny*nz */
    long long relaxations_per_sweep; /* in-bounds (cell, offset) pairs one pass relaxes */
    long long launches;         /* sweep-kernel launches (TILE: one per tile hyperplane of a sweep) */
    double sweep_kernel_ms;     /* sum of sweep-kernel durations (HIP events on the
                                   library's stream; 0 unless timing is enabled) */
    double solve_ms;            /* device time of the whole solve (events) */
    int kernel_variant;         /* which sweep kernel ran (TTSWEEP_KERNEL_*) */
    int fallbacks;              /* solves whose one-launch form gave up (a wait inside it ran into its
                                   wall-clock limit) and that the pass / hyperplane driver then finished:
                                   the result is the same, the time is not */
} ttsweep_stats;

typedef struct ttsweep_ctx ttsweep_ctx;

/* option keys for ttsweep_set_option */
#define TTSWEEP_OPT_TIMING        1   /* 1: time every sweep launch with HIP events */
#define TTSWEEP_OPT_KERNEL        2   /* force a kernel variant (TTSWEEP_KERNEL_*) */
#define TTSWEEP_OPT_MAX_SWEEPS    3   /* safety cap on passes per solve (default 100000) */
#define TTSWEEP_OPT_MAX_BATCH     4   /* ttsweep_solve: at most this many starts per device
                                         batch (0 = as many as device memory holds) */
#define TTSWEEP_OPT_GATE_SPEED_MILLI 5 /* schedule only, never the result: cells (x 1/1000) by
                                          which the distance gate of the STRIP kernel opens per
                                          pass; 0 switches the gate off (default: half the
                                          star's reach) */
#define TTSWEEP_OPT_PAIR_MIN_STARTS 7 /* schedule only: the STRIP kernel relaxes units of two planes
                                         from this many starts per solve on, units of one plane
                                         below (0: always two, a huge value: never).  Default
                                         without this option: two planes when the solve offers
                                         enough units to keep the device busy with them (starts x
                                         one-plane units of a start >= 80 000), else one */
#define TTSWEEP_OPT_GATE_R0_MILLI 6   /* schedule only: gate radius of the first pass, cells x 1/1000
                                         (default: the star's reach + 1) */

#define TTSWEEP_OPT_PREPASS_ENTRIES 8  /* schedule only, never the result: relax the first N entries of
                                         the star (fs[starstart .. starstart+N-1]) to their own fixed
                                         point first, then the whole star from that state - the
                                         pre-processing of old/wavefront-openmp/wave-multistart.c:210-215
                                         (there: N = fsindex[3], the entries no longer than 4 cells,
                                         146 of the 818).  0 (default) switches it off. */

#define TTSWEEP_OPT_ASYNC          9   /* schedule only, never the result: 1 = the STRIP kernel - and the TILE kernel for
                                          the plain 6-neighbour star (column pipelines) - runs a solve as ONE
                                         launch (no passes: planner workgroups hand the due units, nearest to
                                         their start first, to the working workgroups through rings in device
                                         memory, and detect convergence on the device); 0 = a launch pair per
                                         pass; -1 (default) = the library chooses */
#define TTSWEEP_OPT_ASYNC_LOW     10  /* schedule only: a ring is refilled when it holds at most this many ... */
#define TTSWEEP_OPT_ASYNC_HIGH    11  /* ... up to this many units (0: defaults from the grid of workgroups) */
#define TTSWEEP_OPT_ASYNC_SPECIAL 12  /* schedule only: units of a start between two relaxations of its
                                         dead-edge cells in a one-launch solve (default 32) */
#define TTSWEEP_OPT_ASYNC_POLICY  13  /* schedule only: how a planner hands units out in a one-launch solve.
                                         0 = every refill of its ring starts at the unit nearest to the start
                                         (strict priority by distance); 1 (default) = the scan goes round and
                                         round the list, a unit at most once per round, behind the distance
                                         gate (TTSWEEP_OPT_GATE_*: per round instead of per pass) */
#define TTSWEEP_OPT_DEFER_MARGIN_MILLI 14 /* schedule only, never the result (STRIP kernel): an improvement is
                                         reported at once only to the units that are not nearer to the start
                                         than the improved cells by more than this many cells (x 1/1000, may be
                                         negative); the units behind the front hear of it when the start is
                                         otherwise at rest, once, instead of in every pass.  Default 375 (3/8 of a cell);
                                         <= -1000000000 switches the deferral off */
#define TTSWEEP_OPT_ASYNC_WINDOW_MILLI 15 /* schedule only: ring policy 2 - cells (x 1/1000) beyond the nearest unit
                                         with anything to do up to which a start's units are handed out; 0 = no
                                         gate */
#define TTSWEEP_OPT_ASYNC_GATE_MILLI 16 /* schedule only: ring policy 1 - cells (x 1/1000) by which the distance gate
                                         opens per round of a one-launch solve (default 500; 0 = no gate;
                                         TTSWEEP_OPT_GATE_SPEED_MILLI = 0 switches this gate off as well) */
#define TTSWEEP_OPT_ASYNC_GATE_FAST_MILLI 17 /* schedule only: ring policy 1 - cells (x 1/1000) by which the gate opens
                                         in a round that begins with an empty ring (the workers are running dry);
                                         never less than TTSWEEP_OPT_ASYNC_GATE_MILLI */
#define TTSWEEP_OPT_ASYNC_TIMEOUT_MILLI 18 /* wall-clock limit (ms) of every wait inside a one-launch solve; when one
                                         runs into it the launch drains and the pass driver finishes the solve from
                                         the boxes as they stand (same result).  0 (default): ten seconds plus
                                         twenty times the solve's expected duration */

#define TTSWEEP_OPT_TILE_IN_PLACE 19 /* schedule only, never the result (TILE kernel, one launch per solve): 1 (default) =
                                         relax the travel times in the caller's own device arrays when their rows are
                                         whole tiles long (nz % 32 == 0) and 64-byte aligned - no padded copy, no copy
                                         back; 0 = always in the library's padded volumes */

#define TTSWEEP_OPT_QUEUES 20        /* schedule only, never the result: unit queues / planner rings / claim sequences of
                                         a solve, 1 .. 8 (default: the XCDs the device shows, counted at create - 8 on a
                                         whole MI355X, fewer on a partition).  A one-launch solve serves at most 32 starts
                                         per ring: with more starts per queue than that the launch-per-pass driver runs */

#define TTSWEEP_OPT_ASYNC_INUNIT 21   /* schedule only, never the result (STRIP kernel, one launch per solve): how often
                                         a unit that improved is relaxed again, at once, against its OWN planes - the
                                         values it has just stored - before it is handed back (-1, the default: 2 for
                                         solves of 2 and more starts, 0 for a single start and for the eight-wave instance of small shards; 0 .. 8) */

#define TTSWEEP_OPT_ASYNC_HANDOFF 22  /* schedule only, never the result (STRIP kernel, one launch per solve): direct
                                         hand-off - a worker that has improved a plane not only tells the units that
                                         stage it, it also puts the idle ones among them (inside the distance gate) into
                                         the ring itself instead of leaving them to the planner's next scan (1), and
                                         likewise its own unit when bits arrived while it was being relaxed (2; 3 = both).
                                         -1 (default): the library chooses by the size of the solve (small shards: 3);
                                         0 = only the planners publish */

#define TTSWEEP_OPT_ASYNC_WAVES 23    /* schedule only, never the result (STRIP kernel, one launch per solve, one-plane
                                         units): wavefronts that relax a unit - 4 (two workgroups per CU, two units per CU
                                         at a time: throughput) or 8 (one workgroup per CU, all of a CU's wavefronts on
                                         one unit, four planes staged ahead: a hop of the front takes about half as
                                         long - for shards too small to fill the machine).  -1 (default): by the size
                                         of the solve */

#define TTSWEEP_OPT_TILE_ORDER 24     /* schedule only, never the result (TILE kernel, one launch per solve): which
                                         sequence of the eight orderings (+-x, +-y, +-z) the sweeps of each start follow:
                                         table (0 .. 9) + 10 x the corner the first sweep begins at (0: the grid's origin,
                                         1: the corner nearest to the start, 2: the farthest) + 100 x which axis plays
                                         which role of the table (0 .. 4) - column_order_sequence() in
                                         csrc/ttsweep_column.hip (0: the sequence of rounds 3 - 4).  -1 (default): per start, by where
                                         the start lies in the velocity profile of its vertical line (115: z flips with
                                         every sweep - sources at the slow end of a medium that gets faster with depth;
                                         111 for a start at the fast end) - column_order_default() */

#define TTSWEEP_KERNEL_AUTO       0
#define TTSWEEP_KERNEL_CELL       1   /* one thread per cell, star from global memory */
#define TTSWEEP_KERNEL_STRIP      2   /* LDS-staged plane slabs, register strips */
#define TTSWEEP_KERNEL_TILE       3   /* ordered (8-ordering Gauss-Seidel) tile sweeps for small
                                         stars: the HBM-bound regime */

/* ---- information ------------------------------------------------------- */
int ttsweep_abi_version(void);
/* number of HIP devices, or a negative value when HIP cannot be initialised */
int ttsweep_device_count(void);
/* text of the most recent error on this thread ("" if none) */
const char *ttsweep_last_error(void);

/* Optional: start initialising the HIP runtime for `device` on a background thread and
 * return at once (ttsweep_create waits for it).  A host program calls it first thing, so
 * that the few hundred milliseconds a process pays at its first HIP call run beside its
 * own file reading (serial_new/...:77-147) instead of inside its first sweepXYZ call.
 * Never needed for correctness.  Returns 0. */
int ttsweep_warmup(int device);

/* ---- context ----------------------------------------------------------- */
/* Create a solver for an nx*ny*nz grid and the star entries
 * fs[starstart .. starstop-1] (EXCLUSIVE upper bound, as the reference call
 * site passes starsize-1, :160).  Uploads the star to `device`.
 * Replaces: the globals fs[] / nx,ny,nz and the (starstart, starstop)
 * arguments of sweepXYZ (:198).  Every length fs[l].d, starstart <= l < starstop,
 * must be finite and >= 0 (a negative, infinite or NaN length is refused: NULL, with a
 * message).  A length whose half is not a float (a subnormal d with an odd last bit)
 * is accepted; every volume is then solved by the per-cell kernel's instance that
 * rounds as the reference does (see ttsweep_set_velocity).  Returns NULL on failure. */
ttsweep_ctx *ttsweep_create(int device, int nx, int ny, int nz,
                            const ttsweep_fs *fs, int starstart, int starstop);
void ttsweep_destroy(ttsweep_ctx *ctx);

int ttsweep_set_option(ttsweep_ctx *ctx, int key, long long value);

/* Velocity volume (the global `vbox.box.flat`, :65), host or device memory,
 * FLOATBOX layout.  The library keeps its own device copy.  Every value must be finite
 * and >= 0 (zero is accepted as the reference accepts it; a negative velocity, for which
 * the reference's loop :151-170 need not terminate, Inf and NaN are refused: < 0).
 * A volume with a positive value below 2^-124 / (smallest fs[].d of the star) - about 4.7e-39
 * for the reference's delta of 10 - is accepted and solved bit for bit like every other, but
 * slowly: there a delay d * (v[c] + v[o]) can be a denormal number, where the reference's
 * "/ 2.0" of the rounded product (:216) and the fast kernels' multiplication by d / 2 no
 * longer agree in the last bit, so such a volume goes to the per-cell kernel's instance that
 * rounds as the reference does (ttsweep_stats.kernel_variant reads TTSWEEP_KERNEL_CELL, whatever
 * TTSWEEP_OPT_KERNEL asked for; the next volume without such values gets the chosen kernel back).
 * The high end likewise: a volume with a value >= 2^126 / (largest fs[].d of the star) - about
 * 8.5e36 for delta 10 and the 6-neighbour star - goes to that instance, since there the
 * reference's product d * (v[c] + v[o]) can overflow to INFINITY where d / 2 times the sum
 * does not (the pair's delay is then INFINITY, and so is what it offers). */
int ttsweep_set_velocity(ttsweep_ctx *ctx, const float *v_host);
int ttsweep_set_velocity_device(ttsweep_ctx *ctx, const float *v_dev);

/* ---- the hot path ------------------------------------------------------ */
/* Relax nstart travel-time boxes to convergence.
 *   starts[s]  : the start point of box s (global start[], :63)
 *   tt[s]      : box s (global ttboxes[s].flat, :66), FLOATBOX layout; read as
 *                the initial state and overwritten with the converged state.
 * Returns 1 if any travel time improved, 0 if every box was already converged
 * (the two outcomes `anychange != 0` / `== 0` of :163-166), < 0 on error.
 * Where travel times overflow, a finite cell beside an INFINITY one stores
 * delay + t = INFINITY over INFINITY in every reference pass (:228-237): the reference's
 * loop never ends.  The library returns the boxes at which that loop stands still (every
 * later pass leaves every bit as it is), and a solve of those boxes returns 0.
 * Replaces: the whole `while (anychange)` loop of :151-170 over all starts.
 * A call with exactly the arrays and starts of the previous successful call on this context,
 * their contents bit for bit as that call left them (checked with a 128-bit digest of every
 * box; velocity, star and kernel unchanged), is answered with 0 without any device work: it
 * is the confirming pass of a reference-style driver loop. */
int ttsweep_solve(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                  float *const *tt_host);

/* Same, with the boxes in device memory (pointers are device addresses held
 * in a host array).  If init != 0 the incoming contents are ignored and every
 * box starts from the reference initial state (all +INFINITY, start = 0;
 * serial_new/...:139-144), which is then done on the device. */
int ttsweep_solve_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                         float *const *tt_dev, int init);

int ttsweep_get_stats(const ttsweep_ctx *ctx, ttsweep_stats *out);

/* Per-start outcome of the last ttsweep_solve / ttsweep_solve_device call of this context: out[s] = 1 when a
 * travel time of start s improved, 0 when its box was at its fixed point already - what the reference's driver
 * prints and sums as changed[s] (serial_new/sweep-tt-multistart.c:158-164), where the call's return value is the
 * OR over the starts.  Writes min(n, starts of that call) entries and returns their number (< 0 on bad
 * arguments). */
int ttsweep_get_changed(const ttsweep_ctx *ctx, int *out, int n);

/* On-device fixed-point check in the spirit of testconvergence
 * (old/wavefront-openmp/wave-multistart.c:300-347) on serial_new's edge set:
 *   open_edges         (cell, offset) pairs through which one more reference sweep would
 *                      still store a different value (serial_new/...:219-249, evaluated
 *                      without modifying the box; a store of INFINITY over INFINITY, see
 *                      ttsweep_solve, is not counted): 0 iff nothing can improve any more;
 *   cells_infinite     cells still at INFINITY;
 *   cells_unsupported  cells (other than the start) whose travel time is smaller than
 *                      every candidate their live edges offer, i.e. that no store of
 *                      :222-223 / :246-247 can have produced: 0 iff nothing is too small.
 * open_edges == 0 and cells_unsupported == 0 together pin the box to the one fixed point
 * of the relaxation (all delays positive), which is what the reference's loop :151-170
 * converges to.  tt_dev: device memory, FLOATBOX layout.  For grids where no CPU oracle
 * run is feasible (one reference sweep of 1024x1024x512 takes ~40 min).  Any of the
 * three result pointers may be NULL.  Returns 0 on success, < 0 on error. */
int ttsweep_validate_device(ttsweep_ctx *ctx, const ttsweep_start *start, const float *tt_dev,
                            long long *open_edges, long long *cells_infinite,
                            long long *cells_unsupported);

/* ---- rays: shortest paths of converged boxes --------------------------- */
/* The relaxation is the shortest-path (network) ray method: in a converged box every finite travel time
 * other than the start's is delay + T[o] of a live edge from a neighbour o with a smaller T[o] (a store of
 * serial_new/sweep-tt-multistart.c:222-223 / :246-247).  These calls read that back - the ray from each
 * start to each receiver, the receiver's time and, through the hop lengths, one row of dt/dv per ray - for
 * the boxes a solve produced (INTEGRATION.md "Rays").  They change no box and no state of the context: a
 * ttsweep_solve of the same boxes afterwards is still answered without device work.  Indices are int32:
 * grids of more than INT32_MAX cells are refused. */
#define TTSWEEP_HAS_RAYS 1          /* the ray calls below exist (TTSWEEP_ABI_VERSION stays 6) */

/* pred[s][c] values other than a cell index */
#define TTSWEEP_PRED_SOURCE (-1)    /* c is the start of box s */
#define TTSWEEP_PRED_SEED (-2)      /* a finite T[c] no live edge produces: a value the caller seeded (a solve with
                                       init = 0), or a plateau of zero delays */
#define TTSWEEP_PRED_UNREACHED (-3) /* T[c] is not below INFINITY */

/* Predecessors of every cell of nstart boxes, one launch.  For box s with start S = starts[s] and cell c
 * (FLOATBOX index x*ny*nz + y*nz + z): TTSWEEP_PRED_SOURCE if c == S, else TTSWEEP_PRED_UNREACHED if
 * T[c] is INFINITY or NaN, else the SMALLEST FLOATBOX index o over the live pull edges of c (entry +f_l live
 * if c != S, entry -f_l live if c - f_l != S, l in [starstart, starstop), o inside the grid) with
 * T[o] < T[c] and fl(delay + T[o]) == T[c], where delay = fl(fl(d_l * fl(v[c] + v[o])) / 2) exactly as the
 * solve rounds it (:216); TTSWEEP_PRED_SEED if there is none.
 *   tt_dev[s]   : device address of box s (float, FLOATBOX layout), read only
 *   pred_dev[s] : device address of box s's predecessors (int32, FLOATBOX layout), written
 * Returns 0, < 0 on error (NULL arguments, a start outside the grid, no velocity set, a grid of more than
 * INT32_MAX cells: refused before any device work).  Returns when pred is written. */
int ttsweep_predecessors_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                const float *const *tt_dev, int *const *pred_dev);

/* status of a ray */
#define TTSWEEP_RAY_OK 0            /* the path ends at the start */
#define TTSWEEP_RAY_SEED 1          /* the path ends at a TTSWEEP_PRED_SEED cell */
#define TTSWEEP_RAY_UNREACHED 2     /* T at the receiver is INFINITY (or NaN): no cells */
#define TTSWEEP_RAY_INVALID 3       /* pred_dev is out of range, does not strictly decrease T, or names a cell no live
                                       edge of the star reaches with the receiver side's time: no cells */

/* Rays of nstart boxes to nrecv receivers: ray r = s*nrecv + q follows pred_dev[s] (as written by
 * ttsweep_predecessors_device, for the same boxes) from receiver q back to a SOURCE or SEED cell.  Every hop
 * p -> c is checked against the box (0 <= p < nx*ny*nz, T[p] < T[c], a live edge whose candidate is T[c]),
 * so a wrong pred buffer ends a ray as TTSWEEP_RAY_INVALID and never makes a walk run on.
 *   offsets   : host, nstart*nrecv + 1 entries: the exclusive prefix sums of the path cells (offsets[0] = 0);
 *               ray r's cells are [offsets[r], offsets[r+1]) of cells_dev
 *   status    : host, nstart*nrecv entries (TTSWEEP_RAY_*), may be NULL
 *   t_recv    : host, nstart*nrecv entries, T at the receiver, may be NULL
 *   cells_dev : device, int32 FLOATBOX indices, the path source -> receiver (hops + 1 cells)
 *   hop_d_dev : device, float, aligned with cells_dev: the star length d of the hop from cell i to cell i+1
 *               of the path (of duplicate entries the smallest d whose candidate is the later cell's time);
 *               the last cell of every ray holds 0
 * cells_dev and hop_d_dev are written only when both are non-NULL and capacity >= the total, so a caller
 * counts first (NULL buffers), allocates, then calls again.  Replaying the hops from T[path[0]],
 * t = fl(delay(hop_d[h], v[path[h]] + v[path[h+1]]) + t), ends at exactly t_recv for every OK and SEED ray.
 * Returns the total number of path cells (>= 0), < 0 on error (the checks of ttsweep_predecessors_device, a
 * receiver outside the grid, nrecv < 0, offsets NULL). */
long long ttsweep_trace_rays_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                    const float *const *tt_dev, const int *const *pred_dev,
                                    int nrecv, const ttsweep_start *receivers,
                                    long long *offsets, int *status, float *t_recv,
                                    int *cells_dev, float *hop_d_dev, long long capacity);

/* ---- rays: the Frechet operators G m and G^T w without stored paths ---- */
/* G [nstart*nrecv, nx*ny*nz] is the Frechet matrix of the rays of ttsweep_trace_rays_device for the same
 * arguments: every hop of length d (hop_d) between cells a and b of an OK or SEED ray r adds d/2 at (r, a) and
 * at (r, b); UNREACHED and INVALID rays have an empty row.  These calls walk the rays as
 * ttsweep_trace_rays_device does (the same checks per hop, the same statuses, the same hop_d choice) and read
 * or scatter along the walk instead of storing it: the memory they need is the boxes, pred and their outputs.
 * Same arguments and checks as ttsweep_trace_rays_device; also refused: nstart*nrecv > INT32_MAX.  Refusals
 * happen before any device work, except that of a NaN or infinite weight, which is found before g is touched.
 * They change no box and no state of the context.  Both return 0, or < 0 with ttsweep_last_error set. */
#define TTSWEEP_HAS_RAY_OPERATORS 1 /* the two calls below exist (TTSWEEP_ABI_VERSION stays 6) */

/* y = G m.  m_dev: device, double, FLOATBOX layout.  y_dev: device, double, nstart*nrecv entries.  Per ray,
 * in walk order (receiver -> source), from y = 0.0: y = y + (0.5 * (double)d) * (m[c] + m[p]) for every hop
 * p -> c, rounded step by step (no contraction); 0 for an UNREACHED or INVALID ray.
 *   status : host, nstart*nrecv entries (TTSWEEP_RAY_*), may be NULL */
int ttsweep_ray_forward_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                               const float *const *tt_dev, const int *const *pred_dev,
                               int nrecv, const ttsweep_start *receivers,
                               const double *m_dev, double *y_dev, int *status);

/* g = G^T w and hit counts, deterministic: bit-identical from call to call, whatever the scheduling.
 *   w_dev    : device, double, nstart*nrecv entries; NaN or infinite weights are refused
 *   g_dev    : device, double, FLOATBOX layout, written (w_dev and g_dev both NULL: hit counts only)
 *   hits_dev : device, int32, FLOATBOX layout: the number of OK or SEED rays whose path holds the cell; may be NULL
 *   scale    : host, S below, may be NULL
 * g is summed in int64 fixed point, with g_dev as the accumulator: E_w = the largest frexp exponent of the
 * nonzero weights, E_d = the frexp exponent of the largest d among the star's ray entries (offsets that fit the
 * grid), K = ceil(log2(nstart*nrecv)) (0 for one ray), S = 61 - E_w - E_d - K.  The visit of cell x by ray r
 * adds llrint(ldexp(w[r] * (0.5 * ((double)d_in + (double)d_out)), S)), d_in and d_out the lengths of the
 * path's hops into and out of x (0 where there is none); then g[x] = ldexp((double)acc[x], -S).  No sum can
 * overflow (a visit adds less than 2^(61-K), a ray visits a cell at most once: |acc[x]| < 2^61); each visit is
 * rounded by at most 2^-S / 2, so g[x] is within 2^-S * hits[x] / 2 of the sum of the double terms, plus the
 * last rounding to double.  Every weight zero: g = 0 and S = 0. */
int ttsweep_ray_adjoint_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                               const float *const *tt_dev, const int *const *pred_dev,
                               int nrecv, const ttsweep_start *receivers,
                               const double *w_dev, double *g_dev, int *hits_dev, int *scale);

/* ---- rays: pair lists ---------------------------------------------------- */
/* The data of a tomography are not a cross product: an event is picked at some of the stations, a shot has its own
 * receiver spread.  These calls take the rays as a list of npair (box, receiver) pairs instead: ray r is the ray of
 * box pair_box[r] from receiver pair_recv[r], walked exactly as ttsweep_trace_rays_device walks it (the same checks
 * per hop, the same statuses, the same hop_d choice).  A pair may occur more than once: each occurrence is a ray of
 * its own.  Arguments ctx, nstart, starts, tt_dev, pred_dev as for ttsweep_ray_forward_device, then
 *   npair     : the number of pairs
 *   pair_box  : host, npair entries, each in [0, nstart)
 *   pair_recv : host, npair receivers (cells inside the grid)
 * Refused before any device work and before any output is touched: everything ttsweep_ray_forward_device refuses
 * for the shared arguments, npair < 0, npair > INT32_MAX, a NULL pair_box or pair_recv with npair > 0, a pair_box
 * outside [0, nstart) and a receiver outside the grid (ttsweep_last_error names the pair); a NaN or infinite weight
 * is found before g is touched, as in the dense call.  npair == 0 behaves as the dense calls do with nrecv == 0.
 * The calls change no box and no state of the context.  All return 0, or < 0 with ttsweep_last_error set. */
#define TTSWEEP_HAS_RAY_PAIRS 1     /* the three calls below exist (TTSWEEP_ABI_VERSION stays 6) */

/* y = G m and g = G^T w with hit counts over the pair list: the semantics of ttsweep_ray_forward_device and
 * ttsweep_ray_adjoint_device word for word, with nstart*nrecv replaced by npair: y_dev, w_dev and status have npair
 * entries, K = ceil(log2(npair)) (0 for one ray), S = 61 - E_w - E_d - K.  For the pair list
 * pair_box[s*nrecv+q] = s, pair_recv[s*nrecv+q] = receivers[q] every output is the dense call's bit for bit.  g, hits
 * and S do not depend on the order of the pairs (integer sums; S depends on the weights and npair only); y and
 * status follow it. */
int ttsweep_ray_pairs_forward_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                     const float *const *tt_dev, const int *const *pred_dev,
                                     long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                     const double *m_dev, double *y_dev, int *status);
int ttsweep_ray_pairs_adjoint_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                     const float *const *tt_dev, const int *const *pred_dev,
                                     long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                     const double *w_dev, double *g_dev, int *hits_dev, int *scale);

/* The geometry of every ray of the list, read off the same walk without storing a path.  status: host, npair entries,
 * may be NULL.  Every *_dev output is on the device, one entry per pair (recv_hop_dev and src_hop_dev: three int32 per
 * pair, entry 3*r + axis); each may be NULL.  For an OK or SEED ray with hops p -> c in walk order (receiver to
 * source), q the receiver's FLOATBOX index:
 *   t_recv   : T[q]; written for every status
 *   hops     : the number of hops (the path's cells minus 1); 0 for a receiver that is the start or a SEED cell
 *   length   : from 0.0, length = length + (double)d per hop in walk order, each addition rounded on its own
 *   recv_hop : the cell offset (p - c) per axis of the first hop, the one out of the receiver: it points from the
 *              receiver towards the source; recv_d: that hop's d; recv_dt: the one float subtraction T[c] - T[p]
 *   src_hop  : the offset (c - p) of the last hop, p the cell the walk ends at: it points out of the source;
 *              src_d: that hop's d; src_dt: T[c] - T[p]
 *   deep     : the FLOATBOX index of the path cell with the greatest z index, receiver and end cell included; of equal
 *              ones the first met in walk order
 * A ray without a hop has zeros in both *_hop, *_d and *_dt, and deep = q.  An UNREACHED or INVALID ray has hops = 0,
 * length = 0.0, zeros in the hop fields and deep = -1 (t_recv is still T[q]).  Every output is an integer or one
 * singly rounded float or double operation. */
int ttsweep_ray_pairs_geometry_device(ttsweep_ctx *ctx, int nstart, const ttsweep_start *starts,
                                      const float *const *tt_dev, const int *const *pred_dev,
                                      long long npair, const int *pair_box, const ttsweep_start *pair_recv,
                                      int *status, float *t_recv_dev, int *hops_dev, double *length_dev,
                                      int *recv_hop_dev, float *recv_d_dev, float *recv_dt_dev,
                                      int *src_hop_dev, float *src_d_dev, float *src_dt_dev, int *deep_dev);

/* ---- locate: grid-search event location over station travel-time boxes ---- */
/* By reciprocity, box k solved from station k as its start holds T_k[x], the travel time between the station and a
 * candidate hypocentre x.  For each of nevent events with picks o[e][k] and weights w[e][k] (double, [nevent][nbox],
 * device; weights_dev NULL: every weight 1.0; w = 0: station k has no pick for e) every cell x is scored in double,
 * stations in ascending k, the stations with w[e][k] == 0 skipped in every sum, each operation rounded on its own:
 *   W     = 0.0;  W  = W + w[e][k]                                          invW = 1.0 / W
 *   S1    = 0.0;  S1 = S1 + w[e][k] * (o[e][k] - (double)T_k[x])            t0(x) = S1 * invW
 *   J(x)  = 0.0;  J  = J + (w[e][k] * r) * r,   r = (o[e][k] - (double)T_k[x]) - t0(x)
 * the weighted L2 misfit with the origin time eliminated.  x is inadmissible for e when a picked station has
 * T_k[x] >= +INFINITY or J(x) is not below +INFINITY; then J(x) = +INFINITY.  Per event:
 *   cell[e]   the smallest FLOATBOX index among the admissible cells of minimal J, -1 when there is none
 *   misfit[e] J(cell[e]), +INFINITY when there is none
 *   t0[e]     t0(cell[e]), a quiet NaN when there is none
 * Bit-identical from call to call, whatever the launch, the batch or which events share the call.
 *   tt_dev          : host array of nbox device pointers to float boxes (FLOATBOX layout); any float values
 *   cell_dev, misfit_dev, t0_dev : device, nevent entries each, int32 / double / double; each may be NULL
 *   vol_events      : host, nvol event indices in [0, nevent); vol_dev: host array of nvol device pointers to double
 *                     volumes (FLOATBOX layout) that receive J of those events, +INFINITY where inadmissible
 * Refused, before any output is touched: a NaN or infinite pick (also of a station without a pick); a negative,
 * NaN or infinite weight; an event whose weights are all zero; nbox < 1, nevent < 1, nvol < 0 or > 65535, a NULL
 * pointer where one is needed, a volume event outside [0, nevent); nbox * nevent > INT32_MAX; grids of more than
 * INT32_MAX cells.  The boxes and the context's state are left as they are (a following ttsweep_solve of the same
 * boxes is still answered as a confirming pass).  Returns 0, or < 0 with ttsweep_last_error set. */
#define TTSWEEP_HAS_LOCATE 1 /* the call below exists (TTSWEEP_ABI_VERSION stays 6) */
int ttsweep_locate_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev,
                          int nevent, const double *picks_dev, const double *weights_dev,
                          int *cell_dev, double *misfit_dev, double *t0_dev,
                          int nvol, const int *vol_events, double *const *vol_dev);

/* ---- locate window: the search of "locate" over a window and a lattice per event ---- */
/* J(x), t0(x) and admissibility are exactly those of "locate" above: the same operations in the same order, so the
 * same bits.  The candidate set of event e is
 *   C(e) = { (x,y,z) : lo[e][a] <= coord_a <= hi[e][a]  and  (coord_a - lo[e][a]) % stride[a] == 0, each axis a }
 * an axis-aligned window, inclusive, with a lattice anchored at the window's own lo.  Per event:
 *   cell[e]   the smallest FLOATBOX index among the admissible cells of C(e) of minimal J, -1 when there is none
 *   misfit[e] J(cell[e]), +INFINITY when there is none
 *   t0[e]     t0(cell[e]), the quiet NaN of ttsweep_locate_device when there is none
 * With the whole grid and stride 1 these are the outputs of ttsweep_locate_device.  Bit-identical from call to call,
 * whatever the launch, the batch, which events share the call or how their windows repeat (consecutive events with
 * one window share the loads of a cell's travel times; that decides the traffic only).
 *   lo, hi          : host, int32 [nevent][3], inclusive; both NULL: the whole grid for every event
 *   stride          : host, int32 [3], each >= 1; NULL: 1, 1, 1.  A stride beyond the window leaves the node at lo
 *   tt_dev, picks_dev, weights_dev, cell_dev, misfit_dev, t0_dev : as for ttsweep_locate_device; each output may be NULL
 * The call allocates nothing that grows with the grid: its scratch follows the events and the candidates of a batch
 * of events, and the batches are cut under a fixed budget.
 * Refused, before any output is touched: everything ttsweep_locate_device refuses for its arguments, picks and
 * weights; lo without hi or hi without lo; lo[e][a] < 0, hi[e][a] >= n_a or lo[e][a] > hi[e][a] (the message names
 * the event); a stride below 1.  The boxes and the context's state are left as they are (a following ttsweep_solve
 * of the same boxes is still answered as a confirming pass).  Returns 0, or < 0 with ttsweep_last_error set. */
#define TTSWEEP_HAS_LOCATE_WINDOW 1 /* the call below exists (TTSWEEP_ABI_VERSION stays 6) */
int ttsweep_locate_window_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev,
                                 int nevent, const double *picks_dev, const double *weights_dev,
                                 const int *lo, const int *hi, const int *stride,
                                 int *cell_dev, double *misfit_dev, double *t0_dev);

/* ---- locate subcell: the search of "locate" over the nodes of a finer lattice, the boxes interpolated ---- */
/* The candidates of event e are the nodes q = (qx, qy, qz) with lo[e][a] * sub <= q_a <= hi[e][a] * sub on each axis
 * a: `sub` lattice steps per cell edge inside an inclusive window of cells.  Node q stands for the position q / sub,
 * in cells.  Per axis of a node
 *   i = q / sub (integer division)    f = q % sub    j = i + (f != 0)    u = (double)f / (double)sub
 * j never leaves the window (f != 0 implies i < hi), so no cell outside [lo, hi] is read.  The time of station k at
 * the node is interpolated trilinearly in double, every operation rounded on its own, no contraction, with
 * lerp(a, b, u) = a + u * (b - a) (a subtraction, a multiplication, an addition) and T(x,y,z) = (double)T_k[(x*ny + y)*nz + z]:
 *   c00 = lerp(T(ix,iy,iz), T(ix,iy,jz), uz)    c01 = lerp(T(ix,jy,iz), T(ix,jy,jz), uz)
 *   c10 = lerp(T(jx,iy,iz), T(jx,iy,jz), uz)    c11 = lerp(T(jx,jy,iz), T(jx,jy,jz), uz)
 *   c0  = lerp(c00, c01, uy)                    c1  = lerp(c10, c11, uy)            That_k(q) = lerp(c0, c1, ux)
 * J(q) and t0(q) are the formulas of "locate" above with That_k(q) in place of (double)T_k[x]: the same station order,
 * zero weights skipped, the same operations in the same order.  A node is admissible for e exactly when
 * J(q) < +INFINITY.  A node is therefore inadmissible exactly when a picked station has a non-finite value at one of
 * its eight corners (i|j): a non-finite corner always leaves That at +-INF or NaN, and then J is NaN.  Per event:
 *   node[e]   the admissible node of minimal J, ties to the smallest (qx, qy, qz) in lexicographic order;
 *             (-1, -1, -1) when there is none
 *   misfit[e] J(node[e]), +INFINITY when there is none
 *   t0[e]     t0(node[e]), the quiet NaN of ttsweep_locate_device when there is none
 * 1. Where f = 0 on all three axes That_k is the cell's value (a + 0 * (a - a) is a; a float -0.0 becomes +0.0, which
 *    changes no o - T), so J and t0 carry the bits "locate" gives that cell.
 * 2. With sub = 1 the outputs are those of ttsweep_locate_window_device on the same window at stride 1, node being
 *    that cell's (x, y, z).
 * 3. For every sub, misfit[e] <= the misfit[e] of ttsweep_locate_window_device on the same window at stride 1.
 * 4. Bit-identical from call to call, whatever the launch, the batch, which events share the call or how their windows
 *    repeat (the nodes of a small window are scored from a copy of its cells in on-chip memory, those of a large one
 *    from the boxes: the same values, the same operations).
 *   lo, hi          : host, int32 [nevent][3], inclusive, in cells; both NULL: the whole grid for every event
 *   sub             : lattice steps per cell edge, 1 <= sub <= 64
 *   node_dev        : device, int32 [nevent][3]
 *   tt_dev, picks_dev, weights_dev, misfit_dev, t0_dev : as for ttsweep_locate_window_device; each output may be NULL
 * The call allocates nothing that grows with the grid: its scratch follows the events and the nodes of a batch of
 * events, and the batches are cut under a fixed budget.
 * Refused, before any output is touched: everything ttsweep_locate_window_device refuses for its arguments, picks,
 * weights and windows; sub outside 1..64; (n_a - 1) * sub > INT32_MAX on an axis; an event with more than INT32_MAX
 * nodes (the message names the event).  The boxes and the context's state are left as they are.  Returns 0, or < 0
 * with ttsweep_last_error set. */
#define TTSWEEP_HAS_LOCATE_SUBCELL 1 /* the call below exists (TTSWEEP_ABI_VERSION stays 6) */
int ttsweep_locate_subcell_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev,
                                  int nevent, const double *picks_dev, const double *weights_dev,
                                  const int *lo, const int *hi, int sub,
                                  int *node_dev, double *misfit_dev, double *t0_dev);

/* ---- locate confidence: confidence regions of located events, without misfit volumes ---- */
/* J(x), t0(x) and admissibility are exactly those of "locate" above: the same operations in the same order, so the
 * same bits.  Per event e a reference level m[e] (normally misfit[e] of ttsweep_locate_device) and nlevel thresholds
 * delta[e][l] (double, device, [nevent] and [nevent][nlevel], 1 <= nlevel <= 4).  For event e and level l
 *   thr    = m[e] + delta[e][l]                          (one double addition)
 *   R(e,l) = { x admissible for e  and  J(x) <= thr }
 * and with the FLOATBOX index c = (x*ny + y)*nz + z, per (e, l) ([nevent][nlevel] leading dimensions, device):
 *   count  int64      the number of cells of R                                         empty region: 0
 *   sum    int64 [3]  sum of x, of y, of z over R                                                     0
 *   sum2   int64 [6]  sum of xx, yy, zz, xy, xz, yz over R                                            0
 *   lo, hi int32 [3]  the bounding box of R, inclusive                   lo = (nx, ny, nz), hi = (-1, -1, -1)
 *   t0_lo, t0_hi double  the least and greatest t0(x) over R in IEEE totalOrder (-0 below +0)  +INFINITY, -INFINITY
 * t0(x) is finite on every admissible cell, so both extremes are finite whenever count > 0.  m[e] = +INFINITY (an
 * event locate found no cell for) gives the empty region at every level, by definition and before thr is formed
 * (also for delta = +INFINITY).  delta = +INFINITY is allowed and gives every admissible cell.  m is a level, not
 * checked to be the minimum.  Every output is an integer sum, minimum or maximum (t0 through an ordered key), so the
 * results are identical from call to call, whatever the launch, the batch or which events share the call.  Each
 * output may be NULL.  The call allocates nothing that grows with the grid.
 * Refused, before any output is touched: everything ttsweep_locate_device refuses for picks and weights; a NaN or
 * negative m[e]; a NaN or negative delta; nlevel outside 1..4; nbox < 1, nevent < 1, a NULL pointer where one is
 * needed; nbox * nevent > INT32_MAX; grids of more than INT32_MAX cells or with ncells * max(nx, ny, nz)^2 >= 2^63
 * (the second moments could overflow).  The checks are on the bits (-0.0 is zero).  The boxes and the context's
 * state are left as they are.  Returns 0, or < 0 with ttsweep_last_error set. */
#define TTSWEEP_HAS_LOCATE_CONFIDENCE 1 /* the call below exists (TTSWEEP_ABI_VERSION stays 6) */
int ttsweep_locate_confidence_device(ttsweep_ctx *ctx, int nbox, const float *const *tt_dev,
                                     int nevent, const double *picks_dev, const double *weights_dev,
                                     const double *misfit_dev, int nlevel, const double *delta_dev,
                                     long long *count_dev, long long *sum_dev, long long *sum2_dev,
                                     int *lo_dev, int *hi_dev, double *t0_lo_dev, double *t0_hi_dev);

/* ---- fresnel: fat-ray (first Fresnel volume) sensitivities over pairs of boxes ---- */
/* With boxes from a SYMMETRIC star, T_b[x] is also the travel time from x to the start of box b (the reciprocity
 * "locate" relies on), so T_a[x] + T_b[x] - T_a[start_b] is the detour of the path a -> x -> b over the fastest path:
 * zero on the ray, growing away from it.  The cells whose detour is below tau form the fat ray of the pair, weighted by
 * a linear taper.  THE ABI DOES NOT CHECK THAT THE STAR IS SYMMETRIC OR THAT THE BOXES ARE CONVERGED: the arithmetic
 * below is defined for any float values, it only means a Fresnel volume under those two conditions.  No velocity is
 * needed: ctx supplies the grid and the device only.  Arguments shared by the three calls:
 *   nbox, starts : the start cell of every box (host, nbox entries)
 *   tt_dev       : host array of nbox device pointers, float boxes in FLOATBOX layout, any float values
 *   npair        : the number of pairs
 *   pair_a, pair_b : host, int32, npair entries each in [0, nbox).  A pair may repeat, each occurrence counts; a == b
 *                  is allowed
 *   tau          : host, double, npair entries: the half-width of the volume in the boxes' time unit
 *   lo, hi       : host, int32 [npair][3], the inclusive window of cells of every pair; both NULL: the whole grid.
 *                  Cells outside a pair's window are not visited (phi = 0 there)
 *   status       : host, npair entries (TTSWEEP_FRESNEL_*), may be NULL
 * Per pair r with a = pair_a[r], b = pair_b[r]: t_ab = T_a[start_b], one float.  status[r] is TTSWEEP_FRESNEL_OK, or
 * TTSWEEP_FRESNEL_UNREACHED when !(t_ab < +INFINITY) (INFINITY or a NaN); an UNREACHED pair has no cells.  The weight
 * of cell x, every operation rounded on its own (no contraction):
 *   A = (double)T_a[x], B = (double)T_b[x];  phi = 0 if !(A < +INFINITY) or !(B < +INFINITY)
 *   delta = (A + B) - (double)t_ab
 *   phi   = 1.0 - delta / tau[r];   phi = 1.0 if phi > 1.0;   phi = 0 if !(phi > 0.0)   (so also for a NaN)
 * The clamp to 1 is needed: on converged boxes rounding leaves delta slightly negative on and beside the thin ray.
 * Cells with phi = 0 contribute to no output.  With K_c = ceil(log2(nx*ny*nz)) (0 for one cell), K_p =
 * ceil(log2(npair)) (0 for one pair) and E_m, E_w the largest frexp exponents of the nonzero entries of m and w, every
 * sum below is an int64 sum that cannot overflow (a term is below 2^(61-K) and there are at most 2^K of them), and
 * the box limits are integer minima and maxima: all outputs are bit-identical from call to call, whatever the launch,
 * the batching or the order of the pairs.  g, hits and both scales do not depend on the order of the pairs; y, phi,
 * count, the boxes, t_ab and status follow it.  Passing the bounding boxes of the volume call as windows (an empty
 * pair with any valid one-cell window) changes no bit of any output.
 * Refused before any output is touched (ttsweep_last_error names the pair where there is one): a NULL pointer where
 * one is needed; nbox < 1; npair < 0; npair > INT32_MAX; lo without hi or hi without lo; grids of more than INT32_MAX
 * cells; a start outside the grid; a NULL box pointer; a pair index outside [0, nbox); a tau that is NaN, infinite or
 * <= 0; a window outside the grid or with lo > hi; a NaN or infinite m or w - that one is found on the device, before
 * y or g is touched, as in ttsweep_ray_adjoint_device.  npair == 0 succeeds: g and hits are zeroed and the scale is 0.
 * The calls change no box and no state of the context; they allocate nothing that grows with the grid (g and hits are
 * the caller's).  All return 0, or < 0 with ttsweep_last_error set. */
#define TTSWEEP_HAS_FRESNEL 1       /* the three calls below exist (TTSWEEP_ABI_VERSION stays 6) */
#define TTSWEEP_FRESNEL_OK 0
#define TTSWEEP_FRESNEL_UNREACHED 2 /* t_ab is INFINITY or a NaN: the pair has no cells */

/* The volume of every pair.  Every *_dev output is on the device, one entry per pair (lo_dev, hi_dev: three int32 per
 * pair); each may be NULL.                                                                       empty pair:
 *   t_ab_dev  float   t_ab                                                                       (as it is)
 *   count_dev int64   the number of cells with phi > 0                                           0
 *   lo_dev, hi_dev    the bounding box of those cells, inclusive                  (nx, ny, nz), (-1, -1, -1)
 *   phi_dev   double  Phi_r = ldexp((double)sum_x llrint(ldexp(phi_r(x), 60 - K_c)), -(60 - K_c))   0.0 */
int ttsweep_fresnel_volume_device(ttsweep_ctx *ctx, int nbox, const ttsweep_start *starts, const float *const *tt_dev,
                                  long long npair, const int *pair_a, const int *pair_b, const double *tau,
                                  const int *lo, const int *hi, int *status, float *t_ab_dev, long long *count_dev,
                                  int *lo_dev, int *hi_dev, double *phi_dev);

/* y = F m with F[r, x] = phi_r(x).  m_dev: device, double, FLOATBOX layout.  y_dev: device, double, npair entries.
 * S_m = 61 - E_m - K_c and y[r] = ldexp((double)sum_x llrint(ldexp(phi_r(x) * m[x], S_m)), -S_m).  Every m zero: y = 0
 * and S_m = 0.  scale: host, S_m, may be NULL.  With m = 1.0 everywhere y is phi_dev of the volume call bit for bit
 * (E_m = 1). */
int ttsweep_fresnel_forward_device(ttsweep_ctx *ctx, int nbox, const ttsweep_start *starts, const float *const *tt_dev,
                                   long long npair, const int *pair_a, const int *pair_b, const double *tau,
                                   const int *lo, const int *hi, const double *m_dev, double *y_dev, int *status,
                                   int *scale);

/* g = F^T w and hit counts.  w_dev: device, double, npair entries.  g_dev: device, double, FLOATBOX layout, written
 * (w_dev and g_dev both NULL: hit counts only; one without the other is refused unless npair == 0).  hits_dev:
 * device, int32, FLOATBOX layout: the number of pairs with phi_r(x) > 0, may be NULL.  scale: host, S_w, may be NULL.
 * S_w = 61 - E_w - K_p; the visit of cell x by pair r adds llrint(ldexp(w[r] * phi_r(x), S_w)) to an int64 accumulator,
 * which is g_dev itself as in ttsweep_ray_adjoint_device; then g[x] = ldexp((double)acc[x], -S_w).  Every weight zero:
 * g = 0 and S_w = 0. */
int ttsweep_fresnel_adjoint_device(ttsweep_ctx *ctx, int nbox, const ttsweep_start *starts, const float *const *tt_dev,
                                   long long npair, const int *pair_a, const int *pair_b, const double *tau,
                                   const int *lo, const int *hi, const double *w_dev, double *g_dev, int *hits_dev,
                                   int *status, int *scale);

/* Multi-GPU form of ttsweep_solve for a host program: the start points are
 * independent (serial_new/...:158-162; mpi/backup.c:351-363 runs one start per
 * rank), so the starts are dealt over the devices, longest first by estimated cost
 * (distance to the farthest grid corner), at most ceil(nstart / ndev) per device; every device gets its own
 * context and copy of the velocity volume, there is no communication while
 * sweeping, and each device writes its converged boxes straight into the caller's
 * host arrays.  devices may name the same GPU more than once.  Returns 1 / 0 / < 0
 * like ttsweep_solve.  (With the boxes resident in HBM the gather is a collective
 * instead: see bench.py / multistart.py, RCCL over xGMI.) */
int ttsweep_solve_multi(int ndev, const int *devices, int nx, int ny, int nz,
                        const ttsweep_fs *fs, int starstart, int starstop, const float *v_host,
                        int nstart, const ttsweep_start *starts, float *const *tt_host);
/* ... with the per-start outcome (ABI 6): changed[s] = 1 when a travel time of start s improved, 0 when its box was
 * at its fixed point already - what the reference's driver prints and sums as changed[s]
 * (serial_new/sweep-tt-multistart.c:158-164); changed may be NULL (then this is ttsweep_solve_multi). */
int ttsweep_solve_multi_changed(int ndev, const int *devices, int nx, int ny, int nz,
                                const ttsweep_fs *fs, int starstart, int starstop, const float *v_host,
                                int nstart, const ttsweep_start *starts, float *const *tt_host, int *changed);

/* The same with the result set RESIDENT ON A DEVICE - the step the reference's MPI version left as a TODO
 * (mpi/backup.c:381-386: "gather the ttboxes"; its CUDA version moves boxes between devices with peer copies,
 * cuda/cudasweep-tt-multistart.cu:359-369).  The starts are sharded over `devices` as above; every device
 * initialises and solves its shard in its own memory (fresh boxes: +INFINITY, 0 at the start), and the converged
 * boxes are gathered on devices[0], the root: tt_root[s] = device address ON THE ROOT of box s (nx*ny*nz floats,
 * allocated by the caller: the root holds the whole set - for result sets beyond its memory use ttsweep_solve_multi,
 * whose boxes live in host memory).  The root's own starts are solved in their slots.  The gather is ONE group of
 * ncclSend / ncclRecv pairs (RCCL over xGMI: one communicator per listed device, ncclCommInitAll; librccl is
 * loaded at run time) or - where RCCL is missing, refuses the list (a device listed twice) or fails - peer copies
 * (hipMemcpyPeerAsync).  flags: TTSWEEP_MULTI_*.  changed (may be NULL): per start, as ttsweep_get_changed.
 * gather_path (may be NULL): TTSWEEP_GATHER_*.  Returns 1 / 0 / < 0 like ttsweep_solve. */
#define TTSWEEP_MULTI_LOOPBACK 1    /* testing aid: the root's own boxes travel too (a send to itself) - the collective
                                       path then runs on a single device */
#define TTSWEEP_MULTI_NO_RCCL  2    /* peer copies even where RCCL is available */
#define TTSWEEP_GATHER_NONE 0       /* every box was solved on the root */
#define TTSWEEP_GATHER_RCCL 1
#define TTSWEEP_GATHER_PEER 2
int ttsweep_solve_multi_device(int ndev, const int *devices, int nx, int ny, int nz, const ttsweep_fs *fs, int starstart,
                               int starstop, const float *v_host, int nstart, const ttsweep_start *starts,
                               float *const *tt_root, int flags, int *changed, int *gather_path);

/* One-call drop-in for the reference's
 *   int sweepXYZ(int nx,int ny,int nz,int s,int starstart,int starstop)  (:198)
 * with the globals it reads passed explicitly: v = vbox.box.flat,
 * tt = ttboxes[s].flat, fs = fs, (si,sj,sk) = start[s].  Runs to convergence
 * on device 0 and returns > 0 if anything improved, 0 if not (so the
 * reference driver loop terminates after the next call), < 0 on error.
 * Creates and destroys a context per call; use the context API for batches. */
int ttsweep_sweepXYZ(const float *v, float *tt, int nx, int ny, int nz,
                     const ttsweep_fs *fs, int starstart, int starstop,
                     int si, int sj, int sk);

/* ---- host-only helpers (no device needed; used by the CPU test tier) ---- */
/* Build the pull form of the star: fills up to cap entries of
 * (di,dj,dk,flags,h) and returns the entry count (also when cap is too
 * small), < 0 on error.  flags bit0: live unless the centre cell is the
 * start; bit1: live unless the neighbour is the start. */
typedef struct ttsweep_pull_entry {
    int di, dj, dk;
    int flags;
    float h;        /* d/2, so delay = h * (v[c] + v[o]) */
} ttsweep_pull_entry;
int ttsweep_build_pull_star(const ttsweep_fs *fs, int starstart, int starstop,
                            ttsweep_pull_entry *out, int cap);

/* In-bounds (cell, offset) pairs of one reference pass: the closed form
 * sum over l in [starstart,starstop) of prod_axis max(n_axis - |off|, 0). */
long long ttsweep_relaxations_per_sweep(int nx, int ny, int nz, const ttsweep_fs *fs,
                                        int starstart, int starstop);

#ifdef __cplusplus
}
#endif

#endif /* TTSWEEP_H */
