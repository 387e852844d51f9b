// driver_rules.h - decisions of the solve drivers (ttsweep_driver.cpp) that need nothing but their arguments: no device,
// no context, no HIP header.  The limits of the device code (ttsweep_dev.h: ASYNC_RING_STARTS, STRIP_TB, ...) arrive as
// arguments, so that a plain C++ program can exercise every rule under the sanitizers (tests/host/driver_rules_main.cpp).
// (When the caller's boxes are in step with the padded volumes, and when the copy back may be left out: strip_rules.h.)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ttsweep {

// ---- STRIP: unit size and instance of a solve -----------------------------------------------------------------------
// (units1: the one-plane units of one start; an option >= 0 overrides the rule it stands in front of)

// Units of two planes when there are starts enough to fill the machine with them.
// (measured crossovers on 241x241x51: the pass driver from 21 starts on, the one-launch driver - whose shorter units
// pay the same claim and completion - from about 10: 8 starts 14.7 (one plane) / 15.7 ms (two), 12 starts 24.1 / 22.8,
// 16 starts 28.5 / 26.3, 24 starts 42.1 / 36.9)
inline bool use_plane_pairs(int pair_min_starts, long long pair_min_units, bool one_launch_allowed, int nstart, int units1)
{
    if (pair_min_starts >= 0) return nstart >= pair_min_starts;
    return (long long)nstart * units1 >= (one_launch_allowed ? pair_min_units / 2 : pair_min_units);
}

// The latency instance (one-plane units relaxed by all eight waves of a CU, ttsweep_kernels.hip): for solves that
// offer too few units to fill the machine anyway - what bounds them is how long a hop of the front takes.
// (fits: the solve runs one-plane units and the instance's resident grid holds the planners)
inline bool use_latency_instance(bool fits, int waves_option, int waves_lat, long long lat_max_units, int nstart, int units1)
{
    return fits && (waves_option >= 0 ? waves_option == waves_lat : (long long)nstart * units1 < lat_max_units);
}

// A unit that improved is relaxed again against its own planes, at once (measured: 24 starts 34.5 -> 29.4 ms with
// two such passes - the planner hands out a third less -, 3 starts 7.85 -> 7.77, one start 6.38 -> 6.52:
// profiles/r04_inunit.txt)
// (the latency instance: none - its units come round again faster than a pass over their own planes pays:
// 3 starts 7.24 -> 7.13 ms, 1 start 5.16 -> 5.02, profiles/r05_lat_8shares_g3.txt)
inline int inunit_passes(int inunit_option, bool lat, int nstart)
{
    return inunit_option >= 0 ? inunit_option : (lat ? 0 : (nstart >= 2 ? 2 : 0));
}

// Direct hand-off (ttsweep_dev.h, ASYNC_HANDOFF_*): for solves that cannot fill the machine - what bounds them is
// how fast good values travel from unit to unit, and every hop through the planner's scan costs a round of it.
// Every unit of a ring can sit in it at once (taken by a worker, not yet claimed): the rings must hold that.
inline int handoff_bits(int policy, long long longest_ring, int ring_starts_max, int cap, int handoff_option,
                        long long handoff_max_units, int handoff_default, int nstart, int units1)
{
    const bool can = (policy == 1 || policy == 0) && longest_ring + 2 * ring_starts_max <= cap / 2;
    const int want = handoff_option >= 0 ? handoff_option : ((long long)nstart * units1 < handoff_max_units ? handoff_default : 0);
    return can ? want : 0;
}

// ---- STRIP: the rings of a one-launch solve -------------------------------------------------------------------------

// The starts are dealt over at most one ring per XCD.  (0 for a solve without starts: use_async() takes that for 1.)
inline int ring_count(int nstart, int nlists, int max_rings) { return std::min(std::min(nstart, nlists), max_rings); }
inline int starts_per_ring(int nstart, int nrings) { return (nstart + nrings - 1) / nrings; }

// Fill marks of a ring: half / twice its workers where the units of a ring are a few thousand (241 x 241 x 51 x 24:
// 5.8 k per ring - fuller rings relax MORE there: 27.9 / 28.3 / 29.3 / 31.1 ms with 126 / 256 / 512 / 1024); on the
// grids that leave the caches the front is thousands of units wide and a fuller ring is less work and less time
// (512 x 512 x 256 x 8, 33 k units per ring: 288 / 276 / 273 / 269 / 264 / 258 ms with 126 / 256 / 512 / 1024 / 2048 /
// 4096; 1024 x 1024 x 512 x 14: 3.95 -> 3.83 s with 1024) - profiles/r05_big_grid_ring_marks.txt
struct RingMarks { int low, high; };
inline RingMarks ring_marks(int nstart, int nunits, int nrings, int nblocks, int cap, int low_option, int high_option)
{
    const int workers = std::max((nblocks - nrings) / nrings, 1);
    const long long units_per_ring = (long long)nstart * nunits / std::max(nrings, 1);
    const int high0 = units_per_ring >= 16384 ? std::min(4096, cap / 4) : 2 * workers;
    RingMarks m;
    m.low = low_option > 0 ? low_option : std::max(units_per_ring >= 16384 ? high0 / 4 : workers / 2, 8);
    m.high = high_option > 0 ? high_option : high0;
    m.high = std::max(m.high, m.low + 1);
    return m;
}

// list entries in front of the first unit with anything to do that a round of the planner's scan still looks at
inline int ring_scan_slack(int nstart, int nrings) { return 16384 * starts_per_ring(nstart, nrings); }

// entries a ring may publish before the solve counts as not converging
inline long long ring_max_entries(long long max_sweeps, long long longest_ring)
{
    return (long long)std::min<double>((double)max_sweeps * (double)longest_ring, 2.0e9);
}

// The unit grid of one start and where the start lies in it (device axes; tb, k: STRIP_TB, STRIP_K).
struct UnitGrid { int np, n1, btiles, cstrips, tb, k; };
struct StartCell { int sa, sb, sc; };

// Squared distance (cells) from the start to the unit's cells, as float bits: what the planner's gate compares
// (plan_pass_kernel measures the same box).
inline int unit_gate_d2_bits(const UnitGrid &g, const StartCell &at, int unit)
{
    const int cs = unit % g.cstrips, bt = (unit / g.cstrips) % g.btiles, a0 = g.np * (unit / (g.cstrips * g.btiles));
    const int b0 = bt * g.tb, cb0 = cs * g.k, tb_eff = std::min(g.tb, g.n1);
    const float da = (float)std::max(std::max(a0 - at.sa, at.sa - (a0 + g.np - 1)), 0);
    const float db = (float)std::max(std::max(b0 - at.sb, at.sb - (b0 + tb_eff - 1)), 0);
    const float dc = (float)std::max(std::max(cb0 - at.sc, at.sc - (cb0 + g.k - 1)), 0);
    const float d2 = da * da + db * db + dc * dc;
    int bits;
    memcpy(&bits, &d2, sizeof bits);
    return bits;
}

// The rings' lists: ring r serves the starts r, r + nrings, ... (ring_starts[ring_start_off[r] .. [r + 1])); its list
// flat[ring_off[r] .. + ring_len[r]) holds every unit of those starts, each start's nearest first (unit_order), the
// starts interleaved rank by rank.  An entry is the int4 the kernel reads (AsyncSolve::list).
struct RingListEntry { int start_rank, unit, d2_bits, zero; };     // start | rank in its ring << 16
struct RingLists {
    std::vector<RingListEntry> flat;
    std::vector<int> ring_starts, ring_off, ring_len, ring_start_off;  // (nrings, nrings, nrings + 1 offsets)
};
// Returns nullptr, or why the lists cannot be made.
inline const char *build_ring_lists(int nstart, int nrings, int ring_starts_max, int nunits, const UnitGrid &g,
                                    const std::vector<StartCell> &at, const std::vector<std::vector<int>> &unit_order,
                                    RingLists &out)
{
    out = RingLists{};
    out.flat.reserve((size_t)nstart * nunits);
    for (int r = 0; r < nrings; r++) {
        out.ring_off.push_back((int)out.flat.size());
        out.ring_start_off.push_back((int)out.ring_starts.size());
        std::vector<int> mine;
        for (int a = r; a < nstart; a += nrings) mine.push_back(a);
        if ((int)mine.size() > ring_starts_max) return "too many starts for a one-launch solve";
        for (int a : mine) out.ring_starts.push_back(a);
        for (int k = 0; k < nunits; k++)
            for (size_t i = 0; i < mine.size(); i++) {
                const int unit = unit_order[mine[i]][k];
                out.flat.push_back({mine[i] | ((int)i << 16), unit, unit_gate_d2_bits(g, at[mine[i]], unit), 0});
            }
        out.ring_len.push_back((int)out.flat.size() - out.ring_off[r]);
    }
    out.ring_start_off.push_back((int)out.ring_starts.size());
    return nullptr;
}

// ---- TILE: claim sequences of the column driver, resident grids -----------------------------------------------------

// Claim sequences in use: one per XCD, no more than tile positions along a.
inline int column_sequences(int NI, int nlists, int max_seqs)
{
    int nseq = std::min(max_seqs, NI);
    if (nlists >= 1 && nlists < nseq) nseq = nlists;
    return nseq;
}

// Sequence x: the positions (I', J') with I' % nseq == x in the order of the sweep: by level I' + J', then by I';
// tab holds them as I' | J' << 16, sequence x from seq_off[x] on.
inline void column_sequence_table(int NI, int NJ, int nseq, std::vector<int> &tab, int *seq_off, int *seq_len)
{
    tab.clear();
    tab.reserve((size_t)NI * NJ);
    for (int x = 0; x < nseq; x++) {
        seq_off[x] = (int)tab.size();
        for (int lev = 0; lev <= NI + NJ - 2; lev++)
            for (int ip = x; ip < NI; ip += nseq) {
                const int jp = lev - ip;
                if (jp >= 0 && jp < NJ) tab.push_back(ip | (jp << 16));
            }
        seq_len[x] = (int)tab.size() - seq_off[x];
    }
}

// A resident grid: no more workgroups than the device holds at once (cap) or than there is work for (wanted), in whole
// rounds of the XCDs / claim sequences, at least one round.
inline long long resident_grid(long long cap, long long wanted, int round)
{
    return std::max<long long>(std::min(cap, wanted) / round, 1) * round;
}

// TILE pass: workgroups per XCD that take candidates - coprime to the number of active starts, so that one start's
// tiles at consecutive positions go to different workgroups (tile_candidate)
inline int tile_wstride(int per_xcd, int nactive)
{
    auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
    int wstride = per_xcd;
    while (wstride > 1 && gcd(wstride, nactive) != 1) wstride--;
    return wstride;
}

// ---- the one-launch drivers: wall-clock limit, what the column kernel can address -----------------------------------

// Every wait inside a one-launch solve gives up after this much wall clock (100 MHz ticks): ten seconds plus twenty
// times what the solve should take (expect_s: the caller's estimate at a fraction of the machine's rate) - a protocol
// error must not hang the device.  A limit in milliseconds (TTSWEEP_OPT_ASYNC_TIMEOUT_MILLI) > 0 replaces it.
inline long long wait_limit_ticks(double expect_s, int limit_ms)
{
    if (limit_ms > 0) return (long long)limit_ms * 100000ll;
    return (long long)((10.0 + 20.0 * expect_s) * 1.0e8);
}

// The column kernel's staging instructions address a column's rows with 32-bit byte offsets: nine rows and nine
// planes of floats (strides s1, s0) and a line beyond them have to fit.
inline bool column_offsets_fit(long long s0, long long s1) { return (9 * s0 + 9 * s1) * 4 + 64 < 0x7fffffffLL; }

// Can the column driver relax the travel times in the caller's own arrays (no padded copy, no copy back)?  Their rows
// have to be whole tiles long (tile_z cells) and 64-byte aligned.
inline bool column_rows_in_place(int n1, int n2, int tile_z, float *const *tt_dev, int nstart)
{
    if (n2 % tile_z || !column_offsets_fit((long long)n1 * n2, n2)) return false;
    for (int s = 0; s < nstart; s++)
        if (!tt_dev[s] || (reinterpret_cast<uintptr_t>(tt_dev[s]) & 63u)) return false;
    return true;
}

} // namespace ttsweep
