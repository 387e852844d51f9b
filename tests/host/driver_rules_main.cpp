// driver_rules_main.cpp - exercises the host-side rules of the solve drivers (csrc/driver_rules.h) on the CPU; built
// with -fsanitize=address,undefined by tests/test_driver_rules_cpu.py.  Every rule is stated here by its properties,
// not by the loops of the header.  Exit status 0: every check held.
#include "driver_rules.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <set>
#include <string>
#include <utility>
#include <vector>

using namespace ttsweep;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

// the device code's limits (ttsweep_dev.h), as the driver passes them
static const int TB = 64, K = 16, RING_STARTS = 32, MAX_RINGS = 8, COL_SEQS = 8, CAP = 1 << 14;

static int float_bits(float f) { int b; memcpy(&b, &f, sizeof b); return b; }

static UnitGrid unit_grid(int np, int n0, int n1, int n2, int *nunits)
{
    const UnitGrid g{np, n1, (n1 + TB - 1) / TB, (n2 + K - 1) / K, TB, K};
    *nunits = ((n0 + np - 1) / np) * g.btiles * g.cstrips;
    return g;
}

// the least squared distance from the start to a cell of the unit's box, cell by cell
static int brute_d2_bits(const UnitGrid &g, const StartCell &at, int a_group, int bt, int cs)
{
    long long best = LLONG_MAX;
    const int width = g.n1 < g.tb ? g.n1 : g.tb;
    for (int a = a_group * g.np; a < (a_group + 1) * g.np; a++)
        for (int b = bt * g.tb; b < bt * g.tb + width; b++)
            for (int c = cs * g.k; c < (cs + 1) * g.k; c++) {
                const long long d = (long long)(a - at.sa) * (a - at.sa) + (long long)(b - at.sb) * (b - at.sb)
                                  + (long long)(c - at.sc) * (c - at.sc);
                if (d < best) best = d;
            }
    return float_bits((float)best);
}

static void check_gate_distance()
{
    int nunits;
    {   // 4 x 130 x 48, one-plane units: 3 lane tiles (the last one ragged), 3 strips
        const UnitGrid g = unit_grid(1, 4, 130, 48, &nunits);
        CHECK(nunits == 4 * 3 * 3);
        const StartCell at{1, 70, 20};
        auto unit = [&](int a, int bt, int cs) { return (a * g.btiles + bt) * g.cstrips + cs; };
        CHECK(unit_gate_d2_bits(g, at, unit(1, 1, 1)) == float_bits(0.f));          // the unit that holds the start
        CHECK(unit_gate_d2_bits(g, at, unit(2, 1, 1)) == float_bits(1.f));          // one off along a
        CHECK(unit_gate_d2_bits(g, at, unit(0, 1, 1)) == float_bits(1.f));
        CHECK(unit_gate_d2_bits(g, at, unit(1, 0, 1)) == float_bits(49.f));         // along b: cells 0..63, 7 away
        CHECK(unit_gate_d2_bits(g, at, unit(1, 2, 1)) == float_bits(58.f * 58.f));  // cells 128.., 58 away
        CHECK(unit_gate_d2_bits(g, at, unit(1, 1, 0)) == float_bits(25.f));         // along c: cells 0..15, 5 away
        CHECK(unit_gate_d2_bits(g, at, unit(1, 1, 2)) == float_bits(144.f));        // cells 32..47, 12 away
        CHECK(unit_gate_d2_bits(g, at, unit(3, 0, 2)) == float_bits(4.f + 49.f + 144.f));
        for (int a = 0; a < 4; a++)
            for (int bt = 0; bt < 3; bt++)
                for (int cs = 0; cs < 3; cs++) CHECK(unit_gate_d2_bits(g, at, unit(a, bt, cs)) == brute_d2_bits(g, at, a, bt, cs));
    }
    {   // n[1] = 40 < STRIP_TB: the one lane tile is ragged, its last live lane is 39; two-plane units
        const UnitGrid g = unit_grid(2, 5, 40, 33, &nunits);
        CHECK(g.btiles == 1 && g.cstrips == 3 && nunits == 3 * 1 * 3);
        const StartCell at{4, 39, 32};
        auto unit = [&](int a, int cs) { return a * g.cstrips + cs; };
        CHECK(unit_gate_d2_bits(g, at, unit(2, 2)) == float_bits(0.f));
        CHECK(unit_gate_d2_bits(g, at, unit(1, 2)) == float_bits(1.f));             // planes 2, 3
        CHECK(unit_gate_d2_bits(g, at, unit(0, 2)) == float_bits(9.f));             // planes 0, 1
        CHECK(unit_gate_d2_bits(g, at, unit(2, 1)) == float_bits(1.f));             // cells 16..31
        for (int a = 0; a < 3; a++)
            for (int cs = 0; cs < 3; cs++) CHECK(unit_gate_d2_bits(g, at, unit(a, cs)) == brute_d2_bits(g, at, a, 0, cs));
    }
}

// nstart starts on a 5 x 70 x 40 grid, each with a unit order of its own (a permutation of all units)
static void check_ring_lists(int nstart, int nlists, bool refused)
{
    int nunits;
    const UnitGrid g = unit_grid(1, 5, 70, 40, &nunits);
    std::vector<StartCell> at(nstart);
    std::vector<std::vector<int>> order(nstart, std::vector<int>(nunits));
    for (int s = 0; s < nstart; s++) {
        at[s] = {s % 5, (7 * s) % 70, (11 * s) % 40};
        for (int k = 0; k < nunits; k++) order[s][k] = (7 * k + 3 * s) % nunits;   // (7 is coprime to the 30 units)
    }
    const int nrings = ring_count(nstart, nlists, MAX_RINGS);
    CHECK(nrings >= 1 && nrings <= nstart && nrings <= nlists && nrings <= MAX_RINGS);
    CHECK(nrings == nstart || nrings == nlists || nrings == MAX_RINGS);
    RingLists rl;
    const char *why = build_ring_lists(nstart, nrings, RING_STARTS, nunits, g, at, order, rl);
    CHECK((starts_per_ring(nstart, nrings) > RING_STARTS) == refused);
    if (refused) {
        CHECK(why && std::string(why) == "too many starts for a one-launch solve");
        return;
    }
    CHECK(why == nullptr);
    // the offsets and lengths tile the flat list and the list of starts
    CHECK((int)rl.ring_off.size() == nrings && (int)rl.ring_len.size() == nrings && (int)rl.ring_start_off.size() == nrings + 1);
    if ((int)rl.ring_off.size() != nrings || (int)rl.ring_len.size() != nrings || (int)rl.ring_start_off.size() != nrings + 1) return;
    CHECK(rl.ring_off[0] == 0 && rl.ring_start_off[0] == 0);
    for (int r = 0; r + 1 < nrings; r++) CHECK(rl.ring_off[r + 1] == rl.ring_off[r] + rl.ring_len[r]);
    CHECK(rl.ring_off[nrings - 1] + rl.ring_len[nrings - 1] == (int)rl.flat.size());
    CHECK(rl.ring_start_off[nrings] == (int)rl.ring_starts.size() && (int)rl.ring_starts.size() == nstart);
    CHECK(rl.flat.size() == (size_t)nstart * nunits);
    std::set<std::pair<int, int>> seen;
    for (int r = 0; r < nrings; r++) {
        // ring r holds exactly the starts = r (mod nrings), in rising order
        const int m = rl.ring_start_off[r + 1] - rl.ring_start_off[r];
        CHECK(m == (nstart - r + nrings - 1) / nrings && m <= RING_STARTS);
        CHECK(rl.ring_len[r] == m * nunits);
        for (int i = 0; i < m; i++) CHECK(rl.ring_starts[rl.ring_start_off[r] + i] == r + i * nrings);
        // entry k m + i is rank i's k-th unit of its order
        for (int e = 0; e < rl.ring_len[r]; e++) {
            const RingListEntry &x = rl.flat[rl.ring_off[r] + e];
            const int start = x.start_rank & 0xffff, rank = x.start_rank >> 16;
            CHECK(rank == e % m && start == rl.ring_starts[rl.ring_start_off[r] + rank] && start % nrings == r);
            CHECK(x.unit == order[start][e / m]);
            CHECK(x.d2_bits == unit_gate_d2_bits(g, at[start], x.unit) && x.zero == 0);
            CHECK(seen.insert({start, x.unit}).second);     // every (start, unit) pair once
        }
    }
    CHECK(seen.size() == (size_t)nstart * nunits);
}

static void check_fill_marks()
{
    for (int nrings = 1; nrings <= MAX_RINGS; nrings++)
        for (int nblocks : {32, 33, 64, 256, 511, 512, 2048})
            for (int nstart : {1, 3, 24, 255})
                for (int nunits : {1, 30, 5000, 16384, 400000}) {
                    const RingMarks m = ring_marks(nstart, nunits, nrings, nblocks, CAP, 0, 0);
                    CHECK(m.high > m.low && m.low >= 8 && m.high <= CAP / 4);
                }
    // the overrides
    RingMarks m = ring_marks(3, 5000, 3, 512, CAP, 100, 300);
    CHECK(m.low == 100 && m.high == 300);
    m = ring_marks(3, 5000, 3, 512, CAP, 100, 0);
    CHECK(m.low == 100 && m.high == 2 * ((512 - 3) / 3));
    m = ring_marks(3, 5000, 3, 512, CAP, 0, 300);
    CHECK(m.low == ((512 - 3) / 3) / 2 && m.high == 300);
    m = ring_marks(3, 5000, 3, 512, CAP, 300, 100);       // (a high mark at or below the low one: the least above it)
    CHECK(m.low == 300 && m.high == 301);
    // either side of 16384 units per ring: by the workers below, fixed marks from there on
    m = ring_marks(1, 16383, 1, 512, CAP, 0, 0);
    CHECK(m.low == 255 && m.high == 1022);
    m = ring_marks(1, 16384, 1, 512, CAP, 0, 0);
    CHECK(m.low == 1024 && m.high == 4096);
    m = ring_marks(8, 16383, 8, 512, CAP, 0, 0);          // (per ring, not per solve)
    CHECK(m.low == 31 && m.high == 126);
    m = ring_marks(8, 16384, 8, 512, CAP, 0, 0);
    CHECK(m.low == 1024 && m.high == 4096);
    CHECK(ring_scan_slack(1, 1) == 16384 && ring_scan_slack(24, 8) == 3 * 16384 && ring_scan_slack(25, 8) == 4 * 16384);
    CHECK(ring_max_entries(100000, 5000) == 500000000ll && ring_max_entries(100000, 400000) == 2000000000ll);
    CHECK(ring_max_entries(LLONG_MAX, INT_MAX) == 2000000000ll);
}

static void check_column_table()
{
    const int shapes[5][2] = {{1, 1}, {1, 5}, {5, 1}, {3, 4}, {9, 2}};
    for (const auto &shape : shapes)
        for (int want : {1, 3, 8}) {
            const int NI = shape[0], NJ = shape[1];
            const int nseq = column_sequences(NI, want, COL_SEQS);      // (the XCDs of the device stand in for `want`)
            CHECK(nseq == std::min(std::min(want, NI), COL_SEQS));
            std::vector<int> tab;
            int off[COL_SEQS], len[COL_SEQS];
            column_sequence_table(NI, NJ, nseq, tab, off, len);
            CHECK((int)tab.size() == NI * NJ);
            std::set<int> seen;
            int next = 0;
            for (int x = 0; x < nseq; x++) {
                CHECK(off[x] == next && len[x] >= 0 && off[x] + len[x] <= (int)tab.size());
                if (off[x] != next || len[x] < 0 || off[x] + len[x] > (int)tab.size()) return;
                next += len[x];
                for (int e = 0; e < len[x]; e++) {
                    const int I = tab[off[x] + e] & 0xffff, J = tab[off[x] + e] >> 16;
                    CHECK(I < NI && J >= 0 && J < NJ && I % nseq == x);
                    CHECK(seen.insert(I * NJ + J).second);
                    if (e == 0) continue;
                    const int Ip = tab[off[x] + e - 1] & 0xffff, Jp = tab[off[x] + e - 1] >> 16;
                    CHECK(I + J > Ip + Jp || (I + J == Ip + Jp && I > Ip));     // by level, then by I
                }
            }
            CHECK(next == NI * NJ && (int)seen.size() == NI * NJ);
        }
    CHECK(column_sequences(40, 0, COL_SEQS) == COL_SEQS);       // (no census of the XCDs: all sequences)
}

static void check_grids()
{
    for (int round : {1, 3, 8})
        for (long long cap : {1ll, 7ll, 8ll, 256ll, 1024ll, 1030ll})
            for (long long wanted : {1ll, 5ll, 8ll, 9ll, 1000ll, 100000ll, 1ll << 40}) {
                const long long g = resident_grid(cap, wanted, round);
                CHECK(g > 0 && g % round == 0);
                CHECK(cap < round ? g == round : g <= cap);
                CHECK(g <= std::max<long long>(wanted, round));
                CHECK(g + round > std::min(cap, wanted));           // (the most whole rounds that fit)
            }
    for (int per_xcd = 1; per_xcd <= 130; per_xcd++)
        for (int nactive : {1, 2, 6, 24, 30, 255, 2310}) {
            const int w = tile_wstride(per_xcd, nactive);
            CHECK(w >= 1 && w <= per_xcd && std::gcd(w, nactive) == 1);
            for (int larger = w + 1; larger <= per_xcd; larger++) CHECK(std::gcd(larger, nactive) != 1);   // (the largest such)
        }
}

static void check_time_limit()
{
    // the drivers' estimates: STRIP (relaxations of a sweep x starts x 8 at 1e12 / s), columns (cells x starts x 12 bytes x
    // 40 sweeps at 2e12 / s)
    auto strip_s = [](double relax_per_sweep, int nstart) { return relax_per_sweep * nstart * 8.0 / 1.0e12; };
    auto column_s = [](double nx, double ny, double nz, int nstart) { return nx * ny * nz * nstart * 12.0 * 40.0 / 2.0e12; };
    CHECK(wait_limit_ticks(0.0, 0) == 1000000000ll);                // ten seconds of 100 MHz ticks
    CHECK(wait_limit_ticks(1.0, 0) == 3000000000ll);
    CHECK(wait_limit_ticks(1.0e9, 250) == 25000000ll && wait_limit_ticks(0.0, 1) == 100000ll);     // the override wins
    CHECK(wait_limit_ticks(0.0, INT_MAX) == (long long)INT_MAX * 100000ll);
    CHECK(wait_limit_ticks(5.0, -1) == wait_limit_ticks(5.0, 0));
    long long prev = 0;
    for (int n : {8, 64, 241, 512, 1024})
        for (int nstart : {1, 14, 255}) {
            const long long a = wait_limit_ticks(strip_s((double)n * n * (n / 2) * 818, nstart), 0);
            const long long b = wait_limit_ticks(column_s(n, n, n / 2, nstart), 0);
            CHECK(a >= 1000000000ll && b >= 1000000000ll);
            if (nstart == 1) { CHECK(a >= prev); prev = a; }
            CHECK(wait_limit_ticks(strip_s((double)n * n * (n / 2) * 818, nstart + 1), 0) >= a);
            CHECK(wait_limit_ticks(column_s(n + 1, n, n / 2, nstart), 0) >= b);
        }
    // 1024 x 1024 x 512 x 255 starts: hours, not an overflow
    const long long big = wait_limit_ticks(strip_s(1024.0 * 1024 * 512 * 818, 255), 0);
    CHECK(big > 1000000000ll && big < (1ll << 50));
    const long long bigc = wait_limit_ticks(column_s(1024, 1024, 512, 255), 0);
    CHECK(bigc > 1000000000ll && bigc < big);
}

static void check_choices()
{
    // unit size: the option first, else the supply of one-plane units (half the bar where the one-launch solve may run)
    CHECK(use_plane_pairs(4, 80000, true, 4, 1) && !use_plane_pairs(4, 80000, true, 3, 1000000));
    CHECK(use_plane_pairs(0, 80000, false, 1, 1));
    CHECK(!use_plane_pairs(-1, 80000, true, 9, 4444) && use_plane_pairs(-1, 80000, true, 9, 4445));
    CHECK(!use_plane_pairs(-1, 80000, false, 9, 8888) && use_plane_pairs(-1, 80000, false, 9, 8889));
    CHECK(use_plane_pairs(-1, 80000, false, 255, 1 << 30));                       // (no 32-bit product)
    // the latency instance
    CHECK(use_latency_instance(true, -1, 8, 12000, 3, 3999) && !use_latency_instance(true, -1, 8, 12000, 3, 4000));
    CHECK(!use_latency_instance(false, -1, 8, 12000, 1, 1) && !use_latency_instance(false, 8, 8, 12000, 1, 1));
    CHECK(use_latency_instance(true, 8, 8, 12000, 255, 1 << 30) && !use_latency_instance(true, 4, 8, 12000, 1, 1));
    // in-unit passes
    CHECK(inunit_passes(-1, false, 1) == 0 && inunit_passes(-1, false, 2) == 2 && inunit_passes(-1, true, 24) == 0);
    CHECK(inunit_passes(0, false, 24) == 0 && inunit_passes(3, true, 1) == 3);
    // hand-off: only where every unit of the longest ring fits into half a ring, and under policies 0 and 1
    CHECK(handoff_bits(1, CAP / 2 - 2 * RING_STARTS, RING_STARTS, CAP, -1, 12000, 3, 1, 100) == 3);
    CHECK(handoff_bits(1, CAP / 2 - 2 * RING_STARTS + 1, RING_STARTS, CAP, -1, 12000, 3, 1, 100) == 0);
    CHECK(handoff_bits(0, 100, RING_STARTS, CAP, 2, 12000, 3, 1, 100) == 2 && handoff_bits(2, 100, RING_STARTS, CAP, 2, 12000, 3, 1, 100) == 0);
    CHECK(handoff_bits(1, 100, RING_STARTS, CAP, -1, 12000, 3, 3, 3999) == 3 && handoff_bits(1, 100, RING_STARTS, CAP, -1, 12000, 3, 3, 4000) == 0);
    CHECK(handoff_bits(1, 100, RING_STARTS, CAP, 0, 12000, 3, 1, 1) == 0);
    // what the column kernel can address: (9 s0 + 9 s1) 4 + 64 < 2^31 - 1
    CHECK(column_offsets_fit(59652321 - 1, 1) && !column_offsets_fit(59652321, 1));       // s0 + s1 <= 59652321
    CHECK(!column_offsets_fit(1ll << 40, 1ll << 20));
    // in place: rows of whole tiles, every box there and 64-byte aligned
    alignas(64) static float box[64];
    std::vector<float *> boxes = {box, box + 16, box + 32};
    CHECK(column_rows_in_place(7, 64, 32, boxes.data(), 3) && column_rows_in_place(7, 32, 32, boxes.data(), 3));
    CHECK(!column_rows_in_place(7, 48, 32, boxes.data(), 3) && !column_rows_in_place(1 << 20, 64, 32, boxes.data(), 3));
    for (size_t bad = 0; bad < boxes.size(); bad++) {
        std::vector<float *> some = boxes;
        some[bad] = box + 1 + 16 * bad;
        CHECK(!column_rows_in_place(7, 64, 32, some.data(), 3));
        some[bad] = nullptr;
        CHECK(!column_rows_in_place(7, 64, 32, some.data(), 3));
        CHECK(column_rows_in_place(7, 64, 32, some.data(), (int)bad));
    }
}

int main()
{
    check_gate_distance();
    check_ring_lists(1, 8, false);
    check_ring_lists(3, 8, false);                      // fewer starts than rings available
    check_ring_lists(11, 4, false);                     // not a multiple of the rings
    check_ring_lists(29, 8, false);
    check_ring_lists(2 * RING_STARTS, 2, false);        // nrings x limit: accepted
    check_ring_lists(2 * RING_STARTS + 1, 2, true);     // one more: refused
    check_ring_lists(MAX_RINGS * RING_STARTS, 64, false);
    check_ring_lists(MAX_RINGS * RING_STARTS + 1, 64, true);
    check_fill_marks();
    check_column_table();
    check_grids();
    check_time_limit();
    check_choices();
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("driver rules ok\n");
    return failures ? 1 : 0;
}
