"""Shared cases of the STRIP kernel's schedule tests (test_gpu_parity.py, test_gpu_strip_schedules.py): the option
sets, the two grids whose units have neighbours on every axis, a host-side mirror of the library's layout rule, and
the helpers that make fresh boxes, set options and damage converged boxes (shared with test_gpu_strip_stars.py).
Plain module: no test lives here."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCHEDULES = [
    # (one launch per solve?, {option: value}) - every knob that decides WHEN a unit is relaxed or told
    (1, {}),
    (1, {"OPT_ASYNC_POLICY": 0}),
    (1, {"OPT_ASYNC_POLICY": 0, "OPT_ASYNC_LOW": 1, "OPT_ASYNC_HIGH": 2}),
    (1, {"OPT_ASYNC_POLICY": 1, "OPT_ASYNC_GATE_MILLI": 100, "OPT_ASYNC_LOW": 200, "OPT_ASYNC_HIGH": 4000}),
    (1, {"OPT_ASYNC_POLICY": 1, "OPT_ASYNC_GATE_MILLI": 20000, "OPT_ASYNC_SPECIAL": 1}),
    (1, {"OPT_ASYNC_POLICY": 2, "OPT_ASYNC_WINDOW_MILLI": 3000, "OPT_ASYNC_SPECIAL": 1 << 20}),
    (1, {"OPT_ASYNC_POLICY": 2, "OPT_ASYNC_WINDOW_MILLI": 0}),
    (1, {"OPT_DEFER_MARGIN_MILLI": -1000000000}),
    (1, {"OPT_DEFER_MARGIN_MILLI": -4000}),
    (1, {"OPT_DEFER_MARGIN_MILLI": 0, "OPT_GATE_SPEED_MILLI": 0}),
    (1, {"OPT_DEFER_MARGIN_MILLI": 6000, "OPT_PAIR_MIN_STARTS": 0}),
    (1, {"OPT_ASYNC_INUNIT": 0}),
    (1, {"OPT_ASYNC_INUNIT": 1, "OPT_PAIR_MIN_STARTS": 0}),
    (1, {"OPT_ASYNC_INUNIT": 8, "OPT_DEFER_MARGIN_MILLI": 1000}),
    (1, {"OPT_ASYNC_INUNIT": 3, "OPT_PAIR_MIN_STARTS": 0, "OPT_ASYNC_POLICY": 0}),
    # direct hand-off (round 5): workers publish successor units (1), their own unit (2), both; with every ring policy
    # that allows it, a tiny ring fill, no gate, eager deferral, in-unit passes, one- and two-plane units
    (1, {"OPT_ASYNC_HANDOFF": 1}),
    (1, {"OPT_ASYNC_HANDOFF": 2}),
    (1, {"OPT_ASYNC_HANDOFF": 3}),
    (1, {"OPT_ASYNC_HANDOFF": 3, "OPT_PAIR_MIN_STARTS": 0}),
    (1, {"OPT_ASYNC_HANDOFF": 3, "OPT_ASYNC_POLICY": 0, "OPT_ASYNC_LOW": 1, "OPT_ASYNC_HIGH": 2}),
    (1, {"OPT_ASYNC_HANDOFF": 3, "OPT_GATE_SPEED_MILLI": 0, "OPT_DEFER_MARGIN_MILLI": -4000}),
    (1, {"OPT_ASYNC_HANDOFF": 1, "OPT_ASYNC_GATE_MILLI": 100, "OPT_ASYNC_GATE_FAST_MILLI": 100, "OPT_ASYNC_INUNIT": 2}),
    (1, {"OPT_ASYNC_HANDOFF": 3, "OPT_ASYNC_SPECIAL": 1, "OPT_DEFER_MARGIN_MILLI": -1000000000, "OPT_QUEUES": 1}),
    (1, {"OPT_ASYNC_HANDOFF": 3, "OPT_ASYNC_POLICY": 2, "OPT_ASYNC_WINDOW_MILLI": 3000}),     # (policy 2: hand-off stays off)
    # the latency instance (round 5): a unit relaxed by eight waves, four slabs in flight (one-plane units only: with
    # units of two planes the option is ignored)
    (1, {"OPT_ASYNC_WAVES": 8}),
    (1, {"OPT_ASYNC_WAVES": 8, "OPT_ASYNC_INUNIT": 2}),
    (1, {"OPT_ASYNC_WAVES": 8, "OPT_ASYNC_HANDOFF": 3, "OPT_ASYNC_INUNIT": 3, "OPT_DEFER_MARGIN_MILLI": 0}),
    (1, {"OPT_ASYNC_WAVES": 8, "OPT_ASYNC_POLICY": 0, "OPT_ASYNC_LOW": 1, "OPT_ASYNC_HIGH": 2, "OPT_ASYNC_SPECIAL": 1}),
    (1, {"OPT_ASYNC_WAVES": 8, "OPT_PAIR_MIN_STARTS": 0}),
    (1, {"OPT_ASYNC_WAVES": 4, "OPT_PAIR_MIN_STARTS": 1000000}),
    (0, {"OPT_DEFER_MARGIN_MILLI": -1000000000}),
    (0, {"OPT_DEFER_MARGIN_MILLI": -4000}),
    (0, {"OPT_DEFER_MARGIN_MILLI": 0, "OPT_PAIR_MIN_STARTS": 0}),
    (0, {"OPT_DEFER_MARGIN_MILLI": 3000, "OPT_GATE_SPEED_MILLI": 700}),
]

# The comment groups of SCHEDULES by position: the planners' knobs, direct hand-off, the latency instance; the
# launch-pair-per-pass entries close the list.  check_schedule_groups() holds the positions to the entries.
SCHEDULE_GROUPS = {"planner": range(0, 15), "handoff": range(15, 24), "latency": range(24, 30), "passes": range(30, 34)}


def schedule_id(one_launch, options):
    return f"{one_launch}-{'-'.join(f'{k[4:]}={v}' for k, v in options.items()) or 'defaults'}"


def check_schedule_groups():
    assert sorted(i for r in SCHEDULE_GROUPS.values() for i in r) == list(range(len(SCHEDULES)))
    for name, rng in SCHEDULE_GROUPS.items():
        for i in rng:
            one_launch, o = SCHEDULES[i]
            assert one_launch == (name != "passes"), (name, i)
            assert ("OPT_ASYNC_HANDOFF" in o) == (name == "handoff") or name == "latency", (name, i)
            assert ("OPT_ASYNC_WAVES" in o) == (name == "latency"), (name, i)


def fresh_boxes(shape, starts):
    """One box per start as the reference initialises it: INFINITY, 0 at the start."""
    tts = []
    for st in np.asarray(starts).reshape(-1, 3):
        tt = np.full(shape, np.inf, dtype=np.float32)
        tt[tuple(st)] = 0
        tts.append(tt)
    return tts


def set_options(P, sol, one_launch, options, kernel=None):
    """The options of one schedule on a context that has no velocity yet: the kernel when forced, the driver
    (OPT_ASYNC: one launch per solve, or a launch pair per pass), then every knob of the entry."""
    if kernel is not None:
        sol.set_option(P.OPT_KERNEL, kernel)
    if one_launch is not None:
        sol.set_option(P.OPT_ASYNC, one_launch)
    for key, value in options.items():
        sol.set_option(getattr(P, key), value)


# ---------------------------------------------------------------------------
# the layout rule of the STRIP kernel, restated (make_layout_strip in csrc/ttsweep_plan.cpp)
# ---------------------------------------------------------------------------

def strip_constants():
    """(STRIP_K, STRIP_TB) as csrc/ttsweep_dev.h defines them: cells of a strip, lanes of a lane tile."""
    text = open(os.path.join(ROOT, "uoparallel-seismic-project_amd", "csrc", "ttsweep_dev.h")).read()
    out = []
    for name in ("STRIP_K", "STRIP_TB"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, f"{name} not found in ttsweep_dev.h"
        out.append(int(m.group(1)))
    return tuple(out)


class StripLayout:
    """Which user axis becomes the plane axis a, the lane axis b and the strip axis c, and what follows from it."""

    def __init__(self, shape):
        K, TB = strip_constants()
        n = [int(x) for x in shape]

        def util(m, q):
            return m / float(((m + q - 1) // q) * q)

        bax = -1
        for d in range(3):
            if n[d] <= TB and (bax < 0 or n[d] > n[bax]):
                bax = d
        if bax < 0:
            bax = 0
            for d in (1, 2):
                if util(n[d], TB) > util(n[bax], TB) + 1e-12:
                    bax = d
        rest = [d for d in range(3) if d != bax]
        cax, aax = rest[1], rest[0]
        if util(n[rest[0]], K) > util(n[rest[1]], K) + 1e-12:
            cax, aax = rest[0], rest[1]
        self.K, self.TB = K, TB
        self.aax, self.bax, self.cax = aax, bax, cax
        self.planes, self.nb, self.nc = n[aax], n[bax], n[cax]
        self.btiles = (self.nb + TB - 1) // TB
        self.cstrips = (self.nc + K - 1) // K
        self.last_tile_lanes = self.nb - (self.btiles - 1) * TB
        self.last_strip_cells = self.nc - (self.cstrips - 1) * K

    def units(self, planes_per_unit):
        return ((self.planes + planes_per_unit - 1) // planes_per_unit) * self.btiles * self.cstrips

    def block(self, a, b, c):
        """Index of the user's box for slices given along (a, b, c)."""
        idx = [None, None, None]
        idx[self.aax], idx[self.bax], idx[self.cax] = a, b, c
        return tuple(idx)


MAIN_SHAPE = (65, 66, 67)
SECOND_SHAPE = (40, 33, 70)
SEED = 501


def check_layouts():
    """The conditions the schedule tests stand on; a change of STRIP_K, STRIP_TB or the layout rule that breaks one
    of them fails here instead of turning the tests vacuous."""
    m = StripLayout(MAIN_SHAPE)
    assert (m.aax, m.bax, m.cax) == (0, 2, 1), "main grid: a = the 65-axis, b = the 67-axis, c = the 66-axis"
    assert m.btiles >= 2 and 0 < m.last_tile_lanes < m.TB, "main grid: at least 2 lane tiles, the last one ragged"
    assert m.cstrips >= 2 and 0 < m.last_strip_cells < m.K, "main grid: at least 2 strips, the last one ragged"
    assert m.planes % 2 == 1, "main grid: an odd plane count (the last two-plane unit owns one plane)"
    assert (m.btiles, m.last_tile_lanes, m.cstrips, m.last_strip_cells, m.planes) == (2, 3, 5, 2, 65)
    assert (m.units(1), m.units(2)) == (650, 330)
    s = StripLayout(SECOND_SHAPE)
    assert (s.aax, s.bax, s.cax) == (1, 0, 2), "second grid: a = the 33-axis, b = the 40-axis, c = the 70-axis"
    assert s.btiles == 1 and s.last_tile_lanes == 40 and s.cstrips == 5 and s.planes == 33
    return m, s


def star_offsets():
    """The random star of both grids: reach 7 on every axis, asymmetric."""
    offs = np.random.default_rng(SEED).integers(-7, 8, (60, 3)).astype(np.int32)
    return offs[np.any(offs != 0, axis=1)]


def check_star(offs):
    """Reach 7 on every axis; entries that are live in one direction only (the library relaxes fs[0 .. n-2]: the
    reference's exclusive bound), so that the pull star has forward-only and reverse-only entries and dead-edge
    cells exist."""
    live = {tuple(int(x) for x in o) for o in offs[:-1]}
    assert np.abs(offs[:-1]).max(axis=0).tolist() == [7, 7, 7]
    fwd_only = [o for o in live if tuple(-x for x in o) not in live]
    assert fwd_only, "the star is symmetric: no forward-only / reverse-only pull entries"
    return len(fwd_only)


def main_starts():
    """11 starts on the main grid: the centre, both extreme corners, one inside the ragged lane tile, one inside the
    ragged strip, one on the last plane, a duplicate, four seeded random ones.  Batches: [:3], [:8], all."""
    m = StripLayout(MAIN_SHAPE)
    rng = np.random.default_rng(SEED + 1)
    fixed = [(32, 33, 33), (0, 0, 0), (64, 65, 66),
             m.block(20, (m.btiles - 1) * m.TB + 1, 10),            # inside the last lane tile
             m.block(40, 20, (m.cstrips - 1) * m.K),                # inside the last strip
             m.block(m.planes - 1, 5, 30)]                          # on the last plane
    fixed.append(fixed[3])                                          # a duplicate
    rnd = np.stack([rng.integers(0, n, size=4) for n in MAIN_SHAPE], axis=1)
    return np.array(fixed + [tuple(r) for r in rnd], dtype=np.int32)


def second_starts():
    return np.array([(20, 16, 35), (0, 0, 0), (39, 32, 69), (5, 30, 66)], dtype=np.int32)


def velocity(shape):
    return np.random.default_rng(SEED).uniform(0.1, 0.5, size=shape).astype(np.float32)


INF = np.float32(np.inf)


def damage_to_infinity(grid, box, start):
    """INFINITY in a 5x5x5 block across the lane-tile boundary, in one across a strip boundary, in the whole last
    plane and in the ragged lane tile; the start keeps its 0."""
    L = grid.layout
    tile, strip = (L.btiles - 1) * L.TB, 2 * L.K
    box[L.block(slice(30, 35), slice(tile - 2, tile + 3), slice(20, 25))] = INF
    box[L.block(slice(10, 15), slice(10, 15), slice(strip - 2, strip + 3))] = INF
    box[L.block(slice(L.planes - 1, L.planes), slice(None), slice(None))] = INF
    box[L.block(slice(None), slice(tile, L.nb), slice(None))] = INF
    box[tuple(start)] = 0
    return box


def oracle_boxes(oracle, v, offs, starts, tts=None):
    """oracle.converge(order=1) per start (from the boxes tts when given), a few at a time: the checker runs
    outside the interpreter lock."""
    fs = oracle.make_star(offs)
    starts = np.asarray(starts).reshape(-1, 3)

    def one(s):
        tt = None if tts is None else np.ascontiguousarray(tts[s], dtype=np.float32).copy()
        return oracle.converge(v, fs, starts[s], order=1, tt=tt)[0]

    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(one, range(len(starts))))
