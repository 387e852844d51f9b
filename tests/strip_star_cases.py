"""Shared cases of the STRIP kernel's star tests (test_gpu_strip_stars.py, checked without a GPU by
test_strip_star_cases_cpu.py): fourteen stars that between them give the unit-queue relaxation kernel (kernel 2,
sweep_units_kernel) every plane reach ra in 0..7 and every lane reach rb in 1..7, ra != rb, staged planes without
items, planes with fewer items than waves and planes with items for all eight; the grids and starts they are solved
on; and the plan arithmetic of make_layout_strip / upload_strip_plan_np (csrc/ttsweep_plan.cpp) restated in Python
over the library's own pull star.  Plain module: no test lives here.

A star is written in the kernel's device axes - a the plane axis, b the lane axis, c the stride-1 strip axis - and
mapped to user axes through strip_cases.StripLayout(shape), so that a case means the same on any grid.  Every star
ends with a sacrificial entry: the library relaxes fs[0 .. n-2] (the reference's exclusive bound).

Two remarks on the cases:
  * flat_b keeps rb = 1 and one (da, db) column - one item - per non-empty staged plane of the one-plane plans, so
    that 3 of 4 and 7 of 8 waves have empty shares on every plane, but its offsets do move along b: every plane
    offset da comes with ONE lane offset db in {-1, 0, +1}.  With no db at all a box would never leave its start's
    lane row, and no start could have finite cells in both lane tiles (the start condition below).  The clamp
    rb = max(0, 1) of a star without any db is only_c's.
  * dup lists one offset twice with two LENGTHS (the second 1.5 times the first): build_pull_star merges listings of
    equal length, and the second (da, db) column of upload_strip_plan_np exists for exactly this.  The longer edge
    never wins a minimum; what the case sees is a plan that let the second listing's length replace the first's.

The start condition: every (case, start) in use has finite oracle cells in both lane tiles and in at least three
strips, and - where ra > 0 - in more than 2 ra + 2 planes.  only_c and single are exempt BY CONSTRUCTION: the first
never leaves the start's row of cells along c (one lane, one plane), the second walks one line of cells.  No other
case is exempt; a corner start that misses the condition is not used (Case.corner)."""
import numpy as np

import strip_cases as S

SEED = 733
SACRIFICIAL = (1, 1, 1)
PULL_FWD, PULL_REV = 1, 2


# ---------------------------------------------------------------------------
# constants of csrc/ttsweep_dev.h
# ---------------------------------------------------------------------------

def strip_plan_constants():
    """STRIP_MAX_RA, STRIP_CF, STRIP_NS, STRIP_NS_LAT, STRIP_NS_MAX, STRIP_PLANES as csrc/ttsweep_dev.h defines them."""
    import os
    import re
    text = open(os.path.join(S.ROOT, "uoparallel-seismic-project_amd", "csrc", "ttsweep_dev.h")).read()
    out = {}
    for name in ("STRIP_MAX_RA", "STRIP_CF", "STRIP_NS", "STRIP_NS_LAT", "STRIP_NS_MAX", "STRIP_PLANES"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, f"{name} not found in ttsweep_dev.h"
        out[name] = int(m.group(1))
    return out


def strip_supported(pull):
    """strip_supported (ttsweep_plan.cpp): a non-empty pull star of radius <= STRIP_MAX_RA and < STRIP_CF."""
    k = strip_plan_constants()
    radius = max([0] + [max(abs(e[0]), abs(e[1]), abs(e[2])) for e in pull])
    return len(pull) > 0 and radius <= k["STRIP_MAX_RA"] and radius < k["STRIP_CF"]


# ---------------------------------------------------------------------------
# stars, in device axes (da, db, dc)
# ---------------------------------------------------------------------------

def _distinct(offs):
    """Drop (0, 0, 0) and repeats, keep the order."""
    seen, out = set(), []
    for o in offs:
        o = tuple(int(x) for x in o)
        if o != (0, 0, 0) and o not in seen:
            seen.add(o)
            out.append(o)
    return out


def _random(seed, n, ra, rb, rc, first=()):
    """`first`, then seeded offsets with |da| <= ra, |db| <= rb, |dc| <= rc, n entries in all before repeats go."""
    rng = np.random.default_rng(SEED + seed)
    rnd = np.stack([rng.integers(-ra, ra + 1, n), rng.integers(-rb, rb + 1, n), rng.integers(-rc, rc + 1, n)], axis=1)
    return _distinct(list(first) + [tuple(r) for r in rnd][len(first):])


def _reach(ra, rb):
    """Four entries that pin the reach: +-ra along a, +-rb along b, +-7 along c, no two of them opposite."""
    return [(ra, rb, 7), (-ra, rb, -7), (min(ra, 1), -rb, 7), (-min(ra, 1), -rb, -3)]


class Case:
    """live: the live offsets in device axes; longer: indices into the entry list whose length is scaled by 1.5 (dup);
    corner: is the (0, 0, 0) start used; ra, rb: what the name states; exempt: from the start condition."""

    def __init__(self, name, live, ra, rb, corner, longer=(), exempt=False):
        self.name, self.ra, self.rb, self.corner, self.exempt = name, ra, rb, corner, exempt
        self.dev = np.array(list(live) + [SACRIFICIAL], dtype=np.int32)
        self.longer = tuple(longer)

    def offsets(self, shape):
        """The star in the user's axes on a grid of this shape, sacrificial entry included."""
        L = S.StripLayout(shape)
        out = np.zeros_like(self.dev)
        out[:, L.aax], out[:, L.bax], out[:, L.cax] = self.dev[:, 0], self.dev[:, 1], self.dev[:, 2]
        return out

    def fs(self, make_fs, shape):
        """struct FS array by make_fs (the package's or the oracle's: the same lengths), with the longer entries."""
        fs = make_fs(self.offsets(shape))
        for i in self.longer:
            fs["d"][i] = np.float32(1.5) * fs["d"][i]
        return fs

    def without_reach(self):
        """The star less the entries that define its reach: |da| = ra, |db| = rb, |dc| = 7."""
        live = [o for o in self.dev[:-1].tolist() if abs(o[0]) != self.ra and abs(o[1]) != self.rb and abs(o[2]) != 7]
        assert 0 < len(live) < len(self.dev) - 1
        return Case(self.name + "-reach", live, None, None, False)


def _ra_rb(ra, rb, corner=True):
    return Case(f"ra{ra}_rb{rb}", _random(10 * ra + rb, 40, ra, rb, 7, first=_reach(ra, rb)), ra, rb, corner)


def _dup():
    live = _random(91, 14, 2, 2, 4)
    return Case("dup", live + [live[3]], 2, 2, False, longer=[len(live)])


CASES = {c.name: c for c in [
    Case("flat_a", _random(1, 30, 0, 7, 7, first=_reach(0, 7)), 0, 7, True),
    # one db per da, no two live da adjacent; three hops (1, +1), (1, +1), (-2, +1) move three lanes on the spot
    Case("flat_b", [(1, 1, 1), (1, 1, -6), (-2, 1, 3), (-2, 1, -1), (3, -1, 2), (3, -1, -5), (-4, -1, 7), (-4, -1, -2),
                    (5, 0, 4), (5, 0, -3), (-6, 0, 1), (-6, 0, -7), (-6, 0, 6)], 6, 1, True),
    Case("only_c", [(0, 0, 1), (0, 0, -3), (0, 0, 7), (0, 0, -7), (0, 0, 4)], 0, 1, True, exempt=True),
    Case("single", [(2, 3, 5)], 2, 3, False, exempt=True),
    Case("gaps", [(2, 1, 3), (2, -2, -1), (2, 0, 6), (2, 3, -4), (2, -1, 0), (-5, 2, -2), (-5, -1, 5), (-5, 0, -7),
                  (-5, -3, 1), (-5, 1, 4)], 5, 3, True),
    _ra_rb(1, 7), _ra_rb(7, 1), _ra_rb(2, 6), _ra_rb(6, 2), _ra_rb(3, 5), _ra_rb(5, 3), _ra_rb(4, 4),
    Case("c7_edge", _distinct([(a, b, 7 * c) for a, b, c in _random(77, 30, 2, 3, 1)]), 2, 3, True),
    _dup(),
]}
RANDOM_CASES = [n for n in CASES if n.startswith("ra")]
FLAT_CASES = [n for n, c in CASES.items() if c.ra == 0]
BITE_CASES = RANDOM_CASES + ["c7_edge"]
CELL_CASES = ["flat_a", "gaps", "ra7_rb1"]


# ---------------------------------------------------------------------------
# grids and starts
# ---------------------------------------------------------------------------

MAIN_SHAPE = S.MAIN_SHAPE                   # (65, 66, 67): a, b, c = axes 0, 2, 1
TURNED_SHAPE = (67, 65, 66)                 # the same extents, a, b, c = axes 1, 0, 2
GRIDS = {"main": MAIN_SHAPE, "turned": TURNED_SHAPE}


def check_grids():
    """Both grids have the main grid's units (2 lane tiles, the second with 3 live lanes; 5 strips, the last with 2
    live cells; 65 planes) under two different assignments of the user's axes."""
    m, t = S.StripLayout(MAIN_SHAPE), S.StripLayout(TURNED_SHAPE)
    assert sorted(TURNED_SHAPE) == sorted(MAIN_SHAPE)
    assert (m.aax, m.bax, m.cax) == (0, 2, 1) and (t.aax, t.bax, t.cax) == (1, 0, 2)
    assert (m.aax, m.bax, m.cax) != (t.aax, t.bax, t.cax)
    for L in (m, t):
        assert (L.planes, L.nb, L.nc) == (65, 67, 66)
        assert (L.btiles, L.last_tile_lanes, L.cstrips, L.last_strip_cells) == (2, 3, 5, 2)
    return m, t


def matrix():
    """(case, grid): every case on the main grid, every third one on the turned grid."""
    names = list(CASES)
    return [(n, "main") for n in names] + [(n, "turned") for n in names[::3]]


def starts_dev(case):
    """Starts in device axes: the centre, the first lane of the ragged lane tile (next to the tile boundary), and -
    where the case's box from there meets the start condition - the (0, 0, 0) corner."""
    L = S.StripLayout(MAIN_SHAPE)
    out = [(L.planes // 2, L.nb // 2, L.nc // 2), (40, (L.btiles - 1) * L.TB, 2 * L.K + 5)]
    if case.corner:
        out.append((0, 0, 0))
    return out


def starts_of(case, shape):
    L = S.StripLayout(shape)
    return np.array([L.block(*s) for s in starts_dev(case)], dtype=np.int32)


def extent_dev(box, shape):
    """(planes, lane tiles, strips) that hold a finite cell of a box, as sets."""
    L = S.StripLayout(shape)
    idx = np.argwhere(np.isfinite(box))
    return (set(idx[:, L.aax].tolist()), set((idx[:, L.bax] // L.TB).tolist()), set((idx[:, L.cax] // L.K).tolist()))


def meets_start_condition(case, box, shape):
    planes, tiles, strips = extent_dev(box, shape)
    return len(tiles) == 2 and len(strips) >= 3 and (case.ra == 0 or len(planes) > 2 * case.ra + 2)


def units_that_differ(a, b, shape):
    """The one-plane units (plane, lane tile, strip) in which two boxes differ in a bit."""
    L = S.StripLayout(shape)
    idx = np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))
    return {(int(i[L.aax]), int(i[L.bax]) // L.TB, int(i[L.cax]) // L.K) for i in idx}


def damage_in_the_start_plane(layout, box, start):
    """For the flat cases, whose boxes live in the start's plane: INFINITY in a block of that plane across the
    lane-tile boundary and in one across a strip boundary; the start keeps its 0."""
    L = layout
    a = int(start[L.aax])
    tile, strip = (L.btiles - 1) * L.TB, 3 * L.K
    box[L.block(slice(a, a + 1), slice(tile - 4, tile + 2), slice(8, 30))] = np.float32(np.inf)
    box[L.block(slice(a, a + 1), slice(5, 25), slice(strip - 3, strip + 3))] = np.float32(np.inf)
    box[tuple(start)] = 0
    return box


def improves(before, fixed_point):
    """Does a solve from `before` improve a travel time?"""
    return int(not np.array_equal(np.ascontiguousarray(before).view(np.uint32), np.ascontiguousarray(fixed_point).view(np.uint32)))


def oracle_boxes(oracle, case, shape, starts, tts=None):
    """oracle.converge(order=1) per start over the case's star (from the boxes tts when given)."""
    from concurrent.futures import ThreadPoolExecutor
    v = S.velocity(shape)
    fs = case.fs(oracle.make_star, shape)

    def one(s):
        tt = None if tts is None else np.ascontiguousarray(tts[s], dtype=np.float32).copy()
        return oracle.converge(v, fs, starts[s], order=1, tt=tt)[0]

    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(one, range(len(starts))))


# ---------------------------------------------------------------------------
# the plan of a star, restated (make_layout_strip, upload_strip_plan_np in csrc/ttsweep_plan.cpp)
# ---------------------------------------------------------------------------

def device_pull(pull, shape):
    """The library's pull star (di, dj, dk, flags, h) in device axes: (da, db, dc, flags, h), in its order."""
    L = S.StripLayout(shape)
    return [(e[L.aax], e[L.bax], e[L.cax], e[3], e[4]) for e in pull]


def reach(dpull):
    """(ra, rb, rc): plan.ra, plan.rb = max(max |db|, 1), and max |dc| (which STRIP_CF - 1 bounds)."""
    return (max(abs(e[0]) for e in dpull), max(max(abs(e[1]) for e in dpull), 1), max(abs(e[2]) for e in dpull))


def nstaged(ra, np_):
    return 2 * ra + np_


def columns(dpull):
    """{da: [(db, {dc, ...}), ...]}: the (da, db) columns in the order the plan makes them - an offset goes into the
    first column of its (da, db) that does not hold its dc yet, a repeated offset therefore into a second one."""
    per_da = {}
    for da, db, dc, _flags, _h in dpull:
        cols = per_da.setdefault(da, [])
        for cdb, dcs in cols:
            if cdb == db and dc not in dcs:
                dcs.add(dc)
                break
        else:
            cols.append((db, {dc}))
    return per_da


def items(dpull, np_):
    """Per staged plane p (0 .. 2 ra + np - 1) its items [(rowoff, [offsets of own plane 0, of own plane 1])]: own
    plane j relaxes staged plane p with plane offset da = p - ra - j; columns of two own planes with the same row
    offset share an item."""
    ra = reach(dpull)[0]
    per_da = columns(dpull)
    out = []
    for p in range(nstaged(ra, np_)):
        its = []
        for j in range(np_):
            for db, dcs in per_da.get(p - ra - j, []):
                for it in its:
                    if it[0] == db and it[1][j] == 0:
                        it[1][j] = len(dcs)
                        break
                else:
                    its.append((db, [len(dcs) if k == j else 0 for k in range(2)]))
        out.append(its)
    return out


def item_counts(dpull, np_):
    return [len(its) for its in items(dpull, np_)]


def empty_planes(dpull, np_):
    """The staged planes without items: the holes of the kernel's plane_mask."""
    return {p for p, n in enumerate(item_counts(dpull, np_)) if n == 0}


def holes_between(dpull, np_):
    """Empty staged planes that lie strictly between two non-empty ones."""
    counts = item_counts(dpull, np_)
    full = [p for p, n in enumerate(counts) if n]
    return {p for p in empty_planes(dpull, np_) if full and full[0] < p < full[-1]}


def shares(dpull, np_, ns):
    """Per staged plane the items of each of the ns shares: longest processing time first (an item costs its offsets
    plus 3), ties to the earlier item and the lower share."""
    out = []
    for its in items(dpull, np_):
        cost = [sum(it[1]) + 3 for it in its]
        order = sorted(range(len(its)), key=lambda i: -cost[i])         # (stable: the plan's stable_sort)
        load, count = [0] * ns, [0] * ns
        for i in order:
            w = min(range(ns), key=lambda k: load[k])                   # (the first of the least loaded)
            load[w] += cost[i]
            count[w] += 1
        out.append(count)
    return out


def empty_shares(dpull, np_, ns):
    """{staged plane with items: waves without an item of it} - the waves that take the kernel's `ibeg >= iend`
    branch on that plane."""
    return {p: c.count(0) for p, c in enumerate(shares(dpull, np_, ns)) if sum(c)}
