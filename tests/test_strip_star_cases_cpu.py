"""CPU tier: the ground the STRIP star tests (test_gpu_strip_stars.py) stand on, checked where no GPU is: every star
of strip_star_cases.py has the plane reach, the lane reach and the property its name states (restated over the
library's own pull star), the union covers ra 0..7 and rb 1..7, staged planes without items, planes with fewer items
than waves and planes with items for all eight waves, the starts meet the start condition, the restated item lists
agree with a direct count - and the oracle's boxes change in more than one unit when a star loses the entries that
define its reach, so that a kernel or planner that cuts the reach short by one cannot hide."""
import numpy as np
import pytest

import strip_cases as S
import strip_star_cases as C


def dpull_of(pkg, case, shape=C.MAIN_SHAPE):
    pull = pkg.build_pull_star(case.fs(pkg.inputs.make_fs, shape))
    return pull, C.device_pull(pull, shape)


def test_constants_grids_and_matrix():
    k = C.strip_plan_constants()
    assert (k["STRIP_MAX_RA"], k["STRIP_CF"], k["STRIP_PLANES"]) == (7, 8, 2)
    assert (k["STRIP_NS"], k["STRIP_NS_LAT"], k["STRIP_NS_MAX"]) == (4, 8, 8)
    m, t = C.check_grids()
    assert (m.aax, m.bax, m.cax) != (t.aax, t.bax, t.cax)
    assert list(C.CASES) == ["flat_a", "flat_b", "only_c", "single", "gaps", "ra1_rb7", "ra7_rb1", "ra2_rb6", "ra6_rb2",
                             "ra3_rb5", "ra5_rb3", "ra4_rb4", "c7_edge", "dup"]
    mx = C.matrix()
    assert [n for n, g in mx if g == "main"] == list(C.CASES)
    assert [n for n, g in mx if g == "turned"] == ["flat_a", "single", "ra7_rb1", "ra3_rb5", "c7_edge"]
    assert C.FLAT_CASES == ["flat_a", "only_c"] and len(C.RANDOM_CASES) == 7
    assert [n for n, c in C.CASES.items() if c.exempt] == ["only_c", "single"]
    assert set(C.CELL_CASES) <= set(C.CASES)


@pytest.mark.parametrize("grid", list(C.GRIDS))
@pytest.mark.parametrize("name", list(C.CASES))
def test_case_has_the_reach_its_name_states(pkg, oracle, name, grid):
    """... on both grids: the star is written in device axes, so the plan is the same whatever the user's axes are.
    The package and the oracle prepare the same lengths."""
    case, shape = C.CASES[name], C.GRIDS[grid]
    pull, dp = dpull_of(pkg, case, shape)
    assert C.strip_supported(pull), name
    ra, rb, rc = C.reach(dp)
    assert (ra, rb) == (case.ra, case.rb), name
    assert rc <= 7 < C.strip_plan_constants()["STRIP_CF"]
    assert (C.nstaged(ra, 1), C.nstaged(ra, 2)) == (2 * ra + 1, 2 * ra + 2)
    assert sorted(dp) == sorted(dpull_of(pkg, case, C.MAIN_SHAPE)[1])           # (flags and h included)
    flags = [e[3] for e in dp]
    assert flags.count(C.PULL_FWD) > 0 and flags.count(C.PULL_FWD) == flags.count(C.PULL_REV), name
    a = case.fs(pkg.inputs.make_fs, shape)
    b = case.fs(oracle.make_star, shape)
    assert a.tobytes() == b.tobytes(), name
    assert tuple(case.dev[-1]) == C.SACRIFICIAL
    if name.startswith("ra"):
        live = case.dev[:-1]
        assert 35 <= len(live) <= 40 and np.abs(live).max(axis=0).tolist() == [ra, rb, 7]
        assert {int(x) for x in live[:, 0]} >= {ra, -ra} and len(set(np.abs(live[:, 2]).tolist())) >= 6


def test_properties_of_the_named_cases(pkg):
    dp = {n: dpull_of(pkg, c)[1] for n, c in C.CASES.items()}
    # flat_a: no plane offset, nstaged = np, dc to +-7
    assert {e[0] for e in dp["flat_a"]} == {0} and {e[2] for e in dp["flat_a"]} >= {-7, 7}
    assert len(C.item_counts(dp["flat_a"], 1)) == 1 and len(C.item_counts(dp["flat_a"], 2)) == 2
    # flat_b: one lane offset per plane offset, one item per non-empty plane: 3 of 4 and 7 of 8 waves have none
    assert C.reach(dp["flat_b"])[0] >= 5 and {e[1] for e in dp["flat_b"]} == {-1, 0, 1}
    assert all(len(cols) == 1 for cols in C.columns(dp["flat_b"]).values())
    assert set(C.item_counts(dp["flat_b"], 1)) == {0, 1} and max(C.item_counts(dp["flat_b"], 2)) == 2
    assert set(C.empty_shares(dp["flat_b"], 1, 4).values()) == {3} and set(C.empty_shares(dp["flat_b"], 1, 8).values()) == {7}
    assert C.holes_between(dp["flat_b"], 1) == {C.reach(dp["flat_b"])[0]}       # (the own plane itself)
    # only_c: the strip axis alone; rb is the clamp max(0, 1)
    assert {e[:2] for e in dp["only_c"]} == {(0, 0)} and C.reach(dp["only_c"]) == (0, 1, 7)
    # single: one live offset, no component zero
    assert len(C.CASES["single"].dev) == 2 and all(C.CASES["single"].dev[0] != 0) and len(dp["single"]) == 2
    # gaps: da in {+2, -5}: with one-plane units the staged planes |da| in {0, 1, 3, 4} have no item
    assert {int(x) for x in C.CASES["gaps"].dev[:-1, 0]} == {2, -5}
    assert C.empty_planes(dp["gaps"], 1) == {5 + d for d in (0, 1, -1, 3, -3, 4, -4)}
    assert C.holes_between(dp["gaps"], 1) == C.empty_planes(dp["gaps"], 1) and C.holes_between(dp["gaps"], 2) == {2, 5, 6, 9}
    # c7_edge: whatever leaves a strip does so by exactly 7
    assert {e[2] for e in dp["c7_edge"]} == {-7, 0, 7}
    # dup: one offset twice, with two lengths: two pull entries per direction and a second (da, db) column
    dup = C.CASES["dup"]
    assert tuple(dup.dev[-2]) == tuple(dup.dev[3]) and dup.longer == (len(dup.dev) - 2,)
    twice = [e for e in dp["dup"] if e[:3] == tuple(dup.dev[3])]
    assert len(twice) == 2 and twice[1][4] == np.float32(1.5) * twice[0][4]
    cols = C.columns(dp["dup"])[int(dup.dev[3][0])]
    assert len(cols) == len({db for db, _ in cols}) + 1
    assert all(len(c) == len({db for db, _ in c}) for n in C.CASES if n != "dup" for c in C.columns(dp[n]).values())


def test_the_union_covers_every_reach_and_every_share_pattern(pkg):
    dp = {n: dpull_of(pkg, c)[1] for n, c in C.CASES.items()}
    reach = {n: C.reach(d) for n, d in dp.items()}
    assert {r[0] for r in reach.values()} == set(range(0, 8))                   # ra 0..7: both parities, and none
    assert {r[1] for r in reach.values()} == set(range(1, 8))                   # rb 1..7
    assert {r[2] for r in reach.values()} >= {4, 5, 7}
    for ra in range(1, 8):
        assert reach[f"ra{ra}_rb{8 - ra}"][:2] == (ra, 8 - ra)
    assert sum(r[0] != r[1] for r in reach.values()) >= 10 and sum(r[0] > r[1] for r in reach.values()) >= 4
    # empty staged planes strictly between non-empty ones
    assert [n for n in dp if C.holes_between(dp[n], 1)] == ["flat_b", "single", "gaps", "ra7_rb1"]
    assert [n for n in dp if C.holes_between(dp[n], 2)] == ["single", "gaps"]
    # every non-empty plane holds fewer than 4 items: most waves take the `ibeg >= iend` branch on every plane
    sparse = [n for n in dp if max(C.item_counts(dp[n], 1)) < 4]
    assert sparse == ["flat_b", "only_c", "single", "ra7_rb1"]
    for n in sparse:
        assert min(C.empty_shares(dp[n], 1, 4).values()) >= 1 and min(C.empty_shares(dp[n], 1, 8).values()) >= 5
    # a plane with at least 8 items, none of the eight shares empty
    full = [n for n in dp if 0 in C.empty_shares(dp[n], 1, 8).values()]
    assert "flat_a" in full and "ra1_rb7" in full and len(full) >= 4
    assert all(max(C.item_counts(dp[n], 1)) >= 8 for n in full)
    # shares: every item is in exactly one, for both wave counts and unit sizes
    for n, d in dp.items():
        for np_ in (1, 2):
            for ns in (4, 8):
                assert [sum(c) for c in C.shares(d, np_, ns)] == C.item_counts(d, np_), (n, np_, ns)


@pytest.mark.parametrize("name", list(C.CASES))
def test_restated_item_lists_agree_with_a_direct_count(pkg, name):
    """Per plane offset da: the offsets of the first columns are the distinct (da, db, dc) of the pull star, all
    columns together its entries; a one-plane unit has one item per column; a two-plane unit's staged plane p holds the
    row offsets of da = p - ra and of da = p - ra - 1, shared where they are equal."""
    _, dp = dpull_of(pkg, C.CASES[name])
    ra = C.reach(dp)[0]
    cols = C.columns(dp)
    for da in range(-ra, ra + 1):
        entries = [e[:3] for e in dp if e[0] == da]
        got = cols.get(da, [])
        assert sum(len(dcs) for _, dcs in got) == len(entries), (name, da)
        first = {}
        for db, dcs in got:
            first.setdefault(db, dcs)
        assert sum(len(d) for d in first.values()) == len(set(entries)), (name, da)
        assert {(da, db, dc) for db, dcs in got for dc in dcs} == set(entries), (name, da)
    one = C.item_counts(dp, 1)
    assert one == [len(cols.get(p - ra, [])) for p in range(2 * ra + 1)], name
    two = C.items(dp, 2)
    assert len(two) == 2 * ra + 2
    for p, its in enumerate(two):
        own0, own1 = cols.get(p - ra, []), cols.get(p - ra - 1, [])
        assert sum(it[1][0] for it in its) == sum(len(d) for _, d in own0), (name, p)
        assert sum(it[1][1] for it in its) == sum(len(d) for _, d in own1), (name, p)
        if name != "dup":
            assert len(its) == len({db for db, _ in own0} | {db for db, _ in own1}), (name, p)
        assert max(len(own0), len(own1)) <= len(its) <= len(own0) + len(own1), (name, p)


@pytest.fixture(scope="module")
def boxes(oracle):
    """The oracle's boxes of every case from its starts on the main grid (computed once, never written to)."""
    out = {}
    for name, case in C.CASES.items():
        out[name] = C.oracle_boxes(oracle, case, C.MAIN_SHAPE, C.starts_of(case, C.MAIN_SHAPE))
        for b in out[name]:
            b.setflags(write=False)
    return out


@pytest.mark.slow
@pytest.mark.parametrize("name", list(C.CASES))
def test_starts_meet_the_start_condition(oracle, boxes, name):
    """Finite cells in both lane tiles and at least three strips, and with ra > 0 in more than 2 ra + 2 planes, for
    every (case, start) in use; the corner is used exactly where its box meets the condition (only_c: where it is no
    more trivial than the others).  only_c and single are exempt by construction: a row of cells, a line of cells."""
    case = C.CASES[name]
    L = S.StripLayout(C.MAIN_SHAPE)
    dev = C.starts_dev(case)
    assert dev[0] == (32, 33, 33) and dev[1] == (40, 64, 37) and dev[1][1] == (L.btiles - 1) * L.TB
    assert len(dev) == 2 + case.corner and (not case.corner or dev[2] == (0, 0, 0))
    starts = C.starts_of(case, C.MAIN_SHAPE)
    fs = case.fs(oracle.make_star, C.MAIN_SHAPE)
    v = S.velocity(C.MAIN_SHAPE)
    for st, box in zip(starts, boxes[name]):
        assert box[tuple(st)] == 0 and not np.isnan(box).any() and not (box < 0).any()
        open_edges, ninf = oracle.validate(v, box, fs, st)
        assert open_edges == 0 and ninf == int(np.isinf(box).sum()), (name, tuple(st))
        assert np.isfinite(box).sum() > 1, (name, tuple(st))                   # no trivial box
        if not case.exempt:
            assert C.meets_start_condition(case, box, C.MAIN_SHAPE), (name, tuple(st))
    corner = C.oracle_boxes(oracle, case, C.MAIN_SHAPE, np.zeros((1, 3), dtype=np.int32))[0]
    if name == "only_c":
        assert case.corner and np.isfinite(corner).sum() == L.nc
    else:
        assert case.corner == (C.meets_start_condition(case, corner, C.MAIN_SHAPE) and not case.exempt), name
    if name in C.FLAT_CASES:
        for st, box in zip(starts, boxes[name]):
            assert C.extent_dev(box, C.MAIN_SHAPE)[0] == {int(st[L.aax])}      # the start's plane and nothing else
    if name == "flat_a":
        assert all(np.isfinite(b).sum() == L.nb * L.nc for b in boxes[name])    # ... all of it
    if name == "single":
        assert [int(np.isfinite(b).sum()) for b in boxes[name]] == [7, 8]
        assert len(C.extent_dev(boxes[name][1], C.MAIN_SHAPE)[1]) == 2          # the line crosses the lane-tile boundary
    if name == "gaps":
        assert np.isfinite(boxes[name][0]).all()


@pytest.mark.slow
@pytest.mark.parametrize("name", C.BITE_CASES)
def test_the_reach_defining_entries_matter_across_units(oracle, boxes, name):
    """Without the entries with |da| = ra, |db| = rb or |dc| = 7 the box of the centre start is another box, in cells
    of at least two different units: the full-reach edges matter across unit boundaries."""
    case = C.CASES[name]
    less = case.without_reach()
    assert {abs(int(x)) for x in less.dev[:-1, 0]} <= set(range(case.ra)) and np.abs(less.dev[:-1, 2]).max() < 7
    start = C.starts_of(case, C.MAIN_SHAPE)[:1]
    other = C.oracle_boxes(oracle, less, C.MAIN_SHAPE, start)[0]
    units = C.units_that_differ(boxes[name][0], other, C.MAIN_SHAPE)
    assert len(units) >= 2, (name, len(units))
    assert len({u[0] for u in units}) >= 2 and len({u[1] for u in units}) == 2 and len({u[2] for u in units}) >= 2


def test_damage_helpers():
    """damage_to_infinity (shared with the schedule tests) and the flat cases' damage in the start's plane: only
    INFINITY is written, across the lane-tile boundary and a strip boundary; the start keeps its 0."""
    class G:
        layout = S.StripLayout(C.MAIN_SHAPE)
    L = G.layout
    rng = np.random.default_rng(5)
    for dev in ((32, 33, 33), (40, 64, 37)):
        start = L.block(*dev)
        box = rng.uniform(1.0, 2.0, size=C.MAIN_SHAPE).astype(np.float32)
        box[start] = 0
        d = S.damage_to_infinity(G, box.copy(), start)
        assert d[start] == 0 and (d >= box).all() and np.isinf(d[L.block(L.planes - 1, slice(None), slice(None))]).all()
        assert np.isinf(d[L.block(32, 63, 22)]) and np.isinf(d[L.block(32, 64, 22)]) and np.isinf(d[L.block(12, 12, 31)]) \
            and np.isinf(d[L.block(12, 12, 32)])
        p = C.damage_in_the_start_plane(L, box.copy(), start)
        hit = np.argwhere(np.isinf(p))
        assert p[start] == 0 and set(hit[:, L.aax].tolist()) == {dev[0]}
        assert {int(b) // L.TB for b in hit[:, L.bax]} == {0, 1} and {int(c) // L.K for c in hit[:, L.cax]} >= {1, 2, 3}
        assert np.array_equal(p[np.isfinite(p)], box[np.isfinite(p)])
