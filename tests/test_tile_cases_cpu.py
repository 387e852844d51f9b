"""CPU tier: the ground the TILE instance tests (test_gpu_tile_instances.py) stand on, checked where no GPU is: every
star of tile_cases.py lands on the instance, halo and face depth it was written for (restated over the library's own
pull star), the cases cover all seven instances, both R and all four FZ, the constants mirror the sources, the grids
and starts sit on the tile edges they claim, and the oracle's fixed points exist - and, for the stars with
one-directional entries, differ from those of the symmetrised star, so a liveness bug cannot hide."""
import numpy as np
import pytest

import tile_cases as T


def pull_of(pkg, star):
    return pkg.build_pull_star(pkg.inputs.make_fs(star.offs), star.starstart, star.starstop)


def test_the_constants_mirror_the_sources():
    """The tile shape, TILE_ZF, TILE_MAX_R, TILE_MAX_ENT and the entry counts tile_instance switches at: a change
    that moves a star onto another instance, or a grid off its edge, fails here instead of turning the GPU tests
    vacuous."""
    assert T.column_constants()[:3] == (8, 8, 32)
    assert T.tile_constants() == (T.ZFACE_DEPTH, 2, 26)
    limits, ne = T.instance_thresholds()
    assert limits == [6, 18]
    assert ne == [6, 6, 18, 18, "TILE_MAX_ENT", "TILE_MAX_ENT"]
    assert {i[0] for i in T.ALL_INSTANCES if i != T.SIX} == {6, 18, T.tile_constants()[2]}


@pytest.mark.parametrize("name", list(T.STARS))
def test_star_lands_on_its_instance_and_geometry(pkg, name):
    star = T.STARS[name]
    pull = pull_of(pkg, star)
    assert T.tile_instance(pull) == star.instance, (name, len(pull), [e[3] for e in pull])
    assert (T.tile_R(pull), T.tile_fz(pull)) == (star.R, star.FZ), name
    assert T.tile_supports(star.offs, star.starstart, star.starstop), name
    # the support rule's own view of the pull star is the library's
    live = star.live
    assert {tuple(e[:3]) for e in pull} == ({tuple(o) for o in live} | {tuple(-o) for o in live}) - {(0, 0, 0)}
    if star.exact:
        sym = pull_of(pkg, star.symmetrised())
        assert {tuple(e[:3]) for e in sym} == {tuple(e[:3]) for e in pull} and all(e[3] == T.PULL_BOTH for e in sym)
        assert any(e[3] != T.PULL_BOTH for e in pull)
    else:
        assert all(e[3] == T.PULL_BOTH for e in pull)


def test_stars_are_the_ones_the_matrix_names(pkg):
    s = T.STARS
    assert list(s) == ["six_open", "three_0_4", "r2_flat", "tall", "shell18", "deep18", "nonsym_z2", "half26", "asym",
                       "deep26", "six"]
    assert len(s["six_open"].offs) == 6 and s["six_open"].starstop == 5                    # no sacrificial entry: +z is dropped
    assert (s["three_0_4"].starstart, s["three_0_4"].starstop) == (0, 4) and len(s["three_0_4"].offs) == 98
    assert np.array_equal(s["three_0_4"].offs, pkg.inputs.read_triples(pkg.inputs.star_path("3")))
    assert np.array_equal(s["six"].offs, pkg.inputs.read_triples(pkg.inputs.star_path("six")))
    assert [len(pull_of(pkg, s[n])) for n in s] == [6, 6, 6, 6, 18, 18, 12, 26, 22, 26, 6]
    assert tuple(s["nonsym_z2"].offs[-1]) == (2, 1, -1) and tuple(s["half26"].offs[-1]) == (2, 2, 4)
    assert len(s["half26"].live) == 13 and all(tuple(o) > (0, 0, 0) for o in s["half26"].live)
    assert T.EXACT_STARS == ["six_open", "three_0_4", "nonsym_z2", "half26", "asym"]
    # the stars the existing suites feed to the TILE kernel reach four of the seven instances
    rnd = np.random.default_rng(31)
    rnd.uniform(0.1, 0.5, size=(33, 70, 19))
    offs = np.stack([rnd.integers(-2, 3, size=9), rnd.integers(-2, 3, size=9), rnd.integers(-4, 5, size=9)], axis=1)
    offs = offs[np.any(offs != 0, axis=1)].astype(np.int32)
    assert T.tile_instance(pkg.build_pull_star(pkg.inputs.make_fs(offs))) == (18, True)


def test_cases_cover_every_instance_and_geometry():
    assert {s.instance for s in T.STARS.values()} == T.ALL_INSTANCES and len(T.ALL_INSTANCES) == 7
    assert {s.R for s in T.STARS.values()} == {1, 2}
    assert {s.FZ for s in T.STARS.values()} == {1, 2, 3, 4}
    geometry = {(s.R, s.FZ) for s in T.STARS.values()}
    assert {(1, 4), (1, 2), (2, 1), (2, 2), (2, 3), (2, 4)} <= geometry         # R = 1 with FZ > 1, R = 2 with FZ = 1, ...
    cases = T.cases()
    assert [c for c in cases if c[1] == "A"] == [(n, "A") for n in T.STARS]
    deep = ["r2_flat", "tall", "deep18", "nonsym_z2", "asym", "deep26"]
    assert [c for c in cases if c[1] == "B"] == [(n, "B") for n in deep]
    assert [c for c in cases if c[1] == "C"] == [(n, "C") for n in deep]
    # FZ 2 and 3 across a z-tile boundary, and a last z tile with fewer cells than FZ
    assert {T.STARS[n].FZ for n in deep} == {1, 2, 3, 4}
    assert T.GRID_TILES["C"][1] < 3 and T.GRID_TILES["B"][1] == T.ZFACE_DEPTH


@pytest.mark.parametrize("grid", list(T.GRIDS))
def test_grids_and_starts_sit_on_the_tile_edges(grid):
    shape = T.GRIDS[grid]
    tx, ty, tz = T.column_constants()[:3]
    want_tiles, tail = T.GRID_TILES[grid]
    assert T.tiles(shape) == want_tiles and shape[2] - tz * (want_tiles[2] - 1) == tail
    assert shape[0] % tx and shape[1] % ty and shape[2] % tz                    # ragged last tiles on every axis
    assert min(want_tiles) >= 2                                                 # more than one tile on every axis
    st = T.starts_of(grid)
    assert (st >= 0).all() and (st < np.array(shape)).all() and len({tuple(s) for s in st}) == len(st)
    assert [len(range(*b.indices(len(st)))) for b in T.batches(grid)] == [3] * (len(st) // 3)
    if grid == "A":
        assert want_tiles[2] == 3                                               # a z tile with neighbours on both sides
        assert [tuple(s) for s in st] == [(0, 0, 0), (7, 7, 31), (8, 8, 32), (8, 16, 69), (4, 8, 35), (3, 15, 28)]
        assert tuple(st[3]) == tuple(n - 1 for n in shape)
        assert T.tile_of(shape, st[1]) == (0, 0, 0) and T.tile_of(shape, st[2]) == (1, 1, 1)    # across a tile corner
        # in the z halo, at depth 4, of the tile below / the tile above
        assert st[4][2] == tz + T.ZFACE_DEPTH - 1 and T.tile_of(shape, st[4])[2] == 1
        assert st[5][2] == tz - T.ZFACE_DEPTH and T.tile_of(shape, st[5])[2] == 0
    else:
        assert [tuple(s) for s in st] == [(0, 0, 0), tuple(n - 1 for n in shape), (shape[0] // 2, shape[1] // 2, tz)]
    v = T.velocity(shape)
    assert v.dtype == np.float32 and v.shape == shape and (v >= 0.1).all() and (v <= 0.5).all()


def test_damage_only_raises_and_straddles_a_tile_boundary():
    rng = np.random.default_rng(3)
    for shape, start in ((T.GRID_A, (4, 8, 35)), (T.GRID_B, (0, 0, 0)), (T.GRID_C, (9, 9, 33))):
        box = rng.uniform(1.0, 2.0, size=shape).astype(np.float32)
        box[start] = 0
        d = T.damage(box, start)
        assert d.dtype == np.float32 and d[start] == 0 and (d >= box).all()
        dz = np.nonzero(np.isinf(d).any(axis=(0, 1)))[0]
        assert dz.min() < 32 <= dz.max()
        assert ((d > box) & np.isfinite(d)).any() and T.improves(d, box) == 1 and T.improves(box, box) == 0
    # a box nothing was reached in: the damage changes nothing, and a solve of it improves nothing
    empty = T.fresh_boxes(T.GRID_A, [(0, 0, 0)])[0]
    assert T.improves(T.damage(empty, (0, 0, 0)), empty) == 0


@pytest.fixture(scope="module")
def boxes_on_A(oracle):
    """The oracle's boxes of every star, and of the symmetrised EXACT stars, from the six starts on A."""
    v = T.velocity(T.GRID_A)
    out = {n: T.oracle_boxes(oracle, v, s, T.STARTS_A) for n, s in T.STARS.items()}
    for n in T.EXACT_STARS:
        out[n + "+sym"] = T.oracle_boxes(oracle, v, T.STARS[n].symmetrised(), T.STARTS_A)
    return v, out


@pytest.mark.parametrize("name", list(T.STARS))
def test_oracle_fixed_points_on_A(oracle, boxes_on_A, name):
    """Computed, at rest under the oracle's own validator, and every start improves its fresh box - but half26 from
    the origin, which reaches no cell (every entry is lexicographically positive: no edge is centred below the start)."""
    v, boxes = boxes_on_A
    star = T.STARS[name]
    fs = oracle.make_star(star.offs)
    fresh = T.fresh_boxes(T.GRID_A, T.STARTS_A)
    for st, box, f in zip(T.STARTS_A, boxes[name], fresh):
        open_edges, ninf = oracle.validate(v, box, fs, st, star.starstart, star.starstop)
        assert open_edges == 0 and ninf == int(np.isinf(box).sum()), (name, tuple(st))
        if not star.exact:
            assert ninf == 0, (name, tuple(st))
        if name == "half26" and tuple(st) == (0, 0, 0):
            assert ninf == box.size - 1 == 10709 and T.improves(f, box) == 0
        else:
            assert T.improves(f, box) == 1, (name, tuple(st))


@pytest.mark.parametrize("name,differing", [("six_open", 5), ("three_0_4", 5), ("nonsym_z2", 6), ("half26", 5), ("asym", 6)])
def test_exact_stars_differ_from_their_symmetrised_star(boxes_on_A, name, differing):
    """What makes a liveness bug visible: a kernel that treated the one-directional entries as live both ways would
    compute the symmetrised star's box, and that is another box on at least 4 of the 6 starts."""
    assert name in T.EXACT_STARS
    _, boxes = boxes_on_A
    n = sum(T.improves(a, b) for a, b in zip(boxes[name], boxes[name + "+sym"]))
    assert n >= 4, (name, n)
    assert n == differing, (name, n)            # (as counted with seed 1 on grid A)


@pytest.mark.parametrize("grid", ["B", "C"])
def test_oracle_fixed_points_on_B_and_C(oracle, grid):
    v = T.velocity(T.GRIDS[grid])
    names = [n for n, g in T.cases() if g == grid]
    assert len(names) == 6
    for name in names:
        star = T.STARS[name]
        fs = oracle.make_star(star.offs)
        starts = T.starts_of(grid)
        for st, box in zip(starts, T.oracle_boxes(oracle, v, star, starts)):
            open_edges, ninf = oracle.validate(v, box, fs, st, star.starstart, star.starstop)
            assert open_edges == 0 and ninf == int(np.isinf(box).sum()) and np.isfinite(box).sum() > 1, (name, grid, tuple(st))
