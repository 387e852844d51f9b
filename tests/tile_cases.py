"""Shared cases of the TILE sweep kernels' instance and geometry tests (test_gpu_tile_instances.py, checked without a
GPU by test_tile_cases_cpu.py): eleven stars that between them land on every instance ttsweep_tile.hip can launch
(tile_six_kernel and tile_sweep_kernel<NE, EXACT>, NE in {6, 18, 26}) with every halo R in {1, 2} and every face depth
FZ in 1..4, three grids of several tiles per axis with ragged last tiles, starts on tile corners and inside other
tiles' z halos, the damage done to converged boxes, and host-side mirrors of the library's rules (tile_supports;
tile_instance, tile_R, tile_fz over the library's own pull star).  Plain numpy: no test lives here."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from column_cases import CSRC, ROOT, column_constants, grid_id, tile_count, tile_of, tiles    # noqa: F401 (shared)

SEED = 1
INF = np.float32(np.inf)
PULL_BOTH = 3           # PULL_FWD | PULL_REV
SIX = "six"             # tile_six_kernel; the other instances are (NE, EXACT)
ZFACE_DEPTH = 4         # TILE_ZF: the z halo of a staged row, the largest FZ


# ---------------------------------------------------------------------------
# the library's rules, restated (ttsweep_dev.h; tile_supported, make_layout_tile in ttsweep_plan.cpp; tile_instance,
# tile_star_is_six in ttsweep_tile.hip)
# ---------------------------------------------------------------------------

def tile_constants():
    """(TILE_ZF, TILE_MAX_R, TILE_MAX_ENT) as csrc/ttsweep_dev.h defines them."""
    text = open(os.path.join(CSRC, "ttsweep_dev.h")).read()
    out = []
    for name in ("TILE_ZF", "TILE_MAX_R", "TILE_MAX_ENT"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, f"{name} not found in ttsweep_dev.h"
        out.append(int(m.group(1)))
    return tuple(out)


def instance_thresholds():
    """The entry counts tile_instance (ttsweep_tile.hip) switches at, and the NE of the instances it returns for
    them: ([6, 18], [6, 6, 18, 18, 'TILE_MAX_ENT', 'TILE_MAX_ENT'])."""
    text = open(os.path.join(CSRC, "ttsweep_tile.hip")).read()
    body = text[text.index("static tile_sweep_fn tile_instance("):]
    body = body[:body.index("\n}\n")]
    limits = [int(x) for x in re.findall(r"if \(P\.nent <= (\d+)\)", body)]
    ne = [int(x) if x.isdigit() else x for x in re.findall(r"tile_sweep_kernel<(\w+), (?:true|false)>", body)]
    return limits, ne


def tile_supports(offs, starstart=0, starstop=None):
    """Mirror of the library's rule for the TILE kernel (small stars only): the live entries are
    offs[starstart:starstop], starstop = len - 1 by default (the reference's exclusive bound)."""
    live = np.asarray(offs).reshape(-1, 3)[starstart:len(offs) - 1 if starstop is None else starstop]
    pull = {tuple(o) for o in live} | {tuple(-o) for o in live}
    pull.discard((0, 0, 0))
    return 0 < len(pull) <= 26 and all(abs(a) <= 2 and abs(b) <= 2 and abs(c) <= 4 for a, b, c in pull)


def tile_R(pull):
    """make_layout_tile: the halo of the staged image along x and y.  pull: (di, dj, dk, flags, h) entries."""
    return max([1] + [max(abs(e[0]), abs(e[1])) for e in pull])


def tile_fz(pull):
    """make_layout_tile: the layers of a z face."""
    return max([1] + [abs(e[2]) for e in pull])


def tile_star_is_six(pull):
    six = [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
    return len(pull) == 6 and tile_R(pull) == 1 and all(tuple(e[:3]) == o and e[3] == PULL_BOTH for e, o in zip(pull, six))


def tile_instance(pull):
    """tile_instance: SIX, or (NE, EXACT) of the tile_sweep_kernel instance.  (The six kernel also wants a start's
    z faces below 4 GiB, a grid of about 2600^3: far from any grid here.)"""
    max_ent = tile_constants()[2]
    assert 0 < len(pull) <= max_ent
    exact = any(e[3] != PULL_BOTH for e in pull)
    if tile_star_is_six(pull):
        return SIX
    return (6 if len(pull) <= 6 else 18 if len(pull) <= 18 else max_ent, exact)


# ---------------------------------------------------------------------------
# stars
# ---------------------------------------------------------------------------

SACRIFICIAL = (1, 1, 1)         # the last entry of a symmetric star: the reference's exclusive bound drops it


def _pairs(*offsets):
    """Each offset and its opposite, then the sacrificial entry."""
    out = []
    for o in offsets:
        out += [o, tuple(-c for c in o)]
    return np.array(out + [SACRIFICIAL], dtype=np.int32)


def _shell(keep):
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0) and keep(a, b, c)]


def _file_star(name):
    words = open(os.path.join(ROOT, "data", "stars", f"{name}-FS.txt")).read().split()
    n = int(words[0])
    return np.array(words[1:1 + 3 * n], dtype=np.int32).reshape(n, 3)


def _asym():
    return np.load(os.path.join(ROOT, "tests", "golden", "float_range.npz"))["star_asym"].astype(np.int32)


class Star:
    """offs: the star as a caller passes it; [starstart, starstop) its live entries (starstop None: all but the
    last); instance, R, FZ: what the library makes of it."""

    def __init__(self, name, offs, instance, R, FZ, starstart=0, starstop=None):
        self.name, self.offs = name, np.ascontiguousarray(offs, dtype=np.int32).reshape(-1, 3)
        self.instance, self.R, self.FZ = instance, R, FZ
        self.starstart, self.starstop = starstart, len(self.offs) - 1 if starstop is None else starstop

    @property
    def exact(self):
        return self.instance != SIX and self.instance[1]

    @property
    def live(self):
        return self.offs[self.starstart:self.starstop]

    def symmetrised(self):
        """The live offsets, their opposites and a sacrificial entry: every edge live in both directions."""
        return Star(self.name + "+sym", _pairs(*[tuple(int(c) for c in o) for o in self.live]), None, self.R, self.FZ)


STARS = {s.name: s for s in [
    Star("six_open", [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], (6, True), 1, 1),
    Star("three_0_4", _file_star("3"), (6, True), 1, 1, starstart=0, starstop=4),
    Star("r2_flat", _pairs((1, 0, 0), (2, 1, 0), (0, 0, 1)), (6, False), 2, 1),
    Star("tall", _pairs((1, 0, 0), (0, 1, 4), (0, 0, 1)), (6, False), 1, 4),
    Star("shell18", _shell(lambda a, b, c: abs(a) + abs(b) + abs(c) <= 2) + [SACRIFICIAL], (18, False), 1, 1),
    Star("deep18", _pairs((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 3), (1, 1, 0), (1, 0, 2),
                          (0, 1, 2)), (18, False), 2, 3),
    Star("nonsym_z2", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, -1, 0), (0, -1, -2), (1, 0, 2), (2, 1, -1)], (18, True), 1, 2),
    Star("half26", _shell(lambda a, b, c: (a, b, c) > (0, 0, 0)) + [(2, 2, 4)], (26, True), 1, 1),
    Star("asym", _asym(), (26, True), 2, 2),
    Star("deep26", _pairs((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 4), (0, 0, 2), (1, 1, 0),
                          (1, 0, 1), (0, 1, 1), (2, 2, 4), (1, -1, 0), (2, 1, -3)), (26, False), 2, 4),
    Star("six", _file_star("six"), SIX, 1, 1),          # control: the six kernel, under OPT_ASYNC = 0
]}
EXACT_STARS = [n for n, s in STARS.items() if s.exact]
ALL_INSTANCES = {SIX} | {(ne, ex) for ne in (6, 18, 26) for ex in (False, True)}


# ---------------------------------------------------------------------------
# grids, starts, volumes
# ---------------------------------------------------------------------------

GRID_A, GRID_B, GRID_C = (9, 17, 70), (17, 9, 36), (10, 10, 34)
GRIDS = {"A": GRID_A, "B": GRID_B, "C": GRID_C}
# (tiles, cells of the last z tile)
GRID_TILES = {"A": ((2, 3, 3), 6), "B": ((3, 2, 2), 4), "C": ((2, 2, 2), 2)}

# A: the grid's corners, both sides of a tile corner, and two cells in the z halo (depth 4) of the tile below / above
STARTS_A = np.array([(0, 0, 0), (7, 7, 31), (8, 8, 32), (8, 16, 69), (4, 8, 35), (3, 15, 28)], dtype=np.int32)
BATCH = 3               # starts per solve: a launch holds several active starts


def starts_of(grid):
    """A: STARTS_A.  B, C: the origin, the last cell, the cell just past the first z-tile boundary at mid x, mid y."""
    if grid == "A":
        return STARTS_A
    nx, ny, nz = GRIDS[grid]
    return np.array([(0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx // 2, ny // 2, column_constants()[2])], dtype=np.int32)


def batches(grid):
    st = starts_of(grid)
    return [slice(b, min(b + BATCH, len(st))) for b in range(0, len(st), BATCH)]


def cases():
    """(star name, grid name): every star on A; on B and C the stars with FZ > 1 or R = 2."""
    return [(n, g) for g in GRIDS for n, s in STARS.items() if g == "A" or s.FZ > 1 or s.R == 2]


def velocity(shape, seed=SEED):
    """Seeded uniform [0.1, 0.5), as in the other tile tests."""
    return np.random.default_rng(seed).uniform(0.1, 0.5, size=shape).astype(np.float32)


def damage(box, start):
    """A converged box made a state above its fixed point: a block back at INFINITY that straddles the first z-tile
    boundary, a slab across the middle raised by x 1.5, the start back at 0.  Nothing is lowered."""
    nx, ny, nz = box.shape
    tz = column_constants()[2]
    out = box.copy()
    out[nx // 4: nx // 4 + 5, ny // 3: ny // 3 + 5, tz - 6: min(tz + 6, nz)] = INF
    out[: max(nx // 2, 1), :, nz // 2 - 3: nz // 2 + 3] *= np.float32(1.5)
    out[tuple(start)] = 0
    assert (out >= box).all() and np.isinf(out[:, :, tz - 1]).any() and np.isinf(out[:, :, tz]).any()
    return out


def improves(before, fixed_point):
    """Does a solve from `before` improve a travel time (include/ttsweep.h: ttsweep_solve, ttsweep_get_changed)?"""
    return int(not np.array_equal(np.ascontiguousarray(before).view(np.uint32), np.ascontiguousarray(fixed_point).view(np.uint32)))


def fresh_boxes(shape, starts):
    out = []
    for st in np.asarray(starts).reshape(-1, 3):
        tt = np.full(shape, np.inf, dtype=np.float32)
        tt[tuple(st)] = 0
        out.append(tt)
    return out


def oracle_boxes(oracle, v, star, starts):
    """oracle.converge(order=1) per start over the star's live range, a few at a time (the checker runs outside the
    interpreter lock).  A one-directional star need not reach every cell: INFINITY is a result."""
    fs = oracle.make_star(star.offs)
    starts = np.asarray(starts).reshape(-1, 3)
    with ThreadPoolExecutor(max_workers=6) as pool:
        out = list(pool.map(lambda st: oracle.converge(v, fs, st, star.starstart, star.starstop, order=1)[0], starts))
    for st, box in zip(starts, out):
        assert box.shape == v.shape and box.dtype == np.float32 and box[tuple(st)] == 0 and not (box < 0).any() \
            and not np.isnan(box).any(), f"oracle box of {star.name}, start {tuple(st)}"
    return out
