"""Shared cases of the column driver's limit tests (test_gpu_column_limits.py, checked without a GPU by
test_column_cases_cpu.py): the tall grids around COL_MAX_NK, their starts and velocity volumes, the 70 starts of the
batch tests, the damage done to converged boxes, and host-side mirrors of the library's rules that decide which
driver a solve runs on (tile_count, use_column, column_in_place, column_order_default).  Plain numpy: no test lives
here."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uoparallel-seismic-project_amd", "csrc")
SEED = 1207
INF = np.float32(np.inf)


# ---------------------------------------------------------------------------
# the library's rules, restated (ttsweep_dev.h; use_column, column_in_place in ttsweep_driver.cpp;
# column_order_default in ttsweep_column.hip)
# ---------------------------------------------------------------------------

def column_constants():
    """(TILE_X, TILE_Y, TILE_Z, COL_MAX_NK) as csrc/ttsweep_dev.h defines them."""
    text = open(os.path.join(CSRC, "ttsweep_dev.h")).read()
    m = re.search(r"constexpr\s+int\s+TILE_X\s*=\s*(\d+)\s*,\s*TILE_Y\s*=\s*(\d+)\s*,\s*TILE_Z\s*=\s*TTSWEEP_TILE_Z\s*;", text)
    z = re.search(r"#define\s+TTSWEEP_TILE_Z\s+(\d+)", text)
    k = re.search(r"constexpr\s+int\s+COL_MAX_NK\s*=\s*(\d+)\s*;", text)
    assert m and z and k, "TILE_X / TILE_Y / TTSWEEP_TILE_Z / COL_MAX_NK not found in ttsweep_dev.h"
    return int(m.group(1)), int(m.group(2)), int(z.group(1)), int(k.group(1))


def tile_count(n, t):
    return (n + t - 1) // t


def tiles(shape):
    """(NI, NJ, NK) of a grid: z, the caller's stride-1 axis, is the column axis."""
    tx, ty, tz, _ = column_constants()
    return tile_count(shape[0], tx), tile_count(shape[1], ty), tile_count(shape[2], tz)


def column_eligible(shape):
    """use_column, as far as the grid decides it: a column's tiles fit the bits of a mask word."""
    return tiles(shape)[2] <= column_constants()[3]


def in_place_eligible(shape):
    """column_in_place, as far as the grid decides it: the caller's rows are whole tiles long.  (The boxes have to be
    64-byte aligned as well, and TTSWEEP_OPT_TILE_IN_PLACE must not be 0.)"""
    return column_eligible(shape) and shape[2] % column_constants()[2] == 0


def order_default(shape, at_start, least, largest):
    """column_order_default: the sequence of orderings for a start from the velocity values of its vertical line
    (float32 arithmetic, as there)."""
    at_start, least, largest = np.float32(at_start), np.float32(least), np.float32(largest)
    rng = np.float32(largest - least)
    f = np.float32((at_start - least) / rng) if rng > 0 else np.float32(0.5)
    if f < np.float32(0.15):
        return 111, "fast end"
    if f > np.float32(0.85) and shape[2] >= max(shape[0], shape[1]):
        return 111, "slow end"
    return 115, "middle"


def default_orders(shape, v, starts):
    out = []
    for i, j, k in np.asarray(starts).reshape(-1, 3):
        line = v[i, j, :]
        out.append(order_default(shape, line[k], line.min(), line.max()))
    return out


# ---------------------------------------------------------------------------
# A: tall columns
# ---------------------------------------------------------------------------

# (shape, NK, runs as column pipelines?, in the caller's own arrays?)
TALL_GRIDS = [
    ((8, 8, 992), 31, True, True),         # whole rows, in place
    ((9, 8, 1024), 32, True, True),        # in place, ragged x
    ((17, 3, 1000), 32, True, False),      # last tile 8 live cells, padded volumes
    ((3, 10, 1025), 33, False, False),     # one cell too tall: hyperplane launches by rule
    ((12, 9, 1056), 33, False, False),     # whole rows, still too tall
]
NK32_GRIDS = [g[0] for g in TALL_GRIDS if g[1] == 32]
VELOCITIES = ("random", "graded")


def grid_id(shape):
    return "x".join(str(n) for n in shape)


def tall_starts(shape):
    """(0, 0, 0), the far corner, the first cell of the top tile, the last cell of the tile below it, mid-column."""
    nx, ny, nz = shape
    tz = column_constants()[2]
    top = tz * (tiles(shape)[2] - 1)
    return np.array([(0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx // 2, ny // 2, top), (nx // 3, ny - 1, top - 1),
                     (nx - 1, ny // 3, nz // 2)], dtype=np.int32)


def velocity(shape, kind="random", seed=SEED):
    """random: seeded uniform(0.1, 0.5), rough - it costs many sweeps.  graded: delay per distance falling from 0.4
    at z = 0 to 0.15 at the far end with 5 % noise, so that z = 0 is the slow end of every vertical line, the far
    end its fast end and the middle its middle."""
    rng = np.random.default_rng(seed + sum(shape))
    if kind == "random":
        return rng.uniform(0.1, 0.5, size=shape).astype(np.float32)
    assert kind == "graded", kind
    grade = np.linspace(0.4, 0.15, shape[2], dtype=np.float64)[None, None, :]
    return (grade * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=shape))).astype(np.float32)


def damage(box, start):
    """A converged box made a state above its fixed point: a block back at INFINITY that spans the two top tiles of
    its columns, a slab across the middle raised by x 1.5, the start back at 0.  Nothing is lowered."""
    shape = box.shape
    nx, ny, nz = shape
    tz = column_constants()[2]
    top = tz * (tiles(shape)[2] - 1)
    out = box.copy()
    z0, z1 = max(top - 12, 0), min(top + 12, nz)
    out[nx // 4: nx // 4 + 9, ny // 3: ny // 3 + 5, z0:z1] = INF
    out[: max(nx // 2, 1), :, nz // 2 - 3: nz // 2 + 3] *= np.float32(1.5)
    out[tuple(start)] = 0
    assert (out >= box).all() and np.isinf(out).any() and (out[np.isfinite(out)] > box[np.isfinite(out)]).any()
    if top > 0:
        assert z0 < top < z1, "the block spans the two top tiles"
    return out


def damage_heavy(box, start):
    """damage(), and all but the eighth of the box with the smallest x back at INFINITY: nearly a fresh solve's work
    again, from a state that still holds converged values."""
    out = damage(box, start)
    out[max(box.shape[0] // 8, 1):, :, :] = INF
    out[tuple(start)] = 0
    return out


# ---------------------------------------------------------------------------
# B: many starts
# ---------------------------------------------------------------------------

MANY_GRIDS = [(9, 8, 64), (17, 16, 97)]
MANY = 70


def many_starts(shape):
    """70 seeded starts: starts 0 and 64 (one lane of the work counters, s & 63) are the two extreme corners, in
    different tiles; start 5 repeats start 4."""
    rng = np.random.default_rng(SEED + 7 + sum(shape))
    st = np.stack([rng.integers(0, n, size=MANY) for n in shape], axis=1).astype(np.int32)
    st[0] = (0, 0, 0)
    st[64] = tuple(n - 1 for n in shape)
    st[5] = st[4]
    return st


def tile_of(shape, cell):
    tx, ty, tz, _ = column_constants()
    return (int(cell[0]) // tx, int(cell[1]) // ty, int(cell[2]) // tz)


# ---------------------------------------------------------------------------
# C, D, E
# ---------------------------------------------------------------------------

ANY_ADDRESS_GRID = (20, 37, 96)             # kernel 3; E uses it too
ANY_ADDRESS_STARTS = np.array([(3, 30, 7), (19, 0, 95)], dtype=np.int32)
ANY_ADDRESS_OFFSETS = (1, 8, 16)            # floats: 4, 32 and 64 bytes
GUARD = 64                                  # poisoned floats in front of and behind the boxes

# The hand-over: the first of these whose unlimited one-launch solve of handover_starts() reads solve_ms >= 5 in each
# of five runs (five times the 1 ms limit).  Measured on an MI355X: see test_gpu_column_limits.py.
HANDOVER_CANDIDATES = [(72, 64, 256), (96, 96, 256), (128, 128, 256)]


def handover_starts(shape):
    return np.array([(shape[0] // 3, shape[1] // 2, shape[2] // 2), (shape[0] - 2, 1, 40)], dtype=np.int32)


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

def six_offsets():
    """The 6-neighbour star (data/stars/six-FS.txt): a count, then the triples; the last entry is the reference's
    exclusive bound."""
    words = open(os.path.join(ROOT, "data", "stars", "six-FS.txt")).read().split()
    n = int(words[0])
    return np.array(words[1:1 + 3 * n], dtype=np.int32).reshape(n, 3)


def fresh_boxes(shape, starts):
    """One box per start as the reference initialises it: INFINITY, 0 at the start."""
    out = []
    for st in np.asarray(starts).reshape(-1, 3):
        tt = np.full(shape, np.inf, dtype=np.float32)
        tt[tuple(st)] = 0
        out.append(tt)
    return out


def oracle_boxes(oracle, v, offs, starts):
    """oracle.converge(order=1) per start, a few at a time (the checker runs outside the interpreter lock); every
    box has to be finite with 0 at its start."""
    fs = oracle.make_star(offs)
    starts = np.asarray(starts).reshape(-1, 3)
    with ThreadPoolExecutor(max_workers=8) as pool:
        out = list(pool.map(lambda st: oracle.converge(v, fs, st, order=1)[0], starts))
    for st, box in zip(starts, out):
        assert np.isfinite(box).all() and box[tuple(st)] == 0 and (box >= 0).all(), f"oracle box of start {tuple(st)}"
    return out
