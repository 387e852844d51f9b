"""CPU tier: both ends of the float range, pinned to the reference (tests/golden/float_range.npz,
recorded by make_golden.py --float-range from the unmodified reference).

The cases: travel times that overflow partway across the grid (v ~ 1e36-1e37), delays whose
product d (v[c] + v[o]) overflows while d / 2 times the sum does not, blocks where the pair sum
itself is infinite, a star length whose half is not a float (the subnormal 0x116c3), with ordinary
velocities and with v ~ 1e30, lengths from delta = 0.37 and 2500, and a hand-made star with the
same offset twice at lengths one subnormal step apart.

Where a travel time overflows the reference's loop never ends (a finite cell beside an INFINITY one
stores INFINITY over INFINITY in every pass, serial_new/sweep-tt-multistart.c:228-237).  The
fixture holds the box at which it stands still, the pass that first changes no bit and that pass's
store count; the oracle stops there, and the validators count an edge as open only if a store
through it would change a value."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_equal

F32 = np.float32


@pytest.fixture(scope="module")
def fr():
    z = np.load(os.path.join(GOLDEN, "float_range.npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def star_of(z, key, m, make):
    """fs for case `key` through `make` (oracle.make_star or make_fs), hand-made lengths set."""
    fs = make(z[f"star_{m['star']}"], F32(np.uint32(m["delta_bits"]).view(F32)))
    if m["hand_made_d"]:
        fs["d"] = z[f"fsd_{key}"].view(F32)
    return fs


def test_fixture_covers_the_float_range(fr):
    """The recorded cases reach what they are meant to reach: INFINITY left beside finite cells with
    stores in the last pass (the reference would loop for ever), pair sums in the band where the
    reference's product overflows and the half-length product does not, infinite pair sums, lengths with
    an inexact half, and two parallel entries whose halves coincide."""
    z, meta = fr
    assert len(meta) == 24
    looping = {k for k, m in meta.items() if any(m["last_stores"])}
    assert {meta[k]["case"] for k in looping} >= {"overflow_tt", "overflow_tt_fast", "overflow_delay", "inf_sum"}
    for k in looping:
        assert all(n > 0 for n, c in zip(meta[k]["ninf"], meta[k]["last_stores"]) if c), k
    with np.errstate(over="ignore"):
        for key, m in meta.items():
            v, d = z[f"v_{m['case']}"], z[f"fsd_{key}"].view(F32)
            live = d[:-1]
            if m["case"] == "overflow_delay":
                s = (v[:-1] + v[1:]).astype(F32)                    # pair sums along x
                d1 = live[live > 0].min()                            # (the unit offsets)
                band = np.isinf(d1 * s) & np.isfinite((d1 * F32(0.5)) * s)
                assert band.any(), key
            if m["case"] == "inf_sum":
                assert np.isinf((v[:-1] + v[1:]).astype(F32)).any()
            if m["case"].startswith("odd_delta") or m["case"] == "dup_offset":
                h = live * F32(0.5)
                assert ((h + h) != live).any(), key
    d = z["fsd_dup_offset/dup"].view(np.uint32)
    assert sorted(d[[1, 6]].tolist()) == [0x116c3, 0x116c4]
    assert F32(d[1:2].view(F32)[0] * F32(0.5)) == F32(d[6:7].view(F32)[0] * F32(0.5))


def test_star_lengths_match_reference(fr, oracle, pkg):
    """make_fs(offs, delta) and oracle.make_star(offs, delta) give the reference's fs[].d bits, subnormal
    and non-default deltas included."""
    z, meta = fr
    for key, m in meta.items():
        if m["hand_made_d"]:
            continue
        for make in (oracle.make_star, pkg.inputs.make_fs):
            fs = star_of(z, key, m, make)
            assert np.array_equal(fs["d"].view(np.uint32), z[f"fsd_{key}"]), (key, make)


def test_oracle_stops_where_the_reference_stands_still(fr, oracle):
    """The oracle (reference order) ends at the recorded pass with the recorded box; one more pass over it
    stores exactly as often as the reference's last pass did and changes no bit; the eight orderings reach
    the same box."""
    z, meta = fr
    for key, m in meta.items():
        v = z[f"v_{m['case']}"]
        fs = star_of(z, key, m, oracle.make_star)
        for s, start in enumerate(m["starts"]):
            want = z[f"tt_{key}"][s]
            tt, sweeps, _ = oracle.converge(v, fs, start)
            assert sweeps == m["passes"][s], (key, start)
            assert_bit_equal(tt, want, f"{key} start {start}")
            again = tt.copy()
            assert oracle.sweep(v, again, fs, start) == m["last_stores"][s], (key, start)
            assert_bit_equal(again, want, f"{key} start {start}: the pass after rest")
            tt8, _, _ = oracle.converge(v, fs, start, order=1)
            assert_bit_equal(tt8, want, f"{key} start {start}, eight orderings")


def test_validators_report_rest(fr, oracle, pkg):
    """On every recorded box: oracle_validate and torch_checker report (0 open, the INFINITY count, 0 unsupported);
    on the state after one reference pass both count the same open edges (> 0)."""
    import torch
    from torch_checker import fixed_point_counts
    z, meta = fr
    for key, m in meta.items():
        v = z[f"v_{m['case']}"]
        ofs, fs = star_of(z, key, m, oracle.make_star), star_of(z, key, m, pkg.inputs.make_fs)
        tv = torch.from_numpy(v)
        for s, start in enumerate(m["starts"]):
            box = z[f"tt_{key}"][s]
            assert oracle.validate(v, box, ofs, start) == (0, m["ninf"][s]), (key, start)
            assert fixed_point_counts(tv, torch.from_numpy(box.copy()), fs, start) == (0, m["ninf"][s], 0), (key, start)
            if m["passes"][s] > 2:
                one = oracle.tt_init(v.shape, start)
                oracle.sweep(v, one, ofs, start)
                want = oracle.validate(v, one, ofs, start)
                got = fixed_point_counts(tv, torch.from_numpy(one), fs, start)
                assert want[0] > 0 and got[:2] == want and got[2] == 0, (key, start, got, want)


def test_recorder_reproduces_the_fixture_from_the_live_reference(fr, oracle):
    """Beside the reference checkout: make_golden.py's cases, run through the reference again, give the
    recorded velocities, lengths, boxes, pass numbers and last-pass store counts."""
    if oracle.ref() is None:
        pytest.skip("the reference build is not available here; the recorded fixture stands for it")
    sys.path.insert(0, GOLDEN)
    import make_golden as MG
    z, meta = fr
    offs = {"six": MG.SIX, "5": MG.shipped("5"), "asym": MG.asym_star(), "dup": MG.dup_star()[0]}
    n = 0
    for case, shape, v, delta, snames, starts in MG.float_range_cases():
        assert np.array_equal(v.view(np.uint32), z[f"v_{case}"].view(np.uint32)), case
        for sname in snames:
            key = f"{case}/{sname}"
            m = meta[key]
            for s, st in enumerate(starts):
                box, passes, stores, d_bits = MG.ref_fixed_point(
                    v, offs[sname], MG.dup_star()[1] if sname == "dup" else None, delta, st)
                assert (passes, stores) == (m["passes"][s], m["last_stores"][s]), (key, st)
                assert np.array_equal(d_bits, z[f"fsd_{key}"]), key
                assert_bit_equal(box, z[f"tt_{key}"][s], f"{key} start {st}: live reference")
            n += 1
    assert n == len(meta)
