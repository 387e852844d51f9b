#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the REFERENCE ITSELF.

Runs only where the reference checkout exists (this container): it drives the
unmodified reference translation unit (oracle/_ref/libttref.so, built by
oracle/Makefile from /root/reference/serial_new/sweep-tt-multistart.c) and
records inputs and the reference's outputs.  The fixtures are data only
(velocity values, star offsets, start points, travel times, change counts).

  python tests/golden/make_golden.py            # small fixtures (seconds)
  python tests/golden/make_golden.py --big      # + 241x241x51 digests (minutes)
  python tests/golden/make_golden.py --float-range   # float_range.npz only (seconds)
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as O  # noqa: E402


def synth(nx, ny, nz, seed):
    """SURVEY.md Appendix C model."""
    i = np.arange(nx)[:, None, None]
    j = np.arange(ny)[None, :, None]
    k = np.arange(nz)[None, None, :]
    base = (0.18 + 0.10 * k / (nz - 1) + 0.02 * np.sin(i / 9) * np.cos(j / 11)).astype(np.float32)
    u = np.random.default_rng(seed).uniform(-0.005, 0.005, size=(nx, ny, nz))
    return base + u.astype(np.float32)


def shipped(name):
    return O.read_triples(os.path.join(ROOT, "data", "stars", f"{name}-FS.txt"))


# deliberately NOT point-symmetric; the last entry is excluded by the reference's
# exclusive bound (serial_new/sweep-tt-multistart.c:160)
NONSYM = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, -1, 0], [0, -1, -1], [2, 1, -1]], np.int32)
# 6-neighbour shell + a sacrificial last entry
SIX = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1], [1, 1, 1]], np.int32)


def stars():
    return {"3": shipped("3"), "5": shipped("5"), "818": shipped("818"), "nonsym": NONSYM, "six": SIX}


def start_set(shape, offs):
    n = np.array(shape)
    last = np.array(offs[-1])
    mid = n // 2
    # "deadin": start - off[last] lies inside the grid (the dead edge of SURVEY 0-3 exists);
    # "deadout": it lies outside (no dead edge)
    deadin = np.clip(mid + [0, 1, 0], np.maximum(last, 0), n - 1 + np.minimum(last, 0))
    deadout = np.array([n[0] // 3, n[1] // 3, n[2] - 1])
    ax = int(np.flatnonzero(last)[0])
    deadout[ax] = 0 if last[ax] > 0 else n[ax] - 1
    assert np.all(deadin - last >= 0) and np.all(deadin - last < n) and np.all(deadin < n)
    assert np.any(deadout - last < 0) or np.any(deadout - last >= n)
    return {"mid": mid, "corner": np.array([0, 0, 0]), "deadin": deadin, "deadout": deadout}


def small_fixtures():
    grids = {"g24": ((24, 20, 12), 1), "g9": ((9, 7, 5), 2)}
    for gname, (shape, seed) in grids.items():
        v = synth(*shape, seed)
        out = {"v": v}
        meta = {}
        for sname, offs in stars().items():
            out[f"star_{sname}"] = offs
            for stname, st in start_set(shape, offs).items():
                st = np.asarray(st, np.int32)
                (tt,), sweeps = O.ref_converge(v, offs, [st])
                key = f"{sname}_{stname}"
                out[f"tt_{key}"] = tt
                out[f"start_{key}"] = st
                meta[key] = {"sweeps": int(sweeps)}
        # order-dependent single-pass states + change counts pin the sweep body itself
        for sname in ("3", "818", "nonsym"):
            offs = stars()[sname]
            st = np.asarray(start_set(shape, offs)["mid"], np.int32)
            R = O.ref()
            assert R.ttref_setup(*shape, v.reshape(-1), len(offs), offs.reshape(-1).copy(), 10.0, 1,
                                 st.copy())
            counts = []
            for n in range(3):
                counts.append(R.ttref_sweep_default(0))
                out[f"pass{n + 1}_{sname}"] = np.ctypeslib.as_array(R.ttref_tt(0), shape=shape).copy()
            R.ttref_teardown()
            meta[f"pass_{sname}"] = {"counts": counts, "start": st.tolist()}
        # a sub-range of the star (general starstart/starstop)
        offs = stars()["3"]
        st = np.asarray(start_set(shape, offs)["mid"], np.int32)
        (tt,), sweeps = O.ref_converge(v, offs, [st], starstart=5, starstop=60)
        out["tt_3_range_5_60"] = tt
        meta["3_range_5_60"] = {"sweeps": int(sweeps), "start": st.tolist()}
        # the scaled lengths the reference main() computes (:122,:127)
        R = O.ref()
        offs = stars()["818"]
        assert R.ttref_setup(*shape, v.reshape(-1), len(offs), offs.reshape(-1).copy(), 10.0, 1,
                             np.zeros(3, np.int32))
        out["fs_d_818"] = np.array([R.ttref_fs_d(l) for l in range(len(offs))], np.float32)
        R.ttref_teardown()
        out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(HERE, f"{gname}.npz"), **out)
        print(gname, "cases:", len(meta))


def vbox_fixture():
    """A VBOX file written by the reference writer: pins the byte format + checksum."""
    v = synth(6, 5, 4, 3)
    v[1, 2, 3] = -1.5           # bytes >= 0x80 in every position
    path = os.path.join(HERE, "ref_written_6x5x4.vbox")
    assert O.ref().ttref_store_vbox(path.encode(), 1, 1, 1, 6, 5, 4, v.reshape(-1).copy())
    np.save(os.path.join(HERE, "ref_written_6x5x4_values.npy"), v)
    print("vbox fixture", os.path.getsize(path), "bytes")


def live_fixture():
    """The reference's answers on the random inputs of tests/test_oracle.py::test_against_live_reference
    and its reader / writer on the box of tests/test_headers.py::test_reference_reader_accepts_our_writer,
    so that both tests run where the reference is absent."""
    out, meta = {}, {}
    rng = np.random.default_rng(7)
    n = 0
    for shape in ((13, 9, 8), (6, 17, 10)):
        v = rng.uniform(0.1, 0.4, size=shape).astype(np.float32)
        for n_off in (5, 40):
            offs = rng.integers(-3, 4, size=(n_off, 3)).astype(np.int32)
            offs = offs[np.any(offs != 0, axis=1)]
            start = np.array([int(rng.integers(0, m)) for m in shape], np.int32)
            (tt,), sweeps = O.ref_converge(v, offs, [start])
            out.update({f"v_{n}": v, f"offs_{n}": offs, f"start_{n}": start, f"tt_{n}": tt})
            meta[str(n)] = {"sweeps": int(sweeps)}
            n += 1
    # the reference writer's file for that box, and what the reference reader makes of it
    v = synth(5, 4, 3, 9)
    v[0, 0, 0] = -2.0
    path = os.path.join(HERE, "_vbox_tmp.vbox")
    assert O.ref().ttref_store_vbox(path.encode(), 2, 3, 4, 5, 4, 3, v.reshape(-1).copy())
    hdr = np.zeros(6, np.int32)
    got = np.zeros(v.size, np.float32)
    assert O.ref().ttref_load_vbox(path.encode(), hdr, got, got.size) == 1
    assert hdr.tolist() == [2, 3, 4, 5, 4, 3] and np.array_equal(got.reshape(v.shape), v)
    out["vbox_values"] = v
    out["vbox_bytes"] = np.frombuffer(open(path, "rb").read(), np.uint8)
    os.remove(path)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "live_ref.npz"), **out)
    print("live_ref cases:", len(meta))


# ---------------------------------------------------------------------------
# the ends of the float range (float_range.npz)
# ---------------------------------------------------------------------------

# 0x116c3: a subnormal star length whose half is not a float (odd last bit); 0x116c4 is the next
# length up, and both halve to the same float
ODD_SUBNORMAL = int(0x116c3)


def f32_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def asym_star():
    """A random, not point-symmetric star of radius 2 (12 distinct non-zero offsets; the last one
    is the entry the reference's exclusive bound leaves out)."""
    rng = np.random.default_rng(4242)
    offs = []
    while len(offs) < 12:
        o = tuple(int(x) for x in rng.integers(-2, 3, size=3))
        if o != (0, 0, 0) and o not in offs and tuple(-x for x in o) not in offs:
            offs.append(o)
    return np.array(offs, np.int32)


def dup_star():
    """The 6-neighbour shell at length 0x116c4 with +x a second time at 0x116c3 (one subnormal step
    shorter: the shorter edge is the one that counts), and a sacrificial last entry."""
    offs = np.concatenate([SIX[:6], [[1, 0, 0]], SIX[6:]]).astype(np.int32)
    d = np.full(len(offs), 0x116c4, np.uint32)
    d[6] = ODD_SUBNORMAL
    d[-1] = 0
    return offs, d


def float_range_cases():
    """(case, shape, v, delta, star names, starts).  Stars: "six" (the shipped 6-FS), "5" (5-FS),
    "asym" (asym_star), "dup" (dup_star, with its own lengths)."""
    rng = np.random.default_rng(2026)

    def logu(lo, hi, shape):
        return (10.0 ** rng.uniform(np.log10(lo), np.log10(hi), size=shape)).astype(np.float32)

    every = ("six", "5", "asym")
    cases = []
    # (a) travel times overflow partway across the grid; delays finite
    shape = (16, 14, 12)
    cases.append(("overflow_tt", shape, logu(2e36, 1.6e37, shape), 10.0, every,
                  [(8, 7, 6), (0, 0, 0), (15, 2, 11)]))
    # ... and the same below 2^126 / d_max (six: 8.5e36, asym: 2.5e36), where the fast kernels stay
    cases.append(("overflow_tt_fast", shape, logu(1.2e36, 2.4e36, shape), 10.0, ("six", "asym"),
                  [(8, 7, 6), (0, 13, 0)]))
    # (b) the band where d (v[c] + v[o]) overflows while d / 2 (v[c] + v[o]) does not (for d = 10:
    # sums in [3.4e37, 6.8e37)), around a start in a slower region
    shape = (12, 10, 9)
    v = logu(1.2e37, 3.4e37, shape)
    v[4:8, 3:7, 3:6] = logu(1e35, 1e36, (4, 4, 3))
    cases.append(("overflow_delay", shape, v, 10.0, every, [(6, 5, 4), (0, 9, 8)]))
    # (c) blocks where the pair sum itself is infinite; one start inside one of them
    shape = (14, 12, 10)
    v = synth(*shape, 11)
    v[2:6, 3:9, 1:5] = logu(1.8e38, 3.4e38, (4, 6, 4))
    v[9:13, 0:4, 6:10] = np.float32(3.4028235e38)
    cases.append(("inf_sum", shape, v, 10.0, every, [(7, 6, 5), (3, 5, 2)]))
    # (d) a star length with an inexact half: ordinary velocities (denormal delays) and v ~ 1e30
    shape = (12, 10, 9)
    odd = float(f32_bits(ODD_SUBNORMAL))
    cases.append(("odd_delta", shape, synth(*shape, 12), odd, every, [(6, 5, 4), (0, 0, 0)]))
    cases.append(("odd_delta_1e30", shape, logu(1e30, 3e30, shape), odd, every, [(6, 5, 4), (11, 0, 8)]))
    # (e) ordinary lengths other than delta = 10
    cases.append(("delta_0.37", shape, synth(*shape, 13), 0.37, every, [(6, 5, 4), (0, 9, 0)]))
    cases.append(("delta_2500", shape, synth(*shape, 14), 2500.0, every, [(6, 5, 4), (11, 9, 8)]))
    # (f) the same offset twice, lengths one subnormal step apart
    cases.append(("dup_offset", shape, logu(1e30, 3e30, shape), 10.0, ("dup",), [(6, 5, 4), (0, 3, 2)]))
    return cases


def ref_fixed_point(v, offs, fs_d_bits, delta, start, max_passes=2000):
    """Step the reference's own sweepXYZ (call-site bounds, :160) one pass at a time up to the first
    pass that changes no bit.  Returns (box, passes, stores of that last pass, the reference's fs[].d
    bits).  Where a travel time overflows, that pass still stores (INFINITY over INFINITY) and the
    reference's own loop would go on for ever."""
    R = O.ref()
    shape = v.shape
    st = np.asarray(start, np.int32)
    assert R.ttref_setup(*shape, np.ascontiguousarray(v).reshape(-1), len(offs),
                         np.ascontiguousarray(offs).reshape(-1).copy(), np.float32(delta), 1, st.copy())
    if fs_d_bits is not None:
        for l, b in enumerate(fs_d_bits):
            R.ttref_set_fs_d(l, f32_bits(b))
    d_bits = np.array([R.ttref_fs_d(l) for l in range(len(offs))], np.float32).view(np.uint32)
    tt = np.ctypeslib.as_array(R.ttref_tt(0), shape=shape)
    passes = 0
    while True:
        before = tt.copy()
        stores = R.ttref_sweep(0, 0, len(offs) - 1)
        passes += 1
        if np.array_equal(before.view(np.uint32), tt.view(np.uint32)):
            break
        assert passes < max_passes
    box = tt.copy()
    R.ttref_teardown()
    return box, passes, int(stores), d_bits


def float_range_fixture():
    """tests/golden/float_range.npz: the reference's fixed points at both ends of the float range."""
    star_offs = {"six": SIX, "5": shipped("5"), "asym": asym_star(), "dup": dup_star()[0]}
    out = {f"star_{k}": o for k, o in star_offs.items()}
    meta = {}
    for case, shape, v, delta, snames, starts in float_range_cases():
        out[f"v_{case}"] = v
        for sname in snames:
            key = f"{case}/{sname}"
            d_in = dup_star()[1] if sname == "dup" else None
            boxes, rec = [], {"case": case, "star": sname, "starts": [list(s) for s in starts],
                              "delta_bits": int(np.float32(delta).view(np.uint32)),
                              "hand_made_d": d_in is not None, "passes": [], "last_stores": []}
            for st in starts:
                box, passes, stores, d_bits = ref_fixed_point(v, star_offs[sname], d_in, delta, st)
                boxes.append(box)
                rec["passes"].append(passes)
                rec["last_stores"].append(stores)
            rec["ninf"] = [int(np.isinf(b).sum()) for b in boxes]
            out[f"tt_{key}"] = np.stack(boxes)
            out[f"fsd_{key}"] = d_bits
            meta[key] = rec
            print(key, "passes", rec["passes"], "last-pass stores", rec["last_stores"], "INF cells", rec["ninf"])
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "float_range.npz"), **out)
    print("float_range cases:", len(meta), os.path.getsize(os.path.join(HERE, "float_range.npz")), "bytes")


def big_digests():
    """Converged 241x241x51 boxes of the reference: SHA-256 + spot values only."""
    v = synth(241, 241, 51, 20160507)
    res = {}
    path = os.path.join(HERE, "big_digests.json")
    if os.path.exists(path):
        res = json.load(open(path))
    for sname, st in (("3", (120, 120, 50)), ("818", (120, 120, 50))):
        key = f"syn241_{sname}_{st[0]}_{st[1]}_{st[2]}"
        if key in res:
            continue
        t0 = time.time()
        (tt,), sweeps = O.ref_converge(v, shipped(sname), [np.array(st, np.int32)])
        spots = [(0, 0, 0), (113, 119, 49), (118, 118, 49), (240, 240, 0), (0, 240, 50), (60, 200, 25)]
        res[key] = {
            "sha256": hashlib.sha256(tt.tobytes()).hexdigest(),
            "sweeps": int(sweeps),
            "seconds": round(time.time() - t0, 1),
            "spots": {",".join(map(str, p)): int(tt[p].view(np.uint32)) for p in spots},
            "max": float(tt.max()), "mean": float(tt.astype(np.float64).mean()),
        }
        print(key, res[key]["sha256"], sweeps, "sweeps", res[key]["seconds"], "s", flush=True)
        json.dump(res, open(path, "w"), indent=1)


def big_start24(idx, which="24", star="818"):
    """One start of a BASELINE start file (start-24 by default, --big-file 4 for start-4) on
    the 241x241x51 model, 818-FS, through the reference; written to its own file so several
    can run in parallel (merge_big)."""
    v = synth(241, 241, 51, 20160507)
    starts = O.read_triples(os.path.join(ROOT, "data", "starts", f"start-{which}-241-241-51.txt"))
    st = starts[idx]
    t0 = time.time()
    (tt,), sweeps = O.ref_converge(v, shipped(star), [st.astype(np.int32)])
    res = {f"syn241_{star}_{st[0]}_{st[1]}_{st[2]}": {
        "sha256": hashlib.sha256(tt.tobytes()).hexdigest(), "sweeps": int(sweeps),
        "seconds": round(time.time() - t0, 1), "spots": {}, f"start{which}_index": int(idx),
        "max": float(tt.max()), "mean": float(tt.astype(np.float64).mean())}}
    json.dump(res, open(os.path.join(HERE, f"big_part_{star}_{which}_{idx}.json"), "w"), indent=1)
    print(res, flush=True)


def merge_big():
    path = os.path.join(HERE, "big_digests.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    for f in sorted(os.listdir(HERE)):
        if f.startswith("big_part_") and f.endswith(".json"):
            res.update(json.load(open(os.path.join(HERE, f))))
            os.remove(os.path.join(HERE, f))
    json.dump(res, open(path, "w"), indent=1)
    print(sorted(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--big-start", type=int, default=None)
    ap.add_argument("--big-file", default="24")
    ap.add_argument("--big-star", default="818")
    ap.add_argument("--merge-big", action="store_true")
    ap.add_argument("--float-range", action="store_true")
    args = ap.parse_args()
    if args.big_start is not None:
        big_start24(args.big_start, args.big_file, args.big_star)
        sys.exit(0)
    if args.merge_big:
        merge_big()
        sys.exit(0)
    if O.ref() is None:
        sys.exit("reference not available: golden vectors can only be generated beside /root/reference")
    if args.float_range:
        float_range_fixture()
        sys.exit(0)
    small_fixtures()
    vbox_fixture()
    live_fixture()
    if args.big:
        big_digests()
