#!/usr/bin/env python3
"""GPU box: the in-place rotation by slice (bcg_basis_slice_rotate) and one outer iteration of bcg_laplacian_modes, a fresh
process per case.  Timings only: nothing here checks a result.

  basis_slice_rotate_time.py [--out PATH]     default PATH: profiles/basis_slice_rotate_time.json

Rotation: 4 warm-up + 20 timed rounds, HIP-event times from the per-kernel profile, medians.  A round is yardstick, new call,
yardstick again; the yardstick is bcg_basis_rotate on the same fields in the same process, which with all slices listed moves
the same 96 K bytes per site.  Cases: 32^4 and 64^3 x 32, K = 64 as [16] x 4 and as [32] x 2, all slices along directions 3
and 0, and one listed slice along direction 3.  The matrices are unitary, so the fields keep their norm over the rounds.
Accepted: all slices along direction 3 at no more than 1.25 x the yardstick.

laplacian_modes: 64^3 x 32 along direction 3, V = [32, 16] of noise, 32 wanted, degree 16, device-drawn general links (a
bound of 40: every link has |U| <= sqrt(18)), max_iterations 1 against max_iterations 0 in the same process; the difference
of the two profiles is one outer iteration, split by profile key into filter, Gram, rotation and residuals.
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, TIMED = 4, 20
LATTICES = {"32x32x32x32": [32, 32, 32, 32], "64x64x64x32": [64, 64, 64, 32]}
WIDTHS = {"16x4": [16, 16, 16, 16], "32x2": [32, 32]}
MODES_DIMS, MODES_WIDTHS, MODES_WANT, MODES_DEGREE, MODES_BOUND = [64, 64, 64, 32], [32, 16], 32, 16, 40.0


def rotation_case(dims, widths):
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(dims)
    ctx.profiling(True)
    rng = np.random.default_rng(3)
    K = sum(widths)
    V = [bc.block_fermion_field(ctx, w).setGaussian(1 + k) for k, w in enumerate(widths)]

    def unitary(S):
        return np.stack([np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))[0] for _ in range(S)])

    def once(call, key):
        ctx.profile_reset()
        call()
        p = ctx.profile()[key]
        return p["ms"], p["bytes"], p.get("flops", 0.0)

    def series(rounds):
        for _ in range(WARMUP):
            for _, call, key in rounds:
                once(call, key)
        ms, meta = {name: [] for name, _, _ in rounds}, {}
        for _ in range(TIMED):
            for name, call, key in rounds:
                t, nbytes, flops = once(call, key)
                ms[name].append(t)
                meta[name] = (nbytes, flops)
        out = {}
        for name, _, _ in rounds:
            t = np.asarray(ms[name])
            nbytes, flops = meta[name]
            out[name] = {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                         "bytes": nbytes, "TB_per_s": round(nbytes / (np.median(t) * 1e-3) / 1e12, 3),
                         "TFLOP_per_s": round(flops / (np.median(t) * 1e-3) / 1e12, 2)}
        return out

    out = {}
    for direction in (3, 0):
        Q = unitary(dims[direction])
        r = series([("basis_rotate_first", lambda: bc.basis_rotate(V, Q[0]), "basis_rotate"),
                    ("basis_slice_rotate", lambda: bc.basis_slice_rotate(V, Q, direction), "basis_slice_rotate"),
                    ("basis_rotate_second", lambda: bc.basis_rotate(V, Q[0]), "basis_rotate")])
        y1, y2 = r["basis_rotate_first"]["ms_median"], r["basis_rotate_second"]["ms_median"]
        r["basis_slice_rotate_over_basis_rotate"] = round(r["basis_slice_rotate"]["ms_median"] / (0.5 * (y1 + y2)), 3)
        r["yardstick_spread"] = round(abs(y1 - y2) / (0.5 * (y1 + y2)), 4)
        out[f"dir{direction}_all_slices"] = r
    Q1 = unitary(1)
    out["dir3_one_slice"] = series([("basis_slice_rotate", lambda: bc.basis_slice_rotate(V, Q1, 3, [5]), "basis_slice_rotate")])
    return out


def modes_case():
    import torch  # noqa: F401
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(MODES_DIMS)
    ctx.profiling(True)
    links = bc.gauge_field(ctx).setRandom(5)
    profiles = {}
    for limit in (0, 1, 0, 1):  # the first pair warms up
        V = [bc.block_fermion_field(ctx, w).setGaussian(60 + k) for k, w in enumerate(MODES_WIDTHS)]
        ctx.profile_reset()
        r = bc.laplacian_modes(V, links, 3, MODES_WANT, MODES_BOUND, MODES_DEGREE, 1e-10, limit)
        profiles[limit] = (ctx.profile(), r["applications"])
        del V
    (p0, a0), (p1, a1) = profiles[0], profiles[1]
    nf = len(MODES_WIDTHS)
    delta = {k: {"ms": round(p1[k]["ms"] - p0.get(k, {}).get("ms", 0.0), 4), "count": p1[k]["count"] - p0.get(k, {}).get("count", 0)}
             for k in p1 if p1[k]["count"] != p0.get(k, {}).get("count", 0)}
    ms = lambda k: delta.get(k, {}).get("ms", 0.0)  # noqa: E731
    shift_each = ms("shift_sum") / (a1 - a0)  # every application is one shift_sum of one field
    split = {
        "filter_ms": round(shift_each * MODES_DEGREE * nf + ms("axpby") + ms("copy"), 3),
        "gram_ms": round(shift_each * nf + ms("basis_slice_dot") + ms("basis_slice_fold"), 3),
        "rotation_ms": round(ms("basis_slice_rotate"), 3),
        "residuals_ms": round(shift_each * nf + ms("basis_slice_axpy") + ms("slice_dot") + ms("slice_fold"), 3),
    }
    return {"dims": MODES_DIMS, "widths": MODES_WIDTHS, "degree": MODES_DEGREE, "applications_per_iteration": a1 - a0,
            "one_outer_iteration_by_key": delta, "one_outer_iteration": split,
            "total_ms": round(sum(split.values()), 3)}  # the form counters repeat the time of the launch they count


def child(args):
    if args[0] == "modes":
        return modes_case()
    return rotation_case(LATTICES[args[0]], WIDTHS[args[1]])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child(sys.argv[2:])))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "basis_slice_rotate_time.json")
    out = {"warmup": WARMUP, "timed": TIMED, "timing": "HIP events, ms per call; yardstick and new call alternate; timings only"}
    cases = [[lat, w] for lat in LATTICES for w in WIDTHS] + [["modes"]]
    for case in cases:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + case, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(json.dumps({"error": r.returncode, "case": case, "stderr": r.stderr[-2000:]}))
            sys.exit(1)
        out["laplacian_modes" if case == ["modes"] else f"{case[0]}_K64_{case[1]}"] = json.loads(r.stdout.strip().splitlines()[-1])
    with open(path, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
