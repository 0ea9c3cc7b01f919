#!/usr/bin/env python3
"""GPU box: a basis put onto slices (bcg_basis_slice_axpy) at 64^4 in a fresh process.

  basis_slice_axpy_time.py [--out PATH]     default PATH: profiles/basis_slice_axpy_time.json

4 warm-up + 20 timed rounds, HIP-event times from the per-kernel profile (keys basis_slice_axpy and basis_slice_scale, summed
over the launches of a call), medians.
  * V = two fields of 32 columns, m = 16 and m = 32, beta = 1: a round is yardstick, new call, yardstick again.  The yardstick
    is bcg_basis_axpy on the same fields in the same process; with all slices listed along direction 3 and no momentum the
    new call moves the same bytes, is compared time against time and may take up to 1.25 x the yardstick.
  * Recorded with no ratio attached, as TB/s and TFLOP/s on the byte model (48 (K_g + 2 m) bytes per listed site and launch,
    48 (K_g + m) at beta = 0, 8 K_g m flops per row; the slices that are not listed: 48 m per site written, and read unless
    beta = 0): directions 0, 1 and 2; the phase instantiation; one listed slice at beta = 1 and at beta = 0; one generic
    shape, V = [12, 12] at m = 12 (beside its own bcg_basis_axpy).
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, WARMUP, TIMED = [64, 64, 64, 64], 4, 20
NEW_KEYS, OLD_KEYS = ["basis_slice_axpy", "basis_slice_scale"], ["basis_axpy"]


def child():
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(DIMS)
    ctx.profiling(True)
    rng = np.random.default_rng(3)

    def once(call, keys):
        ctx.profile_reset()
        call()
        prof = ctx.profile()
        ms = sum(prof[k]["ms"] for k in keys if k in prof)
        nbytes = sum(prof[k]["bytes"] for k in keys if k in prof)
        return ms, nbytes, prof[keys[0]].get("flops", 0.0), prof[keys[0]]["count"]

    def series(rounds):
        """rounds: (name, call, keys) triples run in turn, WARMUP + TIMED times; per name the ms of every timed round"""
        for _ in range(WARMUP):
            for _, call, keys in rounds:
                once(call, keys)
        ms = {name: [] for name, _, _ in rounds}
        meta = {}
        for _ in range(TIMED):
            for name, call, keys in rounds:
                t, nbytes, flops, launches = once(call, keys)
                ms[name].append(t)
                meta[name] = (nbytes, flops, launches)
        out = {}
        for name, _, _ in rounds:
            t = np.asarray(ms[name])
            nbytes, flops, launches = meta[name]
            e = {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                 "launches_per_call": launches, "bytes": nbytes, "TB_per_s": round(nbytes / (np.median(t) * 1e-3) / 1e12, 3)}
            if flops:
                e["TFLOP_per_s"] = round(flops / (np.median(t) * 1e-3) / 1e12, 2)
            out[name] = e
        return out

    def coeff(S, K, m):  # small, so that beta = 1 over many rounds stays far from overflow
        return 1e-3 * (rng.standard_normal((S, K, m)) + 1j * rng.standard_normal((S, K, m)))

    out = {"dims": DIMS, "warmup": WARMUP, "timed": TIMED, "timing": "HIP events, ms per call; yardstick and new call alternate"}
    V = [bc.block_fermion_field(ctx, 32).setGaussian(1 + k) for k in range(2)]
    L = DIMS[3]
    for m in (16, 32):
        y = bc.block_fermion_field(ctx, m).setGaussian(12)
        C = coeff(L, 64, m)
        r = series([("basis_axpy_first", lambda: bc.basis_axpy(y, V, C[0], 1.0), OLD_KEYS),
                    ("basis_slice_axpy_dir3", lambda: bc.basis_slice_axpy(y, V, C, 3, None, None, 1.0), NEW_KEYS),
                    ("basis_axpy_second", lambda: bc.basis_axpy(y, V, C[0], 1.0), OLD_KEYS)])
        y1, y2 = r["basis_axpy_first"]["ms_median"], r["basis_axpy_second"]["ms_median"]
        r["basis_slice_axpy_dir3_over_basis_axpy"] = round(r["basis_slice_axpy_dir3"]["ms_median"] / (0.5 * (y1 + y2)), 3)
        r["yardstick_spread"] = round(abs(y1 - y2) / (0.5 * (y1 + y2)), 4)
        if m == 16:
            r.update(series([(f"basis_slice_axpy_dir{d}", lambda d=d: bc.basis_slice_axpy(y, V, C, d, None, None, 1.0), NEW_KEYS)
                             for d in (0, 1, 2)]))
            r.update(series([("basis_slice_axpy_dir3_phase", lambda: bc.basis_slice_axpy(y, V, C, 3, None, [1, 2, -1, 0], 1.0), NEW_KEYS),
                             ("basis_slice_axpy_dir3_one_slice_beta1", lambda: bc.basis_slice_axpy(y, V, C[:1], 3, [5], None, 1.0), NEW_KEYS),
                             ("basis_slice_axpy_dir3_one_slice_beta0", lambda: bc.basis_slice_axpy(y, V, C[:1], 3, [5], None, 0.0), NEW_KEYS)]))
        out[f"V32x2_m{m}"] = r
        del y
    del V
    V = [bc.block_fermion_field(ctx, 12).setGaussian(21 + k) for k in range(2)]
    y = bc.block_fermion_field(ctx, 12).setGaussian(23)
    C = coeff(L, 24, 12)
    out["V12x2_m12"] = series([("basis_axpy", lambda: bc.basis_axpy(y, V, C[0], 1.0), OLD_KEYS),
                               ("basis_slice_axpy_dir3", lambda: bc.basis_slice_axpy(y, V, C, 3, None, None, 1.0), NEW_KEYS)])
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child()))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "basis_slice_axpy_time.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(json.dumps({"error": r.returncode, "stderr": r.stderr[-2000:]}))
        sys.exit(1)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    with open(path, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
