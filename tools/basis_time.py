#!/usr/bin/env python3
"""GPU box: the products with a basis of another width (bcg_basis_dot, bcg_basis_axpy) at 64^4 in a fresh process.

  basis_time.py [--out PATH]     default PATH: profiles/basis_time.json

4 warm-up + 20 timed rounds, HIP-event times from the per-kernel profile.  A round is: yardstick, new call, yardstick again --
the yardstick and the new call alternate in one process, and the two yardstick series give the yardstick's own spread.
  * V = two fields of 32 columns, m = 16 (memory-bound by arithmetic: 8 flop per byte):
      basis_dot(V, b)        beside hermitian_dot(a, b) at m = 16, kernel + reduction on both sides;
      basis_axpy(y, V, C)    beside y.add(rhs, M) at m = 16 (beta = 1; beta = 0 is recorded as well).
    Compared in time per byte of the byte models (48 (K_g + m) per site and group for the dot, 48 (K_g + 2 m) for the update,
    2 x 48 m and 3 x 48 m for the yardsticks); the new call may take up to 1.25 x the yardstick's time per byte.
  * V = two fields of 32 columns, m = 32 (16 flop per byte: bound by the fp64 matrix pipe): TFLOP/s recorded, no ratio.
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, WARMUP, TIMED = [64, 64, 64, 64], 4, 20


def child():
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(DIMS)
    ctx.profiling(True)

    def once(call, keys):
        ctx.profile_reset()
        call()
        prof = ctx.profile()
        ms = sum(prof[k]["ms"] for k in keys if k in prof)
        return ms, prof[keys[0]]["bytes"], prof[keys[0]].get("flops", 0.0), prof[keys[0]]["count"]

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
                 "launches_per_call": launches, "bytes": nbytes, "TB_per_s": round(nbytes / (np.median(t) * 1e-3) / 1e12, 3),
                 "ns_per_MB": round(float(np.median(t)) * 1e6 / (nbytes / 1e6), 4)}
            if flops:
                e["TFLOP_per_s"] = round(flops / (np.median(t) * 1e-3) / 1e12, 2)
            out[name] = e
        return out

    def compare(r, new, first, second):
        y1, y2 = r[first]["ns_per_MB"], r[second]["ns_per_MB"]
        r[new + "_time_per_byte_over_yardstick"] = round(r[new]["ns_per_MB"] / (0.5 * (y1 + y2)), 3)
        r[new + "_yardstick_spread"] = round(abs(y1 - y2) / (0.5 * (y1 + y2)), 4)

    out = {"dims": DIMS, "warmup": WARMUP, "timed": TIMED, "timing": "HIP events, ms per call; yardstick and new call alternate"}
    V = [bc.block_fermion_field(ctx, 32).setGaussian(1 + k) for k in range(2)]
    rng = np.random.default_rng(1)
    for m in (16, 32):
        C = (rng.standard_normal((64, m)) + 1j * rng.standard_normal((64, m))) / 64.0
        M = (rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))) / m
        a = bc.block_fermion_field(ctx, m).setGaussian(11)
        b = bc.block_fermion_field(ctx, m).setGaussian(12)
        y = bc.block_fermion_field(ctx, m).setGaussian(13)
        gram_keys, dot_keys = ["gram_pair", "reduce_partials"], ["basis_dot", "basis_fold"]
        r = series([("hermitian_dot_first", lambda: a.hermitian_dot(b), gram_keys),
                    ("basis_dot", lambda: bc.basis_dot(V, b), dot_keys),
                    ("hermitian_dot_second", lambda: a.hermitian_dot(b), gram_keys)])
        compare(r, "basis_dot", "hermitian_dot_first", "hermitian_dot_second")
        # the updates shrink y a little every call (beta = 1 with small coefficients keeps it finite over 3 x 24 calls)
        r.update(series([("add_matrix_first", lambda: y.add(a, M * 1e-3), ["block_axpy"]),
                         ("basis_axpy", lambda: bc.basis_axpy(y, V, C * 1e-3, 1.0), ["basis_axpy"]),
                         ("add_matrix_second", lambda: y.add(a, M * 1e-3), ["block_axpy"]),
                         ("basis_axpy_beta0", lambda: bc.basis_axpy(y, V, C, 0.0), ["basis_axpy"])]))
        compare(r, "basis_axpy", "add_matrix_first", "add_matrix_second")
        compare(r, "basis_axpy_beta0", "add_matrix_first", "add_matrix_second")
        out[f"V32x2_m{m}"] = r
        del a, b, y
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child()))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "basis_time.json")
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
