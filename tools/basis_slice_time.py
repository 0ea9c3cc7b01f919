#!/usr/bin/env python3
"""GPU box: the per-slice products with a basis (bcg_basis_slice_dot) at 64^4 in a fresh process.

  basis_slice_time.py [--out PATH]     default PATH: profiles/basis_slice_time.json

4 warm-up + 20 timed rounds, HIP-event times from the per-kernel profile (keys basis_slice_dot and basis_slice_fold, summed
over the launches of a call), medians.
  * V = two fields of 32 columns, m = 16: a round is yardstick, new call, yardstick again.  The yardstick is bcg_basis_dot
    (kernel + fold) on the same fields in the same process; without momenta the plan gives one launch of 64 columns with the
    same bytes, so basis_slice_dot(V, b, 3) is compared time against time and may take up to 1.25 x the yardstick.
  * Recorded with no ratio attached, as TB/s and TFLOP/s on the byte model (48 (K_g + m) bytes per site and launch,
    8 K_g m pc flops per row): directions 0, 1 and 2; P = 1, 2, 4, 8 momenta along direction 3; m = 32 with V = 2 x 32 (beside
    its own bcg_basis_dot); one generic shape, V = [12, 12] at m = 12.
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, WARMUP, TIMED = [64, 64, 64, 64], 4, 20
MOMENTA = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0], [1, 0, 1, 0], [0, 1, 1, 0], [1, 1, 1, 0], [2, 0, 0, 0]]
SLICE_KEYS, DOT_KEYS = ["basis_slice_dot", "basis_slice_fold"], ["basis_dot", "basis_fold"]


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
                 "launches_per_call": launches, "bytes": nbytes, "TB_per_s": round(nbytes / (np.median(t) * 1e-3) / 1e12, 3)}
            if flops:
                e["TFLOP_per_s"] = round(flops / (np.median(t) * 1e-3) / 1e12, 2)
            out[name] = e
        return out

    out = {"dims": DIMS, "warmup": WARMUP, "timed": TIMED, "timing": "HIP events, ms per call; yardstick and new call alternate"}
    V = [bc.block_fermion_field(ctx, 32).setGaussian(1 + k) for k in range(2)]
    for m in (16, 32):
        b = bc.block_fermion_field(ctx, m).setGaussian(12)
        r = series([("basis_dot_first", lambda: bc.basis_dot(V, b), DOT_KEYS),
                    ("basis_slice_dot_dir3", lambda: bc.basis_slice_dot(V, b, 3), SLICE_KEYS),
                    ("basis_dot_second", lambda: bc.basis_dot(V, b), DOT_KEYS)])
        y1, y2 = r["basis_dot_first"]["ms_median"], r["basis_dot_second"]["ms_median"]
        r["basis_slice_dot_dir3_over_basis_dot"] = round(r["basis_slice_dot_dir3"]["ms_median"] / (0.5 * (y1 + y2)), 3)
        r["yardstick_spread"] = round(abs(y1 - y2) / (0.5 * (y1 + y2)), 4)
        if m == 16:
            r.update(series([(f"basis_slice_dot_dir{d}", lambda d=d: bc.basis_slice_dot(V, b, d), SLICE_KEYS) for d in (0, 1, 2)]))
            r.update(series([(f"basis_slice_dot_dir3_P{P}", lambda P=P: bc.basis_slice_dot(V, b, 3, MOMENTA[:P]), SLICE_KEYS)
                             for P in (1, 2, 4, 8)]))
        out[f"V32x2_m{m}"] = r
        del b
    del V
    V = [bc.block_fermion_field(ctx, 12).setGaussian(21 + k) for k in range(2)]
    b = bc.block_fermion_field(ctx, 12).setGaussian(23)
    out["V12x2_m12"] = series([("basis_dot", lambda: bc.basis_dot(V, b), DOT_KEYS),
                               ("basis_slice_dot_dir3", lambda: bc.basis_slice_dot(V, b, 3), SLICE_KEYS)])
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child()))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "basis_slice_time.json")
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
