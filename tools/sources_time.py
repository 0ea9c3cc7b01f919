#!/usr/bin/env python3
"""GPU box: the source / sink kernels at 64^4, m = 16, in a fresh process.

  sources_time.py [--out PATH]     default PATH: profiles/sources_time.json

4 warm-up + 20 timed calls each, HIP-event times from the per-kernel profile:
  * slice_dot(a, b, dir) for dir = 3 beside hermitian_dot(a, b) on the same fields in the same process (the Gram kernel
    reads the same 2 s V bytes and is the yardstick: expected ratio about 1, accepted up to 1.25; both sides include their
    fold launch, slice_fold and reduce_partials where that is a launch of its own), then dir = 0, 1, 2 and
    a == b (recorded, no bar);
  * fill_noise (Gaussian, Z2) beside fill_random (which has no profile key: host time over 20 enqueued calls and one
    synchronisation, the same way for all three).
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, M, WARMUP, TIMED, PEAK = [64, 64, 64, 64], 16, 4, 20, 8e12


def child():
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(DIMS)
    a = bc.block_fermion_field(ctx, M).setGaussian(1)
    b = bc.block_fermion_field(ctx, M).setGaussian(2)
    field_bytes = ctx.V * 48 * M

    def profiled(call, keys):
        for _ in range(WARMUP):
            call()
        ctx.synchronize()
        ctx.profiling(True)
        ctx.profile_reset()
        for _ in range(TIMED):
            call()
        ctx.synchronize()
        prof = ctx.profile()
        ctx.profiling(False)
        out = {}
        for k in keys:
            v = prof.get(k)
            if not v or not v.get("count"):  # e.g. reduce_partials when the Gram kernel folds its partials itself
                continue
            e = {"ms": round(v["ms"] / v["count"], 4)}
            if v.get("bytes"):
                e["TB_per_s"] = round(v["bytes"] / (v["ms"] * 1e-3) / 1e12, 3)
                e["fraction_of_8TBps"] = round(v["bytes"] / (v["ms"] * 1e-3) / PEAK, 3)
            out[k] = e
        return out

    def host_timed(call):
        for _ in range(WARMUP):
            call()
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(TIMED):
            call()
        ctx.synchronize()
        ms = (time.perf_counter() - t) / TIMED * 1e3
        return {"ms": round(ms, 4), "TB_per_s": round(field_bytes / (ms * 1e-3) / 1e12, 3),
                "fraction_of_8TBps": round(field_bytes / (ms * 1e-3) / PEAK, 3), "timing": "host"}

    out = {"dims": DIMS, "m": M, "warmup": WARMUP, "timed": TIMED, "timing": "HIP events unless an entry says host"}
    out["hermitian_dot"] = profiled(lambda: a.hermitian_dot(b), ["gram_pair", "reduce_partials"])
    for d in (3, 0, 1, 2):
        out[f"slice_dot_dir{d}"] = profiled(lambda: a.slice_dot(b, d), ["slice_dot", "slice_fold"])
    out["slice_dot_dir3_self"] = profiled(lambda: a.slice_dot(a, 3), ["slice_dot", "slice_fold"])
    total = lambda e: sum(v["ms"] for v in e.values())  # noqa: E731  (kernel + fold, on both sides)
    out["slice_dot_dir3_over_hermitian_dot"] = round(total(out["slice_dot_dir3"]) / total(out["hermitian_dot"]), 3)
    out["fill_random"] = host_timed(lambda: b.setRandom(3))
    out["fill_gaussian"] = host_timed(lambda: b.setGaussian(3))
    out["fill_z2"] = host_timed(lambda: b.setZ2(3))
    out["fill_gaussian_over_fill_random"] = round(out["fill_gaussian"]["ms"] / out["fill_random"]["ms"], 3)
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child()))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sources_time.json")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(json.dumps({"error": r.returncode, "stderr": r.stderr[-2000:]}))
        sys.exit(1)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    with open(path, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
