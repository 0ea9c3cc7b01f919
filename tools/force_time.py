#!/usr/bin/env python3
"""GPU box: one fermion-force call (bcg_force_accumulate) at 64^4, m = 16, 4 shifts, X_s from fill_random, in a fresh process.

  force_time.py [--out PATH]     default PATH: profiles/force_time.json
  force_time.py --single         one call with four work fields only (for a counter run: tools/pmc_force.sh)

Two warm-up calls, then 5 timed calls with the work fields of one launch (n_work = 4: F is read and written once) and 5 with
the library's single work field (n_work = 0: four launches), each with the per-kernel profile on for the split between the
stencil (D X_s, key "hop") and the force kernel (key "force"), and 3 projected calls (key "force_project").  Reports ms per
call and the force kernel's GB per launch on its byte model, the rate this gives and its fraction of 8 TB/s.  Prints one JSON
line and writes it to PATH."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, M, RESIDUES, SCALE = [64, 64, 64, 64], 16, [0.4, 0.3, 0.2, 0.1], 1.0
WARMUP, TIMED, PROJECTED, PEAK = 2, 5, 3, 8e12


def child():
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(DIMS)
    D = bc.dirac_op(ctx, 0.1, seed=1)
    X = [bc.block_fermion_field(ctx, M).setRandom(seed=2 + s) for s in range(len(RESIDUES))]
    F = bc.gauge_field(ctx).setZero()

    def timed(n, work, project=False):
        ctx.synchronize()
        ctx.profiling(True)
        ctx.profile_reset()
        t = time.perf_counter()
        for _ in range(n):
            bc.fermion_force(F, X, D, RESIDUES, SCALE, project, work)
        ctx.synchronize()
        ms = (time.perf_counter() - t) / n * 1e3
        prof = ctx.profile()
        ctx.profiling(False)
        out = {"ms_per_call": round(ms, 2)}
        for k, v in prof.items():
            if v.get("count") and (k.startswith("force") or k.startswith("hop")):
                e = {"ms_per_call": round(v["ms"] / n, 3), "launches_per_call": v["count"] / n}
                if v.get("bytes"):
                    e["GB_per_launch"] = round(v["bytes"] / v["count"] / 1e9, 2)
                    e["TB_per_s"] = round(v["bytes"] / (v["ms"] * 1e-3) / 1e12, 3)
                    e["fraction_of_8TBps"] = round(v["bytes"] / (v["ms"] * 1e-3) / PEAK, 3)
                out[k] = e
        return out

    work = [bc.block_fermion_field(ctx, M) for _ in RESIDUES]
    for _ in range(WARMUP):
        bc.fermion_force(F, X, D, RESIDUES, SCALE, False, work)
    one_launch = timed(TIMED, work)
    del work
    per_shift = timed(TIMED, None)
    projected = timed(PROJECTED, [bc.block_fermion_field(ctx, M) for _ in RESIDUES], project=True)
    return {"dims": DIMS, "m": M, "shifts": len(RESIDUES), "n_work_4": one_launch, "n_work_0": per_shift,
            "n_work_4_projected": projected}


def single():
    """--single: one call with four work fields and nothing else (the run tools/pmc_force.sh collects counters of)"""
    import torch  # noqa: F401
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(DIMS)
    D = bc.dirac_op(ctx, 0.1, seed=1)
    X = [bc.block_fermion_field(ctx, M).setRandom(seed=2 + s) for s in range(len(RESIDUES))]
    F = bc.gauge_field(ctx).setZero()
    bc.fermion_force(F, X, D, RESIDUES, SCALE, False, [bc.block_fermion_field(ctx, M) for _ in RESIDUES])
    ctx.synchronize()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child()))
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--single":
        single()
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "force_time.json")
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
