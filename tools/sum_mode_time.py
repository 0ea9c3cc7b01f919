#!/usr/bin/env python3
"""GPU box: the sum mode of SBCGrQ (bcg_sbcgrq_begin_sum: Y = c0 B + sum_s a_s X_s, no X_s kept) next to the ordinary solve.

  sum_mode_time.py            64^4, m = 16, 4 shifts, fixed work: ordinary and sum mode, each in a fresh process
  sum_mode_time.py --share    the per-GPU share of 128^4 (64^3 x 128) in sum mode WITHOUT capacity mode, at the group depth
                              the solver can allocate (to set against the capacity-mode 101.2 ms, profiles/r05_bench_cap128.json)

Each solve: 4 warm-up iterations, 20 timed ones (whole groups of four), then 8 with the per-kernel profile on for the
closing-pass time.  Reports ms per iteration, the closing pass's kernel time per launch, and the planned device bytes
(bcg_sbcgrq_device_bytes with B consumed as the residual block, the X_s replaced by Y in sum mode).  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, SHIFTS, RESIDUES, C0, MASS = 16, [0.0, 1e-6, 1e-4, 1e-2], [0.4, 0.3, 0.2, 0.1], 0.05, 1e-3
WARMUP, TIMED, PROFILED = 4, 20, 8


def child(mode, dims):
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(dims)
    S = len(SHIFTS)
    field = ctx.V * 48 * M
    plan = ctx.sbcgrq_device_bytes(M, S, True)  # X_s and the work fields; B's storage is the residual block (consumed)
    D = bc.dirac_op(ctx, MASS, seed=1)
    B = bc.block_fermion_field(ctx, M).setRandom(seed=2)
    if mode == "ordinary":
        X = [bc.block_fermion_field(ctx, M) for _ in SHIFTS]
        st = bc.SBCGrQState(X, B, D, SHIFTS, 0.0, 0.0, consume_B=True)
        planned = plan
    else:
        Y = bc.block_fermion_field(ctx, M)
        st = bc.SBCGrQSumState(Y, B, D, SHIFTS, RESIDUES, C0, 0.0, 0.0, consume_B=True)
        planned = plan - S * field + field  # Y instead of the X_s
    st.iterate(WARMUP)
    free, total = torch.cuda.mem_get_info(0)
    ctx.synchronize()
    t = time.perf_counter()
    st.iterate(TIMED)
    ctx.synchronize()
    ms = (time.perf_counter() - t) / TIMED * 1e3
    ctx.profiling(True)
    ctx.profile_reset()
    st.iterate(PROFILED)
    ctx.synchronize()
    prof = ctx.profile()
    closing = {k: {"ms_per_launch": round(v["ms"] / v["count"], 3), "launches": v["count"],
                   "GB_per_launch": round(v["bytes"] / v["count"] / 1e9, 1)}
               for k, v in prof.items() if k.startswith("phaseC_multi")}
    st.end()
    return {"mode": mode, "dims": dims, "ms_per_iteration": round(ms, 2), "closing_pass": closing,
            "kernel_ms_per_iteration": {k: round(v["ms"] / PROFILED, 2) for k, v in prof.items()
                                        if v.get("bytes") and not k.startswith("stencil_form_")},
            "planned_GB": round(planned / 1e9, 1), "device_GB_in_use": round((total - free) / 1e9, 1)}


def run(mode, dims, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode] + [str(d) for d in dims],
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        return {"mode": mode, "dims": dims, "error": r.returncode, "stderr": r.stderr[-2000:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        print(json.dumps(child(sys.argv[2], [int(d) for d in sys.argv[3:]])))
        return
    out = {"m": M, "shifts": SHIFTS, "residues": RESIDUES, "c0": C0, "warmup": WARMUP, "timed_iterations": TIMED}
    if "--share" in sys.argv:
        out["share_sum_no_capacity"] = run("share_sum", [64, 64, 64, 128], 900)
        out["capacity_mode_ms_per_iteration_of_record"] = 101.2
    else:
        out["ordinary"] = run("ordinary", [64, 64, 64, 64], 600)
        if "error" not in out["ordinary"]:  # nothing more on the GPU after a failed run
            out["sum"] = run("sum", [64, 64, 64, 64], 600)
        if "error" not in out["ordinary"] and "error" not in out.get("sum", {"error": 1}):
            out["sum_over_ordinary"] = round(out["sum"]["ms_per_iteration"] / out["ordinary"]["ms_per_iteration"], 4)
    print(json.dumps(out))
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
