#!/usr/bin/env python3
"""GPU box: the baryon elementals of a basis (bcg_basis_slice_triple) against the matrix rate of bcg_basis_slice_dot, a fresh
process per case.  Timings only: nothing here checks a result.

  basis_slice_triple_time.py [--out PATH] [--only LATTICE WIDTHS LISTS]     default PATH: profiles/basis_slice_triple_time.json

4 warm-up + 20 timed rounds, HIP-event times from the per-kernel profile, medians.  A round is yardstick, new call, yardstick
again.  The yardstick is bcg_basis_slice_dot(V, b, 3) without momenta on the same 64 columns V against m = 16 in the same
process; its rate is 8 K m flops per row over its time.  The new call's rate is its executed flops (24 per (pair, k, site) of
the tiles actually launched, the profile's figure) over the time of its "basis_slice_triple" launches; the fold is reported
beside it.
Cases (one process each): 32^4 and 64^3 x 32 along direction 3, K = 64 as [16] x 4 and as [32] x 2, identical lists and three
distinct lists; in each, no momenta and one momentum, all slices and one slice.
Condition: on 64^3 x 32 with identical lists, all slices and no momenta the MFMA form reaches at least 0.6 x the yardstick's
rate (recorded as "condition" per width list; the run does not fail on it).
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, TIMED = 4, 20
LATTICES = {"32x32x32x32": [32, 32, 32, 32], "64x64x64x32": [64, 64, 64, 32]}
WIDTHS = {"16x4": [16, 16, 16, 16], "32x2": [32, 32]}
LISTS = ("identical", "distinct")
MOMENTUM = [[1, -1, 2, 0]]
THRESHOLD = 0.6


def case(dims, widths, lists):
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(dims)
    ctx.profiling(True)
    new = lambda seed: [bc.block_fermion_field(ctx, w).setGaussian(seed + k) for k, w in enumerate(widths)]  # noqa: E731
    A = new(1)
    B, C = (A, A) if lists == "identical" else (new(11), new(21))
    b = bc.block_fermion_field(ctx, 16).setGaussian(31)
    K, rows = sum(widths), 3 * ctx.V

    def yardstick():
        ctx.profile_reset()
        bc.basis_slice_dot(A, b, 3)
        return {"ms": ctx.profile()["basis_slice_dot"]["ms"], "flops": 8.0 * K * 16 * rows}

    def triple(slices, momenta):
        ctx.profile_reset()
        bc.basis_slice_triple(A, B, C, 3, slices, momenta)
        p = ctx.profile()
        return {"ms": p["basis_slice_triple"]["ms"], "flops": p["basis_slice_triple"]["flops"], "bytes": p["basis_slice_triple"]["bytes"],
                "fold_ms": p["basis_slice_triple_fold"]["ms"], "mfma_launches": p.get("basis_slice_triple_form_mfma", {}).get("count", 0)}

    def median(samples, key):
        return float(np.median([s[key] for s in samples]))

    out = {}
    for slices_name, slices in (("all_slices", None), ("one_slice", [5])):
        for mom_name, momenta in (("no_momenta", None), ("one_momentum", MOMENTUM)):
            rounds = [("yardstick_first", yardstick), ("triple", lambda: triple(slices, momenta)), ("yardstick_second", yardstick)]
            for _ in range(WARMUP):
                for _, call in rounds:
                    call()
            samples = {name: [] for name, _ in rounds}
            for _ in range(TIMED):
                for name, call in rounds:
                    samples[name].append(call())
            t = median(samples["triple"], "ms")
            y1, y2 = median(samples["yardstick_first"], "ms"), median(samples["yardstick_second"], "ms")
            ms = [s["ms"] for s in samples["triple"]]
            last = samples["triple"][-1]
            rate = last["flops"] / (t * 1e-3) / 1e12
            yard = samples["yardstick_first"][-1]["flops"] / (0.5 * (y1 + y2) * 1e-3) / 1e12
            out[f"{slices_name}_{mom_name}"] = {
                "ms_median": round(t, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                "fold_ms_median": round(median(samples["triple"], "fold_ms"), 4), "executed_flops": last["flops"], "bytes": last["bytes"],
                "mfma_launches": last["mfma_launches"], "TFLOP_per_s": round(rate, 2), "TB_per_s": round(last["bytes"] / (t * 1e-3) / 1e12, 3),
                "yardstick_ms_median": [round(y1, 4), round(y2, 4)], "yardstick_TFLOP_per_s": round(yard, 2),
                "rate_over_yardstick": round(rate / yard, 3)}
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(case(LATTICES[sys.argv[2]], WIDTHS[sys.argv[3]], sys.argv[4])))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "basis_slice_triple_time.json")
    cases = [[lat, w, lists] for lat in LATTICES for w in WIDTHS for lists in LISTS]
    if "--only" in sys.argv:
        k = sys.argv.index("--only")
        cases = [sys.argv[k + 1:k + 4]]
    out = {"warmup": WARMUP, "timed": TIMED, "threshold": THRESHOLD,
           "timing": "HIP events, ms per call; yardstick and new call alternate; timings only"}
    for c in cases:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + c, capture_output=True, text=True, timeout=1100)
        if r.returncode != 0:
            print(json.dumps({"error": r.returncode, "case": c, "stderr": r.stderr[-2000:]}))
            sys.exit(1)
        out[f"{c[0]}_K64_{c[1]}_{c[2]}"] = json.loads(r.stdout.strip().splitlines()[-1])
    out["condition"] = {w: {"rate_over_yardstick": out[f"64x64x64x32_K64_{w}_identical"]["all_slices_no_momenta"]["rate_over_yardstick"],
                            "met": out[f"64x64x64x32_K64_{w}_identical"]["all_slices_no_momenta"]["rate_over_yardstick"] >= THRESHOLD}
                        for w in WIDTHS if f"64x64x64x32_K64_{w}_identical" in out}
    with open(path, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
