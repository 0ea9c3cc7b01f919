#!/usr/bin/env python3
"""GPU box: the per-slice Gram kernels (bcg_field_slice_gram) at 64^4 in a fresh process.

  slice_gram_time.py [--out PATH]     default PATH: profiles/slice_gram_time.json

4 warm-up + 20 timed calls each, HIP-event times from the per-kernel profile (keys slice_gram and slice_gram_fold, summed
over the launches of a call):
  * m = 16: slice_gram(a, b, 3) without momenta beside hermitian_dot(a, b) on the same fields in the same process (the Gram
    kernel reads the same 2 s V bytes and is the yardstick; target: kernel + fold at most 1.25 x hermitian_dot's kernel +
    fold); then directions 0, 1, 2, a == b, and P = 1 (the phase path), 2, 4, 8 momenta along time (recorded, no bar; the
    fp64 rate counts 8 m^2 flops per row and momentum);
  * m = 32 and m = 12 (the generic kernel): direction 3 without momenta and with P = 2, beside hermitian_dot.
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, WARMUP, TIMED, PEAK = [64, 64, 64, 64], 4, 20, 8e12
MOMENTA = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [1, 1, 0, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [1, 1, 1, 0]]


def child():
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(DIMS)

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
            if not v or not v.get("count"):
                continue
            e = {"ms": round(v["ms"] / TIMED, 4), "launches_per_call": v["count"] // TIMED}
            if v.get("bytes"):
                e["TB_per_s"] = round(v["bytes"] / (v["ms"] * 1e-3) / 1e12, 3)
                e["fraction_of_8TBps"] = round(v["bytes"] / (v["ms"] * 1e-3) / PEAK, 3)
            if v.get("flops"):
                e["TFLOP_per_s"] = round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2)
            out[k] = e
        return out

    total = lambda e: sum(v["ms"] for v in e.values())  # noqa: E731  (kernel + fold, on both sides)
    gram_keys, mine = ["gram_pair", "gram_self", "reduce_partials"], ["slice_gram", "slice_gram_fold"]
    out = {"dims": DIMS, "warmup": WARMUP, "timed": TIMED, "timing": "HIP events, ms per call"}
    for m in (16, 32, 12):
        a = bc.block_fermion_field(ctx, m).setGaussian(1)
        b = bc.block_fermion_field(ctx, m).setGaussian(2)
        r = {"hermitian_dot": profiled(lambda: a.hermitian_dot(b), gram_keys)}
        r["slice_gram_dir3"] = profiled(lambda: a.slice_gram(b, 3), mine)
        r["slice_gram_dir3_over_hermitian_dot"] = round(total(r["slice_gram_dir3"]) / total(r["hermitian_dot"]), 3)
        if m == 16:
            for d in (0, 1, 2):
                r[f"slice_gram_dir{d}"] = profiled(lambda: a.slice_gram(b, d), mine)
            r["slice_gram_dir3_self"] = profiled(lambda: a.slice_gram(a, 3), mine)
            for P in (1, 2, 4, 8):
                r[f"slice_gram_dir3_P{P}"] = profiled(lambda: a.slice_gram(b, 3, MOMENTA[:P]), mine)
        else:
            r["slice_gram_dir3_P2"] = profiled(lambda: a.slice_gram(b, 3, MOMENTA[:2]), mine)
        out[f"m{m}"] = r
        del a, b
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child()))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "slice_gram_time.json")
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
