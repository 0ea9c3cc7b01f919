#!/usr/bin/env python3
"""GPU box: the in-place basis rotation and one outer iteration of the low-mode eigensolver, K = 64.

  bench_lowmodes.py [--out PATH] [--shapes 32x32x32x32,64x64x64x32]     default PATH: profiles/lowmodes_time.json

One fresh process per (lattice, width list) -- K = 64 as [16] x 4 and as [32] x 2 -- each under its own time limit, one
at a time.  2 warm-up + 10 timed rounds, HIP-event times from the per-kernel profile.  Per case:
  * basis_rotate(V, Q), Q unitary: ms, and the achieved bytes/s against its model of 96 K bytes per site (every column
    read once and written once);
  * the out-of-place route that needs no rotation kernel: basis_axpy with beta = 0 into four spare fields of 16 columns
    (each reads all of V: 48 (K + 16) bytes per site and call) plus the column copies back (2 x 48 x 16 each) -- the
    same result with a quarter of a second basis and 3.5 times the traffic (240 K + 96 K bytes per site at K = 64);
  * one outer iteration of lowest_modes (degree 16): the profile of a run with max_iterations = 1 minus that of a run
    with max_iterations = 0 on the same start block, grouped into filter (the stencil launches of degree x nv
    applications, the recurrence's axpby and the copy back), Gram / projection (basis_dot, basis_fold and the stencil
    launches of H = V^dagger A V: half of the applications outside the filter), rotation (basis_rotate) and residuals
    (the other half of those applications, block_axpy, gram_self, reduce_partials).
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, TIMED, DEGREE = 2, 10, 16
WIDTHS = {"16x4": [16, 16, 16, 16], "32x2": [32, 32]}


def child(dims, widths):
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(dims)
    ctx.profiling(True)
    K = sum(widths)
    V = [bc.block_fermion_field(ctx, w).setGaussian(1 + k) for k, w in enumerate(widths)]
    rng = np.random.default_rng(1)
    Q, _ = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))
    spare = [bc.block_fermion_field(ctx, 16) for _ in range(K // 16)]
    homes = [(f, c0) for f in V for c0 in range(0, f.N_rhs, 16)]  # where block j of the basis lives

    def rotate():
        bc.basis_rotate(V, Q)

    def out_of_place():
        for j, s in enumerate(spare):
            bc.basis_axpy(s, V, Q[:, 16 * j:16 * (j + 1)], 0.0)
        for (f, c0), s in zip(homes, spare):
            f.copy_columns(c0, s, 0, 16)

    def timed(call, keys):
        ms = []
        for it in range(WARMUP + TIMED):
            ctx.profile_reset()
            call()
            prof = ctx.profile()
            if it >= WARMUP:
                ms.append(sum(prof[k]["ms"] for k in keys if k in prof))
            nbytes = sum(prof[k]["bytes"] for k in keys if k in prof)
        t = float(np.median(ms))
        return {"ms_median": round(t, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "model_bytes": nbytes,
                "TB_per_s": round(nbytes / (t * 1e-3) / 1e12, 3)}

    out = {"dims": dims, "widths": widths, "K": K, "warmup": WARMUP, "timed": TIMED}
    out["basis_rotate"] = timed(rotate, ["basis_rotate"])
    out["axpy_and_copy_back"] = timed(out_of_place, ["basis_axpy", "copy_columns"])
    out["rotate_over_out_of_place_time"] = round(out["basis_rotate"]["ms_median"] / out["axpy_and_copy_back"]["ms_median"], 3)
    del spare

    # one outer iteration: (Ritz step, residuals, filter, Ritz step, residuals) minus (Ritz step, residuals)
    D = bc.dirac_op(ctx, 0.1, seed=5)
    ub = bc.spectral_bound(D, 10, 1)
    profs = []
    for limit in (0, 1):
        for k, v in enumerate(V):
            v.setGaussian(1 + k)
        ctx.profile_reset()
        r = bc.lowest_modes(V, D, K // 2, ub, DEGREE, 1e-10, limit)
        profs.append((ctx.profile(), r["applications"]))
    (p0, a0), (p1, a1) = profs
    keys = sorted(set(p0) | set(p1))
    ms = {k: p1.get(k, {}).get("ms", 0.0) - p0.get(k, {}).get("ms", 0.0) for k in keys}
    hop = sum(t for k, t in ms.items() if k.startswith("hop"))
    nv = len(widths)
    filter_share = DEGREE * nv / float(a1 - a0)  # of the iteration's applications; the rest: H = V^dagger A V and the residuals
    groups = {"filter": hop * filter_share + ms.get("axpby", 0.0) + ms.get("copy", 0.0),
              "gram_projection": ms.get("basis_dot", 0.0) + ms.get("basis_fold", 0.0) + 0.5 * hop * (1.0 - filter_share),
              "rotation": ms.get("basis_rotate", 0.0),
              "residuals": 0.5 * hop * (1.0 - filter_share) + ms.get("block_axpy", 0.0) + ms.get("gram_self", 0.0) + ms.get("reduce_partials", 0.0)}
    total = sum(groups.values())
    out["outer_iteration"] = {"upper_bound": ub, "degree": DEGREE, "applications": a1 - a0, "ms_by_key": {k: round(t, 4) for k, t in ms.items() if t},
                              "ms": {k: round(t, 3) for k, t in groups.items()}, "share": {k: round(t / total, 4) for k, t in groups.items()},
                              "ms_total": round(total, 3)}
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child([int(x) for x in sys.argv[2].split("x")], WIDTHS[sys.argv[3]])))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "lowmodes_time.json")
    shapes = sys.argv[sys.argv.index("--shapes") + 1] if "--shapes" in sys.argv else "32x32x32x32,64x64x64x32"
    out = {"timing": "HIP events, ms per call, median of the timed rounds", "cases": []}
    for shape in shapes.split(","):
        for name in WIDTHS:
            cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", shape, name]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:  # a fault, an abort or the time limit: nothing more is started on the GPU
                out["error"] = {"case": [shape, name], "returncode": r.returncode, "stderr": r.stderr[-2000:]}
                print(json.dumps(out))
                sys.exit(1)
            out["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    with open(path, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
