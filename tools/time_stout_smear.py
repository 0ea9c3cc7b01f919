#!/usr/bin/env python3
"""Times stout smearing and the plaquette on one GPU from the library's own profile (keys "stout_smear", one entry per step,
and "plaquette"): links from bcg_gauge_fill_random, spatial weights (rho = 0.1 off direction 3) and the full table, 3 steps a
call.  Warm-up calls are excluded; every figure is the mean over --reps calls.  Prints one JSON line per lattice and weight
table: ms per step, GB/s on the compulsory bytes (read + write of the smeared directions plus one read of each unsmeared
direction that some staple uses as nu; the plaquette: every link once) and their fraction of --peak.
    python tools/time_stout_smear.py [--dims 64,64,64,32 --dims 64,64,64,64] [--reps 5] [--warmup 2] [--peak 5900]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compulsory_bytes(table, V):
    nd = table.shape[0]
    smeared = [mu for mu in range(nd) if np.any(table[mu] != 0.0)]
    used = [nu for nu in range(nd) if nu not in smeared and np.any(table[:, nu] != 0.0)]
    return 144.0 * V * (2 * len(smeared) + len(used))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", action="append")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--peak", type=float, default=5900.0, help="GB/s the fractions are taken of")
    args = ap.parse_args()
    import blockcg_amd as bc
    for spec in args.dims or ["64,64,64,32", "64,64,64,64"]:
        dims = [int(x) for x in spec.split(",")]
        ctx = bc.Context(dims, device=0)
        nd = len(dims)
        U, out, work = bc.gauge_field(ctx).setRandom(5), bc.gauge_field(ctx), bc.gauge_field(ctx)
        for name, rho, d in (("spatial", 0.1, nd - 1), ("full", 0.1, None)):
            table = bc.api._rho_table(rho, nd, d).copy()
            table[np.arange(nd), np.arange(nd)] = 0.0
            for _ in range(args.warmup):
                bc.stout_smear(out, U, rho, args.steps, dir=d, work=work)
            ctx.synchronize()
            ctx.profiling(True)
            ctx.profile_reset()
            for _ in range(args.reps):
                bc.stout_smear(out, U, rho, args.steps, dir=d, work=work)
            ctx.synchronize()
            p = ctx.profile()["stout_smear"]
            ctx.profiling(False)
            ms = p["ms"] / p["count"]
            gbs = compulsory_bytes(table, ctx.V) / ms / 1e6
            print(json.dumps({"dims": dims, "call": "stout_smear", "weights": name, "steps_timed": p["count"], "ms_per_step": round(ms, 4),
                              "compulsory_GB": round(compulsory_bytes(table, ctx.V) / 1e9, 4), "GBps": round(gbs, 1),
                              "fraction_of_peak": round(gbs / args.peak, 4)}), flush=True)
        for _ in range(args.warmup):
            bc.plaquette(U)
        ctx.profiling(True)
        ctx.profile_reset()
        for _ in range(args.reps):
            bc.plaquette(U)
        p = ctx.profile()["plaquette"]
        ctx.profiling(False)
        ms = p["ms"] / p["count"]
        gbs = 144.0 * nd * ctx.V / ms / 1e6
        print(json.dumps({"dims": dims, "call": "plaquette", "calls_timed": p["count"], "ms_per_call": round(ms, 4), "GBps": round(gbs, 1),
                          "fraction_of_peak": round(gbs / args.peak, 4)}), flush=True)
        del U, out, work
        ctx.close()


if __name__ == "__main__":
    main()
