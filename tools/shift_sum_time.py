#!/usr/bin/env python3
"""GPU box: the covariant nearest-neighbour sum (bcg_dirac_shift_sum) at 64^4 in a fresh process.

  shift_sum_time.py [--out PATH]     default PATH: profiles/shift_sum_time.json

4 warm-up + 20 timed calls of every entry, HIP-event times from the per-kernel profile, the entries of one width ALTERNATING
call by call in one process (one round = one call of each):
  * m = 16: the yardstick, bcg_dirac_hop under bcg_force_generic (k_hop_generic: the same arithmetic and bytes, every link
    entry a global load per lane), twice per round to show its spread; shift_sum(0, 1/2, -1/2, eta) in the tile form
    (condition: at most 1.10 x the yardstick); recorded without a condition: the pipelined plain hop (k_hop4b), the ratio to
    it, laplacian(dir = 3), and shift_sum's generic form;
  * m = 8 and m = 32: the tile form beside the yardstick;  m = 12: the generic form beside the yardstick.
Every entry also as TB/s on the byte model 2 * 48 m V + 144 V (directions with a non-zero coefficient).
Prints one JSON line and writes it to PATH."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, WARMUP, TIMED, PEAK = [64, 64, 64, 64], 4, 20, 8e12


def child():
    import torch  # noqa: F401  (one HIP runtime: see blockcg_amd/_lib.py)
    sys.path.insert(0, ROOT)
    import blockcg_amd as bc
    ctx = bc.Context(DIMS)
    V = ctx.V

    def rounds(entries):
        """entries: name -> (call, profile key, directions read).  Returns name -> ms per call, TB/s."""
        for _ in range(WARMUP):
            for call, _, _ in entries.values():
                call()
        ctx.synchronize()
        ms = {k: 0.0 for k in entries}
        ctx.profiling(True)
        for _ in range(TIMED):
            for name, (call, key, _) in entries.items():
                ctx.profile_reset()
                call()
                ctx.synchronize()
                ms[name] += ctx.profile()[key]["ms"]
        ctx.profiling(False)
        out = {}
        for name, (_, _, dirs) in entries.items():
            t = ms[name] / TIMED
            tbs = (2 * 48.0 * m + 144.0 * dirs) * V / (t * 1e-3) / 1e12
            out[name] = {"ms": round(t, 4), "TB_per_s": round(tbs, 3), "fraction_of_8TBps": round(tbs * 1e12 / PEAK, 3)}
        return out

    out = {"dims": DIMS, "warmup": WARMUP, "timed": TIMED, "timing": "HIP events, ms per call, entries alternating call by call"}
    for m in (16, 8, 32, 12):
        D = bc.dirac_op(ctx, 0.1, seed=3)
        a = bc.block_fermion_field(ctx, m).setGaussian(1)
        b = bc.block_fermion_field(ctx, m)

        def generic_hop():
            ctx.force_generic(True)
            D.D(b, a)
            ctx.force_generic(False)

        def generic_shift():
            ctx.force_generic(True)
            bc.shift_sum(b, a, D, 0.0, 0.5, -0.5, eta=True)
            ctx.force_generic(False)

        entries = {"yardstick_generic_hop": (generic_hop, "hop", 4)}
        if m == 12:
            entries["shift_sum_hop_generic_form"] = (lambda: bc.shift_sum(b, a, D, 0.0, 0.5, -0.5, eta=True), "shift_sum", 4)
        else:
            entries["shift_sum_hop"] = (lambda: bc.shift_sum(b, a, D, 0.0, 0.5, -0.5, eta=True), "shift_sum", 4)
        entries["yardstick_generic_hop_again"] = (generic_hop, "hop", 4)
        if m == 16:
            entries["plain_hop_k_hop4b"] = (lambda: D.D(b, a), "hop", 4)
            entries["laplacian_dir3"] = (lambda: bc.laplacian(b, a, D, 3), "shift_sum", 3)
            entries["shift_sum_hop_generic_form"] = (generic_shift, "shift_sum", 4)
        r = rounds(entries)
        mine = r.get("shift_sum_hop", r.get("shift_sum_hop_generic_form"))
        y1, y2 = r["yardstick_generic_hop"]["ms"], r["yardstick_generic_hop_again"]["ms"]
        r["yardstick_spread"] = round(abs(y1 - y2) / min(y1, y2), 4)
        r["shift_sum_over_yardstick"] = round(mine["ms"] / (0.5 * (y1 + y2)), 3)
        if m == 16:
            r["shift_sum_over_plain_hop"] = round(mine["ms"] / r["plain_hop_k_hop4b"]["ms"], 3)
            r["condition_1.10_met"] = bool(mine["ms"] <= 1.10 * 0.5 * (y1 + y2))
        out[f"m{m}"] = r
        del a, b, D
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        print(json.dumps(child()))
        return
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "shift_sum_time.json")
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
