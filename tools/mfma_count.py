#!/usr/bin/env python3
"""Static v_mfma_f64 count per kernel in device assembly: python tools/mfma_count.py <file.s> [filter-regex]

Make the assembly with  hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only kernels_mfma.hip -o kernels_mfma.s
(add -DBCG_COMPLEX_4M for the four-product form of the complex right-multiplications).  The count is per instantiation
and static: a loop body counts once."""
import re
import sys

rx = re.compile(sys.argv[2]) if len(sys.argv) > 2 else None
cur = None
counts = {}
for ln in open(sys.argv[1]):
    m = re.match(r"^(_Z\S+):", ln)
    if m:
        cur = m.group(1)
        counts.setdefault(cur, 0)
    elif cur and re.match(r"\s+v_mfma_f64", ln):
        counts[cur] += 1
for name, n in counts.items():
    short = re.sub(r"^_ZN3bcg(12_GLOBAL__N_1)?\d+", "", name)
    short = re.sub(r"(EEvl|ENS_|ElP).*", "", short)
    if n == 0 or (rx and not rx.search(short)):
        continue
    print(f"{short:52s} {n:6d}")
