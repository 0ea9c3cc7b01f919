#!/usr/bin/env python3
"""Tuning aid (GPU box): where the cycles of a stencil tile go (plain form), from in-kernel s_memtime stamps.
k_hop4c: library built with -DBCG_HOP4C_STAMPS and BCG_HOP_BUNDLE=0; k_hop4b (the default form): -DBCG_HOP4B_STAMPS and
`python tools/hop_stamps.py 4b`  (tools/build_variant.sh stamps "-DBCG_HOP4B_STAMPS"; BCG_LIB=...); `pipe`: the same build, the
segments of the software-pipelined step; `fact2`: the second pass of the factored pair (HOP_FACT2, with its Gram product) of the
solver's phase A instead of the plain hop, which leaves its stamps behind the Gram partials -- with BCG_HOP_FUSED_B=0; with the
default (1) both factors carry a Gram product and stamp the same place, so what is read is the later launch: the second
factor fused with phase B (k_hop4b_fusedB), whose segment "carry U3, WAIT p, output, stores" holds phase B's products.
`fusedb`: that launch under its own segment names (one SBCGrQ iteration, the stamps of its later launch); `fact1g`: the first
factor with its Gram product alone (k_hop4b<16, HOP_FACT1, GRAM>, through the test aid bcg_debug_fused_first_factor, so that
the fused launch does not overwrite its stamps)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import blockcg_amd as bc  # noqa: E402

dims, m = [64, 64, 64, 64], 16
ctx = bc.Context(dims)
D = bc.dirac_op(ctx, 1e-3, seed=1)
B = bc.block_fermion_field(ctx, m).setRandom(seed=2)
X = [bc.block_fermion_field(ctx, m)]
st = bc.SBCGrQState(X, B, D, [0.0], 0.0, 0.0, consume_B=False)
st.iterate(1)  # allocates the scratch buffer
mode = sys.argv[1] if len(sys.argv) > 1 else ""
y = bc.block_fermion_field(ctx, m)
for _ in range(3):
    if mode in ("fact2", "fusedb"):
        st.iterate(1)
    elif mode == "fact1g":
        ff = ctx.lib.bcg_debug_fused_first_factor
        ff.restype = ctypes.c_int
        ff.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        ctx.check(ff(ctx.h, D.h, D.mass, 0.0, y.h, B.h))
    else:
        D.D(y, B)
ctx.synchronize()
nblk = 512
GRAM_MODES = ("fact2", "fusedb", "fact1g")  # launches with a Gram product: the stamps lie behind its partials
NSEG = 16 if mode in ("4b", "pipe") + GRAM_MODES else 8
skip = 1024 * m * m * 2 if mode in GRAM_MODES else 0  # doubles: the Gram partials of the largest grid (kHopStampsSkipBlocks, kernels_mfma.hpp)
buf = np.zeros(skip + nblk * 4 * NSEG, dtype=np.float64)
lib = ctx.lib
lib.bcg_debug_read_scratch.restype = ctypes.c_int
lib.bcg_debug_read_scratch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
assert lib.bcg_debug_read_scratch(ctx.h, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes) == 0
seg = buf[skip:].reshape(nblk, 4, NSEG)
tiles = 64 ** 4 // 16 // nblk
names = ["park+pace", "barrier", "issue(links,dir0)", "dir0", "dir1", "dir2", "dir3(+x3)", "tail(p,store)"]
if len(sys.argv) > 1 and sys.argv[1] == "4b":
    names = ["pace(thread 0)", "barrier", "issue(DMAs,loads)", "dir0 (LDS only)", "dir1 (+wait loads)", "dir2", "dir3", "tail(park,store)"]
if mode in ("pipe", "fact2", "fact1g"):  # the software-pipelined step (PIPE in hop4b_body)
    names = ["loop overhead", "barrier", "-x3 readback + row DMAs", "dir0", "issue p + link DMAs", "dir1", "issue next rows", "dir2",
             "WAIT +x3 row", "dir3", "carry U3, WAIT p, output, stores", "WAIT links + next rows"]
if mode == "fusedb":  # the same step with the Q rows in p's place and phase B in the tail
    names = ["loop overhead", "barrier", "-x3 readback + row DMAs", "dir0", "issue Q + link DMAs", "dir1",
             "Q rho_prev^-1 (if ahead) + issue next rows", "dir2", "WAIT +x3 row", "dir3",
             "carry U3, T exchange, phase B, stores, Gram", "WAIT links + next rows (+ next Q)"]
tot = seg.sum(axis=2)
print("cycles per tile per wave (s_memtime ticks = shader cycles): total median %.0f" % np.median(tot / tiles))
for i, n in enumerate(names):
    v = seg[:, :, i] / tiles
    print("  %-20s median %7.0f  p10 %7.0f  p90 %7.0f  share %4.1f %%" % (n, np.median(v), np.percentile(v, 10), np.percentile(v, 90),
                                                                       100 * v.sum() / (tot / tiles).sum()))
