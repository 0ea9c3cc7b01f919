"""The case list of the stencil planner's table (tests/golden/hop_plan_table.json): every request below is planned by
tests/cpp/hop_plan_probe.cpp and compared with the plan the table records (test_hop_plan_cpu.py); test_hop_plan_gpu.py
looks its shapes up here.  A case is a dict; `line(case)` is what the probe reads, `label(case)` what a failure prints.

Order matters: the table stores one plan index per case, in the order `cases()` yields them."""
import itertools
import json
import os

MODES = ["HOP_PLAIN", "HOP_SHIFTED", "HOP_RESID", "HOP_FACT1", "HOP_FACT2"]
WIDTHS = [8, 16, 32]
HALF_CHUNK = 16  # the library's default x3 chunk of the half-volume sweep

# default tuning (kernels_mfma.hpp: HopTuning, HopSync)
DEFAULT = dict(patch_walk=1, patch=(0, 8, 8), blocks=512, column_walk=1, bundle_walk=1, bundle_window=4, super_patch=0,
               window=4)
VARIANTS = {
    "default": {},
    "bundle0": dict(bundle_walk=0),
    "bundle2": dict(bundle_walk=2),
    "column_off": dict(column_walk=0),
    "walk_off": dict(patch_walk=0),
    "odd_patch": "odd",              # x1 extent of the patch 3
    "bundle_window0": dict(bundle_window=0),
    "bundle_window-1": dict(bundle_window=-1),
    "blocks480": dict(blocks=480),
    "super1": dict(super_patch=1),
}


def small_base(m):
    """What the GPU tests set on small lattices: BCG_HOP_PATCH = one tile x 2 x 2, BCG_HOP_BLOCKS = 32."""
    return dict(DEFAULT, patch=(4 * (64 // m), 2, 2), blocks=32)


def tuning(m, base, variant):
    t = dict(small_base(m) if base == "small" else DEFAULT)
    v = VARIANTS[variant]
    if v == "odd":
        t["patch"] = (t["patch"][0], 3, t["patch"][2])
    else:
        t.update(v)
    return t


# (dims, split, base tuning, all variants?)
BIG = [[64, 64, 64, 64], [32, 32, 32, 32], [64, 64, 64, 32], [64, 64, 64, 128]]
SMALL = [[16, 8, 8, 8], [32, 8, 8, 6],              # test_factored_stencil.py, test_phase_a_operator.py
         [8, 4, 4, 6], [4, 6, 2, 4], [16, 2, 4, 2], [8, 4, 4, 4], [64, 8, 8, 6], [32, 8, 8, 4],  # test_half_volume.py
         [64, 4, 8, 4], [64, 8, 8, 4], [16, 8, 8, 4],  # test_gpu_parity.py's form test
         [24, 8, 8, 8],                               # L0 no multiple of the tile at m = 8, 16
         [32, 7, 8, 6]]                               # odd L1
VARIED = [[64, 64, 64, 64], [64, 64, 64, 128], [32, 8, 8, 6], [64, 8, 8, 6]]


def lattices():
    none = (0, 0, 0, 0)
    for d in BIG:
        yield d, none, "default"
    for d in SMALL:
        yield d, none, "small"
    for d in SMALL[:3]:  # (small lattices under the default tuning: no patch walk fits)
        yield d, none, "default"
    for mu in range(4):  # each direction marked split
        yield [32, 8, 8, 6], tuple(int(nu == mu) for nu in range(4)), "small"
        yield [64, 64, 64, 64], tuple(int(nu == mu) for nu in range(4)), "default"


def windows(L3):
    """(x3_lo, x3_n, ring, cb) of tile class 0."""
    w = [(0, 0, 0, 0)]
    for ring, n in ((8, 6), (16, 15), (32, 30), (3, 1), (3, 2)):  # (ring 3: the smallest the GPU tests use, chunks of 1)
        w.append((0, n, ring, 0))
    w += [(L3 - 15, 15, 16, 0), (L3 - 1, 1, 3, 0)]  # (windows that end at the last slice)
    w.append((0, 0, 0, 1))
    last = HALF_CHUNK * ((L3 - 1) // HALF_CHUNK)
    w += [(lo, n, 0, 1) for lo, n in ((L3 - 1, 1), (0, 2), (0, 3), (0, HALF_CHUNK), (0, HALF_CHUNK + 1), (last, L3 - last))]
    return list(dict.fromkeys(w))


def cases():
    for dims, split, base in lattices():
        variants = list(VARIANTS) if (dims in VARIED and not any(split) and (base == "small") == (dims in SMALL)) else ["default"]
        for variant, m in itertools.product(variants, WIDTHS):
            t = tuning(m, base, variant)
            # tile class 0 with every window; the classes of the split exchange (2: without and with a tile list, one of
            # them empty) with whole fields, the interior class also with a ring and a checkerboard window
            cw = [(0, -1, w) for w in windows(dims[3])]
            cw += [(cls, n, (0, 0, 0, 0)) for cls, n in ((1, -1), (2, -1), (2, 37), (2, 0))]
            cw += [(1, -1, (0, 6, 8, 0)), (1, -1, (0, 0, 0, 1))]
            for (cls, list_n, win), mode, gram in itertools.product(cw, range(5), (0, 1)):
                yield dict(m=m, dims=dims, split=split, base=base, variant=variant, tune=t, cls=cls, list_n=list_n, win=win,
                           mode=mode, gram=gram, fold=gram)


def line(c):
    """The probe's input: integers.  Checkerboard windows take the compact lattice (x0 halved), as the library passes it."""
    t, (lo, n, ring, cb) = c["tune"], c["win"]
    L = list(c["dims"])
    if cb:
        L[0] //= 2
    v = [c["m"], *L, *c["split"], t["patch_walk"], *t["patch"], t["blocks"], t["column_walk"], t["bundle_walk"],
         t["bundle_window"], t["super_patch"], t["window"], c["cls"], c["list_n"], lo, n, ring, cb, c["mode"], c["gram"], c["fold"]]
    return " ".join(str(x) for x in v)


def label(c):
    return (f"m={c['m']} {'x'.join(map(str, c['dims']))} split={''.join(map(str, c['split']))} {c['base']}/{c['variant']} "
            f"class={c['cls']} list={c['list_n']} window(lo,n,ring,cb)={c['win']} {MODES[c['mode']]} gram={c['gram']}")


def find(all_cases, **want):
    """Index of the one case whose fields equal `want`."""
    hits = [i for i, c in enumerate(all_cases) if all(c[k] == v for k, v in want.items())]
    assert len(hits) == 1, (want, len(hits))
    return hits[0]


def load_table():
    """(plan per case, indices of the requests no caller makes) of tests/golden/hop_plan_table.json.  There, ten consecutive
    cases (the five modes, each without and with the Gram product) make a row: a pattern and a geometry (grid, walk, window:
    the same whatever the mode).  A pattern holds per case 0 declined, 1 unreached (declined, and a request no caller makes),
    2 empty, or [kernel with its LDS bytes, pacing and fold].  "cases" lists (row, repetitions) pairs."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hop_plan_table.json")) as f:
        t = json.load(f)
    plans, unreached = [], set()
    for r, n in zip(t["cases"][::2], t["cases"][1::2]):
        pattern, geometry = t["rows"][r]
        for cell in t["patterns"][pattern] * n:
            if cell == 1:
                unreached.add(len(plans))
            plans.append(("declined", "declined", "empty")[cell] if isinstance(cell, int) else
                         " ".join((t["kernels"][cell[0]], t["pacing"][cell[1]], t["geometry"][geometry])))
    return plans, unreached
