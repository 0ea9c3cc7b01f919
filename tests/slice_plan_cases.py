"""The case list of the per-slice planners' table (tests/golden/slice_plan_table.json): every request below is planned by
tests/cpp/slice_plan_probe.cpp and compared with the plan the table records (test_slice_plan_cpu.py).  A case is a dict;
`line(case)` is what the probe reads, `label(case)` what a failure prints.

Order matters: the table stores one plan index per case, in the order `cases()` yields them."""
import itertools
import json
import os

HALF = 2048 * 32 * 32 // 2  # the half of the context's scratch the calls plan with (kSliceHalf)
GRAM, BASIS, AXPY = 0, 1, 2

SHAPES = [[96], [37], [2048], [5, 3, 2], [7, 5, 3, 3], [4, 2, 4, 2], [8, 8, 8, 8], [16, 16, 16, 4], [16, 16, 8, 4], [64, 64, 64, 64],
          [1024, 1024, 512, 2]]  # the last: a slice along direction 3 has 3 * 2^29 rows, no call is planned
ORIGINS = [(0, 0, 0, 0), (1, 2, 0, 0)]  # the second: as on a rank of a divided lattice; odd sum, the half fields' offset

# widths of V, m, n_mom, bcg_force_generic: the rows of PLAN in tests/test_basis_slice.py
PLAN = [([32, 32], 16, 0, 0), ([32, 32], 16, 1, 0), ([32, 32], 16, 3, 0), ([32, 32], 16, 4, 0), ([32, 32], 16, 5, 0),
        ([16, 32, 16], 16, 2, 0), ([32] * 5, 16, 0, 0), ([32, 16], 32, 0, 0), ([32, 16], 32, 3, 0), ([16, 5, 32], 16, 0, 0),
        ([16, 5, 32], 16, 4, 0), ([12, 12, 12], 5, 3, 0), ([32, 32], 16, 2, 1)]
# the operands of test_basis_slice_with_several_blocks_per_slice (m = 32) and test_basis_slice_on_8x8x8x8 (m = 16) there
MORE = [([32], 32, 0, 0), ([32], 32, 3, 0), ([32, 32, 16], 16, 0, 0), ([32, 32, 16], 16, 3, 0)]
# [2048] along direction 0, where the budget is below one block per slice until the groups give way
# (test_the_group_shrinks_where_the_scratch_is_short is PLAN's first two rows there): a generic group that halves its columns
# (12 12 | 12 at pc = 2, then 12 | 12 | 12, then pc = 1); a quarter of the scratch: no plan
SHORT = [([12, 12, 12], 32, 2, 0, HALF), ([32, 32], 16, 0, 0, HALF // 4)]


def lattices():
    """(dims, origin, parity, dir): every direction, the full field and both parities where the first extent is even."""
    for dims, origin in itertools.product(SHAPES, ORIGINS):
        for parity in ((-1, 0, 1) if dims[0] % 2 == 0 else (-1,)):
            for direction in range(len(dims)):
                yield dims, origin, parity, direction


def cases():
    for dims, origin, parity, direction in lattices():
        lat = dict(dims=dims, origin=origin, parity=parity, dir=direction)
        L = dims[direction]
        Lg = L if not any(origin) else 2 * L  # (the divided lattice: two ranks along dir)
        for m, mfma, n_mom, half in itertools.product((1, 5, 16, 32), (1, 0), range(6), (HALF, HALF // 8, HALF // 128)):
            yield dict(lat, kind=GRAM, m=m, mfma=mfma, L_global=Lg, n_mom=n_mom, half=half)
        for (widths, m, n_mom, generic), half in itertools.product(PLAN + MORE, (HALF, HALF // 8)):
            yield dict(lat, kind=BASIS, widths=widths, m=m, fast=1 - generic, n_mom=n_mom, half=half)
        if dims == [2048]:
            for widths, m, n_mom, generic, half in SHORT:
                yield dict(lat, kind=BASIS, widths=widths, m=m, fast=1 - generic, n_mom=n_mom, half=half)
        for n_slices in dict.fromkeys((1, 2, L, 2048, 4096)):
            yield dict(lat, kind=AXPY, n_slices=n_slices)


def line(c):
    """The probe's input: integers.  Extents beyond the lattice's dimensions are 1, as in the library."""
    L = list(c["dims"]) + [1] * (4 - len(c["dims"]))
    v = [c["kind"], *L, *c["origin"], c["parity"], c["dir"]]
    if c["kind"] == GRAM:
        v += [c["m"], c["mfma"], c["L_global"], c["n_mom"], c["half"]]
    elif c["kind"] == BASIS:
        v += [c["m"], c["fast"], c["n_mom"], c["half"], len(c["widths"]), *c["widths"]]
    else:
        v += [c["n_slices"]]
    return " ".join(str(x) for x in v)


def label(c):
    head = f"{'x'.join(map(str, c['dims']))} origin={c['origin']} parity={c['parity']} dir={c['dir']}"
    if c["kind"] == GRAM:
        return f"slice_gram_plan {head} m={c['m']} mfma={c['mfma']} L_global={c['L_global']} n_mom={c['n_mom']} half={c['half']}"
    if c["kind"] == BASIS:
        return f"basis_slice_plan {head} V={c['widths']} m={c['m']} fast={c['fast']} n_mom={c['n_mom']} half={c['half']}"
    return f"basis_slice_axpy_plan {head} n_slices={c['n_slices']}"


def find(all_cases, **want):
    """Index of the one case whose fields equal `want`."""
    hits = [i for i, c in enumerate(all_cases) if all(c.get(k) == v for k, v in want.items())]
    assert len(hits) == 1, (want, len(hits))
    return hits[0]


def fields(plan):
    """A plan line of the probe as a dict of strings; "no plan": None."""
    return None if plan == "no plan" else dict(kv.split("=", 1) for kv in plan.split())


def load_table():
    """The plan of every case, from tests/golden/slice_plan_table.json: "plans" holds each distinct plan line once, "cases"
    the index of every case's plan."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slice_plan_table.json")) as f:
        t = json.load(f)
    return [t["plans"][i] for i in t["cases"]]
