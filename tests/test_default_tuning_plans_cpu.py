"""What the stencil planner (blockcg_amd/csrc/hop_plan.cpp) decides, under the shipped tuning, for the local lattices of
tests/test_distributed_default_tuning.py.  Host only: tests/cpp/hop_plan_probe.cpp, as in test_hop_plan_cpu.py.

That GPU file sets nothing about the tuning and relies on its lattices being large enough -- 8 patches of one tile x 8 x 8 --
for the production forms: the bundle sweep k_hop4b for whole launches, the paced column sweep k_hop4c for the interior
class, both on a grid of 512 blocks with the XCD patch walk, and the row form k_hop4 over the boundary tile list.  A later
change of the defaults (hop_plan_cases.DEFAULT mirrors HopTuning and HopSync) or of the planner would otherwise turn it
into one more test of the row form without any test failing.  The expectations are written down here, not recorded in
tests/golden/hop_plan_table.json: that table holds what the launcher decided before the planner existed."""
import re
import subprocess

import pytest

import hop_plan_cases as hpc
from test_hop_plan_cpu import probe  # noqa: F401  (the fixture that builds the probe)

PLAIN, SHIFTED = hpc.MODES.index("HOP_PLAIN"), hpc.MODES.index("HOP_SHIFTED")
WHOLE = (0, 0, 0, 0)

# tests/test_distributed_default_tuning.py's cases: (global dims, process grid, m, ring)
GPU_CASES = [
    ([64, 16, 16, 4], [2, 1, 1, 1], 16, 0),
    ([32, 32, 16, 4], [1, 2, 1, 1], 16, 0),
    ([32, 16, 32, 4], [1, 1, 2, 1], 16, 0),
    ([32, 16, 16, 8], [1, 1, 1, 2], 16, 0),
    ([64, 32, 16, 4], [2, 2, 1, 1], 16, 0),
    ([128, 16, 16, 4], [2, 1, 1, 1], 8, 0),
    ([16, 32, 16, 4], [1, 2, 1, 1], 32, 0),
    ([64, 16, 16, 12], [2, 1, 1, 1], 16, 12),
]


def boundary_tiles(L, split, spb):
    """Tiles with a site next to a ghost face (capi_operator.hip: boundary_tile_list)."""
    n = 0
    for x3 in range(L[3]):
        for x2 in range(L[2]):
            for x1 in range(L[1]):
                b123 = any(split[mu] and x in (0, L[mu] - 1) for mu, x in ((1, x1), (2, x2), (3, x3)))
                n += sum(1 for x0b in range(0, L[0], spb) if b123 or (split[0] and (x0b == 0 or x0b + spb == L[0])))
    return n


def expected(m, cls, win, mode, gram):
    """(kernel instantiation, pacing window of the column sweep or None: the bundle sweep's is not this test's subject) -- or
    "declined"."""
    md, g = hpc.MODES[mode], "true" if gram else "false"
    lo, n, ring, _ = win
    if gram and m == 32:
        return "declined"  # the fused Gram product: m = 16 in every form, m = 8 in the column forms
    if ring:  # capacity mode: whole launches with ring addressing; windows under ten slices stay with the column sweep
        return (f"k_hop4b<{m},{md},{g},true,false>", None) if n >= 10 else (f"k_hop4c<{m},{md},{g},0,true>", 4)
    if cls == 0:
        if m == 8 and mode == SHIFTED:  # the bundle sweep at m = 8 serves the plain hop only
            return f"k_hop4c<8,{md},{g},0,false>", 4
        return f"k_hop4b<{m},{md},{g},false,false>", None
    if cls == 1:  # (the register-capped entry point: with the Gram product, and at m = 8)
        return (f"k_hop4c_interior<{m},{md},{g}>", 4) if gram or m == 8 else (f"k_hop4c<{m},{md},{g},1,false>", 4)
    if gram and m != 16:
        return "declined"  # the row form's Gram product: m = 16
    return f"k_hop4<{m},{md},{g},true,0,false>", None


def requests():
    for gdims, grid, m, ring in GPU_CASES:
        L = [d // g for d, g in zip(gdims, grid)]
        assert all(l * g == d and l % 2 == 0 for l, g, d in zip(L, grid, gdims))
        split = tuple(int(g > 1) for g in grid)
        n_list = boundary_tiles(L, split, 4 * (64 // m))
        assert n_list > 0
        # PLAIN and SHIFTED + Gram; SHIFTED alone is what runs where the Gram product is declined (m = 32, m = 8's boundary)
        modes = [(PLAIN, 0), (SHIFTED, 1), (SHIFTED, 0)]
        shapes = [(0, -1, WHOLE), (1, -1, WHOLE), (2, n_list, WHOLE)]
        if ring:  # the serial sweep's windows of ring 12 on 12 slices (C = 10), and the two-slice window at the start
            shapes += [(0, -1, w + (ring, 0)) for w in ((0, 10), (10, 2), (0, 2), (11, 1), (0, 11), (0, 1))]
        for (cls, list_n, win), (mode, gram) in ((s, md) for s in shapes for md in modes):
            # a fold target as the library offers it: whole launches of whole fields with the Gram product
            fold = int(gram and cls == 0 and not win[2])
            yield dict(m=m, dims=L, split=split, base="default", variant="default", tune=dict(hpc.DEFAULT), cls=cls, list_n=list_n,
                       win=win, mode=mode, gram=gram, fold=fold)


PLAN = re.compile(r"(\S+) lds=\d+ pace=(\d+) fold=(\d) grid=(\d+) walk=(\S+) win=(\S+)$")


def test_default_tuning_plans_the_production_forms_on_the_divided_test_lattices(probe):  # noqa: F811
    exe, out = probe
    cases = list(requests())
    assert len(cases) == 8 * 9 + 6 * 3
    infile = out / "default_tuning_cases.txt"
    infile.write_text("".join(hpc.line(c) + "\n" for c in cases))
    got = subprocess.run([exe, str(infile)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(cases)
    wrong = []
    for c, g in zip(cases, got):
        m, L, cls, win = c["m"], c["dims"], c["cls"], c["win"]
        want = expected(m, cls, win, c["mode"], c["gram"])
        if want == "declined":
            if g != "declined":
                wrong.append((hpc.label(c), g, want))
            continue
        pm = PLAN.match(g)
        if not pm:
            wrong.append((hpc.label(c), g, want))
            continue
        kernel, pace, fold, grid, walk, w = pm.group(1), int(pm.group(2)), int(pm.group(3)), int(pm.group(4)), pm.group(5), pm.group(6)
        tile = 4 * (64 // m)
        if cls == 2:  # the tile list: lexicographic, dealt round-robin to at most 512 blocks
            geometry = (min(c["list_n"], 512), f"{L[0]},{L[1]},{L[2]},0,0")
        else:  # 512 blocks, patches of one tile x 8 x 8 dealt to the XCD classes
            geometry = (512, f"{tile},8,8,1,0")
        n = win[1] if win[1] else L[3]
        ok = (kernel == want[0] and (want[1] is None or pace == want[1]) and (grid, walk) == geometry and
              w == f"{win[0]},{n},{win[2]}" and fold == c["fold"])
        if not ok:
            wrong.append((hpc.label(c), g, want, geometry))
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ; first: {wrong[:4]}"
    # what the GPU file is there for occurs: every production form, paced and with ring addressing
    for needle in ("k_hop4b<16,HOP_PLAIN,false,false,false>", "k_hop4b<16,HOP_SHIFTED,true,false,false>", "k_hop4b<16,HOP_SHIFTED,true,true,false>",
                   "k_hop4c<16,HOP_PLAIN,false,1,false>", "k_hop4c_interior<16,HOP_SHIFTED,true>", "k_hop4c<16,HOP_PLAIN,false,0,true>",
                   "k_hop4<16,HOP_SHIFTED,true,true,0,false>", "k_hop4c<8,HOP_SHIFTED,true,0,false>", "k_hop4b<32,HOP_PLAIN,false,false,false>"):
        assert any(g.startswith(needle + " ") for g in got), needle


@pytest.mark.parametrize("dims,m", [([16, 16, 16, 4], 16), ([32, 16, 8, 8], 16)], ids=["4-patches", "half-patch-in-x2"])
def test_smaller_lattices_fall_to_the_row_form(probe, dims, m):  # noqa: F811
    """The contrast: four patches, or an x2 extent that holds no whole patch, and the same request gets k_hop4 -- which is why the
    GPU file's lattices are no smaller."""
    exe, out = probe
    c = dict(m=m, dims=dims, split=(1, 0, 0, 0), base="default", variant="default", tune=dict(hpc.DEFAULT), cls=0, list_n=-1,
             win=WHOLE, mode=PLAIN, gram=0, fold=0)
    infile = out / "row_form_cases.txt"
    infile.write_text(hpc.line(c) + "\n")
    got = subprocess.run([exe, str(infile)], check=True, capture_output=True, text=True).stdout.strip()
    assert got.startswith(f"k_hop4<{m},HOP_PLAIN,false,true,0,false> "), got
