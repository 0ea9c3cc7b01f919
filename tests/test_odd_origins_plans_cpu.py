"""What the stencil planner (blockcg_amd/csrc/hop_plan.cpp) decides for the local lattices of
tests/test_distributed_odd_origins.py, and which ranks of those cases start at an odd coordinate.  Host only:
tests/cpp/hop_plan_probe.cpp, as in test_hop_plan_cpu.py and test_default_tuning_plans_cpu.py.

That GPU file is about the origin terms of the staggered phase eta_mu(x) = (-1)^(x_0 + ... + x_{mu-1}), which every stencil
kernel forms from local coordinate + origin.  An origin is coords * L_local, so it is odd only where a divided direction has
an odd local extent, and then:
  * an odd local L0 is no multiple of the tile: the planner declines every fast form and the general kernel runs;
  * an odd local L1 or L2 fits no 2 x 2 patch and no 2 x 2 bundle: the row form k_hop4 runs in every tile class (0 the
    whole launch, 1 the interior, 2 the boundary list) and in the ring-addressed windows, lexicographic walk, under the
    miniature tuning the multi-rank tests pin and under the shipped tuning alike;
  * the column sweep k_hop4c and the bundle sweep k_hop4b are never planned there (checked below for patches of odd x1
    or x2 extent too), so no test can reach their origin terms at an odd origin.
The fused Gram product of the row form exists at m = 16 only: at m = 8 and m = 32 the request is declined and the solver
runs the shifted hop without it.

The expectations are written down here, so that a later change of the planner or of the case list cannot turn the GPU file
into a test of even origins or of another form."""
import itertools
import re
import subprocess

import pytest

import hop_plan_cases as hpc
from test_default_tuning_plans_cpu import boundary_tiles
from test_hop_plan_cpu import probe  # noqa: F401  (the fixture that builds the probe)

PLAIN, SHIFTED = hpc.MODES.index("HOP_PLAIN"), hpc.MODES.index("HOP_SHIFTED")
WHOLE = (0, 0, 0, 0)
MODES = [(PLAIN, 0), (SHIFTED, 1), (SHIFTED, 0)]

# tests/test_distributed_odd_origins.py's stencil cases: (global dims, process grid, m, ring, overlap settings, tuning,
# the directions whose origin is odd on some rank, the directions mu whose eta_mu flips on some rank)
STENCIL_CASES = [
    ([6, 4, 4, 4], [2, 1, 1, 1], 5, 0, (1,), "small", (0,), (1, 2, 3)),
    ([6, 4, 4, 4], [2, 1, 1, 1], 16, 0, (0,), "small", (0,), (1, 2, 3)),
    ([6, 6, 4, 4], [2, 2, 1, 1], 5, 0, (1,), "small", (0, 1), (1, 2, 3)),
    ([16, 6, 4, 4], [1, 2, 1, 1], 16, 0, (0, 1), "small", (1,), (2, 3)),
    ([16, 4, 6, 4], [1, 1, 2, 1], 16, 0, (1,), "small", (2,), (3,)),
    ([16, 4, 4, 6], [1, 1, 1, 2], 16, 0, (1,), "small", (3,), ()),
    ([16, 6, 6, 4], [1, 2, 2, 1], 16, 0, (1,), "small", (1, 2), (2, 3)),
    ([32, 6, 4, 4], [1, 2, 1, 1], 8, 0, (1,), "small", (1,), (2, 3)),
    ([8, 4, 6, 4], [1, 1, 2, 1], 32, 0, (1,), "small", (2,), (3,)),
    ([16, 6, 4, 12], [1, 2, 1, 1], 16, 12, (0,), "small", (1,), (2, 3)),
    ([16, 9, 4, 4], [1, 3, 1, 1], 16, 0, (1,), "small", (1,), (2, 3)),
    ([16, 6, 4, 4], [1, 2, 1, 1], 16, 0, (1,), "default", (1,), (2, 3)),
]


def rank_coords(grid):
    """Process-grid coordinates of every rank, direction 0 fastest (blockcg_amd.comm.coords_of)."""
    return [c[::-1] for c in itertools.product(*(range(g) for g in grid[::-1]))]


def origins(gdims, grid):
    L = [d // g for d, g in zip(gdims, grid)]
    return [[c * l for c, l in zip(coords, L)] for coords in rank_coords(grid)]


def flipped(origin):
    """The directions mu whose eta_mu = (-1)^(x_0 + ... + x_{mu-1}) differs between local and global coordinates."""
    return tuple(mu for mu in range(1, 4) if sum(origin[:mu]) % 2)


def ranks_that_flip(gdims, grid):
    """Ranks on which a stencil without its origin terms computes another operator."""
    return [r for r, o in enumerate(origins(gdims, grid)) if flipped(o)]


def tuning_of(m, base):
    return dict(hpc.small_base(m)) if base == "small" else dict(hpc.DEFAULT)


def requests():
    for gdims, grid, m, ring, _, base, _, _ in STENCIL_CASES:
        L = [d // g for d, g in zip(gdims, grid)]
        assert all(l * g == d for l, g, d in zip(L, grid, gdims))
        split = tuple(int(g > 1) for g in grid)
        if m not in hpc.WIDTHS:  # the generic width: no request reaches the planner
            continue
        spb = 4 * (64 // m)
        n_list = boundary_tiles(L, split, spb) if L[0] % spb == 0 else 1
        assert n_list > 0
        shapes = [(0, -1, WHOLE), (1, -1, WHOLE), (2, n_list, WHOLE)]
        if ring:  # the serial sweep's windows of ring 12 on 12 slices (C = 10), and the short windows of the overlapped form
            shapes += [(0, -1, w + (ring, 0)) for w in ((0, 10), (10, 2), (0, 2), (11, 1), (0, 11), (0, 1), (0, 5), (5, 5))]
        for (cls, list_n, win), (mode, gram) in ((s, md) for s in shapes for md in MODES):
            fold = int(gram and cls == 0 and not win[2])
            yield dict(m=m, dims=L, split=split, base=base, variant="default", tune=tuning_of(m, base), cls=cls, list_n=list_n,
                       win=win, mode=mode, gram=gram, fold=fold)


def expected(c):
    """The row form's instantiation k_hop4<m, mode, gram, nt, class, ring> -- or "declined"."""
    m, L, cls, win, gram = c["m"], c["dims"], c["cls"], c["win"], c["gram"]
    if L[0] % (4 * (64 // m)):
        return "declined"  # L0 no multiple of the tile: the general kernel
    if gram and m != 16:
        return "declined"  # the row form's Gram product: m = 16
    return f"k_hop4<{m},{hpc.MODES[c['mode']]},{'true' if gram else 'false'},"


PLAN = re.compile(r"(\S+) lds=\d+ pace=(\d+) fold=(\d) grid=(\d+) walk=(\S+) win=(\S+)$")


def plan(probe_fixture, cases, name):
    exe, out = probe_fixture
    infile = out / name
    infile.write_text("".join(hpc.line(c) + "\n" for c in cases))
    got = subprocess.run([exe, str(infile)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(cases)
    return got


def test_case_list_is_the_gpu_files():
    """The two files speak of the same cases (no GPU needed to import the other one's list)."""
    import test_distributed_odd_origins as gpu
    mine = [(d, g, m, r, o, "default" if shipped else "small") for d, g, m, r, os_, shipped in gpu.STENCIL_CASES for o in os_]
    here = [(d, g, m, r, o, base) for d, g, m, r, os_, base, _, _ in STENCIL_CASES for o in os_]
    assert mine == here


@pytest.mark.parametrize("gdims,grid,m,ring,overlaps,base,odd,flips", STENCIL_CASES,
                         ids=[f"{'x'.join(map(str, c[0]))}-grid{'x'.join(map(str, c[1]))}-m{c[2]}-ring{c[3]}-{c[5]}"
                              for c in STENCIL_CASES])
def test_some_rank_starts_at_an_odd_coordinate(gdims, grid, m, ring, overlaps, base, odd, flips):
    """origin = coords * L_local: the directions the case is about are odd on some rank, the others on none; the phases
    that flip there are the ones the case claims; rank 0 starts at the origin and flips nothing."""
    og = origins(gdims, grid)
    assert og[0] == [0, 0, 0, 0]
    for mu in range(4):
        assert any(o[mu] % 2 for o in og) == (mu in odd), (mu, og)
    assert tuple(sorted({mu for o in og for mu in flipped(o)})) == flips, og
    # the og3 case: an odd origin that no phase may see
    assert bool(ranks_that_flip(gdims, grid)) == bool(flips)
    if ring:  # capacity mode: direction 3 undivided, ring | L3
        assert grid[3] == 1 and gdims[3] % ring == 0


def test_which_ranks_a_stencil_without_origin_terms_gets_wrong():
    """What the one-off mutation run must show: the ranks whose D differs.  (The worker's operator
    applies D twice, so their neighbours fail as well, with a smaller error: they read the wrong D P through the ghost
    faces.  In that run the ranks below erred by 0.79 to 0.98, the others by 0.20 to 0.45, none in the og3 case.)"""
    want = {
        ((6, 4, 4, 4), (2, 1, 1, 1)): [1],
        ((6, 6, 4, 4), (2, 2, 1, 1)): [1, 2, 3],     # origins (3,0), (0,3), (3,3): all three phases; eta_2, eta_3; eta_1
        ((16, 6, 4, 4), (1, 2, 1, 1)): [1],
        ((16, 4, 6, 4), (1, 1, 2, 1)): [1],
        ((16, 4, 4, 6), (1, 1, 1, 2)): [],           # og3 enters no phase
        ((16, 6, 6, 4), (1, 2, 2, 1)): [1, 2, 3],
        ((32, 6, 4, 4), (1, 2, 1, 1)): [1],
        ((8, 4, 6, 4), (1, 1, 2, 1)): [1],
        ((16, 6, 4, 12), (1, 2, 1, 1)): [1],
        ((16, 9, 4, 4), (1, 3, 1, 1)): [1],          # origins 0, 3, 6
    }
    seen = set()
    for gdims, grid, *_ in STENCIL_CASES:
        key = (tuple(gdims), tuple(grid))
        seen.add(key)
        assert ranks_that_flip(gdims, grid) == want[key], key
    assert seen == set(want)


def test_odd_local_extents_plan_the_row_form_or_nothing(probe):  # noqa: F811
    cases = list(requests())
    # eleven cases reach the planner (m = 5 does not), nine requests each, and the ring case's eight windows
    assert len(cases) == 10 * 9 + 8 * 3
    got = plan(probe, cases, "odd_origin_cases.txt")
    wrong = []
    for c, g in zip(cases, got):
        m, L, cls, win = c["m"], c["dims"], c["cls"], c["win"]
        want = expected(c)
        if want == "declined":
            if g != "declined":
                wrong.append((hpc.label(c), g, want))
            continue
        pm = PLAN.match(g)
        if not pm:
            wrong.append((hpc.label(c), g, want))
            continue
        kernel, pace, fold, grid, walk, w = pm.group(1), int(pm.group(2)), int(pm.group(3)), int(pm.group(4)), pm.group(5), pm.group(6)
        tiles = L[0] // (4 * (64 // m)) * L[1] * L[2] * (win[1] if win[1] else L[3])
        blocks = c["tune"]["blocks"]
        n = win[1] if win[1] else L[3]
        tcls = 0 if cls == 2 else cls  # (the boundary class gets its tiles from the list: every listed tile is wanted)
        lexicographic = f"{L[0]},{L[1]},{L[2]},0,0"
        if cls != 2 and L[1] % 2 == 0 and L[2] % 2 == 0:
            # the og3 case, L3 = 3 alone odd: the miniature patches fit, the row form walks them (its 4 patches are no
            # multiple of the 8 XCD classes, so the column forms stay out)
            assert L[3] % 2 == 1 and c["base"] == "small"
            lexicographic = f"{4 * (64 // m)},2,2,1,0"
        ok = (kernel.startswith(want) and kernel.endswith(f",{tcls},{'true' if win[2] else 'false'}>") and pace == 0 and fold == 0 and
              grid == min(c["list_n"] if cls == 2 else tiles, blocks) and walk == lexicographic and
              w == f"{win[0]},{n},{win[2]}")
        if not ok:
            wrong.append((hpc.label(c), g, want))
    assert not wrong, f"{len(wrong)} of {len(cases)} plans differ; first: {wrong[:4]}"
    # what the GPU file is there for occurs: the row form in every class, with its Gram product, with ring addressing, at
    # every width, and under the shipped tuning on a grid of 48 blocks
    for needle in ("k_hop4<16,HOP_PLAIN,false,%s,0,false> ", "k_hop4<16,HOP_SHIFTED,true,%s,0,false> ", "k_hop4<16,HOP_PLAIN,false,%s,1,false> ",
                   "k_hop4<16,HOP_SHIFTED,true,%s,1,false> ", "k_hop4<16,HOP_PLAIN,false,%s,0,true> ", "k_hop4<16,HOP_SHIFTED,true,%s,0,true> ",
                   "k_hop4<8,HOP_SHIFTED,false,%s,1,false> ", "k_hop4<32,HOP_SHIFTED,false,%s,1,false> "):
        assert any(g.startswith(needle % "true") or g.startswith(needle % "false") for g in got), needle
    listed = [g for c, g in zip(cases, got) if c["cls"] == 2 and c["dims"][0] % (4 * (64 // c["m"])) == 0 and not (c["gram"] and c["m"] != 16)]
    assert len(listed) >= 20 and all(g.startswith("k_hop4<") for g in listed)
    shipped = [g for c, g in zip(cases, got) if c["base"] == "default" and c["cls"] == 0]
    assert shipped and all(" grid=48 " in g for g in shipped), shipped
    assert not any("k_hop4c" in g or "k_hop4b" in g for g in got)


@pytest.mark.parametrize("patch", [(16, 3, 2), (16, 2, 3), (16, 3, 3), (16, 1, 1)], ids=lambda p: ",".join(map(str, p)))
def test_patches_of_odd_extent_still_plan_the_row_form(probe, patch):  # noqa: F811
    """Why k_hop4c and k_hop4b stay out of scope: a patch that does divide an odd local extent (x1 or x2 extent 3, or 1)
    makes the patch walk possible, and the planner still chooses the row form -- no block count of the miniature or the
    shipped tuning is one block per tile of such a patch slice with whole patches per XCD class, and a bundle needs even
    extents."""
    cases = []
    for L, blocks in itertools.product(([16, 3, 4, 4], [16, 4, 3, 4], [16, 3, 3, 4], [16, 3, 3, 8]), (32, 48, 512)):
        for cls, (mode, gram) in itertools.product((0, 1), MODES):
            cases.append(dict(m=16, dims=L, split=(0, 1, 1, 0), base="small", variant="default",
                              tune=dict(hpc.DEFAULT, patch=patch, blocks=blocks), cls=cls, list_n=-1, win=WHOLE, mode=mode,
                              gram=gram, fold=int(gram and cls == 0)))
    got = plan(probe, cases, "odd_patch_cases.txt")
    for c, g in zip(cases, got):
        want = f"k_hop4<16,{hpc.MODES[c['mode']]},{'true' if c['gram'] else 'false'},"
        assert g.startswith(want) and " pace=0 fold=0 " in g, (hpc.label(c), c["tune"]["patch"], c["tune"]["blocks"], g)
