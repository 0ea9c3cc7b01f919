"""Ties the planner's table (tests/golden/hop_plan_table.json, test_hop_plan_cpu.py) to what runs on the device: for a few
shapes, one application of the operator -- or one phase A where the mode needs it -- with profiling on.  The stencil_form_*
counters that moved must be exactly the forms the table names for the launches of that call, and the result must equal that
of the same call on other kernels: bit for bit against the column sweep (BCG_HOP_BUNDLE=0; same arithmetic per site, as
test_gpu_parity.py holds between the bundle sweep and the ring windows' column sweep) and against the whole intermediate
field for capacity mode; at TOL_KERNEL where the other kernels round differently (the generic half-volume kernel, as
test_half_volume.py compares; the unfactored form of phase A, as test_phase_a_operator.py compares)."""
import collections
import ctypes

import numpy as np
import pytest

from conftest import TOL_KERNEL, rel_err
import hop_plan_cases as hpc

PLAIN, SHIFTED, FACT1, FACT2 = 0, 1, 3, 4
WHOLE, WHOLE_CB = (0, 0, 0, 0), (0, 0, 0, 1)
MASS = 0.3


def _form(plan):
    if plan == "declined":
        return None
    kernel = plan.split(" ")[0]
    if kernel.startswith("k_hop4b<"):
        return "stencil_form_k_hop4b_checkerboard" if kernel.endswith(",true>") else "stencil_form_k_hop4b"
    return "stencil_form_k_hop4c" if kernel.startswith("k_hop4c") else "stencil_form_k_hop4"


class _Table:
    def __init__(self):
        self.cases = list(hpc.cases())
        self.plans, _ = hpc.load_table()

    def form(self, m, dims, win, mode, gram):
        """The form the table names for a whole launch (tile class 0) under the small lattices' tuning."""
        i = hpc.find(self.cases, m=m, dims=dims, split=(0, 0, 0, 0), base="small", variant="default", cls=0, list_n=-1, win=win,
                     mode=mode, gram=gram)
        return _form(self.plans[i])


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


@pytest.fixture(scope="module")
def table():
    return _Table()


def _context(bc, m, dims, monkeypatch, ring=0, **env):
    t = hpc.small_base(m)
    monkeypatch.setenv("BCG_HOP_PATCH", ",".join(map(str, t["patch"])))
    monkeypatch.setenv("BCG_HOP_BLOCKS", str(t["blocks"]))
    for k in ("BCG_HOP_BUNDLE", "BCG_HOP_FACTORED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = bc.Context(dims)
    ctx.capacity_mode(ring)
    ctx.profiling(True)
    return ctx


def _forms(ctx):
    return collections.Counter({k: v["count"] for k, v in ctx.profile().items() if k.startswith("stencil_form_")})


def _apply(bc, orc, m, dims, monkeypatch, parity=None, ring=0, generic=False, **env):
    ctx = _context(bc, m, dims, monkeypatch, ring, **env)
    ctx.force_generic(generic)
    D = bc.dirac_op(ctx, MASS, U=orc.fill_gauge(dims, 71))
    if parity is None:
        B = bc.block_fermion_field(ctx, m, orc.fill_field(m, int(np.prod(dims)), 72))
        out = bc.block_fermion_field(ctx, m)
    else:
        B = bc.block_fermion_field(ctx, m, parity=parity).setRandom(seed=72)
        out = bc.block_fermion_field(ctx, m, parity=parity)
    D.op(out, B)
    return out.download(), _forms(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("m,dims", [(16, [16, 8, 8, 8]), (16, [32, 8, 8, 6]), (8, [64, 8, 8, 4]), (32, [16, 8, 8, 4])],
                         ids=["m16-16x8x8x8", "m16-32x8x8x6", "m8-64x8x8x4", "m32-16x8x8x4"])
def test_operator_runs_the_forms_the_table_names(bc, orc, table, m, dims, monkeypatch):
    want = collections.Counter(table.form(m, dims, WHOLE, mode, 0) for mode in (PLAIN, SHIFTED))
    out, forms = _apply(bc, orc, m, dims, monkeypatch)
    print(f"m = {m}, {dims}: {dict(forms)}; table: {dict(want)}")
    assert forms == want
    assert "stencil_form_k_hop4b" in forms  # (these shapes are here because they reach the bundle sweep)
    column, forms0 = _apply(bc, orc, m, dims, monkeypatch, BCG_HOP_BUNDLE="0")
    assert forms0 == {"stencil_form_k_hop4c": 2}
    assert np.array_equal(out, column)


@pytest.mark.gpu
def test_half_volume_operator_runs_the_form_the_table_names(bc, orc, table, monkeypatch):
    m, dims = 16, [64, 8, 8, 6]  # test_half_volume.py's checkerboard shape
    want = collections.Counter(table.form(m, dims, WHOLE_CB, mode, 0) for mode in (PLAIN, SHIFTED))
    assert want == {"stencil_form_k_hop4b_checkerboard": 2}
    out, forms = _apply(bc, orc, m, dims, monkeypatch, parity=0)
    assert forms == want
    generic, forms_g = _apply(bc, orc, m, dims, monkeypatch, parity=0, generic=True)
    assert not forms_g
    e = rel_err(out, generic)
    print(f"half-volume operator, checkerboard bundle sweep vs generic kernel: {e:.3e}")
    assert e < TOL_KERNEL


@pytest.mark.gpu
def test_capacity_ring_runs_the_forms_the_table_names(bc, orc, table, monkeypatch):
    m, dims, ring = 16, [32, 8, 8, 6], 3  # the smallest ring the suite uses: chunks of one slice
    # the first stencil's windows are counted: one slice (L3 - 1, the chunks' next slice, slice 0 again) and the first two
    want = {table.form(m, dims, win, PLAIN, 0) for win in ((5, 1, ring, 0), (0, 2, ring, 0), (0, 1, ring, 0))}
    out, forms = _apply(bc, orc, m, dims, monkeypatch, ring=ring)
    print(f"ring {ring}: {dict(forms)}; table: {want}")
    assert set(forms) == want and None not in want
    whole, _ = _apply(bc, orc, m, dims, monkeypatch)
    assert np.array_equal(out, whole)


@pytest.mark.gpu
def test_phase_a_runs_the_factored_pair_the_table_names(bc, orc, table, monkeypatch):
    m, dims = 16, [32, 8, 8, 6]
    want = collections.Counter([table.form(m, dims, WHOLE, FACT1, 0), table.form(m, dims, WHOLE, FACT2, 1)])
    assert want == {"stencil_form_k_hop4b": 2}
    want["stencil_form_factored_pair"] = 1
    got = {}
    for tag, env in (("pair", {}), ("column", {"BCG_HOP_BUNDLE": "0"})):
        ctx = _context(bc, m, dims, monkeypatch, **env)
        D = bc.dirac_op(ctx, MASS, U=orc.fill_gauge(dims, 71))
        P = bc.block_fermion_field(ctx, m, orc.fill_field(m, int(np.prod(dims)), 72))
        T = bc.block_fermion_field(ctx, m)
        aid = ctx.lib.bcg_debug_phase_a
        aid.restype = ctypes.c_int
        aid.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        ctx.check(aid(ctx.h, D.h, MASS, 0.05, T.h, P.h))
        got[tag] = (T.download(), _forms(ctx))
    assert got["pair"][1] == want
    # without the bundle sweep the pair has no kernel: the unfactored form on the column sweep, Gram product fused
    assert got["column"][1] == {"stencil_form_k_hop4c": 2}
    e = rel_err(got["pair"][0], got["column"][0])
    print(f"phase A, factored pair vs unfactored column sweep: {e:.3e}")
    assert e < TOL_KERNEL
