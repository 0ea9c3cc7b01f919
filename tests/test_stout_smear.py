"""Stout smearing of the links and the plaquette on the device (include/blockcg_hip.h: bcg_gauge_stout_smear,
bcg_gauge_plaquette) against the numpy restatement tests/stout_ref.py, whose step uses the eigendecomposition where the
kernel uses the Cayley-Hamilton form.  Bound: 1e-13 relative Frobenius error over the whole link field (the kernel-level
convention of the distributed workers); the three formulations of the reference agree to a few 1e-15
(test_stout_smear_cpu.py asserts 2.5e-14), so the bound keeps at least 4x over the reference's own disagreement.
Lattices: [4,4,2,6] (the extent 2 makes x+nu = x-nu), [6,4,4,4], [4,1,4,6] (an extent 1 inside), 3-D, 2-D, and 1-D (no
staple: a copy)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import stout_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-13
LATTICES = [[4, 4, 2, 6], [6, 4, 4, 4], [4, 1, 4, 6], [4, 6, 4], [8, 6], [16]]
INVALID, COMM = 1, 5


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


_contexts = {}


def _ctx(bc, dims):
    key = tuple(dims)
    if key not in _contexts:
        _contexts[key] = bc.Context(list(dims), device=0)
    return _contexts[key]


def asym_table(nd):
    return np.array([[0.12 + 0.01 * mu + 0.003 * nu for nu in range(nd)] for mu in range(nd)])


def pair_table(nd):
    t = np.zeros((nd, nd))
    if nd >= 2:
        t[nd - 1, 0] = 0.17  # one single pair, and not its transpose
    return t


def container(bc, ctx, M=None):
    g = bc.gauge_field(ctx)
    return g if M is None else g.upload(ref.to_lib(M))


def links_of(g):
    return ref.from_lib(g.download())


def make_fields(bc, dims):
    """random non-unitary links from the device generator, and SU(3) links"""
    ctx = _ctx(bc, dims)
    V, nd = ctx.V, len(dims)
    rng = np.random.default_rng(100 + len(dims) + dims[0])
    return {"random": links_of(bc.gauge_field(ctx).setRandom(5)), "su3": ref.random_su3((V, nd), 0.4, rng)}


@pytest.mark.parametrize("dims", LATTICES, ids=lambda d: "x".join(map(str, d)))
def test_against_the_reference(bc, dims):
    ctx = _ctx(bc, dims)
    nd = len(dims)
    worst = 0.0
    for kind, U in make_fields(bc, dims).items():
        gin, out, work = container(bc, ctx, U), container(bc, ctx), container(bc, ctx)
        cases = [("spatial", 0.1, nd - 1, n) for n in (0, 1, 2, 3)] + [("table", asym_table(nd), None, n) for n in (1, 2, 3)] + \
                [("pair", pair_table(nd), None, 2)]
        for name, rho, d, n in cases:
            want = ref.stout_smear(U, rho, dims, n, dir=d)
            got = links_of(bc.stout_smear(out, gin, rho, n, dir=d, work=work))
            err = ref.rel_err(got, want)
            print(dims, kind, name, n, "%.2e" % err)
            assert np.all(np.isfinite(got)) and err <= TOL, (dims, kind, name, n, err)
            worst = max(worst, err)
            table = ref.rho_table(rho, nd, d)
            for mu in range(nd):  # directions that no live term smears are copied bit for bit
                live = dims[mu] > 1 and any(table[mu, nu] != 0.0 and dims[nu] > 1 for nu in range(nd))
                if not live or n == 0:
                    assert np.array_equal(got[:, mu], U[:, mu]), (dims, kind, name, n, mu)
            assert np.array_equal(links_of(gin), U)  # in is not written
    print(dims, "worst %.2e" % worst)


def test_work_rerun_and_operator_links(bc):
    dims = [4, 4, 2, 6]
    ctx = _ctx(bc, dims)
    D = bc.dirac_op(ctx, 0.1, seed=5)
    U = links_of(bc.gauge_field(ctx).setRandom(5))
    out, out2, work = container(bc, ctx), container(bc, ctx), container(bc, ctx)
    for n in (1, 2, 3):
        a = bc.stout_smear(out, D, asym_table(4), n, work=work).download()
        b = bc.stout_smear(out2, D, asym_table(4), n).download()  # work = NULL
        c = bc.stout_smear(out, D, asym_table(4), n, work=work).download()  # once more
        assert np.array_equal(a, b) and np.array_equal(a, c), n
        assert ref.rel_err(ref.from_lib(a), ref.stout_smear(U, asym_table(4), dims, n)) <= TOL


def test_unread_direction_may_hold_nan(bc):
    dims = [4, 4, 2, 6]
    ctx = _ctx(bc, dims)
    rng = np.random.default_rng(3)
    U = ref.random_su3((ctx.V, 4), 0.4, rng)
    U[:, 3] = np.nan
    got = links_of(bc.stout_smear(container(bc, ctx), container(bc, ctx, U), 0.1, 3, dir=3))
    want = ref.stout_smear(U, 0.1, dims, 3, dir=3)
    assert np.all(np.isfinite(got[:, :3])) and ref.rel_err(got[:, :3], want[:, :3]) <= TOL
    assert np.array_equal(got[:, 3].view(np.uint64), U[:, 3].view(np.uint64))


def test_unit_links_and_small_su3(bc):
    dims = [6, 4, 4, 4]
    ctx = _ctx(bc, dims)
    one = np.broadcast_to(np.eye(3, dtype=np.complex128), (ctx.V, 4, 3, 3)).copy()
    got = links_of(bc.stout_smear(container(bc, ctx), container(bc, ctx, one), asym_table(4), 3))
    assert np.all(np.isfinite(got)) and np.abs(got - one).max() <= 1e-15
    rng = np.random.default_rng(4)
    for eps in (1e-3, 1e-6, 1e-9):
        U = ref.random_su3((ctx.V, 4), eps, rng)
        got = links_of(bc.stout_smear(container(bc, ctx), container(bc, ctx, U), asym_table(4), 3))
        err = ref.rel_err(got, ref.stout_smear(U, asym_table(4), dims, 3))
        print("eps", eps, "%.2e" % err)
        assert np.all(np.isfinite(got)) and err <= TOL, (eps, err)


@pytest.mark.parametrize("dims", [[4, 4, 2, 6], [4, 6, 4]], ids=["4d", "3d"])
def test_gauge_covariance_on_the_device(bc, dims):
    """S(U^g) = g S(U) g^dagger for random non-unitary links, both sides smeared on the device"""
    ctx = _ctx(bc, dims)
    nd = len(dims)
    rng = np.random.default_rng(8)
    U = links_of(bc.gauge_field(ctx).setRandom(12))
    g = ref.random_su3((ctx.V,), 1.0, rng)
    Ug = ref.gauge_transform(U, g, dims)
    out = container(bc, ctx)
    a = links_of(bc.stout_smear(out, container(bc, ctx, Ug), asym_table(nd), 2))
    b = ref.gauge_transform(links_of(bc.stout_smear(out, container(bc, ctx, U), asym_table(nd), 2)), g, dims)
    assert ref.rel_err(a, b) <= TOL
    Pa, Pb = bc.plaquette(container(bc, ctx, Ug)), bc.plaquette(container(bc, ctx, U))
    _, scale = ref.plaquette(U, dims, with_scale=True)
    assert np.all(np.abs(Pa - Pb) <= 2 * TOL * scale + 1e-300)


@pytest.mark.parametrize("dims", LATTICES, ids=lambda d: "x".join(map(str, d)))
def test_plaquette(bc, dims):
    ctx = _ctx(bc, dims)
    nd = len(dims)
    for kind, U in make_fields(bc, dims).items():
        g = container(bc, ctx, U)
        P = bc.plaquette(g)
        want, scale = ref.plaquette(U, dims, with_scale=True)
        print(dims, kind, "plaquette error / bound: %.2e" % (np.abs(P - want) / np.maximum(TOL * scale, 1e-300)).max())
        assert P.shape == (nd, nd) and np.all(np.abs(P - want) <= TOL * scale), (dims, kind, P, want)
        assert np.array_equal(P, bc.plaquette(g))  # the same bits
        for mu in range(nd):
            for nu in range(nd):
                if mu == nu or dims[mu] == 1 or dims[nu] == 1:
                    assert P[mu, nu] == 0.0
        assert np.array_equal(links_of(g), U)
    if nd == 4:  # rises under smearing of SU(3) links
        U = make_fields(bc, dims)["su3"]
        before = bc.plaquette(container(bc, ctx, U))
        after = bc.plaquette(bc.stout_smear(container(bc, ctx), container(bc, ctx, U), 0.1, 3, dir=3))
        live = np.array([[mu != nu and dims[mu] > 1 and dims[nu] > 1 for nu in range(4)] for mu in range(4)])
        assert np.all(after[live] > before[live])


def test_laplacian_over_smeared_links(bc):
    dims = [4, 4, 2, 6]
    ctx = _ctx(bc, dims)
    rng = np.random.default_rng(9)
    U = ref.random_su3((ctx.V, 4), 0.4, rng)
    smeared = bc.stout_smear(container(bc, ctx), container(bc, ctx, U), 0.1, 3, dir=3)
    psi = bc.block_fermion_field(ctx, 4).setGaussian(6)
    out = bc.block_fermion_field(ctx, 4)
    got = bc.laplacian(out, psi, smeared, dir=3).download().transpose(0, 2, 1)
    want = ref.laplacian(psi.download().transpose(0, 2, 1), ref.stout_smear(U, 0.1, dims, 3, dir=3), dims, 3)
    assert ref.rel_err(got, want) <= TOL


def test_error_returns_leave_out_untouched(bc):
    dims = [4, 4, 2, 6]
    ctx = _ctx(bc, dims)
    other = bc.Context(dims, device=0)
    gin, out, work = bc.gauge_field(ctx).setRandom(1), bc.gauge_field(ctx).setRandom(2), bc.gauge_field(ctx).setRandom(3)
    foreign = bc.gauge_field(other).setRandom(4)
    before = out.download()
    nan_table = np.full((4, 4), 0.1)
    nan_table[1, 2] = np.nan
    inf_table = np.full((4, 4), 0.1)
    inf_table[3, 0] = np.inf
    bad = [lambda: bc.stout_smear(out, out, 0.1, 1), lambda: bc.stout_smear(out, gin, 0.1, 2, work=out),
           lambda: bc.stout_smear(out, gin, 0.1, 2, work=gin), lambda: bc.stout_smear(out, foreign, 0.1, 1),
           lambda: bc.stout_smear(out, gin, 0.1, 2, work=foreign), lambda: bc.stout_smear(out, gin, 0.1, -1),
           lambda: bc.stout_smear(out, gin, nan_table, 1), lambda: bc.stout_smear(out, gin, inf_table, 1)]
    for k, call in enumerate(bad):
        with pytest.raises(bc.BlockCGError) as e:
            call()
        assert e.value.code == INVALID, k
        assert np.array_equal(out.download(), before), k
    with pytest.raises(bc.BlockCGError) as e:
        bc.stout_smear(foreign, gin, 0.1, 1)
    assert e.value.code == INVALID
    lib = ctx.lib
    dp = nan_table.ctypes.data_as(bc.api.c_dbl_p)
    assert lib.bcg_gauge_stout_smear(ctx.h, out.h, gin.h, None, 1, None) == INVALID
    assert lib.bcg_gauge_stout_smear(ctx.h, None, gin.h, dp, 1, None) == INVALID
    assert lib.bcg_gauge_stout_smear(ctx.h, out.h, None, dp, 1, None) == INVALID
    assert lib.bcg_gauge_stout_smear(None, out.h, gin.h, dp, 1, None) == INVALID
    assert lib.bcg_gauge_plaquette(ctx.h, None, dp) == INVALID
    assert lib.bcg_gauge_plaquette(ctx.h, gin.h, None) == INVALID
    assert lib.bcg_gauge_plaquette(ctx.h, foreign.h, dp) == INVALID
    assert np.array_equal(out.download(), before)
    # a NaN on the diagonal is ignored
    diag = np.full((4, 4), 0.1)
    diag[np.arange(4), np.arange(4)] = np.nan
    got = links_of(bc.stout_smear(out, gin, diag, 1))
    assert ref.rel_err(got, ref.stout_smear(links_of(gin), 0.1, dims, 1)) <= TOL
    # a divided lattice without a bcg_comm
    half = bc.Context(dims, device=0, grid=[2, 1, 1, 1], coords=[0, 0, 0, 0])
    a, b = bc.gauge_field(half).setRandom(1), bc.gauge_field(half).setRandom(2)
    keep = b.download()
    with pytest.raises(bc.BlockCGError) as e:
        bc.stout_smear(b, a, 0.1, 1)
    assert e.value.code == COMM and np.array_equal(b.download(), keep)
    with pytest.raises(bc.BlockCGError) as e:
        bc.plaquette(a)
    assert e.value.code == COMM


def test_profile_keys(bc):
    dims = [6, 4, 4, 4]
    ctx = _ctx(bc, dims)
    gin, out = bc.gauge_field(ctx).setRandom(1), bc.gauge_field(ctx)
    ctx.profiling(True)
    ctx.profile_reset()
    bc.stout_smear(out, gin, 0.1, 3, dir=3)
    bc.plaquette(out)
    prof = ctx.profile()
    ctx.profiling(False)
    assert prof["stout_smear"]["count"] == 3 and prof["plaquette"]["count"] == 1, prof
    assert prof["stout_smear"]["bytes"] == pytest.approx(3 * 2 * 144 * 4 * ctx.V, rel=1e-4)
    assert prof["plaquette"]["bytes"] == pytest.approx(144 * 4 * ctx.V, rel=1e-4)


def test_stout_distillation_example(bc):
    """examples/stout_distillation.cpp on 4^4: plaquettes before and after, Laplacian modes over the smeared container"""
    from test_cpp_dropin import _compile
    exe = _compile(os.path.join(ROOT, "examples", "stout_distillation.cpp"), "stout_distillation")
    r = subprocess.run([exe, "4", "4", "4", "4"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "STOUT_DISTILLATION_OK" in r.stdout, r.stdout + r.stderr
