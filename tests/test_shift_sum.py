"""The covariant nearest-neighbour sum and smearing on the device (include/blockcg_hip.h: bcg_dirac_shift_sum,
bcg_covariant_smear) against their numpy restatement (tests/shift_sum_ref.py): every width class, ragged shapes, an extent
of 1, both kernel forms at the smallest shapes the tile form takes and at two tiles along x0, the identities with
bcg_dirac_hop and hermitian_dot, skipped terms, half fields, smearing, the error returns, and the example end to end.

Tolerance: TOL_KERNEL (1e-13 relative Frobenius error) for one application; n * TOL_KERNEL <= 1e-12 for n <= 10 smearing steps."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, TOL_KERNEL, rel_err
import shift_sum_ref as ref

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, COMM = 1, 2, 5
TOL_SMEAR = 1e-12
# (m, dims): one tile of 256 / m sites along x0, and two (the x0 wrap then crosses a tile border)
TILE_CASES = [(16, [16, 4, 4, 4]), (16, [32, 2, 2, 2]), (8, [32, 2, 2, 2]), (8, [64, 2, 2, 2]), (32, [8, 4, 4, 4]),
              (32, [16, 2, 2, 2])]


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _coefficients(rng, nd):
    return (complex(rng.normal(), rng.normal()), rng.normal(size=nd) + 1j * rng.normal(size=nd),
            rng.normal(size=nd) + 1j * rng.normal(size=nd))


_CASES = {}


def _case(bc, dims, m, unitary=False):
    """Context, links (host and device), one input field (host and device): made once per shape and width, never changed."""
    key = (tuple(dims), m, unitary)
    if key not in _CASES:
        rng = np.random.default_rng(100 + m + 7 * len(_CASES))
        ctx = bc.Context(dims)
        U = ref.unitary_links(rng, dims) if unitary else ref.random_links(rng, dims)
        psi = ref.random_field(rng, ctx.V, m)
        _CASES[key] = (ctx, U, bc.gauge_field(ctx).upload(U), psi, bc.block_fermion_field(ctx, m, host=psi))
    return _CASES[key]


def _forms(ctx):
    prof = ctx.profile()
    return prof.get("shift_form_tile", {}).get("count", 0), prof.get("shift_form_generic", {}).get("count", 0)


def _check_random(bc, dims, m, seed=5):
    ctx, U, links, psi, f = _case(bc, dims, m)
    rng = np.random.default_rng(seed)
    out = bc.block_fermion_field(ctx, m)
    worst = 0.0
    for eta in (False, True):
        c0, fw, bw = _coefficients(rng, len(dims))
        got = bc.shift_sum(out, f, links, c0, fw, bw, eta).download()
        err = rel_err(got, ref.shift_sum(U, dims, psi, c0, fw, bw, eta))
        worst = max(worst, err)
        assert err <= TOL_KERNEL, (dims, m, eta, err)
    assert np.array_equal(_bits(f.download()), _bits(psi))  # `in` untouched
    return worst


@pytest.mark.parametrize("m", [1, 5, 8, 12, 16, 32])
def test_against_the_reference(bc, m):
    print(f"[4,2,4,2], m = {m}: largest error {_check_random(bc, [4, 2, 4, 2], m):.2e}")


@pytest.mark.parametrize("dims,m", [([5, 3, 2], 16), ([7, 5, 3, 3], 12), ([37], 5), ([1, 4, 2, 3], 5), ([1, 4, 2, 3], 16)], ids=str)
def test_ragged_shapes_and_an_extent_of_one(bc, dims, m):
    print(f"{dims}, m = {m}: largest error {_check_random(bc, dims, m):.2e}")


@pytest.mark.parametrize("m,dims", TILE_CASES, ids=str)
def test_tile_form(bc, m, dims):
    """The tile form runs (asserted from the profile), equals the reference, and equals the generic form under force_generic."""
    ctx, U, links, psi, f = _case(bc, dims, m)
    assert dims[0] % (256 // m) == 0
    rng = np.random.default_rng(9)
    out = bc.block_fermion_field(ctx, m)
    for eta in (False, True):
        c0, fw, bw = _coefficients(rng, 4)
        want = ref.shift_sum(U, dims, psi, c0, fw, bw, eta)
        ctx.profiling(True)
        try:
            ctx.profile_reset()
            got = bc.shift_sum(out, f, links, c0, fw, bw, eta).download()
            assert _forms(ctx) == (1, 0), ctx.profile().keys()
            ctx.force_generic(True)
            ctx.profile_reset()
            gen = bc.shift_sum(out, f, links, c0, fw, bw, eta).download()
            assert _forms(ctx) == (0, 1)
        finally:  # the context is shared with later tests of this shape and width
            ctx.force_generic(False)
            ctx.profiling(False)
        e1, e2, e3 = rel_err(got, want), rel_err(gen, want), rel_err(got, gen)
        print(f"{dims}, m = {m}, eta = {eta}: tile {e1:.2e}, generic {e2:.2e}, tile vs generic {e3:.2e}")
        assert max(e1, e2, e3) <= TOL_KERNEL


@pytest.mark.parametrize("dims,m", [([4, 2, 4, 2], 5), ([16, 4, 4, 4], 16)], ids=str)
def test_half_half_eta_is_the_hop(bc, dims, m):
    ctx, U, _, psi, f = _case(bc, dims, m)
    D = bc.dirac_op(ctx, 0.1, U=U)
    hop, out = bc.block_fermion_field(ctx, m), bc.block_fermion_field(ctx, m)
    D.D(hop, f)
    bc.shift_sum(out, f, D, 0.0, 0.5, -0.5, eta=True)
    err = rel_err(out.download(), hop.download())
    print(f"{dims}, m = {m}: shift_sum(0, 1/2, -1/2, eta) vs bcg_dirac_hop {err:.2e}")
    assert err <= TOL_KERNEL


@pytest.mark.parametrize("dims,m", [([4, 2, 4, 2], 5), ([16, 4, 4, 4], 16)], ids=str)
def test_adjoint_identity_through_hermitian_dot(bc, dims, m):
    """phi^dagger S(c0, f, b) psi = (S(conj c0, conj b, conj f) phi)^dagger psi; hermitian_dot computes the lower triangle and
    mirrors it, so the lower triangles are compared."""
    ctx, U, links, psi, f = _case(bc, dims, m)
    rng = np.random.default_rng(11)
    phi = bc.block_fermion_field(ctx, m, host=ref.random_field(rng, ctx.V, m))
    a, b = bc.block_fermion_field(ctx, m), bc.block_fermion_field(ctx, m)
    for eta in (False, True):
        c0, fw, bw = _coefficients(rng, 4)
        bc.shift_sum(a, f, links, c0, fw, bw, eta)
        bc.shift_sum(b, phi, links, np.conj(c0), np.conj(bw), np.conj(fw), eta)
        lhs, rhs = np.tril(phi.hermitian_dot(a)), np.tril(b.hermitian_dot(f))
        scale = np.sqrt(np.trace(phi.hermitian_dot(phi)).real * np.trace(a.hermitian_dot(a)).real)  # |phi| |S psi|
        assert np.linalg.norm(lhs - rhs) <= TOL_KERNEL * scale, (dims, m, eta)


@pytest.mark.parametrize("dims,m", [([4, 2, 4, 2], 5), ([16, 4, 4, 4], 16)], ids=str)
def test_shift_there_and_back_with_unitary_links(bc, dims, m):
    ctx, U, links, psi, f = _case(bc, dims, m, unitary=True)
    a, b = bc.block_fermion_field(ctx, m), bc.block_fermion_field(ctx, m)
    for mu in range(4):
        for first in (+1, -1):
            bc.covariant_shift(a, f, links, mu, first)
            bc.covariant_shift(b, a, links, mu, -first)
            assert rel_err(b.download(), psi) <= TOL_KERNEL, (mu, first)
        assert rel_err(a.download(), ref.shift_sum(U, dims, psi, 0.0, None, np.eye(4)[mu])) <= TOL_KERNEL


@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
def test_terms_with_a_zero_coefficient_are_skipped(bc, generic):
    """Links of direction 3 are NaN: whatever does not use direction 3 is finite and right, whatever does is not finite."""
    dims, m = [16, 4, 4, 4], 16
    ctx, U, _, psi, f = _case(bc, dims, m)
    Un = U.copy()
    Un[:, 3] = np.nan
    links = bc.gauge_field(ctx).upload(Un)
    out = bc.block_fermion_field(ctx, m)
    ctx.force_generic(generic)
    ctx.profiling(True)
    ctx.profile_reset()
    try:
        lap = bc.laplacian(out, f, links, 3).download()
        assert np.all(np.isfinite(lap)) and rel_err(lap, ref.laplacian(U, dims, psi, 3)) <= TOL_KERNEL
        sh = bc.covariant_shift(out, f, links, 1, +1).download()
        assert np.all(np.isfinite(sh)) and rel_err(sh, ref.shift_sum(U, dims, psi, 0.0, np.eye(4)[1], None)) <= TOL_KERNEL
        sh = bc.covariant_shift(out, f, links, 2, -1).download()
        assert np.all(np.isfinite(sh)) and rel_err(sh, ref.shift_sum(U, dims, psi, 0.0, None, np.eye(4)[2])) <= TOL_KERNEL
        for fw, bw in ((1e-300 * np.eye(4)[3], None), (None, 1e-300j * np.eye(4)[3])):  # the probe sees the links at all
            assert not np.all(np.isfinite(bc.shift_sum(out, f, links, 1.0, fw, bw).download()))
        assert _forms(ctx) == ((0, 5) if generic else (5, 0))
    finally:
        ctx.force_generic(False)
        ctx.profiling(False)


@pytest.mark.parametrize("dims,m", [([4, 2, 4, 2], 5), ([4, 2, 4, 2], 16), ([8, 4, 4, 4], 5), ([8, 4, 4, 4], 16)], ids=str)
def test_half_fields(bc, dims, m):
    """S_half(even part) -> odd and S_half(odd part) -> even, merged, equal the full-field call with c0 = 0."""
    ctx, U, links, psi, f = _case(bc, dims, m)
    rng = np.random.default_rng(13)
    even, odd = f.split_parity()
    to_odd, to_even = bc.block_fermion_field(ctx, m, parity=1), bc.block_fermion_field(ctx, m, parity=0)
    full, merged = bc.block_fermion_field(ctx, m), bc.block_fermion_field(ctx, m)
    for eta in (False, True):
        _, fw, bw = _coefficients(rng, 4)
        bc.shift_sum(to_odd, even, links, 0.0, fw, bw, eta)
        bc.shift_sum(to_even, odd, links, 0.0, fw, bw, eta)
        merged.merge_parity(to_even, to_odd)
        bc.shift_sum(full, f, links, 0.0, fw, bw, eta)
        want = ref.shift_sum(U, dims, psi, 0.0, fw, bw, eta)
        assert rel_err(merged.download(), full.download()) <= TOL_KERNEL
        assert rel_err(merged.download(), want) <= TOL_KERNEL
        assert rel_err(to_odd.download(), want[ref.parity_mask(dims, 1)]) <= TOL_KERNEL
    with pytest.raises(bc.BlockCGError) as e:
        bc.shift_sum(to_odd, even, links, 1e-300, fw, bw)
    assert e.value.code == INVALID


@pytest.mark.parametrize("dims,m", [([4, 2, 4, 2], 5), ([16, 4, 4, 4], 16)], ids=str)
def test_smear_is_its_shift_sums(bc, dims, m):
    """smear(n) against n hand-made shift_sum calls bit for bit, and against the reference applied n times; with and without
    a work field; a second call returns the same bits."""
    ctx, U, links, psi, f = _case(bc, dims, m)
    kappa, direction = 0.0625 + 1e-3, 3
    hop = np.full(4, kappa, dtype=np.complex128)
    hop[direction] = 0
    c0 = 1.0 - 2.0 * kappa * 3
    for n in (0, 1, 2, 5):
        a, b = f.copy(), bc.block_fermion_field(ctx, m)
        for _ in range(n):
            bc.shift_sum(b, a, links, c0, hop, hop)
            a, b = b, a
        by_hand = a.download()
        got = bc.smear(f.copy(), links, direction, kappa, n).download()
        assert np.array_equal(_bits(got), _bits(by_hand)), (dims, m, n)
        work = bc.block_fermion_field(ctx, m)
        g = f.copy()
        assert np.array_equal(_bits(bc.smear(g, links, direction, kappa, n, work=work).download()), _bits(by_hand)), (dims, m, n)
        if n == 0:
            assert np.array_equal(_bits(got), _bits(psi))
        err = rel_err(got, ref.smear(U, dims, psi, direction, kappa, n))
        print(f"{dims}, m = {m}, n = {n}: smear vs reference {err:.2e}")
        assert err <= TOL_SMEAR
    every = bc.smear(f.copy(), links, -1, kappa, 2).download()
    assert rel_err(every, ref.smear(U, dims, psi, -1, kappa, 2)) <= TOL_SMEAR


def test_smeared_point_source_stays_on_its_time_slice(bc):
    dims, m, t0 = [8, 8, 8, 4], 3, 2
    rng = np.random.default_rng(17)
    ctx = bc.Context(dims)
    U = ref.unitary_links(rng, dims)
    links = bc.gauge_field(ctx).upload(U)
    src = bc.block_fermion_field(ctx, m).setPointSources([[3, 4, 5, t0]] * 3, [0, 1, 2])
    start = src.download()
    got = bc.smear(src, links, 3, 0.1, 4).download()
    want = ref.smear(U, dims, start, 3, 0.1, 4)
    coords = ref.coordinates(dims)
    off = coords[:, 3] != t0
    assert np.array_equal(got[off], np.zeros_like(got[off]))
    assert rel_err(got, want) <= TOL_SMEAR
    # the spatial profile: |psi|^2 summed over colour and column as a function of the distance from the source
    r2 = (np.minimum((coords[:, :3] - [3, 4, 5]) % 8, ([3, 4, 5] - coords[:, :3]) % 8) ** 2).sum(axis=1)
    prof = lambda a: np.bincount(r2, weights=(np.abs(a) ** 2).sum(axis=(1, 2)))  # noqa: E731
    assert np.max(np.abs(prof(got) - prof(want))) <= TOL_SMEAR * prof(want).sum()
    assert prof(got)[1:].sum() > 0  # it did spread


def test_second_call_returns_the_same_bits(bc):
    for dims, m in (([4, 2, 4, 2], 5), ([16, 4, 4, 4], 16)):
        ctx, U, links, psi, f = _case(bc, dims, m)
        c0, fw, bw = _coefficients(np.random.default_rng(19), 4)
        a, b = bc.block_fermion_field(ctx, m), bc.block_fermion_field(ctx, m)
        bc.shift_sum(a, f, links, c0, fw, bw, True)
        bc.shift_sum(b, f, links, c0, fw, bw, True)
        assert np.array_equal(_bits(a.download()), _bits(b.download()))
        assert np.array_equal(_bits(f.download()), _bits(psi))


def test_invalid_calls_leave_out_alone(bc):
    """Every INVALID / UNSUPPORTED return, with poisoned outputs left as they were.  Every field and link container passed
    is bound to a name that outlives the calls: a handle read off a temporary would be destroyed before the library sees it."""
    dims, m = [4, 2, 4, 2], 5
    ctx, U, links, psi, f = _case(bc, dims, m)
    lib = ctx.lib
    poison = np.full((ctx.V, m, 3), 7.0 - 3.0j)
    half_poison = poison[: ctx.V // 2]
    out = bc.block_fermion_field(ctx, m, host=poison)
    dp = ctypes.POINTER(ctypes.c_double)

    def vec(*v):
        a = np.ascontiguousarray(v, dtype=np.complex128).view(np.float64)
        return a, a.ctypes.data_as(dp)

    zero, one, hops = vec(0.0), vec(1.0), vec(1.0, 2.0, 3.0, 4.0)
    nan_c, inf_h = vec(complex(np.nan, 0.0)), vec(1.0, complex(0.0, np.inf), 0.0, 0.0)
    other = bc.Context(dims)
    half0, half1 = bc.block_fermion_field(ctx, m, parity=0), bc.block_fermion_field(ctx, m, parity=1, host=half_poison)
    half1_too = bc.block_fermion_field(ctx, m, parity=1)
    narrow = bc.block_fermion_field(ctx, 4)
    other_in = bc.block_fermion_field(other, m, host=psi)
    other_out = bc.block_fermion_field(other, m, host=poison)
    other_links = bc.gauge_field(other).upload(U)
    work = bc.block_fermion_field(ctx, m)
    poisoned = ((out, poison), (half1, half_poison), (other_out, poison))

    def untouched(what):
        for field, held in poisoned:
            assert np.array_equal(_bits(field.download()), _bits(held)), what

    cases = {
        "null g": (ctx.h, None, out.h, f.h, one[1], hops[1], hops[1], 0),
        "null out": (ctx.h, links.h, None, f.h, one[1], hops[1], hops[1], 0),
        "null in": (ctx.h, links.h, out.h, None, one[1], hops[1], hops[1], 0),
        "null c0": (ctx.h, links.h, out.h, f.h, None, hops[1], hops[1], 0),
        "out is in": (ctx.h, links.h, out.h, out.h, one[1], hops[1], hops[1], 0),
        "width": (ctx.h, links.h, out.h, narrow.h, one[1], hops[1], hops[1], 0),
        "context of in": (ctx.h, links.h, out.h, other_in.h, one[1], hops[1], hops[1], 0),
        "context of out": (ctx.h, links.h, other_out.h, f.h, one[1], hops[1], hops[1], 0),
        "context of g": (ctx.h, other_links.h, out.h, f.h, one[1], hops[1], hops[1], 0),
        "all of another context": (ctx.h, other_links.h, other_out.h, other_in.h, one[1], hops[1], hops[1], 0),
        "full in, half out": (ctx.h, links.h, half1.h, f.h, zero[1], hops[1], hops[1], 0),
        "half in, full out": (ctx.h, links.h, out.h, half0.h, zero[1], hops[1], hops[1], 0),
        "same parity": (ctx.h, links.h, half1.h, half1_too.h, zero[1], hops[1], hops[1], 0),
        "c0 with halves": (ctx.h, links.h, half1.h, half0.h, one[1], hops[1], hops[1], 0),
        "nan c0": (ctx.h, links.h, out.h, f.h, nan_c[1], hops[1], hops[1], 0),
        "inf fwd": (ctx.h, links.h, out.h, f.h, one[1], inf_h[1], hops[1], 0),
        "inf bwd": (ctx.h, links.h, out.h, f.h, one[1], None, inf_h[1], 0),
    }
    for what, args in cases.items():
        assert lib.bcg_dirac_shift_sum(*args) == INVALID, what
        untouched(what)
    # smearing
    smear_cases = {
        "null g": ((ctx.h, None, out.h, work.h, 3, 0.1, 2), INVALID),
        "null f": ((ctx.h, links.h, None, work.h, 3, 0.1, 2), INVALID),
        "dir -2": ((ctx.h, links.h, out.h, work.h, -2, 0.1, 2), INVALID),
        "dir ndim": ((ctx.h, links.h, out.h, work.h, 4, 0.1, 2), INVALID),
        "n_iter -1": ((ctx.h, links.h, out.h, work.h, 3, 0.1, -1), INVALID),
        "nan kappa": ((ctx.h, links.h, out.h, work.h, 3, float("nan"), 2), INVALID),
        "inf kappa": ((ctx.h, links.h, out.h, work.h, 3, float("inf"), 2), INVALID),
        "work is f": ((ctx.h, links.h, out.h, out.h, 3, 0.1, 2), INVALID),
        "work width": ((ctx.h, links.h, out.h, narrow.h, 3, 0.1, 2), INVALID),
        "work parity": ((ctx.h, links.h, out.h, half0.h, 3, 0.1, 2), INVALID),
        "context of work": ((ctx.h, links.h, out.h, other_in.h, 3, 0.1, 2), INVALID),
        "context of f": ((ctx.h, links.h, other_out.h, work.h, 3, 0.1, 2), INVALID),
        "context of f, no work": ((ctx.h, links.h, other_out.h, None, 3, 0.1, 2), INVALID),
        "context of g": ((ctx.h, other_links.h, out.h, work.h, 3, 0.1, 2), INVALID),
        "half field": ((ctx.h, links.h, half1.h, None, 3, 0.1, 2), UNSUPPORTED),
        "half field and work": ((ctx.h, links.h, half1.h, half1_too.h, 3, 0.1, 2), UNSUPPORTED),
    }
    for what, (args, code) in smear_cases.items():
        assert lib.bcg_covariant_smear(*args) == code, what
        untouched(what)
    assert np.array_equal(_bits(other_in.download()), _bits(psi))
    with pytest.raises(bc.BlockCGError):
        bc.laplacian(out, out, links)
    # and the good calls fill it
    assert lib.bcg_dirac_shift_sum(ctx.h, links.h, out.h, f.h, one[1], hops[1], None, 1) == 0
    assert not np.array_equal(_bits(out.download()), _bits(poison))
    assert lib.bcg_covariant_smear(ctx.h, links.h, out.h, None, -1, 0.1, 1) == 0


def test_divided_lattice_without_a_comm(bc):
    """One rank of a (2,1,1,1) grid with no bcg_comm attached: both calls return BCG_ERR_COMM before anything is launched or
    exchanged, full and half fields, and the poisoned outputs stay as they were."""
    dims, m = [4, 2, 4, 2], 5
    ctx = bc.Context(dims, grid=[2, 1, 1, 1], coords=[0, 0, 0, 0])
    assert ctx.V == int(np.prod(dims)) // 2
    links = bc.gauge_field(ctx).setRandom(3)
    poison = np.full((ctx.V, m, 3), 7.0 - 3.0j)
    inp = bc.block_fermion_field(ctx, m).setGaussian(4)
    out = bc.block_fermion_field(ctx, m, host=poison)
    work = bc.block_fermion_field(ctx, m, host=poison)
    half_in = bc.block_fermion_field(ctx, m, parity=0).setGaussian(5)
    half_out = bc.block_fermion_field(ctx, m, parity=1, host=poison[: ctx.V // 2])
    c = np.array([1.0, 0.0, 0.0, 0.0])  # c0 = 1, then c0 = 0 for the half fields
    hops = np.ones(4, dtype=np.complex128).view(np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    c1, c0, hp = c[:2].ctypes.data_as(dp), c[2:].ctypes.data_as(dp), hops.ctypes.data_as(dp)
    lib = ctx.lib
    assert lib.bcg_dirac_shift_sum(ctx.h, links.h, out.h, inp.h, c1, hp, hp, 1) == COMM
    assert lib.bcg_dirac_shift_sum(ctx.h, links.h, out.h, inp.h, c1, None, None, 0) == COMM  # c0 alone: the same call everywhere
    assert lib.bcg_dirac_shift_sum(ctx.h, links.h, half_out.h, half_in.h, c0, hp, hp, 1) == COMM
    assert lib.bcg_covariant_smear(ctx.h, links.h, out.h, work.h, 3, 0.1, 2) == COMM
    assert lib.bcg_covariant_smear(ctx.h, links.h, out.h, None, -1, 0.1, 1) == COMM
    assert lib.bcg_covariant_smear(ctx.h, links.h, out.h, work.h, 3, 0.1, 0) == COMM  # checked before n_iter = 0 returns
    assert np.array_equal(_bits(out.download()), _bits(poison))
    assert np.array_equal(_bits(work.download()), _bits(poison))
    assert np.array_equal(_bits(half_out.download()), _bits(poison[: ctx.V // 2]))
    with pytest.raises(bc.BlockCGError) as e:
        bc.laplacian(out, inp, links)
    assert e.value.code == COMM
    # argument errors come first, as on every rank of the grid
    assert lib.bcg_dirac_shift_sum(ctx.h, links.h, out.h, out.h, c1, hp, hp, 1) == INVALID
    assert lib.bcg_covariant_smear(ctx.h, links.h, out.h, out.h, 3, 0.1, 2) == INVALID


def test_smeared_correlator_example(bc):
    """examples/smeared_correlator.cpp, built by the recipe of tests/test_cpp_dropin.py and run on 4^4: its 3 x 3 correlator
    matrices are those of the same smearing, solve and slice_gram done here."""
    out = os.path.join(ROOT, "examples", "_build")
    libdir = os.path.join(ROOT, "blockcg_amd", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "smeared_correlator")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "blockcg_amd", "include"),
                        os.path.join(ROOT, "examples", "smeared_correlator.cpp"), "-o", exe, "-L", libdir, "-lblockcg_hip",
                        f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "4", "4", "4", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SMEARED_CORRELATOR_OK" in r.stdout, r.stdout + r.stderr
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.splitlines() if line and line[0] not in "#S"])
    assert rows.shape == (4, 1 + 18)
    ctx = bc.Context([4, 4, 4, 4])
    D = bc.dirac_op(ctx, 0.5, seed=7)
    B = bc.block_fermion_field(ctx, 3).setPointSources([[0, 0, 0, 0]] * 3, [0, 1, 2])
    bc.smear(B, D, 3, 0.1, 4)
    X = [bc.block_fermion_field(ctx, 3)]
    bc.SBCGrQ(X, B, D, [0.0], 1e-12, 1e-12)
    bc.smear(X[0], D, 3, 0.1, 4)
    want = X[0].slice_gram(X[0], 3)  # [t, i, j]
    got = (rows[:, 1::2] + 1j * rows[:, 2::2]).reshape(4, 3, 3)
    assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))
