"""A basis put onto slices (include/blockcg_hip.h: bcg_basis_slice_axpy) against its numpy restatement
(tests/basis_slice_axpy_ref.py): every direction, width class of either form and parity, beta 0 / 1 / another value, all slices /
one / two in descending order, momenta that are negative and beyond the extents; the MFMA form against the generic one; the
same bits on a second call; the slices that are not listed (bit-identical at beta = 1, exact zeros over a NaN start at
beta = 0); the adjoint identity with basis_slice_dot on the device; against basis_axpy and copy_columns; the per-slice
projector; shapes where the walk can go wrong; every width; the launch counts; the error returns; examples/distillation.cpp.

Tolerance: TOL_KERNEL by conftest.rel_err (relative Frobenius error), exactly as tests/test_basis.py applies it to basis_axpy;
the adjoint identity to EPS_DOT = 1e-13 of |y||b|, the bound of tests/test_basis_slice.py for the dot on the same lattice.

The launches, as the launch counts below use them (blockcg_amd/csrc/kernels_basis_slice_axpy.hpp): the groups are those of
basis_axpy -- consecutive fields of one form, MFMA (m and widths in {16, 32}) up to 4 blocks of 16 columns at m = 16 and 3 at
m = 32, generic up to 32 columns and 8 fields -- one launch per group over the listed local slices, and one streaming launch
for the other slices where beta != 1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import basis_slice_axpy_ref as ref
from conftest import ROOT, TOL_KERNEL, rel_err
from test_basis_slice import MOMENTA, PAIRS

pytestmark = pytest.mark.gpu

EPS_DOT = 1e-13
INVALID = 1
BETAS = (0.0, 1.0, -0.5)


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


_contexts = {}


def _ctx(bc, dims):
    key = tuple(dims)
    if key not in _contexts:
        _contexts[key] = bc.Context(list(dims))
        _contexts[key].profiling(True)
    return _contexts[key]


def _momenta(direction, ndim=4):
    """None, then MOMENTA and their negatives with the component along `direction` and beyond ndim set to 0."""
    out = [None]
    for sign in (1, -1):
        for n in MOMENTA:
            q = [sign * v if mu < ndim else 0 for mu, v in enumerate(n)]
            q[direction] = 0
            out.append(q)
    return out


def _slice_sets(L):
    """all slices / one slice / two non-adjacent slices in descending order (L = 2: the two there are)"""
    return (None, [L - 1], [L - 1, L - 3] if L >= 4 else [L - 1, 0])


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _operands(bc, ctx, widths, m, parity, seed=500):
    V = [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(seed + k) for k, w in enumerate(widths)]
    y = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(seed + 50)
    return V, y


def _coefficients(rng, S, K, m):
    return rng.standard_normal((S, K, m)) + 1j * rng.standard_normal((S, K, m))


def _forms(ctx):
    p = ctx.profile()
    return p.get("basis_slice_axpy_form_mfma", {}).get("count", 0), p.get("basis_slice_axpy_form_generic", {}).get("count", 0)


def _one(bc, ctx, y, V, yh, Vh, C, dims, direction, slices, mom, beta, parity, worst, what, both_forms=True):
    """One call in both forms against the restatement and each other, twice from the same start; returns the result."""
    want = ref.basis_slice_axpy(yh, Vh, C, dims, direction, slices, mom, beta, parity)
    L = dims[direction]
    listed = np.isin(ref.slice_of_sites(dims, direction, parity), range(L) if slices is None else slices)
    start = np.full_like(yh, np.nan) if beta == 0.0 else yh
    outs = {}
    for generic in ((False, True) if both_forms else (False,)):
        ctx.force_generic(generic)
        try:
            y.upload(start)
            bc.basis_slice_axpy(y, V, C, direction, slices, mom, beta)
            out = y.download()
            y.upload(start)
            bc.basis_slice_axpy(y, V, C, direction, slices, mom, beta)
            again = y.download()
        finally:
            ctx.force_generic(False)
        e = rel_err(out, want)
        worst[0] = max(worst[0], e)
        assert e <= TOL_KERNEL, (what, generic, e)
        assert np.array_equal(_bits(again), _bits(out)), (what, generic)  # the same bits on a second call
        if beta == 1.0:  # the slices that are not listed keep their bits
            assert np.array_equal(_bits(out[~listed]), _bits(yh[~listed])), (what, generic)
        if beta == 0.0:  # nothing of the NaN start survives; exact zeros off the listed slices
            assert not np.isnan(out).any(), (what, generic)
            assert np.array_equal(_bits(out[~listed]), _bits(np.zeros_like(out[~listed]))), (what, generic)
        outs[generic] = out
    if both_forms:
        assert rel_err(outs[False], outs[True]) <= TOL_KERNEL, what
    return outs[False]


def _sweep(bc, ctx, dims, widths, m, parity, worst, directions=None, momenta_of=_momenta, betas=BETAS, slice_sets=_slice_sets):
    V, y = _operands(bc, ctx, widths, m, parity)
    Vh, yh = [v.download() for v in V], y.download()
    norm_bits = [_bits(v.hermitian_dot(v)).copy() for v in V]
    rng = np.random.default_rng(17)
    K = sum(widths)
    for direction in (range(len(dims)) if directions is None else directions):
        L = dims[direction]
        for slices in slice_sets(L):
            C = _coefficients(rng, L if slices is None else len(slices), K, m)
            for mom in momenta_of(direction):
                for beta in betas:
                    what = (tuple(dims), tuple(widths), m, parity, direction, slices, mom, beta)
                    _one(bc, ctx, y, V, yh, Vh, C, dims, direction, slices, mom, beta, parity, worst, what)
    for v, bits in zip(V, norm_bits):  # V is untouched
        assert np.array_equal(_bits(v.hermitian_dot(v)), bits)


@pytest.mark.parametrize("parity", [None, 0, 1], ids=["full", "even", "odd"])
@pytest.mark.parametrize("widths,m", PAIRS, ids=[f"{'+'.join(map(str, w))}x{m}" for w, m in PAIRS])
def test_basis_slice_axpy_main_sweep(bc, widths, m, parity):
    dims = [4, 2, 4, 2]
    worst = [0.0]
    _sweep(bc, _ctx(bc, dims), dims, widths, m, parity, worst)
    print(f"largest basis-slice-axpy error on {dims}, V = {widths}, m = {m}, parity {parity}: {worst[0]:.3e}")


@pytest.mark.parametrize("widths,m", PAIRS, ids=[f"{'+'.join(map(str, w))}x{m}" for w, m in PAIRS])
def test_adjoint_of_basis_slice_dot(bc, widths, m):
    """sum_j hermitian_dot(y, b)[j, j] with y = basis_slice_axpy(beta = 0, C, p) against sum_t tr(C_t^dagger tau_p(t)), tau_p from
    basis_slice_dot(V, b, dir, [p]), relative to |y||b|."""
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    rng = np.random.default_rng(19)
    K = sum(widths)
    worst = 0.0
    for parity in (None, 0, 1):
        V, b = _operands(bc, ctx, widths, m, parity, seed=520)
        y = bc.block_fermion_field(ctx, m, parity=parity)
        nb = np.linalg.norm(b.download())
        for direction in range(4):
            C = _coefficients(rng, dims[direction], K, m)
            for p in (None, _momenta(direction)[2], _momenta(direction)[8]):
                y.upload(np.full((y.V, m, 3), np.nan))
                bc.basis_slice_axpy(y, V, C, direction, None, p, 0.0)
                lhs = np.trace(y.hermitian_dot(b))
                tau = bc.basis_slice_dot(V, b, direction) if p is None else bc.basis_slice_dot(V, b, direction, [p])[0]
                rhs = np.vdot(C, tau)
                err = abs(lhs - rhs) / (np.linalg.norm(y.download()) * nb)
                worst = max(worst, err)
                assert err <= EPS_DOT, (widths, m, parity, direction, p, err)
    print(f"adjoint identity, V = {widths}, m = {m}: {worst:.3e} of |y||b|")


@pytest.mark.parametrize("widths,m", [([16, 32, 16], 16), ([1, 7, 12], 5), ([32], 32)], ids=["mfma16", "generic", "mfma32"])
def test_all_slices_with_one_matrix_is_basis_axpy(bc, widths, m):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    rng = np.random.default_rng(23)
    for parity in (None, 1):
        V, y = _operands(bc, ctx, widths, m, parity, seed=540)
        yh = y.download()
        z = bc.block_fermion_field(ctx, m, parity=parity)
        C = _coefficients(rng, 1, sum(widths), m)[0]
        for direction in range(4):
            for beta in BETAS:
                z.upload(yh)
                bc.basis_axpy(z, V, C, beta)
                y.upload(yh)
                bc.basis_slice_axpy(y, V, np.repeat(C[None], dims[direction], axis=0), direction, None, None, beta)
                assert rel_err(y.download(), z.download()) <= TOL_KERNEL, (widths, m, parity, direction, beta)


@pytest.mark.parametrize("w,m,first", [(32, 16, 16), (12, 5, 3), (16, 16, 0)])
def test_a_column_selection_is_a_masked_copy_columns(bc, w, m, first):
    """One slice, beta = 0, C the selection of columns first .. first + m - 1 of a: copy_columns, masked to the slice on the host."""
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    C = np.zeros((1, w, m), dtype=np.complex128)
    C[0, first + np.arange(m), np.arange(m)] = 1.0
    for parity in (None, 0):
        (a,), y = _operands(bc, ctx, [w], m, parity, seed=560)
        z = bc.block_fermion_field(ctx, m, parity=parity)
        z.copy_columns(0, a, first, m)
        for direction in range(4):
            t0 = dims[direction] - 1
            want = z.download()
            want[ref.slice_of_sites(dims, direction, parity) != t0] = 0.0
            y.upload(np.full((y.V, m, 3), np.nan))
            bc.basis_slice_axpy(y, [a], C, direction, [t0], None, 0.0)
            assert rel_err(y.download(), want) <= TOL_KERNEL, (w, m, first, parity, direction)


def _orthonormal_per_slice(rng, dims, direction, K, parity):
    """[sites held, K, 3] with V(t)^dagger V(t) = 1 on every slice: QR of Gaussian noise slice by slice"""
    t = ref.slice_of_sites(dims, direction, parity)
    W = np.zeros((len(t), K, 3), dtype=np.complex128)
    for s in range(dims[direction]):
        sel = t == s
        n = int(sel.sum())
        assert 3 * n >= K
        q, _ = np.linalg.qr(rng.standard_normal((3 * n, K)) + 1j * rng.standard_normal((3 * n, K)))
        W[sel] = q.reshape(n, 3, K).transpose(0, 2, 1)
    return W


@pytest.mark.parametrize("m", [16, 5])
def test_projector_is_idempotent(bc, m):
    """V orthonormal on every slice of direction 3 (K = 16; a half field's slice has 16 sites, 48 rows), C = basis_slice_dot(V, b):
    the call is V(t) V(t)^dagger b, and applying it twice equals applying it once."""
    dims, K = [4, 2, 4, 2], 16
    ctx = _ctx(bc, dims)
    rng = np.random.default_rng(29)
    for parity in (None, 0, 1):
        V = [bc.block_fermion_field(ctx, K, parity=parity).upload(_orthonormal_per_slice(rng, dims, 3, K, parity))]
        b = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(7)
        once = bc.block_fermion_field(ctx, m, parity=parity)
        twice = bc.block_fermion_field(ctx, m, parity=parity)
        bc.basis_slice_axpy(once, V, bc.basis_slice_dot(V, b, 3), 3, None, None, 0.0)
        bc.basis_slice_axpy(twice, V, bc.basis_slice_dot(V, once, 3), 3, None, None, 0.0)
        e = rel_err(twice.download(), once.download())
        print(f"projector, m = {m}, parity {parity}: {e:.3e}")
        assert e <= TOL_KERNEL, (m, parity, e)
        assert np.linalg.norm(once.download()) > 0.1 * np.linalg.norm(b.download())  # 16 of a slice's 96 (48) dimensions


@pytest.mark.parametrize("widths,m", [([16], 16), ([1, 7], 5)], ids=["mfma", "generic"])
def test_basis_slice_axpy_in_one_dimension(bc, widths, m):
    """[96]: a slice is one site, 3 rows, less than one step of 16 rows of the MFMA kernel; a half field holds every other slice,
    so a listed slice may hold no site at all."""
    dims = [96]
    worst = [0.0]
    for parity in (None, 0, 1):
        _sweep(bc, _ctx(bc, dims), dims, widths, m, parity, worst, momenta_of=lambda d: [None],
               slice_sets=lambda L: (None, [L - 1], [L - 2, 5, 40]))
    print(f"largest basis-slice-axpy error on {dims}, V = {widths}, m = {m}: {worst[0]:.3e}")


def test_basis_slice_axpy_at_ragged_shapes(bc):
    """Row counts that steps of 16 rows do not divide, odd extents; one non-zero momentum where the lattice has a second
    direction."""
    worst = [0.0]
    for dims, widths, m in (([5, 3, 2], [16, 32], 16), ([7, 5, 3, 3], [32, 3], 12), ([37], [5], 5)):
        nd = len(dims)

        def mom(direction, nd=nd):
            if nd == 1:
                return [None]
            q = [2, -1, 1, 4][:nd] + [0] * (4 - nd)
            q[direction] = 0
            return [None, q]

        _sweep(bc, _ctx(bc, dims), dims, widths, m, None, worst, momenta_of=mom)
    print(f"largest basis-slice-axpy error at ragged shapes: {worst[0]:.3e}")


def test_basis_slice_axpy_with_several_blocks_per_slice(bc):
    """[16,16,16,4], V = 2 x 32, m = 16.  Direction 3: a slice has 12288 rows, 192 blocks of 64 rows when all 4 slices are listed
    (2048 / 4 = 512 allowed, rows / 64 = 192 the most) and as many for two; direction 0: 3072 rows, 48 blocks per slice for 16
    slices and for two.  The other slices at beta = -0.5 take the streaming launch on as many blocks.  Against numpy on the
    whole field."""
    dims = [16, 16, 16, 4]
    ctx = _ctx(bc, dims)
    V, y = _operands(bc, ctx, [32, 32], 16, None, seed=580)
    Vh, yh = [v.download() for v in V], y.download()
    rng = np.random.default_rng(31)
    worst = [0.0]
    for direction, mom in ((3, [1, -2, 17, 0]), (0, [0, 3, 17, -2])):
        L = dims[direction]
        for slices, beta in ((None, 1.0), ([L - 1, 1], -0.5), ([2], 0.0)):
            C = _coefficients(rng, L if slices is None else len(slices), 64, 16)
            _one(bc, ctx, y, V, yh, Vh, C, dims, direction, slices, mom, beta, None, worst, (dims, direction, slices, beta),
                 both_forms=slices is not None)
    print(f"largest basis-slice-axpy error on {dims}: {worst[0]:.3e}")


def test_more_slices_than_blocks_aimed_at(bc):
    """[2048] along direction 0 with all slices listed: the plan aims at 2048 blocks but gives every slice one block at the
    least, so the grid is 2048 blocks of one 3-row slice each (a half field: 2048 blocks, every other one without a site) and
    every slice is covered."""
    dims = [2048]
    ctx = _ctx(bc, dims)
    rng = np.random.default_rng(37)
    worst = [0.0]
    for widths, m, parity in (([32, 32], 16, None), ([16], 16, 1), ([5, 3], 5, None)):
        V, y = _operands(bc, ctx, widths, m, parity, seed=600)
        Vh, yh = [v.download() for v in V], y.download()
        C = _coefficients(rng, 2048, sum(widths), m)
        for beta in (0.0, -0.5):
            _one(bc, ctx, y, V, yh, Vh, C, dims, 0, None, None, beta, parity, worst, (dims, widths, m, parity, beta))
    print(f"largest basis-slice-axpy error on {dims}: {worst[0]:.3e}")


@pytest.mark.parametrize("w", range(1, 33))
def test_every_width(bc, w):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    rng = np.random.default_rng(41)
    mom = [1, -1, 3, 0]
    for widths, m in (([w], 5), ([w], 16), ([16, 5], w)):
        V, y = _operands(bc, ctx, widths, m, None, seed=620)
        Vh, yh = [v.download() for v in V], y.download()
        C = _coefficients(rng, 1, sum(widths), m)
        _one(bc, ctx, y, V, yh, Vh, C, dims, 3, [1], mom, -0.5, None, [0.0], (widths, m), both_forms=False)


# (widths of V, m, bcg_force_generic, (MFMA launches, generic launches)), by the group bounds in the module docstring
PLAN = (
    ([32] * 5, 16, False, (3, 0)),       # 10 blocks in whole fields: 32 32 | 32 32 | 32, the groups of basis_axpy
    ([16, 5], 16, False, (1, 1)),        # the forms alternate: 16 | 5
    ([32, 3], 12, False, (0, 2)),        # generic: 32 columns are a full group, 32 | 3
    ([32, 32], 16, False, (1, 0)),       # 4 blocks, one group
    ([32, 16], 32, False, (1, 0)),       # m = 32: 3 blocks, one group
    ([32, 32], 32, False, (2, 0)),       # m = 32: 4 blocks are one too many, 32 | 32
    ([1, 7, 12], 5, False, (0, 1)),      # 20 generic columns in three fields: one group
    ([32, 32], 16, True, (0, 2)),        # bcg_force_generic: 32 | 32
)


@pytest.mark.parametrize("widths,m,generic,forms", PLAN)
def test_launch_counts_and_bytes(bc, widths, m, generic, forms):
    """The launch counts of either form from the profile, for all slices and for one; with one slice listed at beta = 1 the
    profiled bytes of basis_slice_axpy are 1 / L_dir of the all-slices call, and nothing else is launched."""
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    V, y = _operands(bc, ctx, widths, m, None, seed=640)
    rng = np.random.default_rng(43)
    K = sum(widths)
    ctx.force_generic(generic)
    try:
        for direction in (0, 3):
            L = dims[direction]
            ctx.profile_reset()
            bc.basis_slice_axpy(y, V, _coefficients(rng, L, K, m), direction, None, None, 1.0)
            assert _forms(ctx) == forms
            p_all = ctx.profile()
            ctx.profile_reset()
            bc.basis_slice_axpy(y, V, _coefficients(rng, 1, K, m), direction, [L - 1], None, 1.0)
            assert _forms(ctx) == forms
            p_one = ctx.profile()
            assert p_one["basis_slice_axpy"]["bytes"] * L == p_all["basis_slice_axpy"]["bytes"] > 0
            assert "basis_slice_scale" not in p_one  # keys without a launch are not reported
            ctx.profile_reset()
            bc.basis_slice_axpy(y, V, _coefficients(rng, 1, K, m), direction, [L - 1], None, 0.5)
            assert _forms(ctx) == forms and ctx.profile()["basis_slice_scale"]["count"] == 1
    finally:
        ctx.force_generic(False)


def test_invalid_calls_leave_y_alone(bc):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    lib = ctx.lib
    v16 = bc.block_fermion_field(ctx, 16).setGaussian(1)
    v5 = bc.block_fermion_field(ctx, 5).setGaussian(2)
    y = bc.block_fermion_field(ctx, 8).setGaussian(3)
    half = bc.block_fermion_field(ctx, 8, parity=0).setGaussian(5)
    vhalf = bc.block_fermion_field(ctx, 16, parity=1).setGaussian(6)
    foreign = bc.block_fermion_field(_ctx(bc, [37]), 16).setGaussian(7)
    before, half_before = y.download(), half.download()
    C = np.ones((4, 8, 21), dtype=np.complex128)
    cp = C.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = ctypes.POINTER(ctypes.c_int)

    def handles(*fields):
        return (ctypes.c_void_p * max(1, len(fields)))(*[f.h if f is not None else None for f in fields])

    def ints(*values):
        arr = np.ascontiguousarray(values, dtype=np.intc)
        return arr, arr.ctypes.data_as(ip)

    good = handles(v16, v5)
    keep = [ints(1), ints(0, 1), ints(2), ints(0, 0), ints(1, 0, 0, 0), ints(0, 0, 0, 1), ints(-1), ints(0, 3, 0)]
    one, two, past, twice, mom_ok, mom_dir, negative, thrice = [k[1] for k in keep]
    cases = {
        "nv 0": (y.h, good, 0, 3, 1, one, cp, None, 1.0),
        "nv -1": (y.h, good, -1, 3, 1, one, cp, None, 1.0),
        "null V": (y.h, None, 2, 3, 1, one, cp, None, 1.0),
        "null field": (y.h, handles(v16, None), 2, 3, 1, one, cp, None, 1.0),
        "null C": (y.h, good, 2, 3, 1, one, None, None, 1.0),
        "context": (y.h, handles(v16, foreign), 2, 3, 1, one, cp, None, 1.0),
        "parity of a V": (y.h, handles(v16, vhalf), 2, 3, 1, one, cp, None, 1.0),
        "parity of y": (half.h, good, 2, 3, 1, one, cp, None, 1.0),
        "y among V": (v5.h, good, 2, 3, 1, one, cp, None, 1.0),
        "beta nan": (y.h, good, 2, 3, 1, one, cp, None, float("nan")),
        "beta inf": (y.h, good, 2, 3, 1, one, cp, None, float("inf")),
        "dir -1": (y.h, good, 2, -1, 0, None, cp, None, 1.0),
        "dir ndim": (y.h, good, 2, 4, 0, None, cp, None, 1.0),
        "n_slices -1": (y.h, good, 2, 3, -1, one, cp, None, 1.0),
        "null slices": (y.h, good, 2, 3, 1, None, cp, None, 1.0),
        "slice L": (y.h, good, 2, 3, 1, past, cp, None, 1.0),
        "slice -1": (y.h, good, 2, 3, 1, negative, cp, None, 1.0),
        "slice twice": (y.h, good, 2, 3, 2, twice, cp, None, 1.0),
        "slice twice, apart": (y.h, good, 2, 0, 3, thrice, cp, None, 1.0),
        "momentum along dir": (y.h, good, 2, 3, 2, two, cp, mom_dir, 1.0),
    }
    v5_before = v5.download()
    for what, args in cases.items():
        assert lib.bcg_basis_slice_axpy(*args) == INVALID, what
        assert np.array_equal(_bits(y.download()), _bits(before)), what
        assert np.array_equal(_bits(half.download()), _bits(half_before)), what
        assert np.array_equal(_bits(v5.download()), _bits(v5_before)), what
    assert lib.bcg_basis_slice_axpy(None, good, 2, 3, 1, one, cp, None, 1.0) == INVALID  # NULL y
    # a 3-D lattice: the fourth component must be 0
    ctx3 = _ctx(bc, [4, 2, 2])
    g, y3 = bc.block_fermion_field(ctx3, 5).setGaussian(2), bc.block_fermion_field(ctx3, 5).setGaussian(3)
    y3_before = y3.download()
    assert ctx3.lib.bcg_basis_slice_axpy(y3.h, handles(g), 1, 1, 1, one, cp, mom_dir, 1.0) == INVALID
    assert np.array_equal(_bits(y3.download()), _bits(y3_before))
    with pytest.raises(bc.BlockCGError):
        bc.basis_slice_axpy(y, [v16, v5], np.ones((2, 21, 8)), 4)
    with pytest.raises(bc.BlockCGError):
        bc.basis_slice_axpy(y, [v16, v5], np.ones((1, 21, 8)), 3, [2])
    # and the good call changes y, on the listed slices only
    assert lib.bcg_basis_slice_axpy(y.h, good, 2, 3, 2, two, cp, mom_ok, 1.0) == 0
    assert not np.array_equal(_bits(y.download()), _bits(before))


def test_distillation_example(bc):
    """examples/distillation.cpp on 4^4: a basis orthonormal on every slice, a source on one slice, the solve, the perambulator
    and the smeared sink; its self-check is the source norm (= the number of source columns), the true residual of the solve
    and the idempotent projector."""
    from test_cpp_dropin import _compile
    exe = _compile(os.path.join(ROOT, "examples", "distillation.cpp"), "distillation")
    r = subprocess.run([exe, "4", "4", "4", "4"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "DISTILLATION_OK" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
