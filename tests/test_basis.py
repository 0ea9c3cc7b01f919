"""Products between fields of unequal width (include/blockcg_hip.h: bcg_basis_dot, bcg_basis_axpy, bcg_field_copy_columns)
against their numpy restatement (tests/basis_ref.py), and the deflated solve composed from them.

Tolerances: EPS_DOT = 1e-13 per entry of the dot relative to sqrt(|V_i|^2 |b_j|^2) (the bound of tests/test_slice_gram.py
for sums of this length and shorter ones), TOL_KERNEL for the update, TOL_SOLUTION for the solutions of the deflated solve.
Shapes: rows that are no multiple of 16 and 3-row sites ([5,3,2], [37]), both half parities ([4,2,4,2]), every width class
of either form, both forms in one call, more than one group per call and more than one block per launch; the host's group
walk with the launch counts of the dot and of the update asserted separately (GROUP_WALK); blockcg/basis.hpp run on the device
(tests/cpp/basis_run_probe.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import basis_ref as ref
from conftest import ROOT, TOL_KERNEL, TOL_SOLUTION, rel_err

pytestmark = pytest.mark.gpu

EPS_DOT = 1e-13
INVALID = 1
LATTICES = ([5, 3, 2], [37], [4, 2, 4, 2])
# (widths of V, m, launches of the MFMA form, launches of the generic form) -- the same for the dot and for the update
GENERIC = (([5], 1, 0, 1), ([1, 7, 12], 5, 0, 1), ([8, 8], 8, 0, 1), ([32, 3], 12, 0, 2))
MFMA = (([16], 16, 1, 0), ([32], 16, 1, 0), ([16], 32, 1, 0), ([32], 32, 1, 0), ([16, 32, 16], 16, 1, 0))
MIXED = (([16, 5], 16, 1, 1),)
# The group walk (capi_basis.hip: basis_groups): (widths of V, m, (MFMA, generic) launches of the dot, the same of the update).
# The counts follow from the bounds of kernels_basis.hpp: a generic group holds at most 32 columns and 8 fields; an MFMA group
# at most 4 blocks of 16 columns at m = 16, and at m = 32 2 blocks for the dot and 3 for the update, never more fields than
# blocks; a group ends where the form changes.  The first three rows are the only launches of the update on three blocks at
# m = 32, the first five the only ones of the m = 32 dot (and of its fold) on a second group.
GROUP_WALK = (
    ([16, 16, 16], 32, (2, 0), (1, 0)),        # dot 16 16 | 16; update 16 16 16
    ([32, 16], 32, (2, 0), (1, 0)),            # dot 32 | 16; update 32 16
    ([16, 32], 32, (2, 0), (1, 0)),            # dot 16 | 32; update 16 32
    ([32, 32, 16, 16], 32, (3, 0), (3, 0)),    # dot 32 | 32 | 16 16; update 32 | 32 16 | 16
    ([16, 7, 32], 32, (2, 1), (2, 1)),         # 16 | 7 | 32: the forms alternate
    ([16] * 5, 16, (2, 0), (2, 0)),            # 16 16 16 16 | 16
    ([16, 5, 32, 3, 16], 16, (3, 2), (3, 2)),  # the forms alternate four times
    ([1] * 9, 3, (0, 2), (0, 2)),              # the generic bound of 8 fields, 8 columns in all
    ([4] * 9, 12, (0, 2), (0, 2)),             # 8 fields and 32 columns at once
    ([12, 12, 12], 5, (0, 2), (0, 2)),         # 12 12 | 12: the column bound before the field bound
)


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


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _operands(bc, ctx, widths, m, parity, seed=100):
    V = [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(seed + k) for k, w in enumerate(widths)]
    b = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(seed + 50)
    y = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(seed + 51)
    return V, b, y


def _forms(ctx):
    p = ctx.profile()
    return p.get("basis_form_mfma", {}).get("count", 0), p.get("basis_form_generic", {}).get("count", 0)


def _generic_launches(widths):
    """The generic form takes consecutive fields while they sum to at most 32 columns (and are at most 8 fields)."""
    n, cols, fields = 0, 0, 0
    for w in widths:
        if fields == 0 or cols + w > 32 or fields == 8:
            n, cols, fields = n + 1, 0, 0
        cols, fields = cols + w, fields + 1
    return n


def _dot_error(got, want, scale):
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / scale))


def _case(bc, ctx, widths, m, parity, dot_forms, axpy_forms, worst):
    """dot_forms, axpy_forms: the expected (MFMA, generic) launch counts of basis_dot and of basis_axpy"""
    what = (ctx.dims, widths, m, parity)
    V, b, y = _operands(bc, ctx, widths, m, parity)
    Vh, bh, yh = [v.download() for v in V], b.download(), y.download()
    want, scale = ref.basis_dot(Vh, bh), ref.dot_scale(Vh, bh)
    K = sum(widths)
    rng = np.random.default_rng(K * 100 + m)
    C = rng.standard_normal((K, m)) + 1j * rng.standard_normal((K, m))
    results = {}
    generic_forms = (0, _generic_launches(widths))
    dot_expected = {False: tuple(dot_forms), True: generic_forms}
    axpy_expected = {False: tuple(axpy_forms), True: generic_forms}
    for generic in (False, True):
        ctx.force_generic(generic)
        ctx.profile_reset()
        got = bc.basis_dot(V, b)
        assert _forms(ctx) == dot_expected[generic], (what, "dot")
        err = _dot_error(got, want, scale)
        worst[0] = max(worst[0], err)
        assert err <= EPS_DOT, (what, generic, err)
        assert np.array_equal(_bits(bc.basis_dot(V, b)), _bits(got)), what  # the same bits again
        outs = []
        for beta in (0.0, 1.0, -0.5):
            y.upload(np.full_like(yh, np.nan) if beta == 0.0 else yh)
            ctx.profile_reset()
            bc.basis_axpy(y, V, C, beta)
            assert _forms(ctx) == axpy_expected[generic], (what, "update")
            out = y.download()
            assert np.isfinite(out).all(), (what, beta)
            e = rel_err(out, ref.basis_axpy(yh, Vh, C, beta))
            worst[1] = max(worst[1], e)
            assert e <= TOL_KERNEL, (what, generic, beta, e)
            y.upload(np.full_like(yh, np.nan) if beta == 0.0 else yh)
            bc.basis_axpy(y, V, C, beta)
            assert np.array_equal(_bits(y.download()), _bits(out)), what
            outs.append(out)
        results[generic] = (got, outs)
    ctx.force_generic(False)
    # the MFMA form against the generic one
    assert _dot_error(results[False][0], results[True][0], scale) <= EPS_DOT, what
    for o_fast, o_gen in zip(results[False][1], results[True][1]):
        assert rel_err(o_fast, o_gen) <= TOL_KERNEL, what
    # the operands are untouched
    for v, vh in zip(V, Vh):
        assert np.array_equal(_bits(v.download()), _bits(vh)), what
    assert np.array_equal(_bits(b.download()), _bits(bh)), what


@pytest.mark.parametrize("widths,m,n_mfma,n_generic", GENERIC + MFMA + MIXED)
def test_basis_products(bc, widths, m, n_mfma, n_generic):
    worst = [0.0, 0.0]
    forms = (n_mfma, n_generic)
    for dims in LATTICES:
        _case(bc, _ctx(bc, dims), widths, m, None, forms, forms, worst)
    for parity in (0, 1):
        _case(bc, _ctx(bc, [4, 2, 4, 2]), widths, m, parity, forms, forms, worst)
    print(f"V widths {widths}, m = {m}: dot {worst[0]:.3e} of |V_i||b_j|, update {worst[1]:.3e} relative")


@pytest.mark.parametrize("widths,m,dot_forms,axpy_forms", GROUP_WALK)
def test_group_walk(bc, widths, m, dot_forms, axpy_forms):
    """The host's walk over groups of basis fields, where the dot and the update may cut V differently: the launch counts of
    either call from the profile, and everything test_basis_products checks, on the same lattices and parities."""
    worst = [0.0, 0.0]
    for dims in LATTICES:
        _case(bc, _ctx(bc, dims), widths, m, None, dot_forms, axpy_forms, worst)
    for parity in (0, 1):
        _case(bc, _ctx(bc, [4, 2, 4, 2]), widths, m, parity, dot_forms, axpy_forms, worst)
    print(f"V widths {widths}, m = {m}: dot {worst[0]:.3e} of |V_i||b_j|, update {worst[1]:.3e} relative; "
          f"launches dot {dot_forms}, update {axpy_forms}")


def test_more_than_one_group(bc):
    """Five fields of 32 columns at m = 16: three launches of the MFMA form (64, 64 and 32 columns)."""
    worst = [0.0, 0.0]
    _case(bc, _ctx(bc, [4, 2, 4, 2]), [32] * 5, 16, None, (3, 0), (3, 0), worst)
    print(f"five fields of 32, m = 16: dot {worst[0]:.3e}, update {worst[1]:.3e}")


def test_more_than_one_block(bc):
    """[16,16,8,4], V = two fields of 32, m = 16: 6144 quads on a grid of 1024 blocks, against numpy on the whole field."""
    ctx = _ctx(bc, [16, 16, 8, 4])
    V, b, y = _operands(bc, ctx, [32, 32], 16, None)
    Vh, bh, yh = [v.download() for v in V], b.download(), y.download()
    ctx.profile_reset()
    got = bc.basis_dot(V, b)
    assert _forms(ctx) == (1, 0)
    err = _dot_error(got, ref.basis_dot(Vh, bh), ref.dot_scale(Vh, bh))
    print(f"[16,16,8,4] ([32,32],16): dot {err:.3e} of |V_i||b_j|")
    assert err <= EPS_DOT
    assert np.array_equal(_bits(bc.basis_dot(V, b)), _bits(got))
    C = np.random.default_rng(5).standard_normal((64, 16)) + 1j * np.random.default_rng(6).standard_normal((64, 16))
    bc.basis_axpy(y, V, C, -0.5)
    e = rel_err(y.download(), ref.basis_axpy(yh, Vh, C, -0.5))
    print(f"[16,16,8,4] ([32,32],16): update {e:.3e}")
    assert e <= TOL_KERNEL


@pytest.mark.parametrize("m", [5, 16])
def test_sum_of_slice_gram_is_basis_dot(bc, m):
    ctx = _ctx(bc, [4, 2, 4, 2])
    for parity in (None, 1):
        a = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(3)
        b = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(4)
        scale = ref.dot_scale([a.download()], b.download())
        assert np.max(np.abs(a.slice_gram(b, 3).sum(axis=0) - bc.basis_dot([a], b)) / scale) <= EPS_DOT
        assert np.max(np.abs(a.slice_gram(a, 3).sum(axis=0) - bc.basis_dot([a], a)) / ref.dot_scale([a.download()], a.download())) <= EPS_DOT


@pytest.mark.parametrize("parity", [None, 0, 1])
def test_copy_columns(bc, parity):
    """32 -> 16 -> 5 columns, bit for bit, the other columns of the target unchanged."""
    ctx = _ctx(bc, [4, 2, 4, 2])
    f32 = bc.block_fermion_field(ctx, 32, parity=parity).setGaussian(1)
    f16 = bc.block_fermion_field(ctx, 16, parity=parity).setGaussian(2)
    f5 = bc.block_fermion_field(ctx, 5, parity=parity).setGaussian(3)
    h32, h16, h5 = f32.download(), f16.download(), f5.download()
    f16.copy_columns(3, f32, 19, 9)
    want16 = h16.copy()
    want16[:, 3:12] = h32[:, 19:28]
    assert np.array_equal(_bits(f16.download()), _bits(want16))
    f5.copy_columns(1, f16, 2, 4)
    want5 = h5.copy()
    want5[:, 1:5] = want16[:, 2:6]
    assert np.array_equal(_bits(f5.download()), _bits(want5))
    f32.copy_columns(27, f5, 0, 5)  # and back into the wide field, up to its last column
    want32 = h32.copy()
    want32[:, 27:32] = want5
    assert np.array_equal(_bits(f32.download()), _bits(want32))


def test_invalid_calls_leave_the_outputs_alone(bc):
    ctx = _ctx(bc, [4, 2, 4, 2])
    other = _ctx(bc, [37])
    lib = ctx.lib
    v16 = bc.block_fermion_field(ctx, 16).setGaussian(1)
    v5 = bc.block_fermion_field(ctx, 5).setGaussian(2)
    b = bc.block_fermion_field(ctx, 8).setGaussian(3)
    y = bc.block_fermion_field(ctx, 8).setGaussian(4)
    half = bc.block_fermion_field(ctx, 8, parity=0).setGaussian(5)
    vhalf = bc.block_fermion_field(ctx, 16, parity=1).setGaussian(6)
    foreign = bc.block_fermion_field(other, 16).setGaussian(7)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731

    def handles(*fields):
        return (ctypes.c_void_p * max(1, len(fields)))(*[f.h if f is not None else None for f in fields])

    poison = np.full((8, 21), 7.25 + 1j, dtype=np.complex128)
    out = poison.copy()
    for V, nv, rhs, o in ((handles(v16, v5), 0, b, out), (handles(v16, v5), -1, b, out), (None, 2, b, out),
                          (handles(v16, None), 2, b, out), (handles(v16, v5), 2, None, out), (handles(v16, v5), 2, b, None),
                          (handles(v16, foreign), 2, b, out), (handles(v16, vhalf), 2, b, out), (handles(v16, v5), 2, half, out)):
        rc = lib.bcg_basis_dot(V, nv, rhs.h if rhs is not None else None, dp(o) if o is not None else None)
        assert rc == INVALID
        assert np.array_equal(_bits(out), _bits(poison))
    yh = y.download()
    C = np.ones((8, 21), dtype=np.complex128)
    for target, V, nv, coeff, beta in ((y, handles(v16, v5), 0, C, 1.0), (y, None, 2, C, 1.0), (y, handles(v16, None), 2, C, 1.0),
                                       (y, handles(v16, v5), 2, None, 1.0), (y, handles(v16, foreign), 2, C, 1.0),
                                       (y, handles(v16, vhalf), 2, C, 1.0), (y, handles(v5, y), 2, C, 1.0),
                                       (y, handles(v16, v5), 2, C, float("nan")), (None, handles(v16, v5), 2, C, 1.0)):
        rc = lib.bcg_basis_axpy(target.h if target is not None else None, V, nv, dp(coeff) if coeff is not None else None, beta)
        assert rc == INVALID
        assert np.array_equal(_bits(y.download()), _bits(yh))
    for dst, d0, src, s0, n in ((y, 0, y, 0, 1), (y, 0, None, 0, 1), (None, 0, v16, 0, 1), (y, 0, v16, 0, 0), (y, 0, v16, 0, 9),
                                (y, 4, v16, 0, 5), (y, 0, v16, 12, 5), (y, -1, v16, 0, 2), (y, 0, v16, -1, 2), (y, 0, vhalf, 0, 2),
                                (y, 0, foreign, 0, 2), (y, 0, v16, 0, -3)):
        rc = lib.bcg_field_copy_columns(dst.h if dst is not None else None, d0, src.h if src is not None else None, s0, n)
        assert rc == INVALID
        assert np.array_equal(_bits(y.download()), _bits(yh))
    with pytest.raises(bc.BlockCGError):
        bc.basis_axpy(y, [v16, y], np.ones((24, 8)))


def test_divided_lattice_without_a_comm(bc):
    """One rank of a (2,1,1,1) grid with no bcg_comm attached: basis_dot returns BCG_ERR_COMM before anything is launched, full
    and half fields, and the poisoned result stays as it was."""
    ctx = bc.Context([4, 2, 4, 2], grid=[2, 1, 1, 1], coords=[0, 0, 0, 0])
    for parity in (None, 0):
        V = [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(1 + w) for w in (16, 5)]
        b = bc.block_fermion_field(ctx, 16, parity=parity).setGaussian(9)
        poison = np.full((16, 21), 7.0 - 3.0j)
        out = poison.copy()
        Vh = (ctypes.c_void_p * 2)(*[v.h for v in V])
        assert ctx.lib.bcg_basis_dot(Vh, 2, b.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 5
        assert np.array_equal(_bits(out), _bits(poison))


def _orthonormal_fields(bc, ctx, widths, parity, seed):
    sites = ctx.V if parity is None else ctx.V // 2
    K = sum(widths)
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((3 * sites, K)) + 1j * rng.standard_normal((3 * sites, K)))
    hosts = ref.split_columns(ref.to_field(Q), widths)
    return [bc.block_fermion_field(ctx, w, host=h, parity=parity) for w, h in zip(widths, hosts)], hosts


@pytest.mark.parametrize("widths,m,parity", [([32, 16], 8, None), ([16, 32], 16, 0), ([7, 12], 5, 1)])
def test_deflate(bc, widths, m, parity):
    ctx = _ctx(bc, [4, 2, 4, 2])
    V, Vh = _orthonormal_fields(bc, ctx, widths, parity, 17)
    B = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(9)
    Bh = B.download()
    C = bc.deflate(B, V)
    assert _dot_error(C, ref.basis_dot(Vh, Bh), ref.dot_scale(Vh, Bh)) <= EPS_DOT
    assert rel_err(B.download(), Bh - ref.basis_axpy(None, Vh, ref.basis_dot(Vh, Bh), 0.0)) <= TOL_KERNEL
    left = np.linalg.norm(bc.basis_dot(V, B))
    print(f"deflate {widths}, m = {m}, parity {parity}: |V^dagger B_perp| = {left / np.linalg.norm(Bh):.3e} of |B|")
    assert left <= 1e-13 * np.linalg.norm(Bh)


def test_sbcgrq_deflated(bc):
    """[4,4,4,2], m = 8, V = the 48 lowest eigenvectors of the dense operator as fields of 32 and 16 columns, mass 0.05,
    sigma = (0, 0.05, 0.5), eps 1e-10.  tests/test_basis_cpu.py restates the solve: 48 operator applications deflated against
    69 plain at the lowest shift."""
    p = ref.deflation_problem()
    ctx = _ctx(bc, ref.DEFLATION_DIMS)
    D = bc.dirac_op(ctx, mass=ref.DEFLATION_MASS, U=p["U"])
    B = bc.block_fermion_field(ctx, ref.DEFLATION_M, host=p["B"])
    hosts = ref.split_columns(ref.to_field(p["W"]), ref.DEFLATION_WIDTHS)
    V = [bc.block_fermion_field(ctx, w, host=h) for w, h in zip(ref.DEFLATION_WIDTHS, hosts)]
    sigma = list(ref.DEFLATION_SIGMA)
    X = [bc.block_fermion_field(ctx, ref.DEFLATION_M) for _ in sigma]
    Xp = [bc.block_fermion_field(ctx, ref.DEFLATION_M) for _ in sigma]
    eps = ref.DEFLATION_EPS
    it_deflated = bc.SBCGrQ_deflated(X, B, D, sigma, V, p["evals"], eps, eps)
    it_plain = bc.SBCGrQ(Xp, B, D, sigma, eps, eps)
    assert np.array_equal(_bits(B.download()), _bits(p["B"]))  # the right-hand side is untouched
    res_deflated = bc.true_residuals(X, B, D, sigma)
    res_plain = bc.true_residuals(Xp, B, D, sigma)
    Bv = ref.to_vec(p["B"])
    n = Bv.shape[0]
    errs = []
    for s, sg in enumerate(sigma):
        exact = ref.to_field(np.linalg.solve(p["A"] + sg * np.eye(n), Bv))
        errs.append((rel_err(X[s].download(), exact), rel_err(Xp[s].download(), exact)))
    print(f"operator applications: {it_deflated} deflated against {it_plain} plain")
    print("error against the dense solve (deflated, plain) per shift:", errs)
    print("true residuals, deflated:", res_deflated.max(axis=1), "plain:", res_plain.max(axis=1))
    for s in range(len(sigma)):
        assert errs[s][0] <= TOL_SOLUTION, (s, errs[s])
        assert res_deflated[s].max() <= 10.0 * res_plain[s].max(), (s, res_deflated[s].max(), res_plain[s].max())
    assert it_deflated <= 0.85 * it_plain, (it_deflated, it_plain)


def test_cpp_basis_layer_runs(bc):
    """tests/cpp/basis_run_probe.cpp, built by the recipe of tests/test_cpp_dropin.py: blockcg/basis.hpp on the device -- the
    column-major C[j * K + i], the host mirror around every call, copy_columns, deflate -- checked inside the probe against
    host sums in long double; and its SBCGrQ_deflated (V = 16 orthonormal columns, evals 1 .. 16: no solution of the system,
    but a fixed function of its inputs) against the same calls made here."""
    from test_cpp_dropin import _compile
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "basis_run_probe.cpp"), "basis_run_probe")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "BASIS_PROBE_OK" and "FAILED" not in r.stdout, r.stdout + r.stderr
    applications = [int(line.split()[1]) for line in lines if line.startswith("DEFLATED_APPLICATIONS")]
    hdot = {int(line.split()[1]): np.array([float(v) for v in line.split()[2:]]) for line in lines if line.startswith("HDOT")}
    sigma = [0.0, 0.05, 0.5]
    assert len(applications) == 1 and sorted(hdot) == [0, 1, 2]
    ctx = _ctx(bc, [4, 2, 4, 2])
    q = bc.block_fermion_field(ctx, 16).setGaussian(31)
    q.thinQR()
    D = bc.dirac_op(ctx, 0.5, seed=7)
    B = bc.block_fermion_field(ctx, 8).setGaussian(32)
    X = [bc.block_fermion_field(ctx, 8) for _ in sigma]
    assert bc.SBCGrQ_deflated(X, B, D, sigma, [q], np.arange(1.0, 17.0), 1e-10, 1e-10) == applications[0]
    for s in range(len(sigma)):
        assert hdot[s].shape == (128,)
        got = (hdot[s][0::2] + 1j * hdot[s][1::2]).reshape(8, 8).T  # the probe prints column-major
        want = B.hermitian_dot(X[s])
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"sigma = {sigma[s]}: B^dagger X_s of the C++ layer against the bindings {err:.3e}")
        assert err <= TOL_SOLUTION, (s, err)
