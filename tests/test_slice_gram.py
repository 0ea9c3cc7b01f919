"""Per-slice Gram matrices with momentum projection (include/blockcg_hip.h: bcg_field_slice_gram) against their numpy
restatement (tests/slice_gram_ref.py): every direction, width class and parity, one operand and two, momenta that are
negative and beyond the extents; against slice_dot and hermitian_dot; the same bits on a second call; the error returns;
and examples/momentum_correlator.cpp end to end.

Tolerance: EPS_DOT = 1e-13 relative to sqrt(|a_i|^2_slice |b_j|^2_slice) per entry, the bound tests/test_sources_sinks.py
derives for slice_dot on the same lattices (sums of at most 1536 terms; the phases have modulus 1 to a few ulp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import slice_gram_ref as ref

pytestmark = pytest.mark.gpu

EPS_DOT = 1e-13
INVALID = 1
MOMENTA = ([1, 0, 0, 0], [-1, 1, 0, 1], [2, 1, 3, 1], [5, -3, 0, 2])  # beyond the extents of [4, 2, 4, 2] and negative ones


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


def _momenta(direction, ndim=4):
    """MOMENTA and their negatives (entry P/2 + k is minus entry k), the component along `direction` and beyond ndim set to 0."""
    out = []
    for sign in (1, -1):
        for n in MOMENTA:
            q = [sign * v if mu < ndim else 0 for mu, v in enumerate(n)]
            q[direction] = 0
            out.append(q)
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _check(got, want, scale, worst, what):
    """got, want [P, L, m, m]; scale [L, m, m].  Slices a half field holds no site of: exact zeros."""
    assert got.shape == want.shape, what
    sc = np.broadcast_to(scale, got.shape)
    assert np.array_equal(got[sc == 0], np.zeros_like(got[sc == 0])), what
    held = sc > 0
    err = float(np.max(np.abs(got - want)[held] / sc[held]))
    worst[0] = max(worst[0], err)
    assert err <= EPS_DOT, (what, err)


def _sweep(bc, ctx, dims, m, parity, worst, momenta_of=_momenta, pairs=(False, True)):
    a = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(11)
    b = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(12)
    ah, bh = a.download(), b.download()
    norm_bits = _bits(a.hermitian_dot(a)).copy()
    for self_ in pairs:
        x, xh, y, yh = (a, ah, a, ah) if self_ else (a, ah, b, bh)
        # hermitian_dot computes the lower triangle (i >= j) of x^dagger y and mirrors it (include/blockcg_hip.h), so for two
        # operands the upper triangle comes from (y^dagger x)^dagger
        full = np.tril(x.hermitian_dot(y)) + np.triu(np.conj(y.hermitian_dot(x)).T, 1)
        total = np.sqrt(np.outer((np.abs(xh) ** 2).sum(axis=(0, 2)), (np.abs(yh) ** 2).sum(axis=(0, 2))))
        for direction in range(len(dims)):
            what = (dims, m, parity, direction, self_)
            got0 = x.slice_gram(y, direction)
            want0, scale = ref.slice_gram(xh, yh, dims, direction, None, parity)
            _check(got0[None], want0, scale, worst, what)
            # the diagonal is slice_dot, the sum over the slices hermitian_dot
            dots = x.slice_dot(y, direction)
            dscale = np.einsum("tii->ti", scale)
            derr = np.abs(np.einsum("tii->ti", got0) - dots)
            assert np.all(derr[dscale == 0] == 0) and np.max(derr[dscale > 0] / dscale[dscale > 0]) <= EPS_DOT, what
            assert np.max(np.abs(got0.sum(axis=0) - full) / total) <= EPS_DOT, what
            assert np.array_equal(_bits(x.slice_gram(y, direction)), _bits(got0)), what  # the same bits again
            mom = momenta_of(direction)
            if not mom:
                continue
            gotp = x.slice_gram(y, direction, mom)
            wantp, _ = ref.slice_gram(xh, yh, dims, direction, mom, parity)
            _check(gotp, wantp, scale, worst, what)
            assert np.array_equal(_bits(x.slice_gram(y, direction, mom)), _bits(gotp)), what
            if self_ and len(mom) % 2 == 0:  # C_{-p}(t) = C_p(t)^dagger
                h = len(mom) // 2
                dev = np.abs(gotp[h:] - np.conj(gotp[:h]).transpose(0, 1, 3, 2))
                sc = np.broadcast_to(scale, dev.shape)
                assert np.all(dev[sc == 0] == 0) and np.max(dev[sc > 0] / sc[sc > 0]) <= EPS_DOT, what
    assert np.array_equal(_bits(a.hermitian_dot(a)), norm_bits)  # the operands are untouched


@pytest.mark.parametrize("m", [1, 5, 8, 12, 16, 32])
def test_slice_gram_main_sweep(bc, m):
    dims = [4, 2, 4, 2]
    ctx = bc.Context(dims)
    worst = [0.0]
    for parity in (None, 0, 1):
        _sweep(bc, ctx, dims, m, parity, worst)
    print(f"largest slice-gram error on {dims}, m = {m}: {worst[0]:.3e} of |a_i||b_j| per slice")


@pytest.mark.parametrize("m", [1, 5, 16])
def test_slice_gram_in_one_dimension(bc, m):
    """[96]: a slice is one site, 3 rows, less than one quad of the MFMA kernel.  n_mom = 0 and the zero momentum given
    explicitly (the phase path, all tables 1) return the same bits."""
    dims = [96]
    ctx = bc.Context(dims)
    worst = [0.0]
    for parity in (None, 0, 1):
        _sweep(bc, ctx, dims, m, parity, worst, momenta_of=lambda d: [])
        a = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(11)
        b = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(12)
        for y in (b, a):
            plain = a.slice_gram(y, 0)
            zero = a.slice_gram(y, 0, [[0]])
            assert zero.shape == (1,) + plain.shape
            assert np.array_equal(_bits(zero[0]), _bits(plain)), (m, parity)
    print(f"largest slice-gram error on {dims}, m = {m}: {worst[0]:.3e}")


@pytest.mark.parametrize("m", [16, 32])
def test_slice_gram_on_8x8x8x8(bc, m):
    dims = [8, 8, 8, 8]
    ctx = bc.Context(dims)
    worst = [0.0]
    moms = {0: [[0, 1, 0, 0], [0, -1, 2, 9], [0, 0, 0, 0]], 3: [[1, 0, 0, 0], [-1, 2, 9, 0], [0, 0, 0, 0]]}
    for parity in (None, 1):
        a = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(11)
        b = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(12)
        ah, bh = a.download(), b.download()
        for direction in (0, 3):
            got = a.slice_gram(b, direction, moms[direction])
            want, scale = ref.slice_gram(ah, bh, dims, direction, moms[direction], parity)
            _check(got, want, scale, worst, (m, parity, direction))
            assert np.array_equal(_bits(got[2]), _bits(a.slice_gram(b, direction)))  # the zero momentum: exactly the plain sums
    print(f"largest slice-gram error on {dims}, m = {m}: {worst[0]:.3e}")


def test_slice_gram_at_ragged_shapes(bc):
    """Row counts that quads of 4 and chunks of 16 rows do not divide, odd extents; one non-zero momentum where the lattice
    has a second direction."""
    worst = [0.0]
    for dims, m in (([5, 3, 2], 16), ([7, 5, 3, 3], 12), ([37], 5)):
        nd = len(dims)

        def mom(direction, nd=nd):
            if nd == 1:
                return []
            q = [2, -1, 1, 4][:nd] + [0] * (4 - nd)
            q[direction] = 0
            return [q]

        _sweep(bc, bc.Context(dims), dims, m, None, worst, momenta_of=mom)
    print(f"largest slice-gram error at ragged shapes: {worst[0]:.3e}")


@pytest.mark.parametrize("dims,m", [([16, 16, 16, 4], 16), ([16, 16, 8, 4], 32)], ids=["m16", "m32"])
def test_slice_gram_with_several_blocks_per_slice(bc, dims, m):
    """Three momenta are taken two per launch at both widths (two launches: 2 + 1).  The plan (kernels_slice_gram.hpp) gives
    [16,16,16,4], m = 16: direction 3 has 192 blocks per slice of 12288 rows, direction 0 has 48 per slice of 3072 rows;
    [16,16,8,4], m = 32: direction 3 has 96 blocks per slice of 6144 rows, direction 0 has 24 per slice of 1536 rows;
    chunks of 64 rows (four quads per wave) in all four.  Against numpy on the whole field."""
    ctx = bc.Context(dims)
    a = bc.block_fermion_field(ctx, m).setGaussian(21)
    b = bc.block_fermion_field(ctx, m).setGaussian(22)
    ah, bh = a.download(), b.download()
    worst = [0.0]
    for direction, moms in ((3, [[1, 0, 0, 0], [-2, 3, 17, 0], [0, 5, -1, 0]]), (0, [[0, 1, 0, 0], [0, 3, 17, -2], [0, 0, 5, -1]])):
        got = a.slice_gram(b, direction, moms)
        want, scale = ref.slice_gram(ah, bh, dims, direction, moms)
        _check(got, want, scale, worst, (dims, m, direction))
        assert np.array_equal(_bits(a.slice_gram(b, direction, moms)), _bits(got))
        got0 = a.slice_gram(a, direction)
        want0, scale0 = ref.slice_gram(ah, ah, dims, direction)
        _check(got0[None], want0, scale0, worst, (dims, m, direction, "self"))
    print(f"largest slice-gram error on {dims}, m = {m}: {worst[0]:.3e}")


def test_invalid_calls_leave_out_alone(bc):
    dims, m = [4, 2, 4, 2], 5
    ctx = bc.Context(dims)
    lib = ctx.lib
    a = bc.block_fermion_field(ctx, m).setGaussian(1)
    out = np.full((2, 4, m, m), 7.0 - 3.0j, dtype=np.complex128)
    poison = out.copy()
    dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = ctypes.POINTER(ctypes.c_int)

    def mom(*rows):
        arr = np.ascontiguousarray(rows, dtype=np.intc)
        return arr, arr.ctypes.data_as(ip)

    ok_arr, ok = mom([1, 0, 0, 0])
    cases = {
        "width": (a.h, bc.block_fermion_field(ctx, 4).h, 3, 1, ok, dp),
        "parity": (a.h, bc.block_fermion_field(ctx, m, parity=0).h, 3, 1, ok, dp),
        "context": (a.h, bc.block_fermion_field(bc.Context(dims), m).h, 3, 1, ok, dp),
        "dir -1": (a.h, a.h, -1, 0, None, dp),
        "dir ndim": (a.h, a.h, 4, 0, None, dp),
        "n_mom -1": (a.h, a.h, 3, -1, ok, dp),
        "dir component": (a.h, a.h, 3, 2, mom([1, 0, 0, 0], [0, 1, 0, 4])[1], dp),
        "null momenta": (a.h, a.h, 3, 1, None, dp),
    }
    keep = []
    for what, args in cases.items():
        keep.append(args)
        assert lib.bcg_field_slice_gram(*args) == INVALID, what
        assert np.array_equal(_bits(out), _bits(poison)), what
    assert lib.bcg_field_slice_gram(a.h, a.h, 3, 0, None, None) == INVALID  # NULL out
    # a 3-D lattice: the fourth component must be 0
    ctx3 = bc.Context([4, 2, 2])
    g = bc.block_fermion_field(ctx3, m).setGaussian(2)
    arr, p = mom([1, 0, 0, 1])
    assert ctx3.lib.bcg_field_slice_gram(g.h, g.h, 1, 1, p, dp) == INVALID
    assert np.array_equal(_bits(out), _bits(poison))
    with pytest.raises(bc.BlockCGError):
        a.slice_gram(a, 4)
    # and the good call fills it
    assert lib.bcg_field_slice_gram(a.h, a.h, 3, 1, ok, dp) == 0
    assert not np.array_equal(_bits(out[0, :2]), _bits(poison[0, :2]))


def test_momentum_correlator_example(bc, monkeypatch):
    """examples/momentum_correlator.cpp, built by the recipe of tests/test_cpp_dropin.py and run on 4^4: its p = 0 column is the
    sum over the columns of slice_dot of the same solve done here, its +p and -p columns are complex conjugates."""
    from conftest import ROOT
    out = os.path.join(ROOT, "examples", "_build")
    libdir = os.path.join(ROOT, "blockcg_amd", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "momentum_correlator")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "blockcg_amd", "include"),
                        os.path.join(ROOT, "examples", "momentum_correlator.cpp"), "-o", exe, "-L", libdir, "-lblockcg_hip",
                        f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "4", "4", "4", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MOMENTUM_CORRELATOR_OK" in r.stdout, r.stdout + r.stderr
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.splitlines() if line and line[0] not in "#M"])
    assert rows.shape == (4, 7)
    c0, cp, cm = rows[:, 1] + 1j * rows[:, 2], rows[:, 3] + 1j * rows[:, 4], rows[:, 5] + 1j * rows[:, 6]
    monkeypatch.setenv("BCG_HOP_PATCH", "16,2,2")
    monkeypatch.setenv("BCG_HOP_BLOCKS", "32")
    dims = [4, 4, 4, 4]
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, 0.5, seed=7)
    B = bc.block_fermion_field(ctx, 3).setPointSources([[0, 0, 0, 0]] * 3, [0, 1, 2])
    X = [bc.block_fermion_field(ctx, 3)]
    bc.SBCGrQ(X, B, D, [0.0], 1e-12, 1e-12)
    want = X[0].slice_dot(X[0], 3).sum(axis=1)
    assert np.max(np.abs(c0 - want) / np.abs(want)) <= 1e-10
    assert np.max(np.abs(cp - np.conj(cm)) / np.abs(want)) <= 1e-10
    assert np.max(np.abs(cp.imag)) > 0 or np.max(np.abs(cp - c0)) > 0  # the projection does something
