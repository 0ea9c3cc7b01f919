"""Sources and sinks on the device (include/blockcg_hip.h): noise fields, point / wall sources and the slice dot against their
numpy restatement (tests/sources_ref.py), full and half fields, every width class and direction; then end to end (a
point-source solve measured per time slice, and the heat-bath setGaussian -> SBCGrQ_sum)."""
import ctypes

import numpy as np
import pytest

import sources_ref as ref

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 12, 16, 32)
LATTICES = ([96], [4, 2, 4, 2], [8, 8, 8, 8])
PARITIES = (None, 0, 1)
EPS_DOT = 1e-13  # relative to |a|_slice |b|_slice per entry: sums of at most 8^3 * 3 = 1536 terms, 1536 eps = 3.4e-13 worst case


@pytest.fixture(scope="module")
def bc():
    import blockcg_amd
    return blockcg_amd


def _uniforms(orc, m, dims, seed, parity):
    return orc.fill_field(m, int(np.prod(dims)), seed)[ref.parity_mask(dims, parity)]


@pytest.mark.parametrize("dims", LATTICES, ids=lambda d: "x".join(map(str, d)))
def test_noise_matches_the_definition(bc, orc, dims):
    ctx = bc.Context(dims)
    worst = 0.0
    for m in WIDTHS:
        for parity in PARITIES:
            u = _uniforms(orc, m, dims, 7 + m, parity)
            f = bc.block_fermion_field(ctx, m, parity=parity)
            assert np.array_equal(f.setRandom(7 + m).download(), u)  # fill_random keeps its values
            assert np.array_equal(f.setZ2(7 + m).download(), ref.noise_from_uniforms(u, ref.Z2))
            assert np.array_equal(f.setZ4(7 + m).download(), ref.noise_from_uniforms(u, ref.Z4))
            dev = np.max(np.abs(f.setGaussian(7 + m).download() - ref.noise_from_uniforms(u, ref.GAUSSIAN)))
            worst = max(worst, dev)
    print(f"largest Gaussian deviation from numpy on {dims}: {worst:.3e}")
    assert worst <= 1e-14
    with pytest.raises(bc.BlockCGError) as e:
        f._fill_noise(3, 1)
    assert e.value.code == 1


def _status(ctx, call, *args):
    return getattr(ctx.lib, call)(*args)


def _ip(v):
    a = np.ascontiguousarray(v, dtype=np.intc)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


@pytest.mark.parametrize("dims", LATTICES, ids=lambda d: "x".join(map(str, d)))
def test_point_and_wall_sources(bc, dims):
    ctx = bc.Context(dims)
    nd = len(dims)
    rng = np.random.default_rng(5)
    for m in WIDTHS:
        for parity in PARITIES:
            f = bc.block_fermion_field(ctx, m, parity=parity)
            pts = [[int(rng.integers(0, d)) for d in dims] for _ in range(m)]
            if parity is not None:
                for p in pts:
                    if sum(p) % 2 != parity:
                        p[0] ^= 1  # even extents: stays inside
            col = [int(c) for c in rng.integers(0, 3, m)]
            assert np.array_equal(f.setPointSources(pts, col).download(), ref.point_sources(dims, m, pts, col, parity))
            for direction in range(nd):
                sl = [int(s) for s in rng.integers(0, dims[direction], m)]
                for sp in ((-1, 0, 1) if parity is None else (-1, parity)):
                    got = f.setWallSources(direction, sl, col, sp).download()
                    assert np.array_equal(got, ref.wall_sources(dims, m, direction, sl, col, sp, parity)), (m, parity, direction, sp)


def test_invalid_sources_leave_the_field_alone(bc):
    dims, m = [4, 2, 4, 2], 5
    ctx = bc.Context(dims)
    lib = ctx.lib
    good_pts = np.zeros((m, 4), dtype=np.intc)
    good_col = [0, 1, 2, 0, 1]
    for parity in (None, 1):
        f = bc.block_fermion_field(ctx, m, parity=parity).setRandom(3)
        before = f.download()
        if parity == 1:
            good_pts[:, 0] = 1
        bad = []
        p = good_pts.copy(); p[2, 1] = 2; bad.append(("point", p, good_col))          # x1 outside
        p = good_pts.copy(); p[0, 3] = -1; bad.append(("point", p, good_col))
        bad.append(("point", good_pts, [0, 1, 3, 0, 1]))                                # colour outside 0..2
        bad.append(("point", good_pts, [0, -1, 2, 0, 1]))
        if parity == 1:
            p = good_pts.copy(); p[4, 0] = 2; bad.append(("point", p, good_col))      # site of the other parity
        bad.append(("wall", 4, [0] * m, good_col, -1))                                  # dir outside
        bad.append(("wall", -1, [0] * m, good_col, -1))
        bad.append(("wall", 1, [0, 0, 2, 0, 0], good_col, -1))                          # slice outside
        bad.append(("wall", 1, [0] * m, [0, 1, 2, 3, 0], -1))
        bad.append(("wall", 1, [0] * m, good_col, 2))
        if parity == 1:
            bad.append(("wall", 1, [0] * m, good_col, 0))                               # a half field's other parity
        for case in bad:
            if case[0] == "point":
                pa, pp = _ip(case[1]); ca, cp = _ip(case[2])
                rc = lib.bcg_field_set_point_sources(f.h, pp, cp)
            else:
                sa, sp_ = _ip(case[2]); ca, cp = _ip(case[3])
                rc = lib.bcg_field_set_wall_sources(f.h, case[1], sp_, cp, case[4])
            assert rc == 1, case
            assert np.array_equal(f.download(), before), case
    # a 3-D lattice: the fourth coordinate must be 0
    ctx3 = bc.Context([4, 2, 2])
    g = bc.block_fermion_field(ctx3, 1)
    pa, pp = _ip([[0, 0, 0, 1]]); ca, cp = _ip([0])
    assert ctx3.lib.bcg_field_set_point_sources(g.h, pp, cp) == 1
    # slice dot: mixed widths, parities, contexts, direction
    a = bc.block_fermion_field(ctx, 5)
    out = np.empty((8, 5), dtype=np.complex128)
    dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.bcg_field_slice_dot(a.h, bc.block_fermion_field(ctx, 4).h, 0, dp) == 1
    assert lib.bcg_field_slice_dot(a.h, bc.block_fermion_field(ctx, 5, parity=0).h, 0, dp) == 1
    assert lib.bcg_field_slice_dot(a.h, bc.block_fermion_field(bc.Context(dims), 5).h, 0, dp) == 1
    assert lib.bcg_field_slice_dot(a.h, a.h, 4, dp) == 1 and lib.bcg_field_slice_dot(a.h, a.h, -1, dp) == 1


def _check_slice_dot(bc, ctx, dims, m, parity, worst):
    a = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(11)
    b = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(12)
    ah, bh = a.download(), b.download()
    for x, xh, y, yh in ((a, ah, b, bh), (a, ah, a, ah)):
        diag = np.diag(x.hermitian_dot(y))
        for direction in range(len(dims)):
            got = x.slice_dot(y, direction)
            want, scale = ref.slice_dot(xh, yh, dims, direction, parity)
            assert got.shape == want.shape
            assert np.array_equal(got[scale == 0], want[scale == 0])  # slices a half field holds no site of: exact zeros
            held = scale > 0
            err = np.max(np.abs(got - want)[held] / scale[held])
            worst[0] = max(worst[0], err)
            assert err <= EPS_DOT, (dims, m, parity, direction, err)
            total_scale = np.sqrt((np.abs(xh) ** 2).sum(axis=(0, 2)) * (np.abs(yh) ** 2).sum(axis=(0, 2)))
            assert np.max(np.abs(got.sum(axis=0) - diag) / total_scale) <= EPS_DOT
            assert np.array_equal(x.slice_dot(y, direction).view(np.float64), got.view(np.float64))  # the same bits again


@pytest.mark.parametrize("dims", LATTICES, ids=lambda d: "x".join(map(str, d)))
def test_slice_dot(bc, dims):
    ctx = bc.Context(dims)
    worst = [0.0]
    for m in WIDTHS:
        for parity in PARITIES:
            _check_slice_dot(bc, ctx, dims, m, parity, worst)
    print(f"largest slice-dot error on {dims}: {worst[0]:.3e} of |a||b| per slice")


def test_slice_dot_at_ragged_shapes(bc):
    """Row counts the row kernels' chunks of 16 do not divide (tests/test_ragged_rows.py), odd extents."""
    worst = [0.0]
    for dims, m in (([5, 3, 2], 16), ([7, 5, 3, 3], 12), ([37], 5)):
        assert int(np.prod(dims)) * 3 % 16 != 0
        _check_slice_dot(bc, bc.Context(dims), dims, m, None, worst)


def test_slice_dot_at_production_geometry(bc):
    """64^3 x 8 sites, m = 16, time direction: a launch of the size a large lattice gets (2048 blocks; here 256 blocks per
    slice of 64^3 sites with chunks of 49152 elements, where 64^4 has 32 per slice with chunks of 393216), against
    hermitian_dot's diagonal and against numpy on two slices fetched site by site."""
    dims, m = [64, 64, 64, 8], 16
    ctx = bc.Context(dims)
    a = bc.block_fermion_field(ctx, m).setGaussian(21)
    b = bc.block_fermion_field(ctx, m).setGaussian(22)
    got = a.slice_dot(b, 3)
    assert np.array_equal(a.slice_dot(b, 3).view(np.float64), got.view(np.float64))
    S = 64 ** 3
    # per-column norms from the self products (checked below on the fetched slices)
    na, nb = a.slice_dot(a, 3).real, b.slice_dot(b, 3).real
    diag = np.diag(a.hermitian_dot(b))
    assert np.max(np.abs(got.sum(axis=0) - diag) / np.sqrt(na.sum(axis=0) * nb.sum(axis=0))) <= EPS_DOT
    for t in (0, 5):
        sites = np.arange(t * S, (t + 1) * S)
        ah, bh = a.download_sites(sites), b.download_sites(sites)
        want = (np.conj(ah) * bh).sum(axis=(0, 2))
        scale = np.sqrt((np.abs(ah) ** 2).sum(axis=(0, 2)) * (np.abs(bh) ** 2).sum(axis=(0, 2)))
        assert np.max(np.abs(got[t] - want) / scale) <= EPS_DOT, t
        assert np.max(np.abs(na[t] - (np.abs(ah) ** 2).sum(axis=(0, 2))) / na[t]) <= EPS_DOT


def test_pion_correlator_from_point_sources(bc, monkeypatch):
    monkeypatch.setenv("BCG_HOP_PATCH", "16,2,2")
    monkeypatch.setenv("BCG_HOP_BLOCKS", "32")
    dims, m = [4, 4, 4, 4], 3
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, 0.5, seed=31)
    B = bc.block_fermion_field(ctx, m).setPointSources([[0, 0, 0, 0]] * 3, [0, 1, 2])
    X = [bc.block_fermion_field(ctx, m)]
    bc.SBCGrQ(X, B, D, [0.0], 1e-12, 1e-12)
    assert bc.true_residuals(X, B, D, [0.0]).max() < 2e-12
    C = X[0].slice_dot(X[0], 3)
    Xh = X[0].download()
    want, scale = ref.slice_dot(Xh, Xh, dims, 3)
    assert np.max(np.abs(C - want) / scale) <= EPS_DOT
    assert np.all(C.real > 0)


def test_heat_bath_from_gaussian_noise(bc, monkeypatch):
    monkeypatch.setenv("BCG_HOP_PATCH", "16,2,2")
    monkeypatch.setenv("BCG_HOP_BLOCKS", "32")
    dims, m = [8, 4, 4, 4], 16
    shifts, a, c0 = [1e-3, 0.1], [0.7, -1.3], 0.4
    ctx = bc.Context(dims)
    D = bc.dirac_op(ctx, 0.2, seed=35)
    eta = bc.block_fermion_field(ctx, m).setGaussian(36)
    eta_h = eta.download()
    X = [bc.block_fermion_field(ctx, m) for _ in shifts]
    n = bc.SBCGrQ(X, eta, D, shifts, 1e-10, 1e-12)
    phi = bc.block_fermion_field(ctx, m)
    assert bc.SBCGrQ_sum(phi, eta, D, shifts, a, c0, 1e-10, 1e-12) == n
    Xh = [x.download() for x in X]
    want = c0 * eta_h + sum(ak * x for ak, x in zip(a, Xh))
    scale = abs(c0) * np.linalg.norm(eta_h) + sum(abs(ak) * np.linalg.norm(x) for ak, x in zip(a, Xh))
    assert np.linalg.norm(phi.download() - want) / scale < 1e-12  # the sum-mode tolerance of tests/test_sum_mode.py


def test_correlator_example_through_the_headers():
    """examples/pion_correlator.cpp, built by the recipe of tests/test_cpp_dropin.py: point sources, a solve and slice_dot
    through the drop-in headers."""
    import os
    import subprocess
    from conftest import ROOT
    out = os.path.join(ROOT, "examples", "_build")
    libdir = os.path.join(ROOT, "blockcg_amd", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "pion_correlator")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "blockcg_amd", "include"),
                        os.path.join(ROOT, "examples", "pion_correlator.cpp"), "-o", exe, "-L", libdir, "-lblockcg_hip",
                        f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "4", "4", "4", "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CORRELATOR_OK" in r.stdout, r.stdout + r.stderr
