"""Baryon elementals of a basis, slice by slice (include/blockcg_hip.h: bcg_basis_slice_triple) against their numpy
restatement (tests/basis_slice_triple_ref.py): every direction and parity, width lists of either form, momenta that are
negative and beyond the extents; the MFMA form against the generic one; the same bits on a second call; identical lists
(antisymmetric bit for bit, exact zeros on coinciding indices); slice lists; ragged walks; several blocks per (slice, tile);
covariance under a rotation of the columns; the error returns; blockcg/basis.hpp and examples/baryon_elemental.cpp on the
device.

Tolerance: |got - want| <= EPS_DOT * S per entry with S(s; i, j, k) = sum_x |A_i(x)| |B_j(x)| |C_k(x)| (colour 2-norms of each
site), EPS_DOT = 1e-13 as in tests/test_basis_slice.py for the same walk: no slice here holds more than 4096 sites (12288
addends per entry).  Entries whose scale is 0 -- slices a half field holds no site of -- are exact zeros."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import basis_slice_triple_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

EPS_DOT = 1e-13
INVALID, UNSUPPORTED, COMM = 1, 2, 5
MOMENTA = ([1, 0, 0, 0], [-1, 1, 0, 1], [2, 1, 3, 1], [5, -3, 0, 2])  # those of tests/test_basis_slice.py
IDENTICAL = "identical"
# (widths of A, of B, of C), or (widths, IDENTICAL): the same list three times
MFMA_LISTS = (([16], [16], [16]), ([32], [16], [16, 16]), ([16, 32, 16], IDENTICAL))
GENERIC_LISTS = (([5], [5], [5]), ([1, 7, 12], [8], [3]), ([16, 5], [16], [32, 3]))


def _is_mfma(spec):
    return all(w in (16, 32) for ws in spec if ws != IDENTICAL for w in ws)


def _id(spec):
    return "x".join("+".join(map(str, w)) if w != IDENTICAL else "same" for w in spec)


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
    out = []
    for sign in (1, -1):
        for n in MOMENTA:
            q = [sign * v if mu < ndim else 0 for mu, v in enumerate(n)]
            q[direction] = 0
            out.append(q)
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _fields(bc, ctx, widths, parity, seed):
    return [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(seed + k) for k, w in enumerate(widths)]


def _lists(bc, ctx, spec, parity, seed=500):
    if spec[1] == IDENTICAL:
        A = _fields(bc, ctx, spec[0], parity, seed)
        return A, A, A
    return tuple(_fields(bc, ctx, w, parity, seed + 20 * l) for l, w in enumerate(spec))


def _host(lists):
    cache = {}
    return tuple([cache.setdefault(id(f), f.download()) for f in fl] for fl in lists)


def _forms(ctx):
    p = ctx.profile()
    return p.get("basis_slice_triple_form_mfma", {}).get("count", 0), p.get("basis_slice_triple_form_generic", {}).get("count", 0)


def _worst(diff, scale):
    """max |diff| / scale over the entries with scale > 0, and whether diff is exactly 0 on the others"""
    sc = np.broadcast_to(scale, diff.shape)
    if scale.min() > 0:
        return float(np.max(np.abs(diff) / sc)), True
    held = sc > 0
    return (float(np.max(np.abs(diff[held]) / sc[held])) if held.any() else 0.0), not np.any(diff[~held])


def _check(got, want, scale, worst, what):
    """got, want [P, S, Ka, Kb, Kc]; scale [S, Ka, Kb, Kc]"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if scale.min() == 0:
        assert not np.any(got[np.broadcast_to(scale, got.shape) == 0]), what
    err, _ = _worst(got - want, scale)
    print(f"{what}: {err:.3e}")
    worst[0] = max(worst[0], err)
    assert err <= EPS_DOT, (what, err)


def _close(x, y, scale, what):
    err, zeros = _worst(x - y, scale)
    assert zeros and err <= EPS_DOT, (what, err)


def _sweep(bc, ctx, dims, spec, parity, worst, mfma, momenta_of=_momenta, directions=None):
    lists = _lists(bc, ctx, spec, parity)
    hosts = _host(lists)
    fields = {id(f): f for fl in lists for f in fl}.values()
    norm_bits = [_bits(f.hermitian_dot(f)).copy() for f in fields]
    for direction in (range(len(dims)) if directions is None else directions):
        what = (tuple(dims), _id(spec), parity, direction)
        mom = momenta_of(direction)
        want0, scale = ref.basis_slice_triple(*hosts, dims, direction, None, None, parity)
        wantp = ref.basis_slice_triple(*hosts, dims, direction, None, mom, parity)[0] if mom else None
        results = {}
        for generic in ((False, True) if mfma else (False,)):
            # the forced generic form of an MFMA width list: no momenta and the first two momenta, once each (the generic
            # width lists go through everything in their own right)
            mom_g, again = (mom[:2], False) if generic else (mom, True)
            ctx.force_generic(generic)
            try:
                ctx.profile_reset()
                got0 = bc.basis_slice_triple(*lists, direction)
                assert _forms(ctx) == ((1, 0) if mfma and not generic else (0, 1)), what
                _check(got0[None], want0, scale, worst, what + (generic,))
                if again:  # the same bits on a second call
                    assert np.array_equal(_bits(bc.basis_slice_triple(*lists, direction)), _bits(got0)), what
                gotp = None
                if mom_g:
                    ctx.profile_reset()
                    gotp = bc.basis_slice_triple(*lists, direction, None, mom_g)
                    assert _forms(ctx) == ((len(mom_g), 0) if mfma and not generic else (0, len(mom_g))), what
                    _check(gotp, wantp[:len(mom_g)], scale, worst, what + (generic, "momenta"))
                    if again:
                        assert np.array_equal(_bits(bc.basis_slice_triple(*lists, direction, None, mom_g)), _bits(gotp)), what
                results[generic] = (got0, gotp)
            finally:
                ctx.force_generic(False)
        if len(results) == 2:  # the MFMA form against the generic one
            _close(results[False][0], results[True][0], scale, what)
            if mom:
                _close(results[False][1][:len(results[True][1])], results[True][1], scale, what)
    for f, bits in zip(fields, norm_bits):  # the operands are untouched
        assert np.array_equal(_bits(f.hermitian_dot(f)), bits)


@pytest.mark.parametrize("parity", [None, 0, 1], ids=["full", "even", "odd"])
@pytest.mark.parametrize("spec", MFMA_LISTS + GENERIC_LISTS, ids=_id)
def test_basis_slice_triple_main_sweep(bc, spec, parity):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    worst = [0.0]
    _sweep(bc, ctx, dims, spec, parity, worst, _is_mfma(spec))
    print(f"largest basis-slice-triple error on {dims}, {_id(spec)}: {worst[0]:.3e} of S")


@pytest.mark.parametrize("generic", [False, True], ids=["mfma", "generic"])
def test_identical_lists_are_antisymmetric_bit_for_bit(bc, generic):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    widths = [16, 32, 16]
    V = _fields(bc, ctx, widths, None, 520)
    mom = [[1, -1, 0, 0], [0, 0, 0, 0]]
    ctx.force_generic(generic)
    try:
        ctx.profile_reset()
        T = bc.basis_slice_triple(V, V, V, 3, None, mom)
        # 64 columns: 20 sorted triples of 4 blocks of 16 (MFMA), 120 of 8 blocks of 8 (generic), once per momentum
        prof = ctx.profile()["basis_slice_triple"]
        edge, tiles = (8, 120) if generic else (16, 20)
        assert prof["flops"] == 2 * tiles * 24.0 * edge ** 3 * ctx.V, prof
        assert T.shape == (2, 2, 64, 64, 64)
        for axes in ((0, 1, 3, 2, 4), (0, 1, 2, 4, 3), (0, 1, 4, 3, 2)):
            assert np.array_equal(T, -T.transpose(axes)), axes  # exact equality: only the sign of a zero may differ
        i = np.arange(64)
        for coincide in (T[:, :, i, i, :], T[:, :, i, :, i], T[:, :, :, i, i]):
            assert coincide.size == 2 * 2 * 64 * 64 and np.array_equal(_bits(coincide), _bits(np.zeros_like(coincide)))
        assert np.abs(T[:, :, 0, 1, 2]).min() > 0
        # three separately built arrays of the same handles: the same path, the same bits
        out = np.empty((2, 2, 64, 64, 64), dtype=np.complex128)
        arrs = [(ctypes.c_void_p * 3)(*[v.h for v in V]) for _ in range(3)]
        ns = np.ascontiguousarray([q + [0] * (4 - len(q)) for q in mom], dtype=np.intc)
        ctx.profile_reset()
        rc = ctx.lib.bcg_basis_slice_triple(arrs[0], 3, arrs[1], 3, arrs[2], 3, 3, 0, None, 2, ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert rc == 0
        assert ctx.profile()["basis_slice_triple"]["flops"] == prof["flops"]
        assert np.array_equal(_bits(out.transpose(0, 1, 4, 3, 2)), _bits(T))
        # a copy of the fields as B: the general path (every tile), the same numbers to tolerance
        W = [bc.block_fermion_field(ctx, w).upload(v.download()) for w, v in zip(widths, V)]
        ctx.profile_reset()
        G = bc.basis_slice_triple(V, W, V, 3, None, mom)
        full = (8 if generic else 4) ** 3
        assert ctx.profile()["basis_slice_triple"]["flops"] == 2 * full * 24.0 * edge ** 3 * ctx.V
        h = [v.download() for v in V]
        _, scale = ref.basis_slice_triple(h, h, h, dims, 3)
        _close(G, T, scale, "general path")
    finally:
        ctx.force_generic(False)


@pytest.mark.parametrize("spec", [([16], [16], [16]), ([16, 32, 16], IDENTICAL), ([1, 7, 12], [8], [3])], ids=_id)
def test_slice_lists(bc, spec):
    """One slice, two in descending order, all: a listed subset equals the matching blocks of the all-slices call bit for bit,
    and its profiled bytes are its share of the slices."""
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    for parity, direction in ((None, 2), (1, 0), (0, 3), (None, 0)):
        lists = _lists(bc, ctx, spec, parity, seed=540)
        L = dims[direction]
        mom = [[0, 1, 0, 0] if direction != 1 else [1, 0, 0, 0]]
        ctx.profile_reset()
        full = bc.basis_slice_triple(*lists, direction)
        bytes_full = ctx.profile()["basis_slice_triple"]["bytes"]
        fullp = bc.basis_slice_triple(*lists, direction, None, mom)
        assert full.shape[0] == L and bytes_full > 0
        for sl in ([L - 1], [L - 1, 0], list(range(L)), [1, 0, 2][:L]):
            ctx.profile_reset()
            got = bc.basis_slice_triple(*lists, direction, sl)
            assert ctx.profile()["basis_slice_triple"]["bytes"] * L == bytes_full * len(sl), (spec, direction, sl)
            assert np.array_equal(_bits(got), _bits(full[sl])), (spec, parity, direction, sl)
            gotp = bc.basis_slice_triple(*lists, direction, sl, mom)
            assert np.array_equal(_bits(gotp), _bits(fullp[:, sl])), (spec, parity, direction, sl)
        hosts = _host(lists)
        want, scale = ref.basis_slice_triple(*hosts, dims, direction, [L - 1, 0], mom, parity)
        _check(bc.basis_slice_triple(*lists, direction, [L - 1, 0], mom), want, scale, [0.0], (spec, parity, direction))


def test_basis_slice_triple_at_ragged_shapes(bc):
    """[5,3,2]: 15-site slices along 2, not a multiple of the 4-site step; odd extents; one non-zero momentum where the
    lattice has a second direction."""
    worst = [0.0]
    for dims, specs in (([5, 3, 2], (([16], [16], [16]), ([5], [5], [5]))), ([7, 5, 3, 3], (([32], [16], [16, 16]), ([16, 5], [16], [32, 3]))),
                        ([37], (([16], [16], [16]), ([1, 7, 12], [8], [3])))):
        nd = len(dims)

        def mom(direction, nd=nd):
            if nd == 1:
                return []
            q = [2, -1, 1, 4][:nd] + [0] * (4 - nd)
            q[direction] = 0
            return [q]

        for spec in specs:
            _sweep(bc, _ctx(bc, dims), dims, spec, None, worst, _is_mfma(spec), momenta_of=mom)
    print(f"largest basis-slice-triple error at ragged shapes: {worst[0]:.3e}")


@pytest.mark.parametrize("spec", [([16], [16], [16]), ([5], [16], [3])], ids=_id)
def test_basis_slice_triple_in_one_dimension(bc, spec):
    """[96]: a slice is one site.  n_mom = 0 and the zero momentum share the plan and, with all tables 1, the bits.  A half
    field holds every other slice: the others are exact zeros."""
    dims = [96]
    ctx = _ctx(bc, dims)
    worst = [0.0]
    for parity in (None, 0, 1):
        _sweep(bc, ctx, dims, spec, parity, worst, _is_mfma(spec), momenta_of=lambda d: [])
        lists = _lists(bc, ctx, spec, parity)
        plain = bc.basis_slice_triple(*lists, 0)
        zero = bc.basis_slice_triple(*lists, 0, None, [[0]])
        assert zero.shape == (1,) + plain.shape
        assert np.array_equal(_bits(zero[0]), _bits(plain)), (spec, parity)
        if parity is not None:
            other = plain[1 - parity::2]
            assert other.shape[0] == 48 and np.array_equal(_bits(other), _bits(np.zeros_like(other)))
            assert np.all(np.abs(plain[parity::2]).max(axis=(1, 2, 3)) > 0)
    print(f"largest basis-slice-triple error on {dims}, {_id(spec)}: {worst[0]:.3e}")


@pytest.mark.parametrize("spec", [([16], [16], [16]), ([16, 32, 16], IDENTICAL)], ids=_id)
@pytest.mark.parametrize("dims", [[16, 16, 8, 4], [16, 10, 7, 4]], ids=["2048", "tail"])
def test_several_blocks_per_slice_and_the_fold(bc, dims, spec):
    """One listed slice along 3: 2048 sites ([16,16,8,4]) or 1120 ([16,10,7,4], whose last chunk is short) walked by several
    blocks per tile (the plan aims at 1024 blocks), summed by the fold in block order.  n_mom = 0 and the explicit zero
    momentum: the same bits."""
    ctx = _ctx(bc, dims)
    lists = _lists(bc, ctx, spec, None, seed=560)
    hosts = _host(lists)
    worst = [0.0]
    mom = [[1, -2, 3, 0], [0, 0, 0, 0]]
    got = bc.basis_slice_triple(*lists, 3, [2], mom)
    want, scale = ref.basis_slice_triple(*hosts, dims, 3, [2], mom)
    _check(got, want, scale, worst, (dims, _id(spec)))
    plain = bc.basis_slice_triple(*lists, 3, [2])
    assert np.array_equal(_bits(plain), _bits(got[1]))
    assert np.array_equal(_bits(bc.basis_slice_triple(*lists, 3, [2], mom)), _bits(got))
    ctx.force_generic(True)
    try:
        _check(bc.basis_slice_triple(*lists, 3, [2], mom[:1]), want[:1], scale, worst, (dims, _id(spec), "generic"))
    finally:
        ctx.force_generic(False)
    print(f"largest basis-slice-triple error on {dims}, {_id(spec)}: {worst[0]:.3e}")


def test_covariance_under_a_rotation_of_the_columns(bc):
    """Three columns of a field of width 5 rotated per slice by Q(t) (bcg_basis_slice_rotate, Q = diag(Q3(t), 1, 1)): the
    determinant of the three columns is multiplied by det Q3(t) at every site, so T(t; 0, 1, 2) is.  Q3 unitary times a phase,
    so the columns' site norm N(x) = sqrt(sum_i |A_i(x)|^2) is unchanged and |det| <= N^3: 1e-12 of sum_x N(x)^3."""
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    rng = np.random.default_rng(7)
    for direction in (3, 0):
        (A,) = _fields(bc, ctx, [5], None, 580)
        L = dims[direction]
        before = bc.basis_slice_triple([A], [A], [A], direction)[:, 0, 1, 2]
        h = A.download()
        t = ref.coords(dims)[:, direction]
        N3 = np.array([(np.sqrt((np.abs(h[t == s, :3]) ** 2).sum(axis=(1, 2))) ** 3).sum() for s in range(L)])
        Q = np.zeros((L, 5, 5), dtype=np.complex128)
        dets = np.empty(L, dtype=np.complex128)
        for s in range(L):
            q3 = np.linalg.qr(rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3)))[0] * np.exp(0.3j * (s + 1))
            Q[s, :3, :3] = q3
            Q[s, 3, 3] = Q[s, 4, 4] = 1.0
            dets[s] = np.linalg.det(q3)
        bc.basis_slice_rotate([A], Q, direction)
        after = bc.basis_slice_triple([A], [A], [A], direction)[:, 0, 1, 2]
        assert np.all(np.abs(before) > 0)
        assert np.max(np.abs(after - dets * before) / N3) <= 1e-12, direction


def test_invalid_calls_leave_out_alone(bc):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    lib = ctx.lib
    v16 = bc.block_fermion_field(ctx, 16).setGaussian(1)
    v5 = bc.block_fermion_field(ctx, 5).setGaussian(2)
    v32 = [bc.block_fermion_field(ctx, 32).setGaussian(10 + k) for k in range(2)]
    vhalf = bc.block_fermion_field(ctx, 16, parity=1).setGaussian(6)
    foreign = bc.block_fermion_field(_ctx(bc, [37]), 16).setGaussian(7)
    out = np.full(2 * 2 * 21 * 21 * 21 + 8, 7.0 - 3.0j, dtype=np.complex128)
    poison = out.copy()
    dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = ctypes.POINTER(ctypes.c_int)

    def handles(*fields):
        return (ctypes.c_void_p * max(1, len(fields)))(*[f.h if f is not None else None for f in fields])

    def ints(*rows):
        arr = np.ascontiguousarray(rows, dtype=np.intc)
        return arr, arr.ctypes.data_as(ip)

    ok = ints([1, 0, 0, 0])
    two = ints([1, 0, 0, 0], [0, 1, 0, 4])
    sl = ints(1, 0)
    twice = ints(1, 1)
    outside = ints(0, 2)
    negative = ints(-1)
    good = handles(v16, v5)

    def call(A=good, na=2, B=good, nb=2, C=good, nc=2, d=3, n_slices=2, slices=sl[1], n_mom=1, momenta=ok[1], o=dp):
        return lib.bcg_basis_slice_triple(A, na, B, nb, C, nc, d, n_slices, slices, n_mom, momenta, o)

    invalid = {
        "na 0": dict(na=0), "nb -1": dict(nb=-1), "nc 0": dict(nc=0),
        "null A": dict(A=None), "null B": dict(B=None), "null C": dict(C=None),
        "null field": dict(B=handles(v16, None)), "null first field": dict(A=handles(None, v5)),
        "context": dict(C=handles(v16, foreign)), "mixed parities": dict(B=handles(v16, vhalf)),
        "a half list": dict(C=handles(vhalf), nc=1),
        "dir -1": dict(d=-1, n_mom=0, momenta=None), "dir ndim": dict(d=4, n_mom=0, momenta=None),
        "n_slices -1": dict(n_slices=-1), "null slices": dict(slices=None), "a slice twice": dict(slices=twice[1]),
        "a slice outside": dict(slices=outside[1]), "a negative slice": dict(n_slices=1, slices=negative[1]),
        "n_mom -1": dict(n_mom=-1), "dir component": dict(n_mom=2, momenta=two[1]), "null momenta": dict(momenta=None),
        "null out": dict(o=None),
    }
    for what, kw in invalid.items():
        assert call(**kw) == INVALID, what
        assert np.array_equal(_bits(out), _bits(poison)), what
    wide = handles(v32[0], v32[1], v5)
    many = bc.Context([2048])  # 2048 local slices x 4 tiles of 16^3: 2^25 entries of partials at one block each; 2^24 fit
    f16 = [bc.block_fermion_field(many, 16).setGaussian(20 + k) for k in range(2)]
    unsupported = {
        "a list of 69 columns": lambda: call(B=wide, nb=3),
        # 4 slices x 64^3 x 64 momenta = 2^26 fit; 65 momenta do not
        "more than 2^26 entries": lambda: lib.bcg_basis_slice_triple(handles(*v32), 2, handles(*v32), 2, handles(*v32), 2, 0, 0, None, 65,
                                                                       np.zeros((65, 4), dtype=np.intc).ctypes.data_as(ip), dp),
        "no block for every slice": lambda: many.lib.bcg_basis_slice_triple(handles(*f16), 2, handles(*f16), 2, handles(f16[0]), 1, 0, 0, None, 0,
                                                                            None, dp),
    }
    for what, f in unsupported.items():
        assert f() == UNSUPPORTED, what
        assert np.array_equal(_bits(out), _bits(poison)), what
    with pytest.raises(bc.BlockCGError):
        bc.basis_slice_triple([v16], [v16], [v16], 4)
    with pytest.raises(bc.BlockCGError):
        bc.basis_slice_triple([v16], [v16], [v16], 3, [])
    with pytest.raises(bc.BlockCGError):
        bc.basis_slice_triple([v16], [v16], [v16], 3, None, [])
    # and the good call fills what it owns and no more
    assert call() == 0
    n = 2 * 21 ** 3
    assert not np.any(_bits(out[:n]) == _bits(poison[:n]))
    assert np.array_equal(_bits(out[n:]), _bits(poison[n:]))


def test_divided_lattice_without_a_comm(bc):
    """One rank of a (2,1,1,1) grid with no bcg_comm attached: BCG_ERR_COMM before anything is launched."""
    ctx = bc.Context([4, 2, 4, 2], grid=[2, 1, 1, 1], coords=[0, 0, 0, 0])
    for parity in (None, 0):
        V = [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(1 + w) for w in (16, 5)]
        poison = np.full(2 * 21 ** 3, 7.0 - 3.0j)
        out = poison.copy()
        Vh = (ctypes.c_void_p * 2)(*[v.h for v in V])
        assert ctx.lib.bcg_basis_slice_triple(Vh, 2, Vh, 2, Vh, 2, 3, 0, None, 0, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == COMM
        assert np.array_equal(_bits(out), _bits(poison))


def test_cpp_basis_slice_triple_layer_runs(bc):
    """tests/cpp/basis_slice_triple_probe.cpp, built by the recipe of tests/test_cpp_dropin.py: blockcg/basis.hpp's
    basis_slice_triple on the device, checked inside the probe against host sums in long double."""
    from test_cpp_dropin import _compile
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "basis_slice_triple_probe.cpp"), "basis_slice_triple_probe")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "BASIS_SLICE_TRIPLE_PROBE_OK" and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_baryon_elemental_example(bc):
    """examples/baryon_elemental.cpp on 4^4: a Laplacian basis, its elementals (antisymmetry defect exactly 0) and those with a
    displaced third operand, and the covariance of T(0, 1, 2) under a rotation of the basis."""
    from test_cpp_dropin import _compile
    exe = _compile(os.path.join(ROOT, "examples", "baryon_elemental.cpp"), "baryon_elemental")
    r = subprocess.run([exe, "4", "4", "4", "4"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "BARYON_ELEMENTAL_OK" in r.stdout and "antisymmetry defect 0\n" in r.stdout, r.stdout + r.stderr
