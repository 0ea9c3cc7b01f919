"""The in-place rotation by slice (include/blockcg_hip.h: bcg_basis_slice_rotate) against its numpy restatement
(tests/basis_slice_rotate_ref.py): every direction, full fields and both half parities, all slices / one / two in descending
order, the width lists of either form, random and upper-triangular matrices; permutations and the identity bit for bit; the
slices that are not listed (bit-identical, over a NaN start); the MFMA form against the generic one; the form from the profile
counters; the same bits on a second call; a bystander field; all slices with one matrix against basis_rotate; shapes where
the walk can go wrong; the profiled bytes; the error returns.

Tolerance: TOL_KERNEL by conftest.rel_err (relative Frobenius error), exactly as tests/test_lowmodes.py applies it to
basis_rotate: the sums are K <= 64 terms long in double precision."""
import ctypes

import numpy as np
import pytest

import basis_slice_rotate_ref as ref
from basis_ref import concat
from basis_slice_axpy_ref import slice_of_sites
from conftest import TOL_KERNEL, rel_err

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 2
MFMA_WIDTHS = ([16], [32], [32, 16], [16, 32, 16], [16, 16, 16, 16])
GENERIC_WIDTHS = ([5], [1, 7, 12], [8, 8], [32, 3], [16, 5], [31, 32, 1])


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
    return np.ascontiguousarray(x).view(np.uint64)  # integers: a NaN equals itself


def _slice_sets(L):
    """all slices / one slice / two non-adjacent slices in descending order (L = 2: the two there are)"""
    return (None, [L - 1], [L - 1, L - 3] if L >= 4 else [L - 1, 0])


def _matrices(rng, S, K, kind="random"):
    Q = rng.standard_normal((S, K, K)) + 1j * rng.standard_normal((S, K, K))
    return np.triu(Q) if kind == "upper" else Q


def _fields(bc, ctx, widths, parity, seed=700):
    return [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(seed + k) for k, w in enumerate(widths)]


def _forms(ctx):
    p = ctx.profile()
    return p.get("basis_slice_rotate_mfma", {}).get("count", 0), p.get("basis_slice_rotate_generic", {}).get("count", 0)


def _one(bc, ctx, V, Vh, Q, dims, direction, slices, parity, worst, what, both_forms=True, nan_rest=True):
    """One call in both forms against the restatement and each other, twice from the same start.  nan_rest: the sites of the
    slices that are not listed start as NaN, so a read of them would show in a listed slice and a write in their bits."""
    L = dims[direction]
    listed = np.isin(slice_of_sites(dims, direction, parity), range(L) if slices is None else slices)
    start = [v.copy() for v in Vh]
    if nan_rest:
        for v in start:
            v[~listed] = np.nan
    want = concat(ref.basis_slice_rotate(start, Q, dims, direction, slices, parity))
    mfma = all(w in (16, 32) for w in (v.shape[1] for v in Vh))
    outs = {}
    for generic in ((False, True) if both_forms else (False,)):
        ctx.force_generic(generic)
        try:
            res = []
            for _ in range(2):
                for v, h in zip(V, start):
                    v.upload(h)
                ctx.profile_reset()
                bc.basis_slice_rotate(V, Q, direction, slices)
                res.append(concat([v.download() for v in V]))
            assert _forms(ctx) == ((1, 0) if mfma and not generic else (0, 1)), (what, generic)
        finally:
            ctx.force_generic(False)
        out, again = res
        e = rel_err(out[listed], want[listed]) if listed.any() else 0.0
        worst[0] = max(worst[0], e)
        assert e <= TOL_KERNEL, (what, generic, e)
        assert not np.isnan(out[listed]).any(), (what, generic)
        assert np.array_equal(_bits(again), _bits(out)), (what, generic)  # the same bits on a second call
        assert np.array_equal(_bits(out[~listed]), _bits(concat(start)[~listed])), (what, generic)  # the others keep their bits
        outs[generic] = out
    if both_forms and listed.any():
        assert rel_err(outs[False][listed], outs[True][listed]) <= TOL_KERNEL, what
    return outs[False]


def _sweep(bc, ctx, dims, widths, parity, worst, directions=None, slice_sets=_slice_sets, kinds=("random", "upper")):
    V = _fields(bc, ctx, widths, parity)
    Vh = [v.download() for v in V]
    bystander = bc.block_fermion_field(ctx, 7, parity=parity).setGaussian(3)
    by_bits = _bits(bystander.download()).copy()
    rng = np.random.default_rng(47)
    K = sum(widths)
    for direction in (range(len(dims)) if directions is None else directions):
        L = dims[direction]
        for slices in slice_sets(L):
            for kind in kinds:
                Q = _matrices(rng, L if slices is None else len(slices), K, kind)
                _one(bc, ctx, V, Vh, Q, dims, direction, slices, parity, worst, (tuple(dims), tuple(widths), parity, direction, slices, kind))
    assert np.array_equal(_bits(bystander.download()), by_bits)


@pytest.mark.parametrize("parity", [None, 0, 1], ids=["full", "even", "odd"])
@pytest.mark.parametrize("widths", MFMA_WIDTHS + GENERIC_WIDTHS, ids=lambda w: "+".join(map(str, w)))
def test_basis_slice_rotate_main_sweep(bc, widths, parity):
    dims = [4, 2, 4, 2]
    worst = [0.0]
    _sweep(bc, _ctx(bc, dims), dims, widths, parity, worst)
    print(f"largest basis-slice-rotate error on {dims}, V = {widths}, parity {parity}: {worst[0]:.3e}")


@pytest.mark.parametrize("widths", ([16, 32, 16], [32, 3], [1, 7, 12]), ids=lambda w: "+".join(map(str, w)))
def test_permutations_and_the_identity_move_columns_bit_for_bit(bc, widths):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    K = sum(widths)
    rng = np.random.default_rng(53)
    for parity in (None, 1):
        V = _fields(bc, ctx, widths, parity, seed=720)
        Vh = [v.download() for v in V]
        W = concat(Vh)
        for direction in (0, 3):
            L = dims[direction]
            perms = [rng.permutation(K) if t % 2 == 0 else np.arange(K) for t in range(L)]  # odd slices: the identity
            Q = np.zeros((L, K, K), dtype=np.complex128)
            for t, p in enumerate(perms):
                Q[t, p, np.arange(K)] = 1.0  # column j of the result is column p[j]
            for generic in (False, True):
                ctx.force_generic(generic)
                try:
                    for v, h in zip(V, Vh):
                        v.upload(h)
                    bc.basis_slice_rotate(V, Q, direction)
                finally:
                    ctx.force_generic(False)
                out = concat([v.download() for v in V])
                t_of = slice_of_sites(dims, direction, parity)
                for t, p in enumerate(perms):
                    assert np.array_equal(_bits(out[t_of == t]), _bits(W[t_of == t][:, p])), (widths, parity, direction, t, generic)


@pytest.mark.parametrize("widths", ([16, 32, 16], [1, 7, 12], [32]), ids=lambda w: "+".join(map(str, w)))
def test_all_slices_with_one_matrix_is_basis_rotate(bc, widths):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    K = sum(widths)
    Q = _matrices(np.random.default_rng(59), 1, K)[0]
    for parity in (None, 0):
        V = _fields(bc, ctx, widths, parity, seed=740)
        Vh = [v.download() for v in V]
        bc.basis_rotate(V, Q)
        want = concat([v.download() for v in V])
        for direction in range(4):
            for v, h in zip(V, Vh):
                v.upload(h)
            bc.basis_slice_rotate(V, np.repeat(Q[None], dims[direction], axis=0), direction)
            assert rel_err(concat([v.download() for v in V]), want) <= TOL_KERNEL, (widths, parity, direction)


@pytest.mark.parametrize("widths", ([16], [1, 7]), ids=["mfma", "generic"])
def test_basis_slice_rotate_in_one_dimension(bc, widths):
    """[96]: a slice is one site, 3 rows, less than one step of 16 rows; a half field holds every other slice, so a listed
    slice may hold no site at all."""
    dims = [96]
    worst = [0.0]
    for parity in (None, 0, 1):
        _sweep(bc, _ctx(bc, dims), dims, widths, parity, worst, slice_sets=lambda L: (None, [L - 1], [L - 2, 5, 40]), kinds=("random",))
    print(f"largest basis-slice-rotate error on {dims}, V = {widths}: {worst[0]:.3e}")


def test_basis_slice_rotate_at_ragged_shapes(bc):
    """Row counts that steps of 16 rows do not divide, odd extents."""
    worst = [0.0]
    for dims, widths in (([5, 3, 2], [16, 32]), ([7, 5, 3, 3], [32, 3]), ([37], [5]), ([5, 3, 2], [16, 16, 16, 16])):
        _sweep(bc, _ctx(bc, dims), dims, widths, None, worst, kinds=("random",))
    print(f"largest basis-slice-rotate error at ragged shapes: {worst[0]:.3e}")


def test_basis_slice_rotate_with_several_blocks_per_slice(bc):
    """K = 64.  [16,16,16,4] as [16] x 4: along direction 3 a slice has 12288 rows, 192 blocks of 64 rows; along direction 0
    3072 rows, 48 blocks per slice in runs of 3 rows, so every step of 16 rows straddles sites and runs.  [16,10,7,4] as
    [32] x 2: along direction 3 a slice has 3360 rows, 53 blocks, the last a tail chunk of 32 rows; along direction 0 630 rows,
    10 blocks, the last of 54 rows: a step with rows that are not live."""
    rng = np.random.default_rng(61)
    worst = [0.0]
    for dims, widths, slice_sets in (([16, 16, 16, 4], [16, 16, 16, 16], (None, [2])), ([16, 10, 7, 4], [32, 32], ([3, 1],))):
        ctx = _ctx(bc, dims)
        V = _fields(bc, ctx, widths, None, seed=760)
        Vh = [v.download() for v in V]
        for direction in (3, 0):
            for slices in slice_sets:
                Q = _matrices(rng, dims[direction] if slices is None else len(slices), 64)
                _one(bc, ctx, V, Vh, Q, dims, direction, slices, None, worst, (dims, widths, direction, slices), both_forms=slices is not None)
    print(f"largest basis-slice-rotate error with several blocks per slice: {worst[0]:.3e}")


@pytest.mark.parametrize("widths,generic", [([32, 32], False), ([16, 5], False), ([32, 32], True)])
def test_profiled_bytes_and_forms(bc, widths, generic):
    """One listed slice moves exactly 1 / L_dir of the bytes of the all-slices call: 96 K bytes per listed site."""
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    V = _fields(bc, ctx, widths, None, seed=780)
    K = sum(widths)
    rng = np.random.default_rng(67)
    form = (1, 0) if not generic and all(w in (16, 32) for w in widths) else (0, 1)
    ctx.force_generic(generic)
    try:
        for direction in (0, 3):
            L = dims[direction]
            ctx.profile_reset()
            bc.basis_slice_rotate(V, _matrices(rng, L, K) / K, direction)
            assert _forms(ctx) == form
            p_all = ctx.profile()
            ctx.profile_reset()
            bc.basis_slice_rotate(V, _matrices(rng, 1, K) / K, direction, [L - 1])
            assert _forms(ctx) == form
            p_one = ctx.profile()
            assert p_all["basis_slice_rotate"]["bytes"] == 96.0 * K * V[0].V
            assert p_one["basis_slice_rotate"]["bytes"] * L == p_all["basis_slice_rotate"]["bytes"]
            assert "basis_rotate" not in p_one and "basis_slice_axpy" not in p_one
    finally:
        ctx.force_generic(False)


def test_invalid_and_unsupported_calls_leave_v_alone(bc):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    lib = ctx.lib
    v16 = bc.block_fermion_field(ctx, 16).setGaussian(1)
    v5 = bc.block_fermion_field(ctx, 5).setGaussian(2)
    wide = [bc.block_fermion_field(ctx, 32).setGaussian(10 + k) for k in range(2)]
    v1 = bc.block_fermion_field(ctx, 1).setGaussian(4)
    vhalf = bc.block_fermion_field(ctx, 16, parity=1).setGaussian(6)
    foreign = bc.block_fermion_field(_ctx(bc, [37]), 16).setGaussian(7)
    watched = [v16, v5, v1, vhalf] + wide
    before = [_bits(f.download()).copy() for f in watched]
    Q = np.ones((4, 65, 65), dtype=np.complex128)
    qp = Q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bad = Q.copy()
    bad.flat[500] = np.nan  # K = 21: a call reads 441 entries per listed slice, so 500 is in the second matrix, 440 in the first
    nanp = bad.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bad2 = Q.copy()
    bad2.flat[440] = complex(0.0, np.inf)
    infp = bad2.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = ctypes.POINTER(ctypes.c_int)

    def handles(*fields):
        return (ctypes.c_void_p * max(1, len(fields)))(*[f.h if f is not None else None for f in fields])

    def ints(*values):
        arr = np.ascontiguousarray(values, dtype=np.intc)
        return arr, arr.ctypes.data_as(ip)

    good = handles(v16, v5)
    keep = [ints(1), ints(0, 1), ints(2), ints(0, 0), ints(-1), ints(0, 3, 0)]
    one, two, past, twice, negative, thrice = [k[1] for k in keep]
    cases = {
        "nv 0": (INVALID, (good, 0, 3, 1, one, qp)),
        "nv -1": (INVALID, (good, -1, 3, 1, one, qp)),
        "null V": (INVALID, (None, 2, 3, 1, one, qp)),
        "null field": (INVALID, (handles(v16, None), 2, 3, 1, one, qp)),
        "null Q": (INVALID, (good, 2, 3, 1, one, None)),
        "context": (INVALID, (handles(v16, foreign), 2, 3, 1, one, qp)),
        "parity": (INVALID, (handles(v16, vhalf), 2, 3, 1, one, qp)),
        "field twice": (INVALID, (handles(v16, v5, v16), 3, 3, 1, one, qp)),
        "Q nan": (INVALID, (good, 2, 3, 2, two, nanp)),
        "Q inf": (INVALID, (good, 2, 3, 0, None, infp)),
        "dir -1": (INVALID, (good, 2, -1, 0, None, qp)),
        "dir ndim": (INVALID, (good, 2, 4, 0, None, qp)),
        "n_slices -1": (INVALID, (good, 2, 3, -1, one, qp)),
        "null slices": (INVALID, (good, 2, 3, 1, None, qp)),
        "slice L": (INVALID, (good, 2, 3, 1, past, qp)),
        "slice -1": (INVALID, (good, 2, 3, 1, negative, qp)),
        "slice twice": (INVALID, (good, 2, 3, 2, twice, qp)),
        "slice twice, apart": (INVALID, (good, 2, 0, 3, thrice, qp)),
        "65 columns": (UNSUPPORTED, (handles(wide[0], wide[1], v1), 3, 3, 1, one, qp)),
    }
    for what, (code, args) in cases.items():
        assert lib.bcg_basis_slice_rotate(*args) == code, what
        for f, bits in zip(watched, before):
            assert np.array_equal(_bits(f.download()), bits), what
    with pytest.raises(bc.BlockCGError):
        bc.basis_slice_rotate([v16, v5], np.ones((2, 21, 21)), 4)
    with pytest.raises(ValueError):
        bc.basis_slice_rotate([v16, v5], np.ones((2, 21, 21)), 3, [1])
    # and the good call changes V on the listed slices only
    assert lib.bcg_basis_slice_rotate(good, 2, 3, 1, one, Q[:1, :21, :21].copy().ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
    after = v16.download()
    t_of = slice_of_sites(dims, 3)
    was = before[0].view(np.complex128).reshape(after.shape)  # v16
    assert np.array_equal(_bits(after[t_of != 1]), _bits(was[t_of != 1])) and not np.array_equal(_bits(after[t_of == 1]), _bits(was[t_of == 1]))
