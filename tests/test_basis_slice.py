"""Per-slice products with a basis of another width (include/blockcg_hip.h: bcg_basis_slice_dot) against their numpy
restatement (tests/basis_slice_ref.py): every direction, width class of either form and parity, momenta that are negative and
beyond the extents; against basis_dot (the sum over the slices) and slice_gram (a basis of one field of b's width); the same
bits on a second call; the MFMA form against the generic one; the launch plan by its launch counts; the error returns;
blockcg/basis.hpp and examples/perambulator.cpp on the device.

Tolerance: EPS_DOT = 1e-13 relative to sqrt(|V_i|^2_slice |b_j|^2_slice) per entry, the bound of tests/test_slice_gram.py for
the same walk on the same lattices (sums of at most 12288 terms; the phases have modulus 1 to a few ulp).  Entries whose
scale is 0 -- slices a half field holds no site of -- are exact zeros.

The plan (blockcg_amd/csrc/kernels_basis_slice.hpp), as the launch counts below use it.  MFMA form, m = 16: n_mom <= 1 groups
of 4 blocks of 16 columns and pc = 1; n_mom 2, 3: 2 blocks, pc = 2; n_mom >= 4: 1 block, pc = 4.  m = 32: n_mom <= 1 groups of
2 blocks, pc = 1; n_mom >= 2: 1 block, pc = 2.  Generic form: consecutive generic fields up to 32 columns and 8 fields, pc = 2
from two momenta on.  A group is launched ceil(max(n_mom, 1) / pc) times."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import basis_slice_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

EPS_DOT = 1e-13
INVALID, COMM = 1, 5
MOMENTA = ([1, 0, 0, 0], [-1, 1, 0, 1], [2, 1, 3, 1], [5, -3, 0, 2])  # those of tests/test_slice_gram.py
PAIRS = (([5], 1), ([1, 7, 12], 5), ([8, 8], 8), ([32, 3], 12), ([16], 16), ([32], 16), ([16], 32), ([32], 32),
         ([16, 32, 16], 16), ([16, 5], 16), ([32] * 5, 16))


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
    """MOMENTA and their negatives, the component along `direction` and beyond ndim set to 0."""
    out = []
    for sign in (1, -1):
        for n in MOMENTA:
            q = [sign * v if mu < ndim else 0 for mu, v in enumerate(n)]
            q[direction] = 0
            out.append(q)
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.float64)


def _operands(bc, ctx, widths, m, parity, seed=300):
    V = [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(seed + k) for k, w in enumerate(widths)]
    b = bc.block_fermion_field(ctx, m, parity=parity).setGaussian(seed + 50)
    return V, b


def _forms(ctx):
    p = ctx.profile()
    return p.get("basis_slice_form_mfma", {}).get("count", 0), p.get("basis_slice_form_generic", {}).get("count", 0)


def _check(got, want, scale, worst, what):
    """got, want [P, L, K, m]; scale [L, K, m].  Slices a half field holds no site of: exact zeros."""
    assert got.shape == want.shape, what
    sc = np.broadcast_to(scale, got.shape)
    assert np.array_equal(got[sc == 0], np.zeros_like(got[sc == 0])), what
    held = sc > 0
    err = float(np.max(np.abs(got - want)[held] / sc[held]))
    print(f"{what}: {err:.3e}")
    worst[0] = max(worst[0], err)
    assert err <= EPS_DOT, (what, err)


def _sweep(bc, ctx, dims, widths, m, parity, worst, momenta_of=_momenta, directions=None):
    V, b = _operands(bc, ctx, widths, m, parity)
    Vh, bh = [v.download() for v in V], b.download()
    norm_bits = [_bits(f.hermitian_dot(f)).copy() for f in V + [b]]
    whole = bc.basis_dot(V, b)
    W = np.concatenate(Vh, axis=1)
    total = np.sqrt(np.outer((np.abs(W) ** 2).sum(axis=(0, 2)), (np.abs(bh) ** 2).sum(axis=(0, 2))))
    for direction in (range(len(dims)) if directions is None else directions):
        what = (tuple(dims), tuple(widths), m, parity, direction)
        mom = momenta_of(direction)
        want0, scale = ref.basis_slice_dot(Vh, bh, dims, direction, None, parity)
        wantp = ref.basis_slice_dot(Vh, bh, dims, direction, mom, parity)[0] if mom else None
        results = {}
        for generic in (False, True):
            ctx.force_generic(generic)
            got0 = bc.basis_slice_dot(V, b, direction)
            _check(got0[None], want0, scale, worst, what + (generic,))
            assert np.array_equal(_bits(bc.basis_slice_dot(V, b, direction)), _bits(got0)), what  # the same bits again
            assert np.max(np.abs(got0.sum(axis=0) - whole) / total) <= EPS_DOT, what  # the sum over the slices: basis_dot
            gotp = None
            if mom:
                gotp = bc.basis_slice_dot(V, b, direction, mom)
                _check(gotp, wantp, scale, worst, what + (generic, "momenta"))
                assert np.array_equal(_bits(bc.basis_slice_dot(V, b, direction, mom)), _bits(gotp)), what
            results[generic] = (got0, gotp)
        ctx.force_generic(False)
        # the MFMA form (where the widths select it) against the generic one
        held = scale > 0
        assert np.max(np.abs(results[False][0] - results[True][0])[held] / scale[held]) <= EPS_DOT, what
        if mom:
            sc = np.broadcast_to(scale, results[False][1].shape)
            assert np.max(np.abs(results[False][1] - results[True][1])[sc > 0] / sc[sc > 0]) <= EPS_DOT, what
    for f, bits in zip(V + [b], norm_bits):  # the operands are untouched
        assert np.array_equal(_bits(f.hermitian_dot(f)), bits)


@pytest.mark.parametrize("widths,m", PAIRS, ids=[f"{'+'.join(map(str, w))}x{m}" for w, m in PAIRS])
def test_basis_slice_main_sweep(bc, widths, m):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    worst = [0.0]
    for parity in (None, 0, 1):
        _sweep(bc, ctx, dims, widths, m, parity, worst)
    print(f"largest basis-slice error on {dims}, V = {widths}, m = {m}: {worst[0]:.3e} of |V_i||b_j| per slice")


@pytest.mark.parametrize("m", [1, 5, 8, 12, 16, 32])
def test_a_basis_of_one_field_of_the_same_width_is_slice_gram(bc, m):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    for parity in (None, 0, 1):
        (a,), b = _operands(bc, ctx, [m], m, parity)
        ah, bh = a.download(), b.download()
        for direction in range(4):
            mom = _momenta(direction)
            _, scale = ref.basis_slice_dot([ah], bh, dims, direction, None, parity)
            held = scale > 0
            d0 = np.abs(bc.basis_slice_dot([a], b, direction) - a.slice_gram(b, direction))
            assert np.all(d0[~held] == 0) and np.max(d0[held] / scale[held]) <= EPS_DOT, (m, parity, direction)
            dp = np.abs(bc.basis_slice_dot([a], b, direction, mom) - a.slice_gram(b, direction, mom))
            sc = np.broadcast_to(scale, dp.shape)
            assert np.all(dp[sc == 0] == 0) and np.max(dp[sc > 0] / sc[sc > 0]) <= EPS_DOT, (m, parity, direction)


@pytest.mark.parametrize("widths,m", [([16], 16), ([1, 7], 5)], ids=["mfma", "generic"])
def test_basis_slice_in_one_dimension(bc, widths, m):
    """[96]: a slice is one site, 3 rows, less than one quad of the MFMA kernel.  n_mom = 0 and the zero momentum given
    explicitly are both pc = 1, so they share one plan, and with all tables 1 the phase multiplication is exact: the same
    bits.  A half field holds every other slice: the others are exact zeros."""
    dims = [96]
    ctx = _ctx(bc, dims)
    worst = [0.0]
    for parity in (None, 0, 1):
        _sweep(bc, ctx, dims, widths, m, parity, worst, momenta_of=lambda d: [])
        V, b = _operands(bc, ctx, widths, m, parity)
        plain = bc.basis_slice_dot(V, b, 0)
        zero = bc.basis_slice_dot(V, b, 0, [[0]])
        assert zero.shape == (1,) + plain.shape
        assert np.array_equal(_bits(zero[0]), _bits(plain)), (widths, m, parity)
        if parity is not None:
            other = plain[1 - parity::2]
            assert other.shape[0] == 48 and np.array_equal(_bits(other), _bits(np.zeros_like(other)))
            assert np.all(np.abs(plain[parity::2]).max(axis=(1, 2)) > 0)
    print(f"largest basis-slice error on {dims}, V = {widths}, m = {m}: {worst[0]:.3e}")


def test_basis_slice_at_ragged_shapes(bc):
    """Row counts that quads of 4 and chunks of 16 rows do not divide, odd extents; one non-zero momentum where the lattice
    has a second direction."""
    worst = [0.0]
    for dims, widths, m in (([5, 3, 2], [16, 32], 16), ([7, 5, 3, 3], [32, 3], 12), ([37], [5], 5)):
        nd = len(dims)

        def mom(direction, nd=nd):
            if nd == 1:
                return []
            q = [2, -1, 1, 4][:nd] + [0] * (4 - nd)
            q[direction] = 0
            return [q]

        _sweep(bc, _ctx(bc, dims), dims, widths, m, None, worst, momenta_of=mom)
    print(f"largest basis-slice error at ragged shapes: {worst[0]:.3e}")


@pytest.mark.parametrize("widths,m", [([32, 32, 16], 16), ([32, 16], 32)], ids=["m16", "m32"])
def test_basis_slice_on_8x8x8x8(bc, widths, m):
    """Three momenta, the zero one last.  Its block is bit-identical to the call without momenta: the plans differ in the
    group (m = 16: 4 blocks without momenta, 2 blocks and pc = 2 with three; m = 32: 2 blocks, then 1 block and pc = 2) but
    both have 1024 entries per block, so the budgets are 1024 and 1023 blocks, 128 and 127 per slice, both cut to the slice's
    rows / 64 (24, 12 for a half field along direction 3): the same blocks per slice and chunk, and the rows of an entry are
    added in the same order whatever group its column is in."""
    dims = [8, 8, 8, 8]
    ctx = _ctx(bc, dims)
    worst = [0.0]
    moms = {0: [[0, 1, 0, 0], [0, -1, 2, 9], [0, 0, 0, 0]], 3: [[1, 0, 0, 0], [-1, 2, 9, 0], [0, 0, 0, 0]]}
    for parity in (None, 1):
        V, b = _operands(bc, ctx, widths, m, parity)
        Vh, bh = [v.download() for v in V], b.download()
        for direction in (0, 3):
            got = bc.basis_slice_dot(V, b, direction, moms[direction])
            want, scale = ref.basis_slice_dot(Vh, bh, dims, direction, moms[direction], parity)
            _check(got, want, scale, worst, (widths, m, parity, direction))
            assert np.array_equal(_bits(got[2]), _bits(bc.basis_slice_dot(V, b, direction)))
    print(f"largest basis-slice error on {dims}, V = {widths}, m = {m}: {worst[0]:.3e}")


@pytest.mark.parametrize("dims,widths,m", [([16, 16, 16, 4], [32, 32], 16), ([16, 16, 8, 4], [32], 32)], ids=["m16", "m32"])
def test_basis_slice_with_several_blocks_per_slice(bc, dims, widths, m):
    """Three momenta are taken two per launch at both widths (2 + 1).  [16,16,16,4], m = 16: direction 3 has 192 blocks per
    slice of 12288 rows, direction 0 has 48 per slice of 3072 rows; [16,16,8,4], m = 32: 96 per slice of 6144 rows and 24 per
    slice of 1536 rows; chunks of 64 rows in all four.  Against numpy on the whole field."""
    ctx = _ctx(bc, dims)
    V, b = _operands(bc, ctx, widths, m, None, seed=320)
    Vh, bh = [v.download() for v in V], b.download()
    worst = [0.0]
    for direction, moms in ((3, [[1, 0, 0, 0], [-2, 3, 17, 0], [0, 5, -1, 0]]), (0, [[0, 1, 0, 0], [0, 3, 17, -2], [0, 0, 5, -1]])):
        got = bc.basis_slice_dot(V, b, direction, moms)
        want, scale = ref.basis_slice_dot(Vh, bh, dims, direction, moms)
        _check(got, want, scale, worst, (dims, m, direction))
        assert np.array_equal(_bits(bc.basis_slice_dot(V, b, direction, moms)), _bits(got))
        got0 = bc.basis_slice_dot(V, b, direction)
        want0, _ = ref.basis_slice_dot(Vh, bh, dims, direction)
        _check(got0[None], want0, scale, worst, (dims, m, direction, "no momenta"))
    print(f"largest basis-slice error on {dims}, m = {m}: {worst[0]:.3e}")


# (widths of V, m, n_mom, bcg_force_generic, (MFMA launches, generic launches)), by the rule in the module docstring
PLAN = (
    ([32, 32], 16, 0, False, (1, 0)),          # 4 blocks, one group: the launch of basis_dot
    ([32, 32], 16, 1, False, (1, 0)),          # the same group with the phase arithmetic
    ([32, 32], 16, 3, False, (4, 0)),          # pc = 2: groups 32 | 32, momenta 2 + 1
    ([32, 32], 16, 4, False, (4, 0)),          # pc = 4: four groups of one block
    ([32, 32], 16, 5, False, (8, 0)),          # pc = 4: four groups, momenta 4 + 1 (launches with pc = 4 and pc = 1)
    ([16, 32, 16], 16, 2, False, (2, 0)),      # pc = 2: 16 32a | 32b 16 -- the 32-wide field is split across two launches
    ([32] * 5, 16, 0, False, (3, 0)),          # 10 blocks: 4 | 4 | 2
    ([32, 16], 32, 0, False, (2, 0)),          # m = 32: 2 blocks per group: 32 | 16
    ([32, 16], 32, 3, False, (6, 0)),          # m = 32, pc = 2: three groups of one block, momenta 2 + 1
    ([16, 5, 32], 16, 0, False, (2, 1)),       # the forms alternate: 16 | 5 | 32
    ([16, 5, 32], 16, 4, False, (3, 2)),       # MFMA pc = 4: 16 | 32a | 32b once each; generic pc = 2: 5 twice
    ([12, 12, 12], 5, 3, False, (0, 4)),       # generic: 12 12 | 12, momenta 2 + 1
    ([32, 32], 16, 2, True, (0, 2)),           # bcg_force_generic: 32 | 32, pc = 2
)


@pytest.mark.parametrize("widths,m,n_mom,generic,forms", PLAN)
def test_launch_plan(bc, widths, m, n_mom, generic, forms):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    V, b = _operands(bc, ctx, widths, m, None, seed=340)
    mom = ([[1, 0, 0, 0], [0, 1, 2, 0], [0, 0, 0, 0], [3, 1, 1, 0], [-1, 0, 5, 0]][:n_mom]) or None
    ctx.force_generic(generic)
    try:
        ctx.profile_reset()
        got = bc.basis_slice_dot(V, b, 3, mom)
        assert _forms(ctx) == forms
    finally:
        ctx.force_generic(False)
    want, scale = ref.basis_slice_dot([v.download() for v in V], b.download(), dims, 3, mom)
    _check(got if mom else got[None], want, scale, [0.0], (widths, m, n_mom))


def test_the_group_shrinks_where_the_scratch_is_short(bc):
    """[2048] along direction 0: 2048 slices of 3 rows need 2048 blocks, the half of the scratch holds 2^20 entries.  V = 2 x 32
    at m = 16 without momenta: groups of 4 and of 3 blocks (1024 and 768 entries per block) leave 1024 and 1365 blocks, 2
    blocks leave 2048: two launches.  With one momentum the tables take 3 entries, 2 blocks leave 2047: four launches of 1."""
    dims = [2048]
    ctx = _ctx(bc, dims)
    V, b = _operands(bc, ctx, [32, 32], 16, None, seed=360)
    Vh, bh = [v.download() for v in V], b.download()
    want, scale = ref.basis_slice_dot(Vh, bh, dims, 0)
    for mom, forms in ((None, (2, 0)), ([[0]], (4, 0))):
        ctx.profile_reset()
        got = bc.basis_slice_dot(V, b, 0, mom)
        assert _forms(ctx) == forms, mom
        _check(got if mom else got[None], want, scale, [0.0], (dims, mom))


@pytest.mark.parametrize("w", range(1, 33))
def test_every_width(bc, w):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    mom = [[1, -1, 3, 0]]
    for widths, m in (([w], 5), ([12], w)):
        V, b = _operands(bc, ctx, widths, m, None, seed=380)
        got = bc.basis_slice_dot(V, b, 3, mom)
        want, scale = ref.basis_slice_dot([v.download() for v in V], b.download(), dims, 3, mom)
        _check(got, want, scale, [0.0], (widths, m))


def test_invalid_calls_leave_out_alone(bc):
    dims = [4, 2, 4, 2]
    ctx = _ctx(bc, dims)
    lib = ctx.lib
    v16 = bc.block_fermion_field(ctx, 16).setGaussian(1)
    v5 = bc.block_fermion_field(ctx, 5).setGaussian(2)
    b = bc.block_fermion_field(ctx, 8).setGaussian(3)
    half = bc.block_fermion_field(ctx, 8, parity=0).setGaussian(5)
    vhalf = bc.block_fermion_field(ctx, 16, parity=1).setGaussian(6)
    foreign = bc.block_fermion_field(_ctx(bc, [37]), 16).setGaussian(7)
    out = np.full((2, 2, 8, 21), 7.0 - 3.0j, dtype=np.complex128)
    poison = out.copy()
    dp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = ctypes.POINTER(ctypes.c_int)

    def handles(*fields):
        return (ctypes.c_void_p * max(1, len(fields)))(*[f.h if f is not None else None for f in fields])

    def mom(*rows):
        arr = np.ascontiguousarray(rows, dtype=np.intc)
        return arr, arr.ctypes.data_as(ip)

    ok_arr, ok = mom([1, 0, 0, 0])
    good = handles(v16, v5)
    two = mom([1, 0, 0, 0], [0, 1, 0, 4])
    cases = {
        "nv 0": (good, 0, b.h, 3, 1, ok, dp),
        "nv -1": (good, -1, b.h, 3, 1, ok, dp),
        "null V": (None, 2, b.h, 3, 1, ok, dp),
        "null field": (handles(v16, None), 2, b.h, 3, 1, ok, dp),
        "null b": (good, 2, None, 3, 1, ok, dp),
        "context": (handles(v16, foreign), 2, b.h, 3, 1, ok, dp),
        "parity of a V": (handles(v16, vhalf), 2, b.h, 3, 1, ok, dp),
        "parity of b": (good, 2, half.h, 3, 1, ok, dp),
        "dir -1": (good, 2, b.h, -1, 0, None, dp),
        "dir ndim": (good, 2, b.h, 4, 0, None, dp),
        "n_mom -1": (good, 2, b.h, 3, -1, ok, dp),
        "dir component": (good, 2, b.h, 3, 2, two[1], dp),
        "null momenta": (good, 2, b.h, 3, 1, None, dp),
    }
    for what, args in cases.items():
        assert lib.bcg_basis_slice_dot(*args) == INVALID, what
        assert np.array_equal(_bits(out), _bits(poison)), what
    assert lib.bcg_basis_slice_dot(good, 2, b.h, 3, 0, None, None) == INVALID  # NULL out
    # a 3-D lattice: the fourth component must be 0
    ctx3 = _ctx(bc, [4, 2, 2])
    g = bc.block_fermion_field(ctx3, 5).setGaussian(2)
    arr, p = mom([1, 0, 0, 1])
    assert ctx3.lib.bcg_basis_slice_dot(handles(g), 1, g.h, 1, 1, p, dp) == INVALID
    assert np.array_equal(_bits(out), _bits(poison))
    with pytest.raises(bc.BlockCGError):
        bc.basis_slice_dot([v16, v5], b, 4)
    with pytest.raises(bc.BlockCGError):
        bc.basis_slice_dot([v16, v5], b, 3, [])
    # and the good call fills it
    assert lib.bcg_basis_slice_dot(good, 2, b.h, 3, 1, ok, dp) == 0
    assert not np.array_equal(_bits(out[0]), _bits(poison[0]))
    assert np.array_equal(_bits(out[1]), _bits(poison[1]))  # one momentum: L K m entries and no more


def test_divided_lattice_without_a_comm(bc):
    """One rank of a (2,1,1,1) grid with no bcg_comm attached: BCG_ERR_COMM before anything is launched."""
    ctx = bc.Context([4, 2, 4, 2], grid=[2, 1, 1, 1], coords=[0, 0, 0, 0])
    for parity in (None, 0):
        V = [bc.block_fermion_field(ctx, w, parity=parity).setGaussian(1 + w) for w in (16, 5)]
        b = bc.block_fermion_field(ctx, 16, parity=parity).setGaussian(9)
        poison = np.full((2, 16, 21), 7.0 - 3.0j)
        out = poison.copy()
        Vh = (ctypes.c_void_p * 2)(*[v.h for v in V])
        assert ctx.lib.bcg_basis_slice_dot(Vh, 2, b.h, 3, 0, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == COMM
        assert np.array_equal(_bits(out), _bits(poison))


def test_cpp_basis_slice_layer_runs(bc):
    """tests/cpp/basis_slice_probe.cpp, built by the recipe of tests/test_cpp_dropin.py: blockcg/basis.hpp's basis_slice_dot on
    the device -- entry p L + t of the result, element (i, j) at j K + i, the host mirror around the call -- checked inside
    the probe against host sums in long double and against basis_dot for the sum over t."""
    from test_cpp_dropin import _compile
    exe = _compile(os.path.join(ROOT, "tests", "cpp", "basis_slice_probe.cpp"), "basis_slice_probe")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "BASIS_SLICE_PROBE_OK" and "FAILED" not in r.stdout, r.stdout + r.stderr


def test_perambulator_example(bc):
    """examples/perambulator.cpp on 4^4: its self-check (sources against the basis: zero off the source slice, V(t0)^dagger V(t0)
    on it) and the solve's perambulator, whose sum over t it compares with basis_dot."""
    from test_cpp_dropin import _compile
    exe = _compile(os.path.join(ROOT, "examples", "perambulator.cpp"), "perambulator")
    r = subprocess.run([exe, "4", "4", "4", "4"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "PERAMBULATOR_OK" in r.stdout, r.stdout + r.stderr
