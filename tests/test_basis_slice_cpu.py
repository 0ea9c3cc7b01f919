"""What bcg_basis_slice_dot (include/blockcg_hip.h) needs that runs without a GPU: the numpy restatement
(tests/basis_slice_ref.py) against a plain loop over sites, the symbol in the header, the built library and the bindings,
and the C++ layer and its example through the host compiler."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import basis_ref
import basis_slice_ref as ref
from conftest import ROOT


@pytest.mark.parametrize("dims,widths,m,momenta", [([4, 2, 4, 2], (1, 7, 12), 5, [[1, 0, 0, 0], [-1, 1, 3, 5], [0, 0, 0, 0]]),
                                                   ([5, 3, 2], (16, 3), 4, [[2, -1, 1]])], ids=["4x2x4x2", "5x3x2"])
def test_restatement_against_a_loop_over_sites(dims, widths, m, momenta):
    rng = np.random.default_rng(7)
    parities = (None, 0, 1) if all(d % 2 == 0 for d in dims) else (None,)
    for parity in parities:
        sites = int(np.prod(dims)) // (1 if parity is None else 2)
        V = [basis_ref.random_field(rng, sites, w) for w in widths]
        b = basis_ref.random_field(rng, sites, m)
        for direction in range(len(dims)):
            mom = []
            for n in momenta:
                q = list(n) + [0] * (4 - len(n))
                q[direction] = 0
                mom.append(q)
            for moms in (None, mom):
                got, scale = ref.basis_slice_dot(V, b, dims, direction, moms, parity)
                want = ref.by_sites(V, b, dims, direction, moms, parity)
                assert got.shape == want.shape == ((1 if moms is None else len(moms)), dims[direction], sum(widths), m)
                assert np.max(np.abs(got - want)[:, scale > 0] / scale[scale > 0]) <= 1e-13
                assert np.all(got[:, scale == 0] == 0) and np.all(want[:, scale == 0] == 0)
            # the sum over the slices without momenta is basis_dot
            whole = basis_ref.basis_dot(V, b)
            plain, _ = ref.basis_slice_dot(V, b, dims, direction, None, parity)
            assert np.max(np.abs(plain[0].sum(axis=0) - whole) / basis_ref.dot_scale(V, b)) <= 1e-13


def test_symbol_in_header_library_and_bindings():
    import blockcg_amd
    from blockcg_amd import _lib
    header = open(os.path.join(ROOT, "include", "blockcg_hip.h")).read()
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    lib = ctypes.CDLL(blockcg_amd.LIB_PATH)
    assert re.search(r"\bint\s+bcg_basis_slice_dot\s*\(", header)
    assert "bcg_basis_slice_dot" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bcg_basis_slice_dot"][1]) == 7
    assert hasattr(lib, "bcg_basis_slice_dot")
    assert callable(blockcg_amd.basis_slice_dot)


def test_dropin_header_and_example_build():
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    for src in (os.path.join(inc, "blockcg", "basis.hpp"), os.path.join(ROOT, "tests", "cpp", "basis_slice_probe.cpp"),
                os.path.join(ROOT, "examples", "perambulator.cpp")):
        r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc, src], capture_output=True,
                           text=True)
        assert r.returncode == 0, (src, r.stderr[-3000:])
