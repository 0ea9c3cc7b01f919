"""Per-slice Gram matrices, the part that needs no GPU: the entry point is bound and exported, the drop-in header has the
members, and the numpy reference (tests/slice_gram_ref.py) satisfies the identities the GPU tests lean on."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT
import slice_gram_ref as ref


def test_entry_point_is_bound_and_exported():
    import blockcg_amd
    from blockcg_amd import _lib
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    lib = ctypes.CDLL(blockcg_amd.LIB_PATH)
    assert "bcg_field_slice_gram" in _lib.SIGNATURES
    assert hasattr(lib, "bcg_field_slice_gram")
    assert hasattr(blockcg_amd.block_fermion_field, "slice_gram")


def test_dropin_header_has_the_new_members():
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc,
                        os.path.join(ROOT, "tests", "cpp", "slice_gram_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_reference_identities():
    rng = np.random.default_rng(3)
    dims, m = [4, 2, 4, 2], 5
    for parity in (None, 0, 1):
        V = int(np.prod(dims)) // (1 if parity is None else 2)
        a = rng.normal(size=(V, m, 3)) + 1j * rng.normal(size=(V, m, 3))
        b = rng.normal(size=(V, m, 3)) + 1j * rng.normal(size=(V, m, 3))
        full = np.einsum("xic,xjc->ij", np.conj(a), b)
        for direction in range(4):
            mom = [[1, -1, 2, 5], [-1, 1, -2, -5], [0, 0, 0, 0]]
            for n in mom:
                n[direction] = 0
            got, scale = ref.slice_gram(a, b, dims, direction, None, parity)
            assert got.shape == (1, dims[direction], m, m) and scale.shape == got.shape[1:]
            assert np.max(np.abs(got[0].sum(axis=0) - full)) <= 1e-12 * np.abs(full).max()
            self_, _ = ref.slice_gram(a, a, dims, direction, mom, parity)
            assert np.max(np.abs(self_[1] - np.conj(self_[0]).transpose(0, 2, 1))) <= 1e-12 * np.abs(self_).max()
            zero, _ = ref.slice_gram(a, a, dims, direction, None, parity)
            assert np.array_equal(self_[2], zero[0])
    # momenta are reduced mod L: n and n + L give the same weights
    w = ref.phases(dims, [[1, 0, 3, 1], [5, 0, -1, 3], [-3, 0, 7, -1]], 1)
    assert np.max(np.abs(w[0] - w[1])) <= 1e-15 and np.max(np.abs(w[0] - w[2])) <= 1e-15
