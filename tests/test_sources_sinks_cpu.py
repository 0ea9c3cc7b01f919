"""Sources and sinks, the part that needs no GPU: the four entry points are bound and exported, the noise definitions have
the moments they should (numpy restatement over the oracle's generator; fixed numbers, the generator is deterministic), and
the drop-in header has the new members."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import sources_ref as ref

NAMES = ("bcg_field_fill_noise", "bcg_field_set_point_sources", "bcg_field_set_wall_sources", "bcg_field_slice_dot")
N_SITES, M = 8 ** 4, 16


def test_entry_points_are_bound_and_exported():
    import blockcg_amd
    from blockcg_amd import _lib
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    lib = ctypes.CDLL(blockcg_amd.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("NOISE_GAUSSIAN", "NOISE_Z2", "NOISE_Z4"):
        assert hasattr(blockcg_amd, name)


@pytest.fixture(scope="module", params=[1, 3])
def uniforms(request):
    import oracle
    return oracle.Oracle().fill_field(M, N_SITES, request.param)


def test_gaussian_moments(uniforms):
    z = ref.noise_from_uniforms(uniforms, ref.GAUSSIAN).ravel()
    N = z.size
    assert N == 196608 and np.all(np.isfinite(z.view(np.float64))) and np.abs(z).max() < 6.2
    checks = {
        "mean|z|^2 - 1": (np.mean(np.abs(z) ** 2) - 1.0, 1.0 / np.sqrt(N)),
        "mean Re": (z.real.mean(), 1.0 / np.sqrt(2 * N)),
        "mean Im": (z.imag.mean(), 1.0 / np.sqrt(2 * N)),
        "var Re - 1/2": (z.real.var() - 0.5, 1.0 / np.sqrt(2 * N)),
        "mean|z|^4 - 2": (np.mean(np.abs(z) ** 4) - 2.0, np.sqrt(20.0 / N)),
        "Re mean z^2": (np.mean(z * z).real, 1.0 / np.sqrt(N)),
    }
    for what, (dev, sigma) in checks.items():
        print(f"{what}: {dev / sigma:+.2f} sigma")
        assert abs(dev) <= 4 * sigma, (what, dev / sigma)


def test_z2_moments(uniforms):
    z = ref.noise_from_uniforms(uniforms, ref.Z2).ravel()
    assert np.all(z.imag == 0) and np.all(np.abs(z.real) == 1.0)
    assert abs(z.real.mean()) <= 4 / np.sqrt(z.size)


def test_z4_moments(uniforms):
    z = ref.noise_from_uniforms(uniforms, ref.Z4).ravel()
    N = z.size
    assert np.max(np.abs(np.abs(z) - 1.0)) <= 2.3e-16
    sigma = np.sqrt(3 * N / 16)
    for sr in (-1, 1):
        for si in (-1, 1):
            n = np.count_nonzero((np.sign(z.real) == sr) & (np.sign(z.imag) == si))
            assert abs(n - N / 4) <= 4 * sigma, (sr, si, (n - N / 4) / sigma)


def test_dropin_header_has_the_new_members(tmp_path):
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc,
                        os.path.join(ROOT, "tests", "cpp", "sources_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
