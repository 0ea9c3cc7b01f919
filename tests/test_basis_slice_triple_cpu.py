"""What bcg_basis_slice_triple (include/blockcg_hip.h) needs that runs without a GPU: the numpy restatement
(tests/basis_slice_triple_ref.py) against an epsilon-tensor loop over sites; the planner (basis_slice_triple_plan,
blockcg_amd/csrc/slice_plan.hpp) through a stand-alone probe that links slice_plan.o alone -- tiles sorted and complete, every
listed slice covered exactly once by chunks of whole steps, the partial count within the buffer the plan asks for; the symbol
in the header, the built library and the bindings; and the C++ layer, its probe and the example through the host compiler."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import basis_ref
import basis_slice_triple_ref as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "blockcg_amd", "csrc")
MAX_PARTIALS = 1 << 24  # kTriplePartialEntries
CHUNK_ROWS = 48         # kTripleChunkRows: 16 sites, four steps of four sites
BLOCKS = 1024           # kTripleBlocks


@pytest.mark.parametrize("dims,widths,momentum", [([4, 2, 4, 2], ((1, 4), (3,), (2, 2)), [-1, 1, 3, 5]), ([5, 3, 2], ((3,), (2, 1), (4,)), [2, -1, 1])],
                         ids=["4x2x4x2", "5x3x2"])
def test_restatement_against_a_loop_over_sites(dims, widths, momentum):
    rng = np.random.default_rng(17)
    parities = (None, 0, 1) if all(d % 2 == 0 for d in dims) else (None,)
    for parity in parities:
        sites = int(np.prod(dims)) // (1 if parity is None else 2)
        A, B, C = ([basis_ref.random_field(rng, sites, w) for w in ws] for ws in widths)
        for direction in range(len(dims)):
            L = dims[direction]
            q = list(momentum) + [0] * (4 - len(momentum))
            q[direction] = 0
            for slices in (None, [L - 1], [L - 1, 0]):
                for mom in (None, [q, [0, 0, 0, 0]]):
                    got, scale = ref.basis_slice_triple(A, B, C, dims, direction, slices, mom, parity)
                    want = ref.by_sites(A, B, C, dims, direction, slices, mom, parity)
                    assert got.shape == want.shape and scale.shape == got.shape[1:]
                    sc = np.broadcast_to(scale, got.shape)
                    assert np.all(got[sc == 0] == 0) and np.all(want[sc == 0] == 0)
                    assert np.all(np.abs(got - want)[sc > 0] <= 1e-14 * sc[sc > 0]), (parity, direction, slices)
                    if mom is not None:  # the zero momentum is the call without momenta
                        plain, _ = ref.basis_slice_triple(A, B, C, dims, direction, slices, None, parity)
                        assert np.array_equal(plain[0], got[1])
        # one list three times: antisymmetric to rounding, which the device makes exact
        T, scale = ref.basis_slice_triple(A, A, A, dims, 0, None, None, parity)
        assert np.all(np.abs(T + T.transpose(0, 1, 3, 2, 4)) <= 1e-14 * scale)


# ---- the planner -------------------------------------------------------------------------------------------------------
def _requests():
    lattices = (([4, 2, 4, 2], [0, 0, 0, 0]), ([5, 3, 2, 1], [0, 0, 0, 0]), ([16, 16, 8, 4], [0, 0, 0, 0]), ([16, 10, 7, 4], [0, 0, 0, 0]),
                ([3, 4, 4, 3], [3, 0, 0, 3]), ([96, 1, 1, 1], [0, 0, 0, 0]), ([64, 64, 64, 32], [0, 0, 0, 0]), ([2048, 1, 1, 1], [0, 0, 0, 0]))
    lists = ((([16],) * 3, 0), (([16, 32, 16],) * 3, 1), (([32], [16], [16, 16]), 0), (([5],) * 3, 1), (([1, 7, 12], [8], [3]), 0),
             (([16, 5], [16], [32, 3]), 0), (([32, 32],) * 3, 1), (([32, 32, 5], [16], [16]), 0))
    out = []
    for (L, origin), (widths, identical) in itertools.product(lattices, lists):
        even = all(x % 2 == 0 for x in L[:sum(1 for x in L if x > 1)])
        for parity, direction, fast, n_slices in ((-1, 3 if L[3] > 1 else 0, 1, 1), (-1, 0, 1, L[0]), (0 if even else -1, 0, 1, 2), (-1, 0, 0, 1)):
            out.append(dict(L=L, origin=origin, parity=parity, dir=direction, identical=identical, fast=fast,
                            n_slices=min(n_slices, L[direction]), n_mom=n_slices % 3, widths=widths))
    return out


def _line(rq):
    v = rq["L"] + rq["origin"] + [rq["parity"], rq["dir"], rq["identical"], rq["fast"], rq["n_slices"], rq["n_mom"]]
    for w in rq["widths"]:
        v += [len(w)] + list(w)
    return " ".join(map(str, v))


def _build_probe(out):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the probe is compiled with the compiler that builds the library")
    exe = str(out / "basis_slice_triple_plan_probe")
    subprocess.run(["make", "-C", CSRC, "-s", "../_build/slice_plan.o"], check=True)  # (built with the library; here if it is not)
    main = exe + ".o"
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-c", os.path.join(ROOT, "tests", "cpp", "basis_slice_triple_plan_probe.cpp"), "-o", main],
                   check=True)
    subprocess.run([hipcc, main, os.path.join(ROOT, "blockcg_amd", "_build", "slice_plan.o"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    out = tmp_path_factory.mktemp("basis_slice_triple_plan_probe")
    exe = _build_probe(out)
    requests = _requests()
    infile = out / "requests.txt"
    infile.write_text("".join(_line(r) + "\n" for r in requests))
    got = subprocess.run([exe, str(infile)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(requests) >= 36
    return requests, got, infile


def _fields(line):
    return dict(kv.split("=") for kv in line.split())


def test_the_plans(plans):
    requests, got, _ = plans
    refused = 0
    for rq, line in zip(requests, got):
        K = [sum(w) for w in rq["widths"]]
        mfma = bool(rq["fast"]) and all(w in (16, 32) for ws in rq["widths"] for w in ws)
        edge = 16 if mfma else 8
        nt = [(k + edge - 1) // edge for k in K]
        tiles = [t for t in itertools.product(*map(range, nt)) if not rq["identical"] or t[0] <= t[1] <= t[2]]
        if max(K) > 64 or rq["n_slices"] * len(tiles) * edge ** 3 > MAX_PARTIALS:
            assert line == "no plan", (rq, line)
            refused += 1
            continue
        p = _fields(line)
        assert (int(p["mfma"]), int(p["edge"]), int(p["pc"])) == (int(mfma), edge, 1), (rq, line)
        # the tiles: sorted, complete, none twice
        listed = [tuple(map(int, t.split(":"))) for t in p["tiles"].split(";") if t]
        assert listed == sorted(tiles) and len(set(listed)) == len(listed), (rq, line)
        # the walk: every row of a slice in exactly one chunk, chunks of whole 16-site rounds, no empty block
        nbps, chunk, n_virtual = int(p["nbps"]), int(p["chunk"]), int(p["n_virtual"])
        assert chunk % CHUNK_ROWS == 0 and chunk % 12 == 0 and chunk % 16 == 0, (rq, line)
        assert nbps >= 1 and (nbps - 1) * chunk < n_virtual <= nbps * chunk, (rq, line)
        # the partials it asks for: what the grid writes, within the bound
        grid = rq["n_slices"] * len(tiles) * nbps
        assert int(p["partials"]) == grid * edge ** 3 <= MAX_PARTIALS, (rq, line)
        # the grid aims at BLOCKS: never more than one round above it unless one block per (slice, tile) already is
        assert grid <= max(BLOCKS, rq["n_slices"] * len(tiles)), (rq, line)
        # a large slice and few tiles: the device is filled (rounding the chunk up to 48 rows loses a fifth at the most here)
        if n_virtual >= 4 * CHUNK_ROWS * BLOCKS and rq["n_slices"] * len(tiles) <= BLOCKS // 4:
            assert grid > BLOCKS // 2, (rq, line)
    assert 0 < refused < len(requests)


def test_the_plan_is_a_pure_function(plans):
    requests, got, infile = plans
    exe = os.path.join(os.path.dirname(str(infile)), "basis_slice_triple_plan_probe")
    again = subprocess.run([exe, str(infile)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert again == got


# ---- the layers ----------------------------------------------------------------------------------------------------------
def test_symbol_in_header_library_and_bindings():
    import blockcg_amd
    from blockcg_amd import _lib
    header = open(os.path.join(ROOT, "include", "blockcg_hip.h")).read()
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    lib = ctypes.CDLL(blockcg_amd.LIB_PATH)
    assert re.search(r"\bint\s+bcg_basis_slice_triple\s*\(", header)
    assert "bcg_basis_slice_triple" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bcg_basis_slice_triple"][1]) == 12
    assert hasattr(lib, "bcg_basis_slice_triple")
    assert callable(blockcg_amd.basis_slice_triple)


def test_dropin_header_probe_and_example_build():
    inc = os.path.join(ROOT, "blockcg_amd", "include")
    for src in (os.path.join(inc, "blockcg", "basis.hpp"), os.path.join(ROOT, "tests", "cpp", "basis_slice_triple_probe.cpp"),
                os.path.join(ROOT, "examples", "baryon_elemental.cpp")):
        r = subprocess.run(["g++", "-std=c++14", "-O0", "-Wall", "-Wextra", "-fsyntax-only", "-I", inc, src], capture_output=True,
                           text=True)
        assert r.returncode == 0, (src, r.stderr[-3000:])
