"""CPU checks of the sum-mode interface (bcg_sbcgrq_begin_sum / bcg_sbcgrq_solve_sum, blockcg::SBCGrQ_sum): the C header
compiles as C99 with the new declarations, the library exports them, and a C++ program calling blockcg::SBCGrQ_sum compiles
against the drop-in headers (tests/test_sum_mode.py runs it on the GPU)."""
import os
import subprocess

import pytest

from conftest import ROOT

INC = os.path.join(ROOT, "blockcg_amd", "include")
LIBDIR = os.path.join(ROOT, "blockcg_amd", "_build")
OUT = os.path.join(ROOT, "examples", "_build")

C99_SRC = r"""
#include "blockcg_hip.h"
#include <stddef.h>
int main(void) {
  int (*begin)(bcg_context*, const bcg_gauge*, double, bcg_field*, bcg_field*, int, const double*, const double*, double,
               double, double, int, bcg_sbcgrq_state**) = bcg_sbcgrq_begin_sum;
  int (*solve)(bcg_context*, const bcg_gauge*, double, bcg_field*, bcg_field*, int, const double*, const double*, double,
               double, double, int, int, int*, double*, bcg_sbcgrq_trace*) = bcg_sbcgrq_solve_sum;
  return (begin != NULL && solve != NULL) ? 0 : 1;
}
"""


def _lib():
    import blockcg_amd
    if not os.path.exists(blockcg_amd.LIB_PATH):
        blockcg_amd.build()
    return blockcg_amd.load()


def build_sum_probe():
    """g++ on tests/cpp/sum_probe.cpp against the drop-in headers (test_cpp_dropin.py's recipe); returns the executable."""
    _lib()
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "sum_probe")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", INC, os.path.join(ROOT, "tests", "cpp", "sum_probe.cpp"),
           "-o", exe, "-L", LIBDIR, "-lblockcg_hip", f"-Wl,-rpath,{LIBDIR}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "sum_c99.c"
    src.write_text(C99_SRC)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-c", str(src), "-o", str(tmp_path / "sum_c99.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_sum_entry_points():
    lib = _lib()
    for name in ("bcg_sbcgrq_begin_sum", "bcg_sbcgrq_solve_sum"):
        assert hasattr(lib, name)


def test_python_interface_present():
    import blockcg_amd
    assert callable(blockcg_amd.SBCGrQ_sum) and issubclass(blockcg_amd.SBCGrQSumState, blockcg_amd.SBCGrQState)


def test_python_rejects_mismatched_residues():
    from blockcg_amd.api import _sum_args
    with pytest.raises(ValueError):
        _sum_args([0.0, 0.1], [1.0])


def test_cpp_program_compiles_against_dropin_headers():
    assert os.path.exists(build_sum_probe())
