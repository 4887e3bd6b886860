"""The launch rules of every sweep kernel family (csrc/psa_launch_rules.h: check mode, workgroup size, grid, lanes per point,
dynamic LDS bytes) on the CPU: tests/c/launch_rules_client.cpp holds the expectations, worked out by hand from the launchers,
and is built with the host C++ compiler alone -- no HIP, no library, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "psa-simulation-ode-rk-mvp-dispersion_amd", "csrc")
INC = os.path.join(ROOT, "include")
ALLOWED = {"stdint.h", "stddef.h", "cstddef", "cstdint", "psa_rk4.h"}


def _includes(path):
    src = open(path, encoding="utf-8").read()
    return src, re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", src, re.M)


def test_the_rules_header_is_plain_cpp():
    src, inc = _includes(os.path.join(CSRC, "psa_launch_rules.h"))
    assert inc and set(inc) <= ALLOWED, inc
    assert not re.search(r"\bhip[A-Z_]\w*|__device__|__global__|__host__", src)
    _, inc_abi = _includes(os.path.join(INC, "psa_rk4.h"))      # what it includes in turn
    assert set(inc_abi) <= {"stdint.h", "stddef.h"}, inc_abi


def test_launch_rules_client(tmp_path):
    test_the_rules_header_is_plain_cpp()
    cxx = shutil.which("g++") or next((p for p in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                                       if os.path.exists(p)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "launch_rules_client")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", INC,
                    os.path.join(ROOT, "tests", "c", "launch_rules_client.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "launch_rules_client ok" in out.stdout
