"""The host half of the native handles (csrc/sf_weights.h: number formats, the weight store, the carver) as a stand-alone C++
program under the address and undefined-behaviour sanitizers.  No GPU, no HIP: the header is plain C++17."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "weight_store_main.cpp")
CSRC = os.path.join(ROOT, "streamformer_amd", "csrc")


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_weight_store_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.fail("no C++ compiler found (g++, clang++ or the clang++ of ROCm)")
    exe = str(tmp_path / "weight_store_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + CSRC, SRC, "-o", exe]
    if "clang" not in os.path.basename(cxx):
        cmd += ["-static-libasan", "-static-libubsan"]      # as clang links them: the program runs in whatever environment the suite has
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "all checks passed" in ran.stdout
