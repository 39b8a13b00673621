"""The host's half of the one-pass reads (lasp_amd/csrc/laspj_reads_host.cpp: k_read_check's
wave-item layout and the fold of read_any/3, lasp_core.erl:372-414) on the CPU."""

import os
import shutil
import subprocess

from lasp_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_fold_under_host_sanitizers(tmp_path):
    """A stand-alone program over the host source, built with the address and undefined-
    behaviour sanitizers, compares read_fold with the fold written as the reference writes
    it over 4000 random calls and must end clean.  Nothing loaded into Python runs under a
    sanitizer."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    cands = [os.path.join(rocm, "llvm", "bin", "clang++"),
             os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("clang++")]
    cxx = next((c for c in cands if c and os.path.exists(c)), None)
    assert cxx is not None, "no host clang++ beside hipcc"
    exe = str(tmp_path / "reads_host_check")
    # plain host C++ (the source holds no kernels): the HIP headers only declare
    cmd = [cxx, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "c", "reads_host_check.cpp"),
           os.path.join(build.CSRC, "laspj_reads_host.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "4000 rounds, 0 bad" in res.stdout
