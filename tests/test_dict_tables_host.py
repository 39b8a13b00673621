"""The wire codec's dictionary builder (lasp_amd/csrc/laspj_dict_tables.cpp: every table of
a device dictionary, its block layout and image, and a patch's rows) on the CPU."""

import os
import shutil
import subprocess

from lasp_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dict_tables.txt")


def test_dict_tables_under_host_sanitizers(tmp_path):
    """A stand-alone program over the two host sources, built with the address and
    undefined-behaviour sanitizers: the facts, block size and image hash of one small
    dictionary per branch of the builder against tests/golden/dict_tables.txt (recorded from
    the builder as it stood inside laspj_etf_dict_create), the arrays it refuses, and patches
    against rebuilds; each image in a heap block of exactly its size.  Nothing loaded into
    Python runs under a sanitizer."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    cands = [os.path.join(rocm, "llvm", "bin", "clang++"),
             os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("clang++")]
    cxx = next((c for c in cands if c and os.path.exists(c)), None)
    assert cxx is not None, "no host clang++ beside hipcc"
    exe = str(tmp_path / "dict_tables_check")
    # plain host C++ (the sources hold no kernels): the HIP headers only declare
    cmd = [cxx, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "c", "dict_tables_check.cpp"),
           os.path.join(build.CSRC, "laspj_dict_tables.cpp"),
           os.path.join(build.CSRC, "laspj_host.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "13 dictionaries, 0 bad" in res.stdout
