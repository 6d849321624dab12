"""The level-of-detail tree as a type (LodTree, LodWork of mesh2splat_amd/csrc/m2s_lodtree.h) under AddressSanitizer + UBSan:
tests/lodtree/lodtree_check.cpp is built with the HOST compiler against a malloc-backed stand-in for the runtime calls the header makes,
linked with no HIP runtime, and run as a child process of its own.  What it asserts is listed in that file."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_lodtree_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the sanitizers' runtime linked into the program where the compiler has it as an archive (the program then runs the same whatever
    # else the process loads), else its shared form
    for link in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run([cxx, *SAN, *link, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if r.returncode == 0:
            break
    else:
        pytest.skip(f"{cxx} lacks the sanitizer runtime: {(r.stderr.strip().splitlines() or ['link failed'])[-1]}")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "lodtree_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), *SAN, *link,
           os.path.join(ROOT, "tests", "lodtree", "lodtree_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "lodtree_check ok" in r.stdout, r.stdout + r.stderr
