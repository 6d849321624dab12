"""The two transitions m2s_set_carry_sh adds to mesh2splat_amd/csrc/m2s_recstate.h (Rewrite::MergeWithSh, Rewrite::LodCutWithSh) under
AddressSanitizer + UBSan: tests/recstate/recstate_sh_check.cpp is built with the HOST compiler — the header includes nothing but
<cstdint> — linked with no HIP runtime, and run as a child process of its own, the way tests/test_recstate_cpu.py runs its program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_recstate_sh_transitions_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for link in (["-static-libasan", "-static-libubsan"], []):
        r = subprocess.run([cxx, *SAN, *link, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if r.returncode == 0:
            break
    else:
        pytest.skip(f"{cxx} lacks the sanitizer runtime: {(r.stderr.strip().splitlines() or ['link failed'])[-1]}")
    exe = tmp_path / "recstate_sh_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *SAN, *link, os.path.join(ROOT, "tests", "recstate", "recstate_sh_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "recstate_sh_check ok" in r.stdout, r.stdout + r.stderr
