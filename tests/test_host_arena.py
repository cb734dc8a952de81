"""The workspace arena of csrc/gtf_arena.h on the CPU: host_arena_check.cpp carves
gtf_score.hip's carve_fin layout dry and for real and checks offsets, alignment and totals."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which("hipcc") or shutil.which("hipcc", path="/opt/rocm/bin")


@pytest.mark.skipif(HIPCC is None, reason="no hipcc to build the check with")
def test_host_arena(tmp_path):
    exe = str(tmp_path / "host_arena_check")
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(HERE, "host_arena_check.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_arena_check: ok" in r.stdout
