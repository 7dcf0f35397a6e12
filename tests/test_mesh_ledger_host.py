"""CPU: the bookkeeping of the incremental mesh (tandem_amd/csrc/fusion_host.h MeshUpdateLedger -- when an update must mesh its whole
box again, which scans it folds in, when the baseline advances), checked by the stand-alone program tests/cpp/mesh_ledger_check.cpp:
plain g++ -Wall -Werror, and once more under AddressSanitizer and UBSan.  A plain executable with its own main: nothing preloaded,
nothing loaded into Python.  The cases are listed in the program; DESIGN.md "Where streaming and meshing live"."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mesh_ledger_check.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan+ubsan"])
def test_mesh_update_ledger(tmp_path, flags):
    exe = str(tmp_path / "mesh_ledger_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mesh_ledger_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
