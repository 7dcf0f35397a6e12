"""CPU: the scatter (plane-major) order of k_conv_m's Winograd consumer (tandem_amd/csrc/conv_march.h march_consumer_ws, march_plan.h
march_plane_feeds / march_plane_completes) replayed on the host by tests/cpp/march_scatter_emul.hip: every product issued exactly once and per
output plane in the gather order, the ring protocol for rings of 2, 3 and 4 slots, the result against a direct convolution.
No device code runs here; the GPU side is tests/test_conv_march_scatter_gpu.py (the same shapes)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "cpp", "march_scatter_emul.hip")
# -DDR_PARITY_HOOKS: the planner as the parity library has it (the small layers of the GPU test get a marching plan there)
FLAGS = ["--offload-arch=gfx950", "-O2", "-std=c++17", "-DDR_PARITY_HOOKS", "-Wno-unused-function", "-Wno-pass-failed", "-Wno-unused-result"]


def _hipcc():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("needs hipcc to compile the host emulation")
    return HIPCC if os.path.exists(HIPCC) else "hipcc"


@pytest.fixture(scope="module")
def emul_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("march_scatter_emul") / "march_scatter_emul"
    subprocess.check_call([_hipcc()] + FLAGS + [SRC, "-o", str(exe)])
    out = subprocess.run([str(exe), "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    return out.stdout


def test_scatter_walk_matches_direct_convolution(emul_output):
    text = emul_output
    lines = [l for l in text.splitlines() if " plan scatter " in l]
    assert len(lines) >= 50 and all(" ok " in l for l in lines), text[-4000:]
    assert "SCATTER MARCH EMULATION: all ok" in text
    # the three instances, both pass structures, every ring size, long ranges
    for needle in ("ci=8 nup=6", "ci=16 nup=12", "ci=16 nup=9", "NPO=2", " R=2 ", " R=3 ", " R=4 ", "Dc=1:", "Dc=2:", "grid 8x1 steps 45"):
        assert any(needle in l for l in lines), needle
    assert max(float(l.split("max rel err ")[1].rstrip(")")) for l in lines) < 6e-6  # (the bound of the gather order's emulation)


def test_gpu_cases_split_and_cross_columns(emul_output):
    """The two grid cases of the GPU test do what their names say at the planned grid."""
    found = {}
    for m in re.finditer(r"^(\S+)\s+planned grid: (\d+) segments start inside a column, (\d+) ranges cross a column$", emul_output, re.M):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    assert found["gpu_mid_column"][0] > 0, found
    assert found["gpu_cross"][0] > 0 and found["gpu_cross"][1] > 0, found
    assert found["c8"][0] > 0, found

