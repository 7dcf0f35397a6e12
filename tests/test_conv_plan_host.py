"""CPU: the convolution planner as a host-only header (tandem_amd/csrc/conv_plan.h), compiled alone with g++ -Wall -Werror -- no HIP header, no
device.  tests/cpp/conv_plan_check.cpp builds every rank of the ranking for the small cases of the kernel emulation (tests/cpp/conv_emul.hip), one
fused-skip, one split-input and the up2 calls, with and without the tuned swap, and holds every plan to what the kernels assume of it: the ranks
are pairwise different (family, ci, ct, pt, tile) plans; LDS within 160 KiB; a halo below 65536 positions whose magic numbers divide every position
exactly; grid.x a multiple of 8; the instance in its family's list; every tap offset inside the staged tile; the classes' table and weight offsets
increasing and inside the uploaded arrays; conv_family() of the launch equal to the candidate's code, and to the row's for every tuned row.  The
same source runs as a stand-alone program under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "conv_plan_check.cpp")


def _run(exe, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DR_")}
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_plan_check") / "conv_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", SRC, "-o", exe])
    r = _run(exe)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_every_rank_of_every_case_is_a_plan_the_kernels_accept(walk):
    assert "conv_plan_check ok" in walk
    ranks = {l.split()[0]: int(l.split()[1]) for l in walk.splitlines() if l.endswith(" ranks")}
    assert len(ranks) == 28 and all(n >= 3 for n in ranks.values()), ranks
    for name in ("conv2d_5x5_s2_8_16", "x8_prob_8_1", "deconv_16_8_skip", "up2_32_8_inplace_add.py1", "conv3d_64_64_D1", "fz_head_32_8",
                 "split16_xpair3d_32_8", "up2_16_8.py1"):
        assert name in ranks, name
    # the walk really went through a ranking of every family's candidates, not a handful of plans
    assert ranks["conv3d_32_32"] > 100 and ranks["split16_xpair3d_32_8"] < ranks["xpair3d_32_8"], ranks


def test_every_tuned_row_is_walked_and_rebuilt(walk):
    line = [l for l in walk.splitlines() if " tuned rows, " in l]
    assert len(line) == 1, walk[-2000:]
    rows, plans = int(line[0].split()[0]), int(line[0].split()[3])
    with open(os.path.join(ROOT, "tandem_amd", "csrc", "conv_tuned.h")) as f:
        table = [l for l in f if l.lstrip().startswith("{") and "sentinel" not in l]
    assert rows == len(table) and plans > 40 * rows, (rows, len(table), plans)


def test_parity_build_of_the_header_compiles_alone(tmp_path):
    """-DDR_PARITY_HOOKS turns hook_env() into getenv(): the same walk, with the parity-only switches at their defaults."""
    exe = str(tmp_path / "conv_plan_check_hooks")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DDR_PARITY_HOOKS", SRC, "-o", exe])
    r = _run(exe)
    assert r.returncode == 0 and "conv_plan_check ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_sanitizer_run_of_the_stand_alone_program(tmp_path):
    """conv_plan.h under AddressSanitizer and UBSan: a plain executable, nothing preloaded, nothing loaded into Python."""
    exe = str(tmp_path / "conv_plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", SRC, "-o", exe])
    r = _run(exe, "rows-rank0")  # every rank of the cases, the tuned rows' layers at rank 0
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "conv_plan_check ok" in r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
