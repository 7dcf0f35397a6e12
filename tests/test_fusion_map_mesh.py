"""CPU: the mesh-scope surface of the C ABI (drf_set_mesh_scope, drf_mesh_stats) is declared, exported and typed; a null
handle is refused without a device; the C++ shim's DrFusion::SetMeshScope compiles and links with plain g++."""
import ctypes as C
import os
import re
import subprocess

import pytest

from fusion_helpers import abi_module, check_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("drf_set_mesh_scope", "drf_mesh_stats")


@pytest.fixture(scope="module")
def L():
    return abi_module()


def test_symbols_declared_exported_and_typed(L):
    src = check_symbols(L, NEW)
    assert re.search(r"DRF_MESH_RESIDENT\s*=\s*0\s*,\s*DRF_MESH_MAP\s*=\s*1", src)
    from tandem_amd import dr_fusion
    assert (dr_fusion.MESH_RESIDENT, dr_fusion.MESH_MAP) == (0, 1)


def test_null_handle_is_an_argument_error(L):
    lib = L.lib()
    out = (C.c_uint64 * 3)()
    for scope in (0, 1, 7):
        assert lib.drf_set_mesh_scope(None, scope) == 1
    assert lib.drf_mesh_stats(None, out) == 1
    assert "NULL handle" in lib.dr_last_error().decode()


PROGRAM = r"""
#include "dr_fusion.h"
int main(int argc, char **argv) {
  if (argc < 2) return 0;  // linked, never run without a device
  DrFusionOptions o{};
  DrFusion f(o);
  f.SetMeshScope(DRF_MESH_MAP);
  float lo[3] = {-1.f, -1.f, -1.f}, hi[3] = {1.f, 1.f, 1.f};
  f.SaveMeshToFile(argv[1], lo, hi);
  f.SetMeshScope(DRF_MESH_RESIDENT);
  return 0;
}
"""


def test_shim_set_mesh_scope_compiles_and_links_with_gcc(L, tmp_path):
    src, exe = tmp_path / "mesh_scope.cpp", str(tmp_path / "mesh_scope")
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x", "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert subprocess.run([exe]).returncode == 0
