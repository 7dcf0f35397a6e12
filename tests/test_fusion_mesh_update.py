"""CPU: the incremental-mesh surface of the C ABI (drf_extract_mesh_update_async, drf_mesh_update_size,
drf_get_mesh_update_sync, drf_mesh_update_reset, drf_mesh_update_stats) is declared, exported and typed; a null handle is
refused without a device; the C++ shim's members compile and link with plain g++; and MeshPatches, the consumer rule in
numpy, applies, replaces, deletes, clears and assembles in packed-key order on hand-made updates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from fusion_helpers import abi_module, check_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("drf_extract_mesh_update_async", "drf_mesh_update_size", "drf_get_mesh_update_sync", "drf_mesh_update_reset",
       "drf_mesh_update_stats")


@pytest.fixture(scope="module")
def L():
    return abi_module()


CTYPE_OF = {"drf_t *": C.c_void_p, "const float": C.POINTER(C.c_float), "float *": C.POINTER(C.c_float), "size_t": C.c_size_t,
            "size_t *": C.POINTER(C.c_size_t), "int *": C.POINTER(C.c_int), "int32_t *": C.POINTER(C.c_int32),
            "uint64_t *": C.POINTER(C.c_uint64), "uint64_t": C.POINTER(C.c_uint64)}


def declared_argtypes(src, name):
    """The ctypes argument list the header's declaration of `name` implies (arrays decay to pointers)."""
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        array = arg.endswith("]")
        arg = re.sub(r"\[\d*\]$", "", arg)
        typ = re.sub(r"\s*\w+$", "", arg).strip()  # drop the parameter name
        if typ.endswith("*"):
            typ = typ[:-1].strip() + " *"
        key = typ if not array else typ.replace(" *", "")
        if typ == "const float" and not array:
            raise AssertionError(arg)
        out.append(CTYPE_OF[key])
    return out


def test_symbols_declared_exported_and_typed(L):
    src = check_symbols(L, NEW)
    for name in NEW:
        res, args = L.SIGNATURES[name]
        assert res is C.c_int
        assert args == declared_argtypes(src, name), name
    m = re.search(r"#define\s+DRF_MESH_UPDATE_MAX_SCANS\s+(\d+)", src)
    assert m and int(m.group(1)) >= 1
    from tandem_amd import dr_fusion
    assert dr_fusion.MESH_UPDATE_MAX_SCANS == int(m.group(1))
    for member in ("ExtractMeshUpdateAsync", "GetMeshUpdateSync", "mesh_update_reset", "mesh_update_stats", "mesh_update_size"):
        assert callable(getattr(dr_fusion.DrFusion, member)), member


def test_null_handle_and_null_pointers_are_argument_errors(L):
    lib = L.lib()
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    nb, nt, num, full = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
    coords, first = (C.c_int32 * 3)(), (C.c_uint64 * 2)()
    v, c = (C.c_float * 9)(), (C.c_float * 9)()
    out = (C.c_uint64 * 4)()
    assert lib.drf_extract_mesh_update_async(None, lo, hi) == 1
    assert "NULL handle" in lib.dr_last_error().decode()
    assert lib.drf_mesh_update_size(None, C.byref(nb), C.byref(nt), C.byref(full)) == 1
    assert lib.drf_get_mesh_update_sync(None, 1, 3, C.byref(nb), coords, first, C.byref(num), v, c, C.byref(full)) == 1
    assert lib.drf_mesh_update_reset(None) == 1
    assert lib.drf_mesh_update_stats(None, out) == 1
    assert "NULL handle" in lib.dr_last_error().decode()


PROGRAM = r"""
#include "dr_fusion.h"
int main(int argc, char **argv) {
  if (argc < 2) return 0;  // linked, never run without a device
  DrFusionOptions o{};
  DrFusion f(o);
  float lo[3] = {-1.f, -1.f, -1.f}, hi[3] = {1.f, 1.f, 1.f};
  f.ExtractMeshUpdateAsync(lo, hi);
  f.GetMeshUpdateSync();
  size_t tri = 0;
  long sum = 0;
  for (size_t i = 0; i < f.dr_mesh_update_blocks; ++i) {
    const int32_t *c = &f.dr_mesh_update_coords[3 * i];
    sum += c[0] + c[1] + c[2];
    tri += (size_t) (f.dr_mesh_update_first[i + 1] - f.dr_mesh_update_first[i]);
  }
  if (3 * tri != f.dr_mesh_num || (f.dr_mesh_update_blocks == 0 && sum != 0)) return 2;
  f.ResetMeshUpdate();
  static_assert(DRF_MESH_UPDATE_MAX_SCANS >= 1, "published");
  return f.dr_mesh_vert && f.dr_mesh_cols ? 0 : 3;
}
"""


def test_shim_mesh_update_members_compile_and_link_with_gcc(L, tmp_path):
    src, exe = tmp_path / "mesh_update.cpp", str(tmp_path / "mesh_update")
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tandem_amd", "libdr"), str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "tandem_amd"), "-ldr_mi355x", "-Wl,-rpath," + os.path.join(ROOT, "tandem_amd")])
    assert subprocess.run([exe]).returncode == 0


# ---- MeshPatches on hand-made updates ----
def tri(tag, n):
    """n triangles whose every float is `tag + row / 1000`: recognisable, order-revealing rows."""
    v = (tag + np.arange(n * 9, dtype=np.float32) / 1000).reshape(3 * n, 3)
    return v, v + 0.5


def update(full, patches):
    """patches: [(coords, ntri, tag)] in the order given -> the tuple GetMeshUpdateSync returns."""
    coords = np.array([p[0] for p in patches], np.int32).reshape(-1, 3)
    first = np.zeros(len(patches) + 1, np.uint64)
    vs, cs = [np.empty((0, 3), np.float32)], [np.empty((0, 3), np.float32)]
    for i, (_, n, tag) in enumerate(patches):
        first[i + 1] = first[i] + np.uint64(n)
        v, c = tri(tag, n)
        vs.append(v); cs.append(c)
    return full, coords, first, np.concatenate(vs), np.concatenate(cs)


def expect(items):
    vs = [tri(tag, n)[0] for n, tag in items] + [np.empty((0, 3), np.float32)]
    cs = [tri(tag, n)[1] for n, tag in items] + [np.empty((0, 3), np.float32)]
    return np.concatenate(vs), np.concatenate(cs)


def same(got, want):
    return all(g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))


def test_mesh_patches_apply_replace_delete_and_full():
    from tandem_amd.dr_fusion import MeshPatches
    m = MeshPatches()
    assert same(m.assemble(), expect([])) and m.assemble()[0].shape == (0, 3)
    m.apply(update(True, [((0, 0, 0), 2, 1.0), ((0, 0, 1), 1, 2.0), ((1, 0, 0), 3, 3.0)]))
    assert m.num_triangles() == 6
    assert same(m.assemble(), expect([(2, 1.0), (1, 2.0), (3, 3.0)]))
    # replace one block (more triangles than before), leave the others
    m.apply(update(False, [((0, 0, 1), 4, 5.0)]))
    assert same(m.assemble(), expect([(2, 1.0), (4, 5.0), (3, 3.0)]))
    # an empty patch deletes; an empty patch for an unknown block is nothing; a new block appears in its place
    m.apply(update(False, [((0, 0, 0), 0, 0.0), ((0, 5, 0), 1, 6.0), ((7, 7, 7), 0, 0.0)]))
    assert set(m.blocks) == {(0, 0, 1), (0, 5, 0), (1, 0, 0)}
    assert same(m.assemble(), expect([(4, 5.0), (1, 6.0), (3, 3.0)]))
    # an update that lists nothing changes nothing
    m.apply(update(False, []))
    assert same(m.assemble(), expect([(4, 5.0), (1, 6.0), (3, 3.0)]))
    # full clears first
    m.apply(update(True, [((2, 2, 2), 1, 9.0)]))
    assert set(m.blocks) == {(2, 2, 2)} and same(m.assemble(), expect([(1, 9.0)]))
    m.apply(update(True, []))
    assert m.blocks == {} and m.num_triangles() == 0
    # the store owns its rows: the caller's arrays may be reused
    u = update(True, [((0, 0, 0), 1, 1.0)])
    m.apply(u)
    u[3][:] = -1.0
    assert same(m.assemble(), expect([(1, 1.0)]))


def test_mesh_patches_assemble_in_packed_key_order_with_negative_coordinates():
    from tandem_amd.dr_fusion import MeshPatches, pack_block_key
    blocks = [(-300, 4, 4), (-1, -1, -1), (-1, -1, 0), (-1, 0, -5), (0, -2, 9), (0, 0, -1), (0, 0, 0), (0, 1, -7), (3, -9, 2), (255, 0, 0), (256, -1, 5)]
    # ascending packed key = lexicographic (x, y, z) on the signed coordinates, thanks to the 2^20 bias
    keys = pack_block_key(np.array(blocks))
    assert list(keys) == sorted(keys) and len(set(int(k) for k in keys)) == len(blocks)
    assert int(pack_block_key(np.array([0, 0, 0]))) == (1 << 62) | (1 << 41) | (1 << 20)
    assert int(pack_block_key(np.array([-1, 2, -3]))) == (((1 << 20) - 1) << 42) | (((1 << 20) + 2) << 21) | ((1 << 20) - 3)
    rng = np.random.default_rng(0)
    order = rng.permutation(len(blocks))
    m = MeshPatches()
    # fed in a scrambled order, over several updates: assembly is by key, not by arrival
    m.apply(update(True, [(blocks[i], 1 + int(i) % 3, float(i)) for i in order[:6]]))
    m.apply(update(False, [(blocks[i], 1 + int(i) % 3, float(i)) for i in order[6:]]))
    assert same(m.assemble(), expect([(1 + i % 3, float(i)) for i in range(len(blocks))]))
