"""CPU: the C-ABI shared library loads, exports every symbol include/dr_mi355x.h declares, and refuses to run
without a GPU (no CPU fallback in the product path).  No compute calls here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "dr_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(dr[mft]?_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    if not os.path.isfile(os.path.join(ROOT, "tandem_amd", "libdr_mi355x.so")):
        g.build()
    from tandem_amd import _lib
    return _lib


def test_header_declares_the_reference_surface():
    names = header_functions()
    for need in ("drm_create", "drm_destroy", "drm_call_async", "drm_ready", "drm_wait", "drm_get_result",
                 "drf_create", "drf_destroy", "drf_integrate_scan_async", "drf_render_async",
                 "drf_get_render_result", "drf_extract_mesh_async", "drf_get_mesh_sync", "drf_save_mesh",
                 "drf_synchronize"):
        assert need in names


def test_library_exports_every_declared_symbol(built):
    L = C.CDLL(built.LIB_PATH)
    missing = [n for n in header_functions() if not hasattr(L, n)]
    assert not missing, missing
    assert set(header_functions()) == set(built.SIGNATURES), "ctypes table and header disagree"
    assert b"gfx950" in built.lib().dr_version()


def test_options_struct_matches_reference_layout(built):
    # DrFusionOptions, dr_fusion.h:18-36: 16 four-byte fields in this order
    names = [f[0] for f in built.FusionOptions._fields_]
    assert names == ["voxel_size", "num_buckets", "bucket_size", "num_blocks", "block_size", "max_sdf_weight",
                     "truncation_distance", "max_sensor_depth", "min_sensor_depth", "num_render_streams", "fx", "fy",
                     "cx", "cy", "height", "width"]
    assert C.sizeof(built.FusionOptions) == 64


def test_no_gpu_means_loud_failure(built, trained_blob):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from tandem_amd.dr_mvsnet import DrMvsnet
    from tandem_amd.dr_fusion import DrFusion, DrFusionOptions
    with pytest.raises(built.DrError) as e:
        DrMvsnet(trained_blob)
    assert e.value.code == 3 and "no CPU fallback" in str(e.value)
    with pytest.raises(built.DrError) as e:
        DrFusion(DrFusionOptions(num_blocks=1000, num_buckets=1000))
    assert e.value.code == 3


def test_regression_and_filter_hooks_check_their_arguments_first(built):
    """drm_debug_regress / drm_debug_prob_regress / drm_debug_edge_filter: wrong shapes are DR_ERR_ARG before any device is touched (so also here, without
    one): a prev that is not (h / 2, w / 2) -- the x2 upsampling would read outside it --, no planes, a rank beyond the last value."""
    from tandem_amd import dr_mvsnet as M
    for prev in (np.ones((2, 3), np.float32), np.ones((3, 2), np.float32)):
        with pytest.raises(AssertionError):
            M.debug_regress(np.zeros((4, 4, 4), np.float32), prev=prev, half_range=0.1, full_range=0.2)
    L, f32p = built.lib(), built.f32p
    z = np.zeros(4 * 4 * 4 * 8, np.float32)
    o = np.zeros(64, np.float32)
    thr = C.c_uint()
    p = lambda a: a.ctypes.data_as(f32p)  # noqa: E731
    assert L.drm_debug_regress(0, p(z), 4, 4, 4, p(z), 2, 3, 0.5, 0.1, 0.1, 0.2, p(o), p(o), None) == 1
    assert L.drm_debug_regress(0, p(z), 0, 4, 4, None, 0, 0, 0.5, 0.1, 0.0, 0.0, p(o), p(o), None) == 1
    assert L.drm_debug_prob_regress(0, p(z), p(z), 4, 4, 4, p(z), 1, 1, 0.5, 0.1, 0.1, 0.2, p(z), p(o), p(o), None) == 1
    assert L.drm_debug_prob_regress(0, p(z), None, 4, 4, 4, None, 0, 0, 0.5, 0.1, 0.0, 0.0, p(z), p(o), p(o), None) == 1
    assert L.drm_debug_edge_filter(0, p(z), p(z), 4, 4, None, 16, p(o), p(o), p(o), C.byref(thr)) == 1
    assert L.drm_debug_edge_filter(0, p(z), p(z), 0, 4, None, 0, p(o), p(o), p(o), C.byref(thr)) == 1
    assert b"rank 16 of 16" in L.dr_last_error() or b"H, W" in L.dr_last_error()


def test_missing_blob_is_an_io_error(built):
    from tandem_amd.dr_mvsnet import DrMvsnet
    with pytest.raises(built.DrError) as e:
        DrMvsnet("/nonexistent/model.tdmw")
    assert e.value.code == 4


def test_product_path_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "tandem_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "import oracle" not in txt and "from oracle" not in txt and "libtsdf_oracle" not in txt, f
                assert not re.search(r'#include\s*[<"][^>"]*oracle', txt), f


def test_product_library_reads_only_the_documented_switches():
    """every DR_* name the PRODUCT library can pass to getenv is one of the sixteen INTEGRATION.md lists; the superseded
    generations and settled A/Bs are read through hook_env() (csrc/dr_host.h), i.e. by the parity build only, and their kernels
    (k_tail, k_tail_m, k_conv_b, k_costvol / k_costvol4, ...) are not in the product's code object at all."""
    import subprocess
    lib = os.path.join(ROOT, "tandem_amd", "libdr_mi355x.so")
    if not os.path.isfile(lib):
        pytest.skip("library not built")
    names = set(re.findall(r"^DR_[A-Z0-9_]+$", subprocess.run(["strings", lib], capture_output=True, text=True).stdout, re.M))
    allowed = {"DR_RCCL_LIB", "DR_FUSION_PRIORITY", "DR_MVS_NO_SIDE_STREAM", "DR_CONV_PRINT", "DR_AUTOTUNE_ONLY", "DR_CONV_NO_TUNED", "DR_CONV_RANK", "DR_CONV_ASYNC",
               "DR_CONV_MARCH", "DR_CONV_ROWMARCH", "DR_CONV_WINO", "DR_CV_DCHUNK1", "DR_CV_DCHUNK2", "DR_CV_DCHUNK3", "DR_PROB_ZCHUNK", "DR_HIST_BLOCKS"}
    assert names == allowed, (sorted(names - allowed), sorted(allowed - names))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in allowed:
        assert n in doc or (n.startswith("DR_CV_DCHUNK") and "DR_CV_DCHUNK1..3" in doc), n
    syms = subprocess.run(["strings", lib], capture_output=True, text=True).stdout
    for k in ("k_tail", "k_conv_b", "k_costvol4", "k_costvolILi"):
        assert not re.search(r"_ZN2dr\d+%s" % k, syms), k


def test_weight_blob_roundtrip(tmp_path):
    from tandem_amd import weights as Wt
    sd = Wt.random_state((48, 32, 8), seed=3)
    p = str(tmp_path / "w.tdmw")
    Wt.write_blob(p, sd, depth_num=(48, 4, 4))
    meta, back = Wt.read_blob(p)
    assert meta["depth_num"] == (48, 4, 4) and meta["view_aggregation"] is True
    assert list(back) == list(sd)
    for k in sd:
        assert np.array_equal(sd[k], back[k])


def test_scene_generator_is_deterministic():
    from synth import scene
    a, b = scene.make_window(64, 96, 3, seed=5), scene.make_window(64, 96, 3, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a["bgrs"], b["bgrs"]))
    assert a["ref_index"] == 1 and a["c2ws"].shape == (3, 4, 4)


def test_views_keep_their_owner_alive():
    """numpy views of library-owned memory (GetResultView, alloc_images) must not dangle after DrMvsnet.close().  The
    views are built on a ctypes buffer that references an owner object; the release runs when the LAST view is gone."""
    import ctypes as C
    import gc
    import numpy as np
    from tandem_amd.dr_mvsnet import _Owned, _view
    backing = (C.c_uint8 * 64)()
    released = []
    owner = _Owned(released.append, 1234)
    a = np.frombuffer(_view(C.addressof(backing), 64, owner), np.uint8)
    b = a[8:24].reshape(4, 4)
    del owner, a
    gc.collect()
    assert released == []          # b still looks at the memory
    b[0, 0] = 7
    assert backing[8] == 7
    del b
    gc.collect()
    assert released == [1234]      # released exactly once, after the last view
