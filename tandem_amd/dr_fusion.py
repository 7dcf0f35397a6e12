"""Python mirror of TANDEM's `DrFusion` operator (tandem/libdr/dr_fusion/src/dr_fusion/dr_fusion.h:18-73)
on top of the C ABI of libdr_mi355x.so: same method names, call order contract and argument meaning.
Protocol violations raise DrError (the reference prints and exit()s)."""
import collections
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import FusionOptions, check, fptr, u8p, f32p


def DrFusionOptions(**kw):
    """struct DrFusionOptions (dr_fusion.h:18-36).  Defaults = what TANDEM runs (FullSystem.cpp:259-276)."""
    d = dict(voxel_size=0.01, num_buckets=1000000, bucket_size=10, num_blocks=1000000, block_size=8,
             max_sdf_weight=64, truncation_distance=0.04, max_sensor_depth=10.0, min_sensor_depth=0.1,
             num_render_streams=1, fx=500.0, fy=500.0, cx=319.5, cy=239.5, height=480, width=640)
    d.update(kw)
    return FusionOptions(**d)


# drf_set_mesh_scope: what the mesh calls cover (include/dr_mi355x.h)
MESH_RESIDENT, MESH_MAP = 0, 1
# drf_set_render_scope: what RenderAsync ray-casts
RENDER_RESIDENT, RENDER_MAP = 0, 1
# drf_set_locate_scope: what locate_system / locate_frame read
LOCATE_RESIDENT, LOCATE_MAP = 0, 1
# drf_set_search_scope: what the score stage of score_poses / search_frame and their colour forms reads
SEARCH_RESIDENT, SEARCH_MAP = 0, 1


MESH_UPDATE_MAX_SCANS = 16  # DRF_MESH_UPDATE_MAX_SCANS: one scan more between two updates makes the next one full
# drf_align_result_t.status
ALIGN_CONVERGED, ALIGN_MAX_ITERS, ALIGN_DEGENERATE, ALIGN_LOST = 0, 1, 2, 3
ALIGN_STATUS = ("converged", "max_iters", "degenerate", "lost")


class AlignResult(collections.namedtuple("AlignResult", "T T32 sums samples valid0 valid cost0 cost iterations status")):
    """drf_align_result_t: T (4, 4) float64 src-world to ref-world in metres, T32 the same rounded to float32 (what transform_map
    takes), sums (28,) the last system evaluated, samples / valid0 / valid, cost0 / cost, iterations, status (ALIGN_*)."""
    __slots__ = ()


class ExposureResult(collections.namedtuple("ExposureResult", AlignResult._fields + ("gain", "offset", "ext", "photometric", "held"))):
    """drf_exposure_result_t: AlignResult's fields (level 0's), the gain and offset the call ended on (frame intensity ~ gain *
    model intensity + offset, the offset in units of the three-channel sum), ext (17,) = sums[28..44] of the last evaluation, the
    photometric terms it added, and the evaluations whose step held the exposure."""
    __slots__ = ()


def compensate_exposure(bgr, gain, offset):
    """The frame's colour image brought to the map's exposure, on the host: per channel clip(floor((c - offset / 3) / gain + 0.5),
    0, 255), the inverse of frame ~ gain * model + offset with the offset split evenly over the three channels.  bgr (H, W, 3)
    uint8; gain and offset as track_exposure_frame returns them.  What saturated in the frame stays lost."""
    c = np.asarray(bgr, np.uint8).astype(np.float64)
    return np.clip(np.floor((c - float(offset) / 3.0) / float(gain) + 0.5), 0.0, 255.0).astype(np.uint8)


class AlignError(RuntimeError):
    """A registration that ran but found no pose (ALIGN_DEGENERATE, ALIGN_LOST); .result is the AlignResult."""

    def __init__(self, result, msg):
        super().__init__(msg)
        self.result = result


class SearchEntry(collections.namedtuple("SearchEntry", "index score cost counts track_status locate_status samples valid located_cost T")):
    """drf_search_entry_t: the candidate's index, its score, cost and counts (samples, valid, unobserved, outside) of the score
    stage, the statuses of its tracking and localisation (ALIGN_*, -1: did not run), the localisation's samples / valid / cost, and
    T (4, 4) float64 camera-to-world: the located pose, else the tracked one, else the candidate's own."""
    __slots__ = ()


class SearchResult(collections.namedtuple("SearchResult", "T32 status winner refined n_candidates entries scores")):
    """drf_search_result_t: T32 (4, 4) float32 the pose found (the winner's; the best-scoring candidate's if there is none), status
    (ALIGN_*), winner (index into entries, -1: none), refined, n_candidates, entries (SearchEntry, ascending score) and scores (every
    candidate's, in index order; None unless asked for)."""
    __slots__ = ()


class SearchColourEntry(collections.namedtuple("SearchColourEntry", SearchEntry._fields + ("photo", "final_score", "final_photo"))):
    """drf_search_colour_entry_t: SearchEntry's fields (score is the colour score), photo of the score stage, and final_score /
    final_photo: the colour score of the located float pose (0 for an entry that did not qualify)."""
    __slots__ = ()


def pose_rotations(yaw_deg=(0.0,), pitch_deg=(0.0,), roll_deg=(0.0,)):
    """The rotations of a search lattice as search_frame takes them: an (n, 9) float64 array, one row-major matrix
    Ry(yaw) Rx(pitch) Rz(roll) per combination, yaw outermost and roll innermost -- turns about the WORLD axes y, x and z.  The one
    place that calls cos or sin: the library itself takes rotations as data."""
    out = []
    for y in np.atleast_1d(np.asarray(yaw_deg, np.float64)):
        for p in np.atleast_1d(np.asarray(pitch_deg, np.float64)):
            for r in np.atleast_1d(np.asarray(roll_deg, np.float64)):
                cy, sy, cp, sp, cr, sr = (f(np.deg2rad(a)) for a in (y, p, r) for f in (np.cos, np.sin))
                Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
                Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
                Rz = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
                out.append((Ry @ Rx @ Rz).reshape(9))
    return np.ascontiguousarray(out, np.float64)


def pack_block_key(coords):
    """The packed key that orders blocks in every extraction: x, then y, then z, each biased by 2^20 (21 bits each)."""
    c = np.asarray(coords, np.int64) + (1 << 20)
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


class MeshPatches:
    """The consumer's side of the incremental mesh: {block -> its triangle rows}.  apply() takes what GetMeshUpdateSync
    returns -- a full update empties the store first, every listed block's entry is replaced (an empty patch deletes it) --
    and assemble() concatenates the entries in ascending packed-key order, which is byte for byte the full extraction over
    the same box at the moment the update was launched.  Pure numpy: a viewer keeps one of these per mesh."""

    def __init__(self):
        self.blocks = {}  # (bx, by, bz) -> (vert (3t, 3) float32, cols (3t, 3) float32)

    def apply(self, update):
        full, coords, first, vert, cols = update
        coords = np.asarray(coords, np.int32).reshape(-1, 3)
        first = np.asarray(first, np.uint64).astype(np.int64)
        assert len(first) == len(coords) + 1, "first has one row more than there are blocks"
        if full:
            self.blocks.clear()
        for i, c in enumerate(coords):
            k, a, b = tuple(int(v) for v in c), 3 * int(first[i]), 3 * int(first[i + 1])
            if b > a:
                self.blocks[k] = (np.array(vert[a:b], np.float32), np.array(cols[a:b], np.float32))
            else:
                self.blocks.pop(k, None)
        return self

    def assemble(self):
        """(vert, cols), each (3 * triangles, 3) float32."""
        if not self.blocks:
            return np.empty((0, 3), np.float32), np.empty((0, 3), np.float32)
        keys = list(self.blocks)
        order = np.argsort(pack_block_key(np.array(keys, np.int64)), kind="stable")
        return (np.concatenate([self.blocks[keys[i]][0] for i in order]).reshape(-1, 3),
                np.concatenate([self.blocks[keys[i]][1] for i in order]).reshape(-1, 3))

    def num_triangles(self):
        return sum(len(v) for v, _ in self.blocks.values()) // 3


def streaming_min_radius(options):
    """drf_streaming_min_radius: the smallest exact streaming radius for these options (host-only)."""
    r = C.c_float()
    check(_lib.lib().drf_streaming_min_radius(C.byref(options), C.byref(r)))
    return float(r.value)


def map_info(path):
    """drf_map_info: validates the whole map file (host-only) and returns (voxel_size, number of blocks)."""
    vs, n = C.c_float(), C.c_uint64()
    check(_lib.lib().drf_map_info(os.fsencode(path), C.byref(vs), C.byref(n)))
    return float(vs.value), int(n.value)


class DrFusion:
    def __init__(self, options, device=0):
        self.options = options
        self._h = C.c_void_p()
        self._L = _lib.lib()  # the library this handle belongs to (tests may switch the process default, _lib.switch)
        check(self._L.drf_create(C.byref(options), int(device), C.byref(self._h)))
        self._hw = (options.height, options.width)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.drf_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def IntegrateScanAsync(self, bgr, depth, pose):
        """dr_fusion.h:50: bgr H*W*3 u8, depth H*W f32 metres (0 invalid), pose 16 f32 row-major cam-to-world."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        assert bgr.size == self._hw[0] * self._hw[1] * 3 and depth.size == self._hw[0] * self._hw[1]
        check(self._L.drf_integrate_scan_async(self._h, bgr.ctypes.data_as(u8p), fptr(depth), fptr(pose)))

    def RenderAsync(self, camera_poses):
        """dr_fusion.h:52: exactly num_render_streams poses."""
        poses = [np.ascontiguousarray(p, np.float32).reshape(16) for p in camera_poses]
        arr = (f32p * max(len(poses), 1))(*[fptr(p) for p in poses])
        check(self._L.drf_render_async(self._h, arr, len(poses)))

    def GetRenderResult(self, copy=True):
        """dr_fusion.h:54: returns (bgr list, depth list).  copy=True: copies of the library-owned pinned buffers; copy=False: what the C++ member hands
        out -- views of those buffers, valid until the NEXT GetRenderResult (tsdf_volume.cu:846-872, the "blocked" / "free" sets)."""
        n = self.options.num_render_streams
        pb, pd = (u8p * max(n, 1))(), (f32p * max(n, 1))()
        check(self._L.drf_get_render_result(self._h, pb, pd, n))
        H, W = self._hw
        bgrs = [np.ctypeslib.as_array(pb[i], shape=(H, W, 3)) for i in range(n)]
        depths = [np.ctypeslib.as_array(pd[i], shape=(H, W)) for i in range(n)]
        if copy:
            bgrs, depths = [b.copy() for b in bgrs], [d.copy() for d in depths]
        return bgrs, depths

    def ExtractMeshAsync(self, lower_corner, upper_corner):
        """dr_fusion.h:60: marching cubes over the lattice lower + g * voxel_size, legal after GetRenderResult."""
        lo, up = (np.ascontiguousarray(a, np.float32) for a in (lower_corner, upper_corner))
        check(self._L.drf_extract_mesh_async(self._h, fptr(lo), fptr(up)))

    def GetMeshSync(self):
        """dr_fusion.h:61: fills the public members dr_mesh_num (vertices = 3 * triangles), dr_mesh_vert, dr_mesh_cols
        ((num, 3) float32: positions, RGB colours in [0, 1]) and returns (vert, cols)."""
        ntri = C.c_size_t()
        check(self._L.drf_mesh_num_triangles(self._h, C.byref(ntri)))
        nv = 3 * ntri.value
        vert, cols = np.empty((max(nv, 1), 3), np.float32), np.empty((max(nv, 1), 3), np.float32)
        num = C.c_size_t()
        check(self._L.drf_get_mesh_sync(self._h, max(nv, 1), C.byref(num), fptr(vert), fptr(cols)))
        self.dr_mesh_num, self.dr_mesh_vert, self.dr_mesh_cols = int(num.value), vert[:nv], cols[:nv]
        return self.dr_mesh_vert, self.dr_mesh_cols

    def mesh_num_triangles(self):
        """Size of the pending mesh (waits for the extraction, does not consume it)."""
        ntri = C.c_size_t()
        check(self._L.drf_mesh_num_triangles(self._h, C.byref(ntri)))
        return int(ntri.value)

    def GetMesh(self, lower_corner, upper_corner):
        """dr_fusion.h:58 (DrMesh): synchronous extraction."""
        self.ExtractMeshAsync(lower_corner, upper_corner)
        return self.GetMeshSync()

    def SaveMeshToFile(self, filename, lower_corner, upper_corner):
        lo, up = (np.ascontiguousarray(a, np.float32) for a in (lower_corner, upper_corner))
        check(self._L.drf_save_mesh(self._h, str(filename).encode(), fptr(lo), fptr(up)))

    def render_device_pointers(self, stream=0):
        """(d_bgr, d_depth) device pointers of a render stream's result, valid until the next RenderAsync."""
        b, d = C.c_void_p(), C.c_void_p()
        check(self._L.drf_get_render_device(self._h, stream, C.byref(b), C.byref(d)))
        return b.value, d.value

    def Synchronize(self):
        check(self._L.drf_synchronize(self._h))

    # ---- introspection / measurement hooks (no reference counterpart) ----
    def stats(self):
        out = (C.c_uint64 * 4)()
        check(self._L.drf_stats(self._h, out))
        return dict(blocks=int(out[0]), updated_last=int(out[1]), updated_total=int(out[2]), mismatches=int(out[3]))

    def visited_blocks(self):
        """Blocks k_integrate has read so far (4 KB each): with stats()["updated_total"] the kernel's exact HBM bytes."""
        v = C.c_uint64()
        check(self._L.drf_visited_blocks(self._h, C.byref(v)))
        return int(v.value)

    def export_blocks(self):
        """Canonical dump: dict {(bx,by,bz): uint8[4096]} (512 voxels x {f32 sdf, u8 b,g,r, u8 weight})."""
        n = self.stats()["blocks"]
        coords = np.empty((max(n, 1), 3), np.int32)
        vox = np.empty((max(n, 1), 4096), np.uint8)
        got = C.c_int()
        check(self._L.drf_export_blocks(self._h, n, coords.ctypes.data_as(C.POINTER(C.c_int32)),
                                           vox.ctypes.data_as(u8p), C.byref(got)))
        return {tuple(int(v) for v in coords[i]): vox[i] for i in range(got.value)}

    def fast_div_status(self):
        """(enabled, mismatches) of the exact fast division self-check run at construction."""
        en, mm = C.c_int(), C.c_uint64()
        check(self._L.drf_fast_div_status(self._h, C.byref(en), C.byref(mm)))
        return bool(en.value), int(mm.value)

    def test_combine(self, a, b, max_weight):
        """Test hook: Combine(a[i], b[i]) by the integration kernel's device function; a, b: (n, 8) uint8 voxels."""
        a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        assert a.shape == b.shape and a.shape[1] == 8
        out = np.empty_like(a)
        check(self._L.drf_test_combine(self._h, a.shape[0], a.ctypes.data_as(u8p), b.ctypes.data_as(u8p), int(max_weight),
                                          out.ctypes.data_as(u8p)))
        return out

    def bench_sequence(self, d_bgr, d_depth, poses, render=True):
        """BASELINE configs[3] loop over frames resident in HBM (device pointers; poses (n, 16) float32): dict of
        milliseconds -- total (hipEvents), allocate / integrate / raycast / d2h sums, host wall clock."""
        ps = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        ms = (C.c_float * 6)()
        check(self._L.drf_bench_sequence(self._h, C.c_void_p(d_bgr), C.c_void_p(d_depth), fptr(ps), ps.shape[0], int(bool(render)), ms))
        return dict(total=ms[0], allocate=ms[1], integrate=ms[2], raycast=ms[3], d2h=ms[4], wall=ms[5])

    def bench_last_render(self, back=0, stream=0):
        """(bgr, depth) COPIES of the last (back=0) / second-to-last (back=1) ray-cast bench_sequence wrote for `stream` (test hook)."""
        b, d = C.c_void_p(), C.c_void_p()
        check(self._L.drf_bench_render_host(self._h, stream, back, C.byref(b), C.byref(d)))
        H, W = self._hw
        bgr = np.ctypeslib.as_array(C.cast(b, u8p), shape=(H, W, 3)).copy()
        depth = np.ctypeslib.as_array(C.cast(d, C.POINTER(C.c_float)), shape=(H, W)).copy()
        return bgr, depth

    # ---- streaming: bounded device pool + host store (include/dr_mi355x.h, DESIGN.md "Streaming voxel blocks") ----
    def set_streaming(self, radius, host_capacity_blocks=0):
        """radius 0 = off; otherwise >= streaming_min_radius(options).  host_capacity_blocks 0 = unbounded host store."""
        check(self._L.drf_set_streaming(self._h, float(radius), int(host_capacity_blocks)))

    def stream_out_region(self, lower, upper):
        """Moves every resident block whose origin lies in [lower, upper] to the host store."""
        lo, up = (np.ascontiguousarray(a, np.float32) for a in (lower, upper))
        check(self._L.drf_stream_out_region(self._h, fptr(lo), fptr(up)))

    def stream_in_region(self, lower, upper):
        """Brings every stored block whose origin lies in [lower, upper] back into the pool (DrError DR_ERR_CAPACITY, nothing moved, if they do not fit)."""
        lo, up = (np.ascontiguousarray(a, np.float32) for a in (lower, upper))
        check(self._L.drf_stream_in_region(self._h, fptr(lo), fptr(up)))

    def streaming_stats(self):
        out = (C.c_uint64 * 6)()
        check(self._L.drf_streaming_stats(self._h, out))
        return dict(resident=int(out[0]), host=int(out[1]), streamed_out=int(out[2]), streamed_in=int(out[3]), bytes_moved=int(out[4]),
                    last_scan_us=int(out[5]))

    def export_host_blocks(self):
        """The host store as export_blocks() formats the resident blocks."""
        n = self.streaming_stats()["host"]
        coords = np.empty((max(n, 1), 3), np.int32)
        vox = np.empty((max(n, 1), 4096), np.uint8)
        got = C.c_int()
        check(self._L.drf_export_host_blocks(self._h, n, coords.ctypes.data_as(C.POINTER(C.c_int32)), vox.ctypes.data_as(u8p), C.byref(got)))
        return {tuple(int(v) for v in coords[i]): vox[i] for i in range(got.value)}

    # ---- map files (include/dr_mi355x.h "map files", DESIGN.md "Saving and loading the map") ----
    def save_map(self, path, chunk_blocks=0):
        """The whole map -- resident blocks and host store -- to a file that depends on the map alone (tandem_amd.map_file
        reads it).  Changes nothing in the engine.  chunk_blocks bounds the pinned staging (0 = min(num_blocks, 8192))."""
        check(self._L.drf_save_map(self._h, os.fsencode(path), int(chunk_blocks)))

    def load_map(self, path, chunk_blocks=0):
        """A saved map into this engine, whose map must be empty: into the pool in key order (streaming off) or into the host
        store (streaming on).  DrError on a bad file (DR_ERR_IO), another voxel_size (DR_ERR_ARG), too many blocks
        (DR_ERR_CAPACITY) or a non-empty map (DR_ERR_PROTOCOL); the engine then stays empty and usable."""
        check(self._L.drf_load_map(self._h, os.fsencode(path), int(chunk_blocks)))

    def merge_map(self, path, chunk_blocks=0):
        """A saved map of the same world (same voxel_size and frame) merged into this engine's map: the union of the blocks, shared
        blocks combined voxel by voxel as a weighted average (include/dr_mi355x.h drf_merge_map states the rule).  DrError on a
        bad file (DR_ERR_IO), another voxel_size (DR_ERR_ARG) or too many new blocks (DR_ERR_CAPACITY); then nothing changed,
        except after a file that changed while it was read (DR_ERR_IO, merge_stats() tells how far the merge got)."""
        check(self._L.drf_merge_map(self._h, os.fsencode(path), int(chunk_blocks)))

    def merge_stats(self):
        """Last merge_map: (blocks in the file, blocks added, blocks combined in the pool, blocks combined in the host store,
        voxels taken verbatim, voxels averaged)."""
        out = (C.c_uint64 * 6)()
        check(self._L.drf_merge_stats(self._h, out))
        return tuple(int(v) for v in out)

    def transform_map(self, src, T, dst, chunk_blocks=0):
        """The map file src moved into this engine's world frame and written to dst: T (4x4, row-major, rigid) maps file-world to
        engine-world, p_engine = R p_file + t, and the surface is resampled on the engine's lattice (include/dr_mi355x.h
        drf_transform_map states the rule).  The engine's own map is not touched; merge_map(dst) or load_map(dst) follow.  DrError
        on a bad motion or another voxel_size (DR_ERR_ARG), a bad file (DR_ERR_IO) or a source that does not fit on the device
        (DR_ERR_CAPACITY); no partial dst is left."""
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        check(self._L.drf_transform_map(self._h, os.fsencode(src), T.ctypes.data_as(C.POINTER(C.c_float)), os.fsencode(dst), int(chunk_blocks)))

    def transform_stats(self):
        """Last transform_map: (source blocks, candidate destination blocks evaluated, blocks written, voxels written with
        weight > 0, voxels refused for a partly weighted neighbourhood, device bytes held for the source)."""
        out = (C.c_uint64 * 6)()
        check(self._L.drf_transform_stats(self._h, out))
        return tuple(int(v) for v in out)

    @staticmethod
    def _options(struct, word, opt):
        """opt as the options struct of the align / locate / track calls (None: all defaults)"""
        if not opt:
            return None
        unknown = set(opt) - {f[0] for f in struct._fields_}
        if unknown:
            raise TypeError("unknown %s option(s): %s" % (word, ", ".join(sorted(unknown))))
        return struct(**opt)

    def _image(self, dtype, channels, image):
        """An H*W*channels image of the engine's camera, or an integer device pointer to one: (is a device pointer, the argument,
        what keeps it alive)"""
        if isinstance(image, (int, np.integer)):
            return True, C.c_void_p(int(image)), None
        image = np.ascontiguousarray(image, dtype)
        assert image.size == self._hw[0] * self._hw[1] * channels
        return False, fptr(image) if dtype is np.float32 else C.c_void_p(image.ctypes.data), image

    def _align_result(self, r, T32, raise_on_failure):
        """What align_map, locate_frame, track_frame and track_colour_frame return, or raise as an AlignError that carries it"""
        res = AlignResult(T=np.array(r.T, np.float64).reshape(4, 4), T32=T32.reshape(4, 4), sums=np.array(r.sums, np.float64), samples=int(r.samples),
                          valid0=int(r.valid0), valid=int(r.valid), cost0=float(r.cost0), cost=float(r.cost), iterations=int(r.iterations),
                          status=int(r.status))
        if raise_on_failure and res.status in (ALIGN_DEGENERATE, ALIGN_LOST):
            raise AlignError(res, self._L.dr_last_error().decode(errors="replace"))
        return res

    def align_system(self, src, ref, T, **opt):
        """The registration's Gauss-Newton system at the pose T (4x4, row-major, rigid, src-world to ref-world): (sums (28,)
        float64, (samples, valid, invalid)).  sums[27] / valid is the mean robust squared residual in voxels^2 -- the score of a
        pose hypothesis -- and valid / samples the overlap.  opt: the fields of drf_align_options_t (include/dr_mi355x.h states
        the rule).  The engine's own map is not touched."""
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        o = self._options(_lib.AlignOptions, "align", opt)
        sums, counts = np.zeros(28, np.float64), (C.c_uint64 * 3)()
        check(self._L.drf_align_system(self._h, os.fsencode(src), os.fsencode(ref), fptr(T), C.byref(o) if o else None,
                                       sums.ctypes.data_as(_lib.f64p), counts))
        return sums, tuple(int(v) for v in counts)

    def align_map(self, src, ref, T_init=None, raise_on_failure=True, **opt):
        """Registers the map file src to the map file ref from T_init (default: the identity) and returns an AlignResult; its T32
        goes straight into transform_map(src, T32, dst), and merge_map(dst) into an engine that holds ref follows.  The call
        refines: T_init must bring the source surface inside the reference's truncation band.  A registration that ends
        ALIGN_DEGENERATE or ALIGN_LOST raises AlignError (which carries the result) unless raise_on_failure is false."""
        T = np.ascontiguousarray(np.eye(4) if T_init is None else T_init, np.float32).reshape(16)
        o = self._options(_lib.AlignOptions, "align", opt)
        T32, r = np.zeros(16, np.float32), _lib.AlignResultStruct()
        check(self._L.drf_align_map(self._h, os.fsencode(src), os.fsencode(ref), fptr(T), C.byref(o) if o else None, fptr(T32), C.byref(r)))
        return self._align_result(r, T32, raise_on_failure)

    def align_stats(self):
        """Last align_system / align_map: (source blocks, reference blocks, samples, valid samples at the last evaluation, system
        evaluations, device bytes held during the call)."""
        out = (C.c_uint64 * 6)()
        check(self._L.drf_align_stats(self._h, out))
        return tuple(int(v) for v in out)

    # ---- locating a depth frame in the map (include/dr_mi355x.h drf_locate_frame, DESIGN.md "Locating a depth frame in the map") ----
    def locate_system(self, depth, pose, **opt):
        """The localisation's Gauss-Newton system of the depth image (H*W float32 metres, or an integer device pointer to one) at
        the pose (16 float32, row-major, camera-to-world) against the map this engine holds: (sums (28,) float64, (samples, valid,
        unobserved, outside)).  sums[27] / valid is the mean robust squared residual in voxels^2, the score of a pose hypothesis.
        opt: the fields of drf_locate_options_t.  The map is not touched."""
        dev, d, keep = self._image(np.float32, 1, depth)
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        o = self._options(_lib.LocateOptions, "locate", opt)
        sums, counts = np.zeros(28, np.float64), (C.c_uint64 * 4)()
        call = self._L.drf_locate_system_device if dev else self._L.drf_locate_system
        check(call(self._h, d, fptr(pose), C.byref(o) if o else None, sums.ctypes.data_as(_lib.f64p), counts))
        return sums, tuple(int(v) for v in counts)

    def locate_frame(self, depth, pose_init, raise_on_failure=True, **opt):
        """Refines pose_init (camera-to-world) so that the depth image lies on the surface of the map this engine holds and returns
        an AlignResult (T, T32: camera-to-world); T32 is the pose IntegrateScanAsync takes to continue the map.  The call refines:
        pose_init must bring the points inside the truncation band (from farther off, track_frame first; with only a place, search_frame).  Only resident blocks are read (locate_stats()[5] counts the
        blocks in the host store) unless set_locate_scope(LOCATE_MAP) was called.  A refinement that ends ALIGN_DEGENERATE or ALIGN_LOST raises AlignError (which carries the
        result) unless raise_on_failure is false."""
        dev, d, keep = self._image(np.float32, 1, depth)
        pose = np.ascontiguousarray(pose_init, np.float32).reshape(16)
        o = self._options(_lib.LocateOptions, "locate", opt)
        T32, r = np.zeros(16, np.float32), _lib.AlignResultStruct()
        call = self._L.drf_locate_frame_device if dev else self._L.drf_locate_frame
        check(call(self._h, d, fptr(pose), C.byref(o) if o else None, fptr(T32), C.byref(r)))
        return self._align_result(r, T32, raise_on_failure)

    def locate_stats(self):
        """Last locate_system / locate_frame: (grid positions, samples, valid samples at the last evaluation, system evaluations,
        device bytes held during the call, blocks in the host store at the call)."""
        out = (C.c_uint64 * 6)()
        check(self._L.drf_locate_stats(self._h, out))
        return tuple(int(v) for v in out)

    def set_locate_scope(self, scope, stage_capacity_blocks=0):
        """LOCATE_RESIDENT (default): locate_system / locate_frame read the pool; LOCATE_MAP: the pool and the host store -- the
        same bits as on an engine whose pool holds the whole map, and no block moves.  The stored blocks an evaluation can read are
        staged through stage_capacity_blocks blocks of device scratch (0 = min(num_blocks, 8192)); a call that needs more raises
        DrError DR_ERR_CAPACITY and changes nothing."""
        check(self._L.drf_set_locate_scope(self._h, int(scope), int(stage_capacity_blocks)))

    def locate_stage_stats(self):
        """Last locate_system / locate_frame: (stagings made, blocks in the largest staging, blocks staged in total, evaluations
        that read a staging); all 0 in resident scope or with nothing to stage."""
        out = (C.c_uint64 * 4)()
        check(self._L.drf_locate_stage_stats(self._h, out))
        return tuple(int(v) for v in out)

    # ---- tracking a depth frame against the ray-cast model (include/dr_mi355x.h drf_track_frame, DESIGN.md "Tracking a depth frame") ----
    def _track_images(self, images):
        """The images of a tracking call in the C ABI's order, each (dtype, channels, image); an image None is one the call does
        without.  (Are they device pointers, the arguments, what keeps them alive.)"""
        got = [self._image(*i) if i[2] is not None else (None, None, None) for i in images]
        where = {g[0] for g in got if g[0] is not None}
        assert len(where) == 1, "all images on the host or all on the device"
        return where.pop(), [g[1] for g in got], got

    def _track_system(self, name, lead, images, model_pose, pose, o, ncounts):
        """What track_system, track_colour_system and track_pyramid_system do behind their options o: one evaluation by the C
        function `name` (or its _device twin), lead its arguments before the images, ncounts counters back."""
        dev, args, keep = self._track_images(images)
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        mpose = np.ascontiguousarray(model_pose, np.float32).reshape(16)
        sums, counts = np.zeros(28, np.float64), (C.c_uint64 * ncounts)()
        call = getattr(self._L, name + "_device" if dev else name)
        check(call(self._h, *lead, *args, fptr(mpose), fptr(pose), C.byref(o) if o else None, sums.ctypes.data_as(_lib.f64p), counts))
        return sums, tuple(int(v) for v in counts)

    def _track_frame(self, name, images, pose_init, o, raise_on_failure):
        """What track_frame, track_colour_frame and track_pyramid_frame do behind their options o"""
        dev, args, keep = self._track_images(images)
        pose = np.ascontiguousarray(pose_init, np.float32).reshape(16)
        T32, r = np.zeros(16, np.float32), _lib.AlignResultStruct()
        call = getattr(self._L, name + "_device" if dev else name)
        check(call(self._h, *args, fptr(pose), C.byref(o) if o else None, fptr(T32), C.byref(r)))
        return self._align_result(r, T32, raise_on_failure)

    def track_system(self, depth, model_depth, model_pose, pose, **opt):
        """One evaluation of the tracking's Gauss-Newton system: the depth image at the pose against model_depth, a ray-cast at
        model_pose (both images H*W float32 metres, or both integer device pointers): (sums (28,) float64, (samples, valid,
        unassociated, rejected)).  opt: the fields of drf_track_options_t.  No map is read."""
        o = self._options(_lib.TrackOptions, "track", opt)
        return self._track_system("drf_track_system", (), [(np.float32, 1, depth), (np.float32, 1, model_depth)], model_pose, pose, o, 4)

    def track_frame(self, depth, pose_init, raise_on_failure=True, **opt):
        """Tracks the depth image against the ray-cast model of the map this engine holds from pose_init (camera-to-world), which
        need only be good to decimetres and some ten degrees, and returns an AlignResult (T, T32: camera-to-world).  It ends within
        locate_frame's reach: track first, then locate_frame(depth, result.T32) for the sub-voxel part.  The renders follow
        set_render_scope and set_render_bands; the public render buffers and the map are not touched.  ALIGN_MAX_ITERS is a usable
        pose; ALIGN_DEGENERATE or ALIGN_LOST raises AlignError (which carries the result) unless raise_on_failure is false."""
        o = self._options(_lib.TrackOptions, "track", opt)
        return self._track_frame("drf_track_frame", [(np.float32, 1, depth)], pose_init, o, raise_on_failure)

    def track_stats(self):
        """Last track_system / track_frame: (grid positions, samples, valid samples at the last evaluation, system evaluations,
        renders, device bytes held)."""
        out = (C.c_uint64 * 6)()
        check(self._L.drf_track_stats(self._h, out))
        return tuple(int(v) for v in out)

    # ---- searching a pose lattice (include/dr_mi355x.h drf_search_frame, DESIGN.md "Searching a pose lattice") ----
    def score_poses(self, depth, poses, **opt):
        """The localisation's cost, without its Jacobian, of the depth image (H*W float32 metres, or an integer device pointer) at
        each of the n poses ((n, 4, 4) or (n, 16) float32, camera-to-world) against the resident map, in one kernel: (cost (n,)
        float64, counts (n, 4) uint32 = samples, valid, unobserved, outside, score (n,) float64; lower is better).  cost and
        counts are locate_system's sums[27] and counts at that pose, bit for bit.  opt: the fields of drf_score_options_t."""
        dev, d, keep = self._image(np.float32, 1, depth)
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        n = len(poses)
        o = self._options(_lib.ScoreOptions, "score", opt)
        cost, counts, score = np.zeros(n, np.float64), np.zeros((n, 4), np.uint32), np.zeros(n, np.float64)
        call = self._L.drf_score_poses_device if dev else self._L.drf_score_poses
        check(call(self._h, d, fptr(poses), n, C.byref(o) if o else None, cost.ctypes.data_as(_lib.f64p), counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                   score.ctypes.data_as(_lib.f64p)))
        return cost, counts, score

    def search_frame(self, depth, anchors, rotations=None, half=(0, 0, 0), trans_step=0.0, top_k=0, score_only=False, accept_valid=0.0, score=None, track=None,
                     locate=None, all_scores=False, raise_on_failure=True):
        """Finds the depth image in the map from a lattice of poses: every anchor ((n, 4, 4) float32 camera-to-world) turned by
        every rotation ((m, 9) float64, pose_rotations(); default: the identity) and moved by -half .. half offsets of trans_step
        metres (0: 2 * truncation_distance) along the world axes is scored in one kernel, the top_k (0: 8) best are tracked
        (track: drf_track_options_t fields) and located (locate: drf_locate_options_t fields), and the one with the most located
        valid samples wins.  score: drf_score_options_t fields.  Returns a SearchResult; one that found no pose raises AlignError
        (which carries it; T32 is then the best-scoring candidate) unless raise_on_failure is false."""
        dev, d, keep = self._image(np.float32, 1, depth)
        anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 16)
        rot = np.ascontiguousarray(np.eye(3).reshape(1, 9) if rotations is None else rotations, np.float64).reshape(-1, 9)
        so = self._options(_lib.ScoreOptions, "score", score or {}) or _lib.ScoreOptions()
        o = _lib.SearchOptions(score=so, trans_step=trans_step, half=(C.c_int * 3)(*[int(v) for v in half]), top_k=int(top_k), score_only=int(bool(score_only)),
                               accept_valid=float(accept_valid))
        to, lo = self._options(_lib.TrackOptions, "track", track or {}), self._options(_lib.LocateOptions, "locate", locate or {})
        n = len(anchors) * len(rot) * int(np.prod([2 * int(v) + 1 for v in half]))
        scores = np.zeros(max(n, 1), np.float64) if all_scores and 0 < n <= 1 << 24 else None
        T32, r = np.zeros(16, np.float32), _lib.SearchResultStruct()
        call = self._L.drf_search_frame_device if dev else self._L.drf_search_frame
        check(call(self._h, d, fptr(anchors), len(anchors), rot.ctypes.data_as(_lib.f64p), len(rot), C.byref(o), C.byref(to) if to else None,
                   C.byref(lo) if lo else None, fptr(T32), C.byref(r), scores.ctypes.data_as(_lib.f64p) if scores is not None else None))
        entries = [SearchEntry(index=int(e.index), score=float(e.score), cost=float(e.cost), counts=tuple(int(v) for v in e.counts), track_status=int(e.track_status),
                               locate_status=int(e.locate_status), samples=int(e.samples), valid=int(e.valid), located_cost=float(e.located_cost),
                               T=np.array(e.T, np.float64).reshape(4, 4)) for e in r.entries[:r.n_entries]]
        res = SearchResult(T32=T32.reshape(4, 4), status=int(r.status), winner=int(r.winner), refined=int(r.refined), n_candidates=int(r.n_candidates),
                           entries=entries, scores=scores)
        if raise_on_failure and res.status in (ALIGN_DEGENERATE, ALIGN_LOST):
            raise AlignError(res, self._L.dr_last_error().decode(errors="replace"))
        return res

    def search_stats(self):
        """Last score_poses / search_frame or their colour forms: (candidates, grid positions, samples, chunks, renders and system evaluations of the
        refinement, device bytes held by the score stage, blocks in the host store at the call)."""
        out = (C.c_uint64 * 8)()
        check(self._L.drf_search_stats(self._h, out))
        return tuple(int(v) for v in out)

    def set_search_scope(self, scope, stage_capacity_blocks=0):
        """SEARCH_RESIDENT (default): the score stage of score_poses / search_frame and their colour forms reads the pool;
        SEARCH_MAP: the pool and the host store -- the same bits as on an engine whose pool holds the whole map, and no block
        moves.  The candidates are planned into passes whose stored blocks fit stage_capacity_blocks blocks of device scratch
        (0 = min(num_blocks, 8192)); a single slab of the lattice that needs more raises DrError DR_ERR_CAPACITY and changes
        nothing.  The refinement keeps its own scopes: a search of the whole map wants set_render_scope(RENDER_MAP) and
        set_locate_scope(LOCATE_MAP) too."""
        check(self._L.drf_set_search_scope(self._h, int(scope), int(stage_capacity_blocks)))

    def search_stage_stats(self):
        """Last search call of either family: (stagings made, blocks in the largest staging, blocks staged in total, score
        launches that read a staging); all 0 in resident scope or with nothing to stage."""
        out = (C.c_uint64 * 4)()
        check(self._L.drf_search_stage_stats(self._h, out))
        return tuple(int(v) for v in out)

    # ---- searching with colour (include/dr_mi355x.h drf_search_colour_frame, DESIGN.md "Searching with colour") ----
    def score_colour_poses(self, bgr, depth, poses, **opt):
        """score_poses with the appearance term from the voxel colours: the frame's colour image (H*W*3 uint8 BGR, as
        IntegrateScanAsync takes it) beside its depth, both on the host or both integer device pointers.  Returns (cost, photo,
        counts, score): cost and counts are score_poses' bit for bit, photo (n,) float64 is the capped, Huber-weighted sum of the
        squared intensity differences between the map's trilinear colour and the frame at the valid samples, and score carries both.
        opt: the fields of drf_score_options_t, photo_weight and photo_cap."""
        dev, args, keep = self._track_images([(np.uint8, 3, bgr), (np.float32, 1, depth)])
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        n = len(poses)
        o = None
        if opt:
            opt = dict(opt)
            w, cap = opt.pop("photo_weight", 0.0), opt.pop("photo_cap", 0.0)
            o = _lib.ScoreColourOptions(self._options(_lib.ScoreOptions, "score", opt) or _lib.ScoreOptions(), w, cap)
        cost, photo, counts, score = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros((n, 4), np.uint32), np.zeros(n, np.float64)
        call = self._L.drf_score_colour_poses_device if dev else self._L.drf_score_colour_poses
        check(call(self._h, *args, fptr(poses), n, C.byref(o) if o else None, cost.ctypes.data_as(_lib.f64p), photo.ctypes.data_as(_lib.f64p),
                   counts.ctypes.data_as(C.POINTER(C.c_uint32)), score.ctypes.data_as(_lib.f64p)))
        return cost, photo, counts, score

    def search_colour_frame(self, bgr, depth, anchors, rotations=None, half=(0, 0, 0), trans_step=0.0, top_k=0, score_only=False, accept_valid=0.0, photo_weight=0.0,
                            photo_cap=0.0, score=None, track=None, levels=0, coarse_renders=0, track_photo_weight=0.0, locate=None, all_scores=False,
                            raise_on_failure=True):
        """search_frame where geometry alone is ambiguous -- one wall, a corridor: the candidates are scored with the appearance
        term (score_colour_poses), the top_k smallest colour scores are tracked with the frame's colour image (track_pyramid_frame's
        rule: track, levels, coarse_renders, track_photo_weight) and located, and the entry whose located pose has the smallest
        colour score (final_score) wins.  bgr and depth both on the host or both integer device pointers.  Returns a SearchResult
        whose entries are SearchColourEntry; one that found no pose raises AlignError unless raise_on_failure is false."""
        dev, args, keep = self._track_images([(np.uint8, 3, bgr), (np.float32, 1, depth)])
        anchors = np.ascontiguousarray(anchors, np.float32).reshape(-1, 16)
        rot = np.ascontiguousarray(np.eye(3).reshape(1, 9) if rotations is None else rotations, np.float64).reshape(-1, 9)
        so = self._options(_lib.ScoreOptions, "score", score or {}) or _lib.ScoreOptions()
        o = _lib.SearchColourOptions(_lib.SearchOptions(score=so, trans_step=trans_step, half=(C.c_int * 3)(*[int(v) for v in half]), top_k=int(top_k),
                                                        score_only=int(bool(score_only)), accept_valid=float(accept_valid)), photo_weight, photo_cap)
        to, lo = self._track_pyramid_options(levels, coarse_renders, track_photo_weight, track or {}), self._options(_lib.LocateOptions, "locate", locate or {})
        n = len(anchors) * len(rot) * int(np.prod([2 * int(v) + 1 for v in half]))
        scores = np.zeros(max(n, 1), np.float64) if all_scores and 0 < n <= 1 << 24 else None
        T32, r = np.zeros(16, np.float32), _lib.SearchColourResultStruct()
        call = self._L.drf_search_colour_frame_device if dev else self._L.drf_search_colour_frame
        check(call(self._h, *args, fptr(anchors), len(anchors), rot.ctypes.data_as(_lib.f64p), len(rot), C.byref(o), C.byref(to) if to else None,
                   C.byref(lo) if lo else None, fptr(T32), C.byref(r), scores.ctypes.data_as(_lib.f64p) if scores is not None else None))
        entries = [SearchColourEntry(index=int(e.index), score=float(e.score), cost=float(e.cost), counts=tuple(int(v) for v in e.counts),
                                     track_status=int(e.track_status), locate_status=int(e.locate_status), samples=int(e.samples), valid=int(e.valid),
                                     located_cost=float(e.located_cost), T=np.array(e.T, np.float64).reshape(4, 4), photo=float(e.photo),
                                     final_score=float(e.final_score), final_photo=float(e.final_photo)) for e in r.entries[:r.n_entries]]
        res = SearchResult(T32=T32.reshape(4, 4), status=int(r.status), winner=int(r.winner), refined=int(r.refined), n_candidates=int(r.n_candidates),
                           entries=entries, scores=scores)
        if raise_on_failure and res.status in (ALIGN_DEGENERATE, ALIGN_LOST):
            raise AlignError(res, self._L.dr_last_error().decode(errors="replace"))
        return res

    # ---- tracking with colour (include/dr_mi355x.h drf_track_colour_frame, DESIGN.md "Tracking with colour") ----
    @staticmethod
    def _track_colour_options(photo_weight, opt):
        if not opt and not photo_weight:
            return None
        return _lib.TrackColourOptions(DrFusion._options(_lib.TrackOptions, "track", opt) or _lib.TrackOptions(), photo_weight)

    def track_colour_system(self, bgr, depth, model_bgr, model_depth, model_pose, pose, photo_weight=0.0, **opt):
        """One evaluation of the tracking's system with the photometric term: the frame (bgr H*W*3 uint8, depth H*W float32) at the
        pose against the model's colour and depth, a ray-cast at model_pose (all four on the host or all four integer device
        pointers): (sums (28,) float64, (samples, valid, unassociated, rejected, photometric terms added)).  photo_weight: voxels
        per intensity unit, 0 = 1/27 times huber; opt: the fields of drf_track_options_t.  No map is read."""
        o = self._track_colour_options(photo_weight, opt)
        images = [(np.uint8, 3, bgr), (np.float32, 1, depth), (np.uint8, 3, model_bgr), (np.float32, 1, model_depth)]
        return self._track_system("drf_track_colour_system", (), images, model_pose, pose, o, 5)

    def track_colour_frame(self, bgr, depth, pose_init, raise_on_failure=True, photo_weight=0.0, **opt):
        """track_frame with the frame's colour image (as IntegrateScanAsync takes it) and a photometric term next to the geometric
        one: it holds the motion inside a plane, which track_frame leaves open (on one wall track_frame is ALIGN_DEGENERATE, this
        call is not).  Both images on the host, or both integer device pointers.  Returns an AlignResult whose cost carries both
        terms; ALIGN_DEGENERATE or ALIGN_LOST raises AlignError unless raise_on_failure is false."""
        o = self._track_colour_options(photo_weight, opt)
        return self._track_frame("drf_track_colour_frame", [(np.uint8, 3, bgr), (np.float32, 1, depth)], pose_init, o, raise_on_failure)

    def track_colour_stats(self):
        """Last track_colour_system / track_colour_frame: track_stats' fields; the device bytes are a buffer of these calls' own."""
        out = (C.c_uint64 * 6)()
        check(self._L.drf_track_colour_stats(self._h, out))
        return tuple(int(v) for v in out)

    # ---- tracking coarse to fine (include/dr_mi355x.h drf_track_pyramid_frame, DESIGN.md "Tracking coarse to fine") ----
    @staticmethod
    def _track_pyramid_options(levels, coarse_renders, photo_weight, opt):
        if not opt and not photo_weight and not levels and not coarse_renders:
            return None
        colour = DrFusion._track_colour_options(photo_weight, opt) or _lib.TrackColourOptions()
        return _lib.TrackPyramidOptions(colour, levels, coarse_renders)

    def track_reduce(self, level, max_jump, bgr, depth):
        """The pyramid's reduction of a full-resolution pair to `level` (2^level x 2^level blocks; max_jump in metres is the
        level's own): (bgr (H_L, W_L, 3) uint8 or None, depth (H_L, W_L) float32).  bgr None reduces the depth alone.  With integer
        device pointers, bgr and depth are (input, output) pairs of them and nothing is returned."""
        if isinstance(depth, tuple):
            cin, cout = bgr if bgr is not None else (None, None)
            check(self._L.drf_track_reduce_device(self._h, int(level), float(max_jump), cin, depth[0], cout, depth[1]))
            return None
        dev, d, keep = self._image(np.float32, 1, depth)
        assert not dev
        hl, wl = (self._hw[0] >> level, self._hw[1] >> level) if 0 <= level < 31 else (0, 0)
        dout = np.zeros((hl, wl), np.float32)
        c, cout = None, None
        if bgr is not None:
            _, c, ckeep = self._image(np.uint8, 3, bgr)
            cout = np.zeros((hl, wl, 3), np.uint8)
        check(self._L.drf_track_reduce(self._h, int(level), float(max_jump), c, d, C.c_void_p(cout.ctypes.data) if cout is not None else None,
                                       dout.ctypes.data_as(_lib.f32p)))
        return cout, dout

    def track_pyramid_system(self, level, bgr, depth, model_bgr, model_depth, model_pose, pose, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
        """One evaluation at `level` of the pyramid: both full-resolution pairs are reduced to the level, then
        track_colour_system's rule (bgr and model_bgr None: track_system's) with the level's camera: (sums (28,) float64, (samples,
        valid, unassociated, rejected, photometric terms added)).  All images on the host or all integer device pointers."""
        o = self._track_pyramid_options(levels, coarse_renders, photo_weight, opt)
        images = [(np.uint8, 3, bgr), (np.float32, 1, depth), (np.uint8, 3, model_bgr if bgr is not None else None), (np.float32, 1, model_depth)]
        return self._track_system("drf_track_pyramid_system", (int(level),), images, model_pose, pose, o, 5)

    def track_pyramid_frame(self, bgr, depth, pose_init, raise_on_failure=True, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
        """track_colour_frame (bgr None: track_frame) coarse to fine: `levels` (0 = 3) halvings of frame and model, the coarsest
        first with `coarse_renders` (0 = 3) renders each, then the full-resolution call from the pose they reach.  It cures a
        render that aliases the map's texture and minima at the texture's scale; it is no global search.  levels=1 is the
        single-level call bit for bit.  Returns level 0's AlignResult; then locate_frame(depth, result.T32)."""
        o = self._track_pyramid_options(levels, coarse_renders, photo_weight, opt)
        return self._track_frame("drf_track_pyramid_frame", [(np.uint8, 3, bgr), (np.float32, 1, depth)], pose_init, o, raise_on_failure)

    def track_pyramid_stats(self):
        """Last track_reduce / track_pyramid_*: (grid positions, samples, valid samples -- each summed over the levels' last
        evaluations -- evaluations, renders, device bytes held, levels run, levels abandoned)."""
        out = (C.c_uint64 * 8)()
        check(self._L.drf_track_pyramid_stats(self._h, out))
        return tuple(int(v) for v in out)

    def track_pyramid_level_stats(self, level):
        """Level `level` of the last track_pyramid_frame: (status, renders, evaluations, valid samples at its last evaluation)."""
        out = (C.c_uint64 * 4)()
        check(self._L.drf_track_pyramid_level_stats(self._h, int(level), out))
        return tuple(int(v) for v in out)

    # ---- tracking under a change of exposure (include/dr_mi355x.h drf_track_exposure_frame, DESIGN.md "Tracking under a change of exposure") ----
    _EXPOSURE_FIELDS = ("gain_init", "offset_init", "gain_min", "gain_max", "eps_gain", "eps_offset")

    @staticmethod
    def _track_exposure_options(levels, coarse_renders, photo_weight, opt):
        own = {k: opt.pop(k) for k in DrFusion._EXPOSURE_FIELDS if k in opt}
        pyramid = DrFusion._track_pyramid_options(levels, coarse_renders, photo_weight, opt)
        if pyramid is None and not own:
            return None
        return _lib.TrackExposureOptions(pyramid or _lib.TrackPyramidOptions(), **own)

    def track_exposure_system(self, level, bgr, depth, model_bgr, model_depth, model_pose, pose, gain=1.0, offset=0.0, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
        """One evaluation at `level` of the 8 x 8 system of pose, gain and offset, at the pose and the exposure (gain, offset):
        (sums (45,) float64 -- [0..27] track_pyramid_system's layout, [28..44] the gain and offset columns -- and (samples, valid,
        unassociated, rejected, photometric terms added)).  At (1, 0) sums[:28] are track_pyramid_system's bits.  All four images
        on the host or all integer device pointers; the colour images are required."""
        o = self._track_exposure_options(levels, coarse_renders, photo_weight, dict(opt))
        dev, args, keep = self._track_images([(np.uint8, 3, bgr), (np.float32, 1, depth), (np.uint8, 3, model_bgr), (np.float32, 1, model_depth)])
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        mpose = np.ascontiguousarray(model_pose, np.float32).reshape(16)
        sums, counts = np.zeros(45, np.float64), (C.c_uint64 * 5)()
        call = self._L.drf_track_exposure_system_device if dev else self._L.drf_track_exposure_system
        check(call(self._h, int(level), *args, fptr(mpose), fptr(pose), float(gain), float(offset), C.byref(o) if o else None, sums.ctypes.data_as(_lib.f64p), counts))
        return sums, tuple(int(v) for v in counts)

    def track_exposure_frame(self, bgr, depth, pose_init, raise_on_failure=True, levels=0, coarse_renders=0, photo_weight=0.0, **opt):
        """track_pyramid_frame with colour for a frame whose exposure differs from the map's: gain and offset (frame ~ gain * model
        + offset) are solved next to the pose, from gain_init (0 = 1) and offset_init, the gain kept in [gain_min, gain_max] (0 =
        0.25, 4).  On a map of one colour the exposure is held and the call is track_pyramid_frame bit for bit.  Returns an
        ExposureResult; compensate_exposure(bgr, result.gain, result.offset) is the frame to integrate."""
        o = self._track_exposure_options(levels, coarse_renders, photo_weight, dict(opt))
        dev, args, keep = self._track_images([(np.uint8, 3, bgr), (np.float32, 1, depth)])
        pose = np.ascontiguousarray(pose_init, np.float32).reshape(16)
        T32, r = np.zeros(16, np.float32), _lib.ExposureResultStruct()
        call = self._L.drf_track_exposure_frame_device if dev else self._L.drf_track_exposure_frame
        check(call(self._h, *args, fptr(pose), C.byref(o) if o else None, fptr(T32), C.byref(r)))
        try:
            a = self._align_result(r.pose, T32, raise_on_failure)
        except AlignError as e:
            a = e.result
            e.result = ExposureResult(*a, gain=float(r.gain), offset=float(r.offset), ext=np.array(r.ext, np.float64), photometric=int(r.photometric), held=int(r.held))
            raise
        return ExposureResult(*a, gain=float(r.gain), offset=float(r.offset), ext=np.array(r.ext, np.float64), photometric=int(r.photometric), held=int(r.held))

    def track_exposure_stats(self):
        """Last track_exposure_*: track_pyramid_stats' fields; the device bytes are a buffer of these calls' own."""
        out = (C.c_uint64 * 8)()
        check(self._L.drf_track_exposure_stats(self._h, out))
        return tuple(int(v) for v in out)

    def track_exposure_level_stats(self, level):
        """Level `level` of the last track_exposure_frame: (status, renders, evaluations, valid samples at its last evaluation)."""
        out = (C.c_uint64 * 4)()
        check(self._L.drf_track_exposure_level_stats(self._h, int(level), out))
        return tuple(int(v) for v in out)

    def set_render_scope(self, scope, stage_capacity_blocks=0):
        """RENDER_RESIDENT (default): renders read the pool; RENDER_MAP: the pool and the host store -- any pose renders as on an
        engine whose pool never ran out, the stored blocks in reach staged through stage_capacity_blocks blocks of device scratch
        (0 = min(num_blocks, 8192)); a RenderAsync that needs more raises DrError DR_ERR_CAPACITY and changes nothing."""
        check(self._L.drf_set_render_scope(self._h, int(scope), int(stage_capacity_blocks)))

    def render_stats(self):
        """Last RenderAsync: (stored blocks staged, bytes uploaded, poses that selected the whole store, 1 if it waited for the scan)."""
        out = (C.c_uint64 * 4)()
        check(self._L.drf_render_stats(self._h, out))
        return tuple(int(v) for v in out)

    def set_render_bands(self, max_passes):
        """0 or 1 (default): off.  2..64: a RENDER_MAP RenderAsync whose stored blocks exceed the staging runs in up to max_passes
        depth bands, staged and ray-cast one after the other -- the same images bit for bit; DR_ERR_CAPACITY only if no such
        plan exists."""
        check(self._L.drf_set_render_bands(self._h, int(max_passes)))

    def render_band_stats(self):
        """Last RenderAsync: (passes, blocks staged by the largest pass, blocks staged over all passes, 1 if it was banded)."""
        out = (C.c_uint64 * 4)()
        check(self._L.drf_render_band_stats(self._h, out))
        return tuple(int(v) for v in out)

    def set_mesh_scope(self, scope):
        """MESH_RESIDENT (default): meshes cover the pool; MESH_MAP: the pool and the host store, without moving a block."""
        check(self._L.drf_set_mesh_scope(self._h, int(scope)))

    def mesh_stats(self):
        """Last extraction: (blocks meshed, host blocks uploaded -- once per chunk that stages them, chunks)."""
        out = (C.c_uint64 * 3)()
        check(self._L.drf_mesh_stats(self._h, out))
        return tuple(int(v) for v in out)

    # ---- incremental mesh (include/dr_mi355x.h, DESIGN.md "Incremental mesh") ----
    def ExtractMeshUpdateAsync(self, lower_corner, upper_corner):
        """Launches a mesh update over the box: only the blocks whose triangles may have changed since the last update that
        was fetched are meshed again (all of them when the update is full).  Legal where ExtractMeshAsync is."""
        lo, up = (np.ascontiguousarray(a, np.float32) for a in (lower_corner, upper_corner))
        check(self._L.drf_extract_mesh_update_async(self._h, fptr(lo), fptr(up)))

    def mesh_update_size(self):
        """(listed blocks, triangles, full) of the pending update; waits for it, does not consume it."""
        nb, nt, full = C.c_size_t(), C.c_size_t(), C.c_int()
        check(self._L.drf_mesh_update_size(self._h, C.byref(nb), C.byref(nt), C.byref(full)))
        return int(nb.value), int(nt.value), bool(full.value)

    def GetMeshUpdateSync(self):
        """(full, coords (n, 3) int32, first (n + 1,) uint64, vert, cols): block i owns triangles [first[i], first[i + 1]) of
        vert / cols ((3 * triangles, 3) float32 as GetMeshSync's).  MeshPatches.apply takes the tuple."""
        nb, nt, _ = self.mesh_update_size()
        coords, first = np.empty((max(nb, 1), 3), np.int32), np.zeros(nb + 1, np.uint64)
        vert, cols = np.empty((max(3 * nt, 1), 3), np.float32), np.empty((max(3 * nt, 1), 3), np.float32)
        n, num, full = C.c_size_t(), C.c_size_t(), C.c_int()
        check(self._L.drf_get_mesh_update_sync(self._h, nb, max(3 * nt, 1), C.byref(n), coords.ctypes.data_as(C.POINTER(C.c_int32)),
                                               first.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(num), fptr(vert), fptr(cols), C.byref(full)))
        return bool(full.value), coords[:n.value], first, vert[:num.value], cols[:num.value]

    def GetMeshUpdate(self, lower_corner, upper_corner):
        self.ExtractMeshUpdateAsync(lower_corner, upper_corner)
        return self.GetMeshUpdateSync()

    def mesh_update_reset(self):
        """The next update is full."""
        check(self._L.drf_mesh_update_reset(self._h))

    def mesh_update_stats(self):
        """Last update launched: dict(scope=blocks in scope, meshed=blocks meshed again, scans=scans folded in, full)."""
        out = (C.c_uint64 * 4)()
        check(self._L.drf_mesh_update_stats(self._h, out))
        return dict(scope=int(out[0]), meshed=int(out[1]), scans=int(out[2]), full=bool(out[3]))

    def export_all_blocks(self):
        """The whole map: resident blocks and the host store merged (a block is in exactly one of them)."""
        a, b = self.export_blocks(), self.export_host_blocks()
        both = a.keys() & b.keys()
        assert not both, "blocks both resident and stored: %s" % sorted(both)[:3]
        a.update(b)
        return a

    def bench_integrate(self, bgrs, depths, poses):
        """Uploads the scans once, then times back-to-back allocate+integrate of all of them (HBM-resident)."""
        L = self._L
        n = len(bgrs)
        bg = np.ascontiguousarray(np.stack(bgrs), np.uint8)
        dp = np.ascontiguousarray(np.stack(depths), np.float32)
        ps = np.ascontiguousarray(np.stack([np.asarray(p, np.float32).reshape(16) for p in poses]), np.float32)
        d_b, d_d = C.c_void_p(), C.c_void_p()
        check(L.dr_device_alloc(0, bg.nbytes, C.byref(d_b)))
        check(L.dr_device_alloc(0, dp.nbytes, C.byref(d_d)))
        try:
            check(L.dr_memcpy_h2d(d_b, bg.ctypes.data_as(C.c_void_p), bg.nbytes))
            check(L.dr_memcpy_h2d(d_d, dp.ctypes.data_as(C.c_void_p), dp.nbytes))
            ms, kms = C.c_float(), C.c_float()
            check(L.drf_bench_integrate(self._h, d_b, d_d, fptr(ps), n, C.byref(ms), C.byref(kms)))
        finally:
            L.dr_device_free(d_b)
            L.dr_device_free(d_d)
        return ms.value, kms.value
