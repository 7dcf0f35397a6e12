// volume_kernels.h -- the TSDF volume on the device: the voxel, the block index (dense grid, presence bitmap, open-addressing
// table, bump pool), the coordinate maps, allocation and integration, and the small kernels every engine path shares.  Included by
// dr_fusion.hip first of the kernel headers (k_publish is launched by render_ops.h); raycast_kernels.h, stream_kernels.h, the pose kernels and mesh_kernels.h build on it.
//
// Replaces tandem/libdr/dr_fusion/src (CUDA, managed memory, try-lock hash inserts):
//   HashTable / Heap        tsdfvh/hash_table.cu, heap.cu  -> dense direct-mapped block grid (512^3 cells, one load per
//                                                           look-up) + presence bitmap + request list for block
//                                                           coordinates in [-256, 256)^3; a lock-free open-addressing
//                                                           table (64-bit CAS) outside it; bump pool
//   AllocateFromDepthKernel tsdfvh/tsdf_volume.cu:317-434 -> k_allocate   (one lane per pixel, DDA; new blocks are requested
//                                                           once per wave) + k_alloc_commit (pool slots, bitmap, superblock flags)
//   IntegrateScanKernel     tsdfvh/tsdf_volume.cu:436-513 -> k_cull (allocated blocks whose centre projects into the image)
//                                                           + k_integrate (one 64-lane wave per VISIBLE block, 8 voxels
//                                                           per lane, coalesced 4 KB block read-modify-write, one 12-byte
//                                                           pixel record per voxel) + k_fold_counter
//   GenerateRgbDepthKernel  tsdfvh/tsdf_volume.cu:600-632 -> k_raycast2 (one lane per pixel, sphere tracing; exact 3-instruction
//                                                           division verified against IEEE for all dividends, shared
//                                                           corner coordinates, empty-superblock skip) + k_raycast_fix;
//                                                           k_raycast = the literal form (DR_RAYCAST_V1, parity hook)
//   TsdfVolume::{IntegrateScanAsync,RenderAsync,GetRenderResult}  tsdf_volume.cu:515-737 -> FusionEngine
//   MeshExtractor / ExtractMeshAsync / GetMeshSync  marching_cubes/mesh_extractor.cu, tsdf_volume.cu:739-838
//                                                         -> mesh_kernels.h (per allocated block, LDS neighbourhood)
//
// Semantics follow the canonical form fixed by the CPU oracle (oracle/tsdf_oracle.c header): the voxel
// state keyed by block coordinate is bit-identical; hash slots and pool indices are implementation detail.
// fp32 arithmetic is written in the reference's expression order and compiled with -ffp-contract=off;
// divisions and square roots are IEEE-correct (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt).
#pragma once
#include "dr_common.h"
#include "fusion_host.h"  // kBS and the host's statement of the block key

namespace dr {

constexpr int kMaxDDA = 4096;  // cap on DDA steps per ray (the reference loops unboundedly)
constexpr unsigned long long kEmptyKey = ~0ull;

struct Voxel {  // tsdfvh/voxel.h:13-19 -- 8 bytes
  float sdf;
  unsigned char c[3];
  unsigned char weight;
};
static_assert(sizeof(Voxel) == 8, "voxel layout");

struct PixRec { float dep, sd; unsigned col; };  // written by k_allocate (one lane per pixel), read by k_integrate

struct FusionDev {  // everything the kernels need, passed by value
  drf_options_t o;
  unsigned long long *keys;  // [cap] packed block coordinate or kEmptyKey
  int *vals;                 // [cap] pool index
  unsigned cmask;            // cap - 1
  unsigned long long *blk_key;  // [num_blocks] key of pool block i
  Voxel *vox;                // [num_blocks * 512]
  int *n_alloc;              // allocated pool blocks
  int *err;                  // [0] pool exhausted, [1] coordinate out of packing range
  unsigned long long *cnt;   // [0] voxels updated by the current scan, [1] total, [2] round-trip mismatches
  float *sd;                 // [H*W] per-pixel surface distance |GetPoint3d(i, depth)| of the current scan
  unsigned char *super[2];   // per level: 1 = some block of this superblock of the dense grid is allocated (ray-cast empty-space skip)
  PixRec *pix;               // [H*W] {depth, surface distance, packed BGR} of the current scan: ONE gather per voxel in k_integrate
  unsigned *present;         // kPresentBits^3-bit map: bit set <=> that block is allocated (a cache of `grid`, no state)
  // Dense direct-mapped block index for the block coordinates [-256, 256)^3 (+-10 m at 5 mm voxels, +-20 m at 1 cm): one
  // int per cell, 512 MiB of the 288 GB -- 0 = absent, -1 = requested by the allocation pass of the current scan,
  // p + 1 = pool block p.  A block lookup inside the region is ONE load (ray-cast: 9 lookups per sphere-tracing step);
  // blocks outside it live in the open-addressing table above (keys / vals).
  int *grid;
  unsigned *req;             // [num_blocks] grid cells requested by the current scan (k_allocate -> k_alloc_commit)
  int *req_count;
  int *vis;                  // [num_blocks] pool blocks that pass IntegrateScanKernel's per-block test for the current scan
  int *vis_count;            // (k_cull -> k_integrate; == req_count + 1)
  unsigned *wg_upd;          // [integrate grid] voxels updated per workgroup of k_integrate (summed by k_fold_counter)
  float vs_rcp, fx_rcp, fy_rcp;  // correctly rounded reciprocals of voxel_size, fx, fy for the exact fast divisions below
  int fast_div;              // 1: the three reciprocals passed the exhaustive check against IEEE division (verify_fast_div)
};
constexpr int kPresentBits = 9;  // blocks within [-256, 256)^3: 16 MiB bitmap, L2/MALL resident
constexpr int kGridBits = kPresentBits;

// ---- CUDA float->int conversion semantics (cvt.rzi: saturate, NaN -> 0), see oracle header (4) ----
// v_cvt_i32_f32 IS that conversion (truncate, saturate, NaN -> 0: CDNA ISA "V_CVT_I32_F32"); written as inline asm
// because a C cast leaves out-of-range inputs undefined for the optimiser.  tests/test_fusion_gpu.py holds the kernels
// to the oracle's explicit branches bit for bit, out-of-range projections included.
__device__ inline int f2i(float f) {
  int r;
  asm("v_cvt_i32_f32_e32 %0, %1" : "=v"(r) : "v"(f));
  return r;
}
__device__ inline unsigned char f2u8(float f) {
  if (!(f > 0.0f)) return 0;
  if (f >= 255.0f) return 255;
  return (unsigned char)f;
}

// Exact fp32 division by a per-engine constant b (voxel_size, fx, fy) in three instructions instead of the ~12 of the IEEE
// sequence (v_div_scale/v_rcp/4 v_fma/v_div_fmas/v_div_fixup + two denormal-mode switches): with y = RN(1/b),
//   q0 = RN(a*y);  r = a - b*q0 (exact, one FMA);  q = RN(q0 + r*y)  ==  RN(a/b)
// (Markstein's correction step: q0 is within one ulp of a/b, the FMA residual is exact, the final FMA rounds correctly).
// Not taken on trust: FusionEngine's constructor checks q against a/b for ALL 2^32 dividends for each of the three
// divisors (k_verify_fast_div, ~10 ms each) and the kernels use the IEEE division if any finite dividend with
// 2^-100 <= |a| <= 2^100 (or a = 0) disagrees; dividends outside that range always take the IEEE path (in_fast_range).
__device__ inline float div_exact(float a, float b, float y) {
  const float q0 = a * y;
  const float r = __builtin_fmaf(-q0, b, a);
  return __builtin_fmaf(r, y, q0);
}
__device__ inline bool in_fast_range(float a) {  // 0, or 2^-100 <= |a| <= 2^100 (also false for NaN / Inf)
  const float m = fabsf(a);
  return a == 0.0f || (m >= 7.8886090522101181e-31f && m <= 1.2676506002282294e30f);
}
__global__ void k_verify_fast_div(float b, float y, unsigned long long *mismatches) {
  unsigned long long bad = 0;
  for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < (1ull << 32); i += (unsigned long long)gridDim.x * blockDim.x) {
    const float a = __uint_as_float((unsigned)i);
    if (!in_fast_range(a)) continue;
    const float q = div_exact(a, b, y), e = a / b;
    // +-0 compare equal on purpose: every use adds a signed 0.5 / subtracts floor() / feeds f2i (see get_voxel2)
    if (!(q == e)) ++bad;
  }
  if (bad) atomicAdd(mismatches, bad);
}

struct F3 { float x, y, z; };
struct I3 { int x, y, z; };
struct Mat { float m[16]; };

__device__ inline float norm3(F3 v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }  // utils.h:44-46
__device__ inline F3 xform(const Mat &T, F3 v) {                                          // matrix_utils.h:914-922
  F3 r;
  r.x = T.m[0] * v.x + T.m[1] * v.y + T.m[2] * v.z + T.m[3] * 1.0f;
  r.y = T.m[4] * v.x + T.m[5] * v.y + T.m[6] * v.z + T.m[7] * 1.0f;
  r.z = T.m[8] * v.x + T.m[9] * v.y + T.m[10] * v.z + T.m[11] * 1.0f;
  return r;
}
__device__ inline F3 point3d(const drf_options_t &o, int i, float depth) {  // utils.h:93-101
  const int v = i / o.width, u = i - o.width * v;
  F3 p;
  p.z = depth;
  p.x = ((float)u - o.cx) * p.z / o.fx;
  p.y = ((float)v - o.cy) * p.z / o.fy;
  return p;
}
__device__ inline void project(const drf_options_t &o, F3 p, int &px, int &py) {  // utils.h:103-108
  const float x = (o.fx * p.x) / p.z + o.cx;
  const float y = (o.fy * p.y) / p.z + o.cy;
  px = f2i(roundf(x));
  py = f2i(roundf(y));
}
__device__ inline float signf_(float n) { return (float)((n > 0) - (n < 0)); }
__device__ inline int signi(float n) { return (n > 0) - (n < 0); }

// ---- block-coordinate hash table ----
__device__ inline bool pack_key(I3 p, unsigned long long &k) {
  const int B = 1 << 20;
  if (p.x < -B || p.x >= B || p.y < -B || p.y >= B || p.z < -B || p.z >= B) return false;
  k = ((unsigned long long)(unsigned)(p.x + B) << 42) | ((unsigned long long)(unsigned)(p.y + B) << 21) | (unsigned long long)(unsigned)(p.z + B);
  return true;
}
// index of block p among the n ascending packed keys (binary search), -1 if it is not there
__device__ inline int find_sorted_key(const unsigned long long *keys, int n, I3 p) {
  unsigned long long key;
  if (!pack_key(p, key)) return -1;
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
  return lo < n && keys[lo] == key ? lo : -1;
}
__device__ inline I3 unpack_key(unsigned long long k) {
  const int B = 1 << 20;
  I3 p;
  p.x = (int)((k >> 42) & 0x1fffff) - B;
  p.y = (int)((k >> 21) & 0x1fffff) - B;
  p.z = (int)(k & 0x1fffff) - B;
  return p;
}
__device__ inline unsigned hash_key(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return (unsigned)k;
}
__device__ inline bool grid_index(I3 p, unsigned &idx) {  // dense region [-256, 256)^3, z fastest
  constexpr int H = 1 << (kGridBits - 1);
  const unsigned x = (unsigned)(p.x + H), y = (unsigned)(p.y + H), z = (unsigned)(p.z + H);
  if ((x | y | z) >> kGridBits) return false;
  idx = (x << (2 * kGridBits)) | (y << kGridBits) | z;
  return true;
}
// Occupancy of the dense grid at two coarser levels, for the ray-caster's empty-space skip: a "superblock" of level L is
// a cube of (1 << kSuperShift[L])^3 blocks; super[L][i] = 1 as soon as any block inside it is allocated.
// Level 0: 32^3 blocks (1.28 m at 5 mm voxels, 4 KiB of flags), level 1: 8^3 blocks (0.32 m, 256 KiB).
constexpr int kSuperLevels = 2;
constexpr int kSuperShift[kSuperLevels] = {5, 3};
template <int SH>
__device__ inline unsigned super_index(unsigned idx) {
  constexpr unsigned M = (1u << kGridBits) - 1;
  const unsigned x = idx >> (2 * kGridBits), y = (idx >> kGridBits) & M, z = idx & M;
  return ((x >> SH) << (2 * (kGridBits - SH))) | ((y >> SH) << (kGridBits - SH)) | (z >> SH);
}
__device__ inline int find_block_table(const FusionDev &d, I3 p) {  // blocks outside the dense region
  unsigned long long key;
  if (!pack_key(p, key)) return -1;
  unsigned s = hash_key(key) & d.cmask;
  for (unsigned probe = 0; probe <= d.cmask; ++probe) {
    const unsigned long long cur = d.keys[s];
    if (cur == key) return __hip_atomic_load(&d.vals[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // -1 while the inserting lane has not stored the pool index yet (vals starts at -1)
    if (cur == kEmptyKey) return -1;
    s = (s + 1) & d.cmask;
  }
  return -1;
}
__device__ inline int find_block(const FusionDev &d, I3 p) {
  unsigned idx;
  if (grid_index(p, idx)) return d.grid[idx] - 1;  // 0 / -1 (absent / only requested) -> negative
  return find_block_table(d, p);
}
// Insert-if-absent (HashTable::AllocateBlock, hash_table.cu:80-115, without the try-lock drop).
// The allocation DDA asks for ~60 blocks per pixel and, once a map exists, almost all of them are there already: a dense
// presence bitmap answers that with one load from a 16 MiB array.  A block that is NOT there yet is wanted by every ray
// that crosses it -- a few hundred lanes at about the same moment -- so the insert itself is made once per block:
//   * inside the dense region the first lane to turn the block's grid cell from 0 (absent) to -1 (requested) appends the
//     cell to the request list (lanes of one wave that want the same cell elect one of them first, so the word is hit by
//     one CAS per wave instead of one per lane; everybody else sees -1 with a plain load); k_alloc_commit then hands out
//     the pool blocks, one lane per request, no contention.  (Measured on the BASELINE configs[3] loop: the old path --
//     atomic load + CAS + atomicOr per lane per new block -- took 0.42-1.4 ms per frame while the map grew, 0.04 built.)
//   * outside it (|block coordinate| >= 256) the open-addressing table takes the insert directly, as before.
__device__ inline void allocate_block_table(const FusionDev &d, I3 p) {
  unsigned long long key;
  if (!pack_key(p, key)) { d.err[1] = 1; return; }
  unsigned s = hash_key(key) & d.cmask;
  for (unsigned probe = 0; probe <= d.cmask; ++probe) {
    unsigned long long cur = __hip_atomic_load(&d.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return;
    if (cur == kEmptyKey) {
      cur = atomicCAS(&d.keys[s], kEmptyKey, key);
      if (cur == kEmptyKey) {  // we own the slot: take a pool block
        const int idx = atomicAdd(d.n_alloc, 1);
        if (idx >= d.o.num_blocks) { d.err[0] = 1; return; }  // (vals[s] stays -1: the key is there, the block is not)
        d.blk_key[idx] = key;
        __hip_atomic_store(&d.vals[s], idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // readers in OTHER kernels see -1 or idx, never garbage
        atomicAdd(&d.n_alloc[3], 1);  // blocks living in the table (outside the dense grid)
        return;
      }
      if (cur == key) return;
    }
    s = (s + 1) & d.cmask;
  }
  d.err[0] = 1;
}
// Called by every lane of the wave in lockstep (`want` false for lanes that have nothing to insert at this DDA step).
__device__ inline void allocate_block(const FusionDev &d, I3 p, bool want) {
  unsigned idx = 0;
  const bool in_grid = want && grid_index(p, idx);
  bool need = in_grid && !((d.present[idx >> 5] >> (idx & 31)) & 1u);
  if (need) need = __hip_atomic_load(&d.grid[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
  unsigned long long todo = __ballot(need);
  if (todo) {
    const int lane = (int)(threadIdx.x & 63);
    bool won = false;
    while (todo) {  // one CAS per distinct cell per wave
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned lidx = (unsigned)__builtin_amdgcn_readlane((int)idx, leader);
      const unsigned long long same = __ballot(need && idx == lidx);
      if (lane == leader) won = atomicCAS(&d.grid[idx], 0, -1) == 0;
      todo &= ~same;
    }
    const unsigned long long wm = __ballot(won);  // the wave's new requests go to the list with ONE atomicAdd
    if (wm) {
      int base = 0;
      if (lane == __ffsll((long long)wm) - 1) base = atomicAdd(d.req_count, __popcll(wm));
      base = __builtin_amdgcn_readlane(base, __ffsll((long long)wm) - 1);
      if (won) {
        const int r = base + __popcll(wm & ((1ull << lane) - 1));
        if (r < d.o.num_blocks) d.req[r] = idx; else d.err[0] = 1;
      }
    }
  }
  if (want && !in_grid) allocate_block_table(d, p);
}
// One lane per requested cell: take a pool block (one atomicAdd per wave), publish it in the grid and the bitmap.
__global__ __launch_bounds__(256) void k_alloc_commit(const FusionDev d) {
  const int n = min(*d.req_count, d.o.num_blocks);
  const int lane = threadIdx.x & 63;
  for (int i0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63; i0 < n; i0 += gridDim.x * blockDim.x) {
    const int i = i0 + lane;
    const bool act = i < n;
    const unsigned long long m = __ballot(act);
    int base = 0;
    if (lane == 0) base = atomicAdd(d.n_alloc, __popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (!act) continue;
    const int p = base + __popcll(m & ((1ull << lane) - 1));
    const unsigned idx = d.req[i];
    if (p >= d.o.num_blocks) { d.err[0] = 1; d.grid[idx] = 0; continue; }
    constexpr int H = 1 << (kGridBits - 1);
    I3 c; c.x = (int)(idx >> (2 * kGridBits)) - H; c.y = (int)((idx >> kGridBits) & ((1u << kGridBits) - 1)) - H; c.z = (int)(idx & ((1u << kGridBits) - 1)) - H;
    unsigned long long key = 0;
    pack_key(c, key);
    d.blk_key[p] = key;
    d.grid[idx] = p + 1;
    atomicOr(&d.present[idx >> 5], 1u << (idx & 31));
    d.super[0][super_index<kSuperShift[0]>(idx)] = 1;  // plain stores: every writer writes the same value
    d.super[1][super_index<kSuperShift[1]>(idx)] = 1;
  }
}

// ---- coordinate maps, tsdf_volume.cu:109-145 ----
__device__ inline I3 world_to_global_voxel(const drf_options_t &o, F3 p) {
  const float vs = o.voxel_size;
  I3 r;
  r.x = f2i(p.x / vs + signf_(p.x) * 0.5f);
  r.y = f2i(p.y / vs + signf_(p.y) * 0.5f);
  r.z = f2i(p.z / vs + signf_(p.z) * 0.5f);
  return r;
}
__device__ inline int floor_div(int v, int bs) { return v < 0 ? (v - bs + 1) / bs : v / bs; }
__device__ inline int pos_mod(int v, int bs) { const int r = v % bs; return r < 0 ? r + bs : r; }
__device__ inline void world_to_block_local(const drf_options_t &o, F3 p, I3 &blk, int &local) {
  const I3 v = world_to_global_voxel(o, p);
  constexpr int bs = kBS;
  blk.x = floor_div(v.x, bs); blk.y = floor_div(v.y, bs); blk.z = floor_div(v.z, bs);
  local = pos_mod(v.x, bs) * bs * bs + pos_mod(v.y, bs) * bs + pos_mod(v.z, bs);  // voxel_block.h:37-41
}

// ------------------------------------------------------------------ allocation
__global__ __launch_bounds__(256) void k_allocate(const FusionDev d, const unsigned char *__restrict__ bgr, const float *__restrict__ depth, const Mat T) {
  const drf_options_t &o = d.o;
  const int size = o.height * o.width;
  const float trunc = o.truncation_distance;
  const float bsz = o.block_size * o.voxel_size;
  F3 start; start.x = T.m[3]; start.y = T.m[7]; start.z = T.m[11];
  // every lane of a wave walks its own ray, but the insert helper is called in lockstep (it elects one lane per distinct
  // block): lanes without a (valid) pixel, and lanes whose ray has ended, go along with want = false
  const int i_end = ((size + 63) / 64) * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < i_end; i += gridDim.x * blockDim.x) {
    bool live = i < size;
    const float dep = live ? depth[i] : 0.0f;
    // IntegrateScanKernel recomputes distance(0, GetPoint3d(idx, depth[idx])) for every voxel that projects to
    // pixel idx (tsdf_volume.cu:485-486); it depends on the pixel only, so it is evaluated once here.
    if (live) {
      const float sdist = norm3(point3d(o, i, dep));
      d.sd[i] = sdist;
      PixRec r; r.dep = dep; r.sd = sdist;
      r.col = (unsigned)bgr[3 * i] | ((unsigned)bgr[3 * i + 1] << 8) | ((unsigned)bgr[3 * i + 2] << 16);
      d.pix[i] = r;
    }
    if (dep < o.min_sensor_depth || dep > o.max_sensor_depth) live = false;
    const F3 point = xform(T, point3d(o, live ? i : 0, dep));
    if (point.x == 0 && point.y == 0 && point.z == 0) live = false;
    F3 dv; dv.x = point.x - start.x; dv.y = point.y - start.y; dv.z = point.z - start.z;
    const float dn = norm3(dv);
    F3 dir; dir.x = dv.x / dn; dir.y = dv.y / dn; dir.z = dv.z / dn;
    const float surf = norm3(dv);
    const float reach = surf + trunc;
    F3 re; re.x = start.x + dir.x * reach; re.y = start.y + dir.y * reach; re.z = start.z + dir.z * reach;
    I3 bp, be, st;
    bp.x = f2i(floorf(start.x / bsz)); bp.y = f2i(floorf(start.y / bsz)); bp.z = f2i(floorf(start.z / bsz));
    be.x = f2i(floorf(re.x / bsz)); be.y = f2i(floorf(re.y / bsz)); be.z = f2i(floorf(re.z / bsz));
    st.x = signi(dir.x); st.y = signi(dir.y); st.z = signi(dir.z);
    F3 dt, mt;
    dt.x = (dir.x != 0) ? fabsf(bsz / dir.x) : FLT_MAX;
    dt.y = (dir.y != 0) ? fabsf(bsz / dir.y) : FLT_MAX;
    dt.z = (dir.z != 0) ? fabsf(bsz / dir.z) : FLT_MAX;
    const float bdx = (bp.x + (float)st.x) * bsz, bdy = (bp.y + (float)st.y) * bsz, bdz = (bp.z + (float)st.z) * bsz;
    mt.x = (dir.x != 0) ? (bdx - start.x) / dir.x : FLT_MAX;
    mt.y = (dir.y != 0) ? (bdy - start.y) / dir.y : FLT_MAX;
    mt.z = (dir.z != 0) ? (bdz - start.z) / dir.z : FLT_MAX;
    I3 diff; diff.x = diff.y = diff.z = 0;
    bool neg = false;
    if (bp.x != be.x && dir.x < 0) { diff.x--; neg = true; }
    if (bp.y != be.y && dir.y < 0) { diff.y--; neg = true; }
    if (bp.z != be.z && dir.z < 0) { diff.z--; neg = true; }
    allocate_block(d, bp, live);
    if (__any(live && neg)) {
      if (live && neg) { bp.x += diff.x; bp.y += diff.y; bp.z += diff.z; }
      allocate_block(d, bp, live && neg);
    }
    int steps = 0;
    for (;;) {
      const bool go = live && (bp.x != be.x || bp.y != be.y || bp.z != be.z) && steps++ < kMaxDDA;
      if (!__any(go)) break;
      if (go) {
        if (mt.x < mt.y) {
          if (mt.x < mt.z) { bp.x += st.x; mt.x += dt.x; } else { bp.z += st.z; mt.z += dt.z; }
        } else {
          if (mt.y < mt.z) { bp.y += st.y; mt.y += dt.y; } else { bp.z += st.z; mt.z += dt.z; }
        }
      }
      allocate_block(d, bp, go);
    }
  }
}

// ------------------------------------------------------------------ integration
// Voxel::Combine (voxel.h:21-50).  The colour channels are  uchar((c*w + vc*vw) / (w + vw))  with integer-valued
// operands (c, vc <= 255, w <= 255, vw = 1): the quotient is either an exact integer or at least 1/(w+vw) away from
// one, so the truncated IEEE quotient equals floor(num/den) and can be taken from a 1-ulp reciprocal with a bias of
// half that gap -- bit-identical to the reference's division, a quarter of the instructions.
// (IntegrateScanKernel always passes vw = 1; the general case keeps the division.)
__device__ inline void combine(Voxel &a, const Voxel &b, unsigned char max_weight) {
  const float w = (float)a.weight, vw = (float)b.weight;
  const float den = w + vw;
  if (b.weight == 1) {
    const float r = __builtin_amdgcn_rcpf(den), bias = 0.5f * r;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.c[k] = (unsigned char)(int)(((float)a.c[k] * w + (float)b.c[k]) * r + bias);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.c[k] = f2u8(((float)a.c[k] * w + (float)b.c[k] * vw) / den);
  }
  a.sdf = (a.sdf * w + b.sdf * vw) / den;
  unsigned char nw = (unsigned char)(a.weight + b.weight);
  if (nw > max_weight) nw = max_weight;
  a.weight = nw;
}

// Test hook (drf_test_combine): the SAME device function on arbitrary voxel pairs, so that the reciprocal shortcut above can be
// checked exhaustively against the reference's Voxel::Combine.
__global__ void k_test_combine(const Voxel *__restrict__ a, const Voxel *__restrict__ b, Voxel *__restrict__ out, size_t n, int max_weight) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Voxel v = a[i];
    combine(v, b[i], (unsigned char)max_weight);
    out[i] = v;
  }
}

// One WAVE per allocated pool block (4 waves per workgroup, grid-strided): per-block work (pose transform of the
// block origin, frustum test) is done once per wave, then 8 iterations of 64 voxels (lane = y*8+z of slab x), each
// a coalesced 512-byte read-modify-write of the block.
// IntegrateScanKernel's per-block test (tsdf_volume.cu:451-470: block origin in front of the camera plane, block centre
// projects into the image) for EVERY allocated block, one LANE per block; survivors go to the visible list (one
// atomicAdd per wave).  The map keeps growing while the camera sees a room-sized part of it: with one wave per allocated
// block this test was half of k_integrate's instructions at 110 k blocks and would dominate at a million.
// The test itself, a pure function of (block coordinates, Ti, options): shared with the mesh update's selection kernel
// (mesh_update_kernels.h), which must agree with the visible list to the last bit.  pc = the block origin in the camera frame.
__device__ inline bool cull_block_visible(const drf_options_t &o, const I3 P, const Mat &Ti, F3 &pc) {
  constexpr int bs = kBS;
  const float vs = o.voxel_size;
  F3 position; position.x = P.x * vs * bs; position.y = P.y * vs * bs; position.z = P.z * vs * bs;
  pc = xform(Ti, position);
  if (pc.z < 0) return false;
  F3 center;  // tsdf_volume.cu:461-465 -- the half-block offset is added in double
  center.x = (float)((double)pc.x + 0.5 * (double)vs * (double)bs);
  center.y = (float)((double)pc.y + 0.5 * (double)vs * (double)bs);
  center.z = (float)((double)pc.z + 0.5 * (double)vs * (double)bs);
  int cx, cy;
  project(o, center, cx, cy);
  return cx >= 0 && cy >= 0 && cx < o.width && cy < o.height;
}
__global__ __launch_bounds__(256) void k_cull(const FusionDev d, const Mat Ti) {
  const drf_options_t &o = d.o;
  const int lane = threadIdx.x & 63;
  const int n_blocks = min(*d.n_alloc, o.num_blocks);  // written by k_alloc_commit earlier on this stream
  __shared__ int wcount[4], wbase;
  for (int e0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63; (e0 & ~255) < n_blocks; e0 += gridDim.x * blockDim.x) {  // uniform per workgroup
    const int e = e0 + lane;
    bool vis = false;
    if (e < n_blocks) {
      F3 pc;
      vis = cull_block_visible(o, unpack_key(d.blk_key[e]), Ti, pc);
    }
    // one atomicAdd per WORKGROUP and iteration (a single address takes ~10^8 atomics/s: one per wave was measurable)
    const unsigned long long m = __ballot(vis);
    const int wave = threadIdx.x >> 6;
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      const int tot = wcount[0] + wcount[1] + wcount[2] + wcount[3];
      wbase = tot ? atomicAdd(d.vis_count, tot) : 0;
    }
    __syncthreads();
    int base = wbase;
    for (int w = 0; w < wave; ++w) base += wcount[w];
    if (vis) d.vis[base + __popcll(m & ((1ull << lane) - 1))] = e;
    __syncthreads();
  }
}

// A voxel is 8 bytes at an 8-byte-aligned address, but `Voxel` itself only promises the alignment of its float: read as a
// struct it becomes a dword load plus a byte load per field (18 gathers per ray-cast sample).  One 64-bit load instead,
// and one 128-bit load for two voxels that are neighbours in z.
struct alignas(8) Voxel8 { unsigned lo, hi; };
struct __attribute__((packed, aligned(8))) Voxel16 { unsigned a, b, c, d; };
__device__ inline Voxel unpack_voxel(unsigned lo, unsigned hi) {
  Voxel v;
  v.sdf = __uint_as_float(lo);
  v.c[0] = (unsigned char)(hi & 255u); v.c[1] = (unsigned char)((hi >> 8) & 255u); v.c[2] = (unsigned char)((hi >> 16) & 255u);
  v.weight = (unsigned char)(hi >> 24);
  return v;
}
__device__ inline Voxel load_voxel(const Voxel *p) {
  const Voxel8 t = *reinterpret_cast<const Voxel8 *>(p);
  return unpack_voxel(t.lo, t.hi);
}

// One WAVE per VISIBLE block (k_cull's list).
#ifndef DR_INTEGRATE_WAVES
#define DR_INTEGRATE_WAVES 1
#endif
__global__ __launch_bounds__(256, DR_INTEGRATE_WAVES) void k_integrate(const FusionDev d, const unsigned char *__restrict__ bgr,
                                                   const float *__restrict__ depth, const Mat T, const Mat Ti) {
  const drf_options_t &o = d.o;
  constexpr int bs = kBS;
  const float vs = o.voxel_size, trunc = o.truncation_distance, inv_vs = 1.0f / o.voxel_size;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int by = lane >> 3, bz = lane & 7;
  unsigned upd = 0;
  const int n_vis = *d.vis_count;
  // The block of iteration i is named by two dependent look-ups (vis[] -> blk_key[]).  Both are wave-uniform (scalar
  // loads) and fetched ahead -- the list entry two blocks ahead, the key one block ahead -- so that no iteration starts
  // with a round trip to L2 before it can issue its voxel loads.
  const int stride = gridDim.x * 4;
  int iv = blockIdx.x * 4 + wave;
  int e_next = iv < n_vis ? d.vis[iv] : 0;
  int e_next2 = iv + stride < n_vis ? d.vis[iv + stride] : 0;
  unsigned long long key_next = d.blk_key[e_next];
  for (; iv < n_vis; iv += stride) {
    const int e = e_next;
    const I3 P = unpack_key(key_next);
    e_next = e_next2;
    key_next = d.blk_key[e_next];
    e_next2 = iv + 2 * stride < n_vis ? d.vis[iv + 2 * stride] : 0;
    F3 position; position.x = P.x * vs * bs; position.y = P.y * vs * bs; position.z = P.z * vs * bs;
    const F3 pc = xform(Ti, position);
    Voxel *blk_vox = d.vox + (size_t)e * (bs * bs * bs);
    // the block's 4 KB first: these are the loads that go to HBM, and nothing below depends on them until the combine --
    // the corner test, 8 projections and 8 pixel gathers run under their latency (sched_barrier: hipcc otherwise sinks
    // them behind the gathers).  Requesting the NEXT block's 4 KB here as well (two blocks per wave in flight, 121 VGPRs)
    // measured 8 % slower: after the changes above the kernel is bound by vector-ALU issue, not by latency.
    Voxel cur8[bs];
#pragma unroll
    for (int bx = 0; bx < bs; ++bx) cur8[bx] = load_voxel(blk_vox + bx * (bs * bs) + lane);
    __builtin_amdgcn_sched_barrier(0);
    // UpdateVoxel's world -> cam -> world round trip (below) is, per voxel, the map  vp -> T*(Ti*vp)  = an affine map
    // plus fp32 rounding noise (< 1e-4 m for |coordinates| < 64 m).  An affine deviation is extremal at the corners of
    // the block's voxel lattice, so if its 8 corner voxels come back within 0.1 voxel of themselves, every voxel of the
    // block comes back within 0.1 + noise/vs < 0.25 voxel, i.e. onto itself (see the per-voxel test's comment): the
    // round trip is then skipped for the whole block.  Lanes 0..7 test one corner each; any failure, a far-away block or
    // a sub-2 mm grid leaves the per-voxel test in charge.
    bool block_same = false;
    {
      const int kx = (lane & 1) ? bs - 1 : 0, ky = (lane & 2) ? bs - 1 : 0, kz = (lane & 4) ? bs - 1 : 0;
      F3 cv; cv.x = position.x + kx * vs; cv.y = position.y + ky * vs; cv.z = position.z + kz * vs;
      const F3 cw = xform(T, xform(Ti, cv));
      const bool near = fabsf(cw.x * inv_vs - (float)(P.x * bs + kx)) < 0.1f && fabsf(cw.y * inv_vs - (float)(P.y * bs + ky)) < 0.1f &&
                        fabsf(cw.z * inv_vs - (float)(P.z * bs + kz)) < 0.1f;
      const bool small = fabsf(cv.x) < 64.f && fabsf(cv.y) < 64.f && fabsf(cv.z) < 64.f && fabsf(pc.x) < 64.f && fabsf(pc.y) < 64.f && fabsf(pc.z) < 64.f;
      block_same = (__ballot(near && small) & 0xffull) == 0xffull && vs >= 0.002f;
    }
    if (block_same) {
      // Fast path (every voxel is known to map onto itself): the 8 slabs' loads are independent, so issue all of them
      // before any is consumed -- the kernel is bound by the depth -> surface/colour -> voxel load chain, not by ALU.
      F3 vpc[bs];
      int pix[bs];
      float dep8[bs], sd8[bs];
      unsigned col8[bs];
#pragma unroll
      for (int bx = 0; bx < bs; ++bx) {
        F3 vp; vp.x = position.x + bx * vs; vp.y = position.y + by * vs; vp.z = position.z + bz * vs;
        vpc[bx] = xform(Ti, vp);
        int ix, iy;
        project(o, vpc[bx], ix, iy);
        const bool inb = ix >= 0 && iy >= 0 && ix < o.width && iy < o.height;
        pix[bx] = inb ? iy * o.width + ix : -1;
        const int idx = inb ? pix[bx] : 0;
        const PixRec r = d.pix[idx];  // depth[idx], d.sd[idx], bgr[3 idx ..] in one 12-byte gather
        dep8[bx] = r.dep; sd8[bx] = r.sd; col8[bx] = r.col;
      }
#pragma unroll
      for (int bx = 0; bx < bs; ++bx) {
        const float dep = dep8[bx], sd = sd8[bx];
        if (pix[bx] < 0 || dep <= 0 || dep < o.min_sensor_depth || dep > o.max_sensor_depth) continue;
        const float vd = norm3(vpc[bx]);
        Voxel v;
        bool hit = false;
        if (vd > sd - trunc && vd < sd + trunc && dep < o.max_sensor_depth) { v.sdf = sd - vd; hit = true; }
        else if (vd < sd - trunc) { v.sdf = trunc; hit = true; }
        if (!hit) continue;
        v.c[0] = (unsigned char)(col8[bx] & 255u); v.c[1] = (unsigned char)((col8[bx] >> 8) & 255u); v.c[2] = (unsigned char)((col8[bx] >> 16) & 255u);
        v.weight = 1;
        Voxel cur = cur8[bx];
        combine(cur, v, (unsigned char)o.max_sdf_weight);
        blk_vox[bx * (bs * bs) + lane] = cur;
        ++upd;
      }
      continue;
    }
#pragma unroll 2
    for (int bx = 0; bx < bs; ++bx) {
      const int li = bx * (bs * bs) + lane;
      F3 vp; vp.x = position.x + bx * vs; vp.y = position.y + by * vs; vp.z = position.z + bz * vs;
      vp = xform(Ti, vp);
      int ix, iy;
      project(o, vp, ix, iy);
      if (!(ix >= 0 && iy >= 0 && ix < o.width && iy < o.height)) continue;
      const int idx = iy * o.width + ix;
      const float dep = depth[idx];
      if (dep <= 0) continue;
      if (dep < o.min_sensor_depth) continue;
      if (dep > o.max_sensor_depth) continue;
      const float sd = d.sd[idx];
      const float vd = norm3(vp);
      Voxel v;
      bool hit = false;
      if (vd > sd - trunc && vd < sd + trunc && dep < o.max_sensor_depth) { v.sdf = sd - vd; hit = true; }
      else if (vd < sd - trunc) { v.sdf = trunc; hit = true; }
      if (!hit) continue;
      v.c[0] = bgr[3 * idx]; v.c[1] = bgr[3 * idx + 1]; v.c[2] = bgr[3 * idx + 2];
      v.weight = 1;
      // UpdateVoxel re-derives block and voxel from the world position (tsdf_volume.cu:303-315):
      //   g = trunc(wp/vs + sign(wp)*0.5) per axis, block = floor(g/8), local = g mod 8.
      // Sufficient test without the three divisions: if |wp * (1/vs) - n| < 0.25 for this lane's own global voxel
      // index n on every axis, then |wp/vs - n| < 0.3 and the truncation above yields exactly n (for n = 0 as well),
      // i.e. the round trip lands on this lane's voxel.  Otherwise the literal path decides.
      Voxel *dst = blk_vox + li;
      if (!block_same) {
      const F3 wp = xform(T, vp);
      const bool same = fabsf(wp.x * inv_vs - (float)(P.x * bs + bx)) < 0.25f && fabsf(wp.y * inv_vs - (float)(P.y * bs + by)) < 0.25f &&
                        fabsf(wp.z * inv_vs - (float)(P.z * bs + bz)) < 0.25f;
      if (!same) {
        I3 blk; int local;
        world_to_block_local(o, wp, blk, local);
        if (blk.x != P.x || blk.y != P.y || blk.z != P.z || local != li) {
          atomicAdd(&d.cnt[2], 1ull);
          const int target = find_block(d, blk);
          if (target < 0) continue;
          dst = d.vox + (size_t)target * (bs * bs * bs) + local;
        }
      }
      }
      Voxel cur = *dst;
      combine(cur, v, (unsigned char)o.max_sdf_weight);
      *dst = cur;
      ++upd;
    }
  }
  // voxels updated: one plain store per workgroup (k_fold_counter adds them up) instead of an atomicAdd per wave on one
  // address -- with one block per wave that atomic was the longest thing the kernel did
  for (int off = 32; off > 0; off >>= 1) upd += __shfl_down(upd, off);
  __shared__ unsigned wupd[4];
  if (lane == 0) wupd[wave] = upd;
  __syncthreads();
  if (threadIdx.x == 0) d.wg_upd[blockIdx.x] = wupd[0] + wupd[1] + wupd[2] + wupd[3];
}

__global__ void k_zero_int(int *p) { if (threadIdx.x == 0 && blockIdx.x == 0) *p = 0; }

__global__ __launch_bounds__(256) void k_fold_counter(unsigned long long *cnt, int *req_count, const unsigned *wg_upd, int n_wg) {
  // end of scan: this scan's update count -> last / total, request and visible lists emptied
  __shared__ unsigned long long part[256];
  unsigned long long a = 0;
  for (int i = threadIdx.x; i < n_wg; i += 256) a += wg_upd[i];
  part[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) { if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off]; __syncthreads(); }
  if (threadIdx.x == 0) { const unsigned long long u = part[0] + cnt[0]; cnt[1] += u; cnt[3] = u; cnt[0] = 0; cnt[4] += (unsigned long long)req_count[1]; req_count[0] = 0; req_count[1] = 0; }  // cnt[4]: blocks k_integrate visited (each one a 4 KB read), all scans
}
__global__ void k_fill_keys(unsigned long long *keys, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) keys[i] = kEmptyKey;
}

// Hands a finished render to the host: both images are written straight into the pinned result buffers by ONE kernel (16-byte
// stores over PCIe) instead of two copy-engine transfers behind the ray-cast -- each of those costs its own launch and completion
// latency, which for 2 MB is most of the time (0.14 ms for the pair against 0.05 ms here, DESIGN.md "render hand-off").
__global__ __launch_bounds__(256) void k_publish(const unsigned char *__restrict__ a, unsigned char *__restrict__ ha, size_t na,
                                                 const unsigned char *__restrict__ b, unsigned char *__restrict__ hb, size_t nb) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  const size_t qa = na >> 4, qb = nb >> 4;
  for (size_t i = t; i < qa + qb; i += nt) {
    if (i < qa) reinterpret_cast<uint4 *>(ha)[i] = reinterpret_cast<const uint4 *>(a)[i];
    else reinterpret_cast<uint4 *>(hb)[i - qa] = reinterpret_cast<const uint4 *>(b)[i - qa];
  }
  for (size_t i = (qa << 4) + t; i < na; i += nt) ha[i] = a[i];
  for (size_t i = (qb << 4) + t; i < nb; i += nt) hb[i] = b[i];
}

}  // namespace dr
