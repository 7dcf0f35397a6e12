// dr_fusion.hip -- MI355X engine behind the DrFusion operator API (C ABI: include/dr_mi355x.h).
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
#include <cfloat>
#include <climits>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include <rocprim/rocprim.hpp>  // device radix sort (block keys) and exclusive scan (triangle offsets) of the mesh path

#include "dr_common.h"
#include "fusion_host.h"  // the host half of the map: block keys (kBS), reach bounds, host store, chunk planner
#include "hip_owner.h"    // HipOwner, DeviceBuf, PinnedBuf: what the engine takes from the runtime
#include "map_file.h"     // the map file: MapWriter, MapReader (host only)
#define DR_MC_CONST __device__ static const
#include "mc_tables.h"

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

// ------------------------------------------------------------------ raycast
}  // namespace dr
#include "raycast_kernels.h"  // k_raycast2 / k_raycast_fix (k_raycast: parity build), resident and STAGED (map-scope renders)
namespace dr {

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

#include "stream_kernels.h"
#include "align_kernels.h"  // k_map_align / k_align_fold (drf_align_system, drf_align_map)
#include "locate_kernels.h"  // k_map_locate (drf_locate_system, drf_locate_frame)
#include "track_kernels.h"   // k_track_model, k_track (drf_track_system, drf_track_frame)
#include "track_colour_kernels.h"  // k_track_model_colour, k_track_colour (drf_track_colour_system, drf_track_colour_frame)
#include "track_pyramid_kernels.h"  // k_track_reduce (drf_track_reduce, drf_track_pyramid_system, drf_track_pyramid_frame)

}  // namespace dr
#include "mesh_kernels.h"
#include "mesh_update_kernels.h"
#include "map_ops.h"  // MapIo: what the map-file operations share; drf_transform_map / drf_align_* whole
namespace dr {

// cofactor inverse on the host in the reference's term order (matrix_utils.h:958-1083), fp32, no contraction
static void inverse4_host(const float *e, float *out) {
  float inv[16];
  auto t3 = [&](int a, int b, int c) { return e[a] * e[b] * e[c]; };
  inv[0] = t3(5, 10, 15) - t3(5, 11, 14) - t3(9, 6, 15) + t3(9, 7, 14) + t3(13, 6, 11) - t3(13, 7, 10);
  inv[4] = -t3(4, 10, 15) + t3(4, 11, 14) + t3(8, 6, 15) - t3(8, 7, 14) - t3(12, 6, 11) + t3(12, 7, 10);
  inv[8] = t3(4, 9, 15) - t3(4, 11, 13) - t3(8, 5, 15) + t3(8, 7, 13) + t3(12, 5, 11) - t3(12, 7, 9);
  inv[12] = -t3(4, 9, 14) + t3(4, 10, 13) + t3(8, 5, 14) - t3(8, 6, 13) - t3(12, 5, 10) + t3(12, 6, 9);
  inv[1] = -t3(1, 10, 15) + t3(1, 11, 14) + t3(9, 2, 15) - t3(9, 3, 14) - t3(13, 2, 11) + t3(13, 3, 10);
  inv[5] = t3(0, 10, 15) - t3(0, 11, 14) - t3(8, 2, 15) + t3(8, 3, 14) + t3(12, 2, 11) - t3(12, 3, 10);
  inv[9] = -t3(0, 9, 15) + t3(0, 11, 13) + t3(8, 1, 15) - t3(8, 3, 13) - t3(12, 1, 11) + t3(12, 3, 9);
  inv[13] = t3(0, 9, 14) - t3(0, 10, 13) - t3(8, 1, 14) + t3(8, 2, 13) + t3(12, 1, 10) - t3(12, 2, 9);
  inv[2] = t3(1, 6, 15) - t3(1, 7, 14) - t3(5, 2, 15) + t3(5, 3, 14) + t3(13, 2, 7) - t3(13, 3, 6);
  inv[6] = -t3(0, 6, 15) + t3(0, 7, 14) + t3(4, 2, 15) - t3(4, 3, 14) - t3(12, 2, 7) + t3(12, 3, 6);
  inv[10] = t3(0, 5, 15) - t3(0, 7, 13) - t3(4, 1, 15) + t3(4, 3, 13) + t3(12, 1, 7) - t3(12, 3, 5);
  inv[14] = -t3(0, 5, 14) + t3(0, 6, 13) + t3(4, 1, 14) - t3(4, 2, 13) - t3(12, 1, 6) + t3(12, 2, 5);
  inv[3] = -t3(1, 6, 11) + t3(1, 7, 10) + t3(5, 2, 11) - t3(5, 3, 10) - t3(9, 2, 7) + t3(9, 3, 6);
  inv[7] = t3(0, 6, 11) - t3(0, 7, 10) - t3(4, 2, 11) + t3(4, 3, 10) + t3(8, 2, 7) - t3(8, 3, 6);
  inv[11] = -t3(0, 5, 11) + t3(0, 7, 9) + t3(4, 1, 11) - t3(4, 3, 9) - t3(8, 1, 7) + t3(8, 3, 5);
  inv[15] = t3(0, 5, 10) - t3(0, 6, 9) - t3(4, 1, 10) + t3(4, 2, 9) + t3(8, 1, 6) - t3(8, 2, 5);
  const float det = e[0] * inv[0] + e[1] * inv[4] + e[2] * inv[8] + e[3] * inv[12];
  const float detr = 1.0f / det;
  for (int i = 0; i < 16; ++i) out[i] = inv[i] * detr;
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

// A (bgr, depth) image pair of the engine's camera as a tracking call is given it: both on the host, or both on the device.
// bgr null: the depth alone.
struct FramePair {
  const void *bgr, *depth;
  bool on_host;
  static FramePair host(const uint8_t *bgr, const float *depth) { return {bgr, depth, true}; }
  static FramePair device(const void *bgr, const void *depth) { return {bgr, depth, false}; }
  bool has(bool colour) const { return depth && (!colour || bgr); }  // the images a call with or without colour reads
};

// ------------------------------------------------------------------ engine
constexpr int kDefaultFusionPriority = 1;  // 0 least (the reference's), 1 normal (measured best in the TandemBackend loop), 2 greatest
class FusionEngine {
  struct Render {
    hipStream_t stream;
    unsigned char *d_bgr, *h_bgr[2], *hd_bgr[2];   // hd_*: the pinned result buffers as the device addresses them
    float *d_depth, *h_depth[2], *hd_depth[2];
    int *d_flag;  // pixels the fast ray-caster handed to the literal pass
    RayState *d_band = nullptr;  // per-pixel state of a depth-banded render (allocated by the first one)
    hipEvent_t done, cast;  // result on the host / ray-cast kernels finished (the volume may be written again)
  };

 public:
  FusionEngine(const drf_options_t &o, int device) : device_(device), o_(o), mio_(own_, device, o.voxel_size, (size_t)std::min(o.num_blocks, kStageBlocks)) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device) fail(DR_ERR_DEVICE, "DrFusion: no HIP device %d (found %d) -- the MI355X path has no CPU fallback", device, n);
    if (o.block_size != 8) fail(DR_ERR_UNSUPPORTED, "DrFusion: block_size must be 8 (got %d)", o.block_size);
    if (o.num_blocks >= (1 << 30) - 1) fail(DR_ERR_UNSUPPORTED, "DrFusion: num_blocks must be below 2^30 - 1 (got %d)", o.num_blocks);
    if (o.height <= 0 || o.width <= 0 || o.num_blocks <= 0 || o.num_buckets <= 0 || o.bucket_size <= 0 || o.num_render_streams < 0)
      fail(DR_ERR_ARG, "DrFusion: invalid options");
    DR_HIP(hipSetDevice(device_));
    // Stream priority of the integrate and render streams.  The reference creates them at the LEAST priority with a note that
    // higher may be better (tsdf_volume.cu:64-70).  DR_FUSION_PRIORITY=low|normal|high selects it here; see DESIGN.md
    // "TandemBackend loop" for the measurement behind the default.
    int least, greatest;
    DR_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    int lo = kDefaultFusionPriority == 2 ? greatest : (kDefaultFusionPriority == 1 ? 0 : least);
    if (const char *e = getenv("DR_FUSION_PRIORITY")) lo = !strcmp(e, "high") ? greatest : (!strcmp(e, "normal") ? 0 : (!strcmp(e, "low") ? least : lo));
    int_stream_ = mio_.stream = own_.stream(lo);
    npix_ = (size_t)o.height * o.width;
    size_t cap = 1024;
    const size_t want = std::max((size_t)o.num_buckets * (size_t)o.bucket_size, (size_t)2 * o.num_blocks);
    while (cap < want) cap <<= 1;
    d_.o = o;
    d_.keys = own_.device<unsigned long long>(cap);
    d_.vals = own_.device<int>(cap);
    // -1 everywhere: an insert publishes the key (CAS) BEFORE it stores the pool index, so a concurrent reader -- the ray-cast of scan k
    // beside the allocation of scan k + 1 (enqueue_scan) -- may match a key whose value is not there yet; it then reads -1 = absent, which
    // is the state the block was in a moment ago (its voxels are still all unobserved: the same ray-cast result either way)
    DR_HIP(hipMemsetAsync(d_.vals, 0xFF, cap * sizeof(int), int_stream_));
    d_.cmask = (unsigned)(cap - 1);
    d_.blk_key = own_.device<unsigned long long>(o.num_blocks);
    d_.vox = own_.device<Voxel>((size_t)o.num_blocks * 512, int_stream_);  // hash_table.cu:28-32
    d_.n_alloc = own_.device<int>(4, int_stream_);
    d_.err = d_.n_alloc + 1;
    d_.cnt = own_.device<unsigned long long>(8, int_stream_);
    d_.sd = own_.device<float>(npix_);
    d_.pix = own_.device<PixRec>(npix_);
    for (int l = 0; l < kSuperLevels; ++l) d_.super[l] = own_.device<unsigned char>((size_t)1 << (3 * (kGridBits - kSuperShift[l])), int_stream_);
    d_.present = own_.device<unsigned>((size_t)1 << (3 * kPresentBits - 5), int_stream_);
    d_.grid = own_.device<int>((size_t)1 << (3 * kGridBits), int_stream_);
    d_.req = own_.device<unsigned>(o.num_blocks);
    d_.req_count = own_.device<int>(4, int_stream_);
    d_.vis_count = d_.req_count + 1;
    d_.vis = own_.device<int>(o.num_blocks);
    d_.wg_upd = own_.device<unsigned>(65536);
    setup_fast_div();
    hipLaunchKernelGGL(k_fill_keys, dim3(1024), dim3(256), 0, int_stream_, d_.keys, cap);
    d_bgr_in_ = own_.device<unsigned char>(npix_ * 3);
    d_depth_in_ = own_.device<float>(npix_);
    h_bgr_in_ = own_.pinned<unsigned char>(npix_ * 3);
    h_depth_in_ = own_.pinned<float>(npix_);
    // 12 workgroups per CU: enough to keep every SIMD's 4 resident waves busy, few enough that the blocks being worked on
    // at any moment are neighbours in the pool (sweep on the bench map: 1024 / 3072 / 4096 / 6144 / 8192 / 16384
    // workgroups -> 0.341 / 0.327 / 0.329 / 0.363 / 0.443 / 0.697 ms per scan)
    integrate_grid_ = std::min(cdiv(o.num_blocks, 4), 3072);
    if (const char *e = hook_env("DR_INT_GRID")) integrate_grid_ = std::min(65536, std::max(1, atoi(e)));  // tuning hook
    int_done_ = own_.event();
    for (int i = 0; i < o.num_render_streams; ++i) {
      Render r;
      r.stream = own_.stream(lo);
      r.d_bgr = own_.device<unsigned char>(npix_ * 3);
      r.d_depth = own_.device<float>(npix_);
      r.d_flag = own_.device<int>(4);
      for (int k = 0; k < 2; ++k) {  // double-buffered host results ("blocked"/"free", tsdf_volume.cu:846-872)
        r.h_bgr[k] = own_.pinned<unsigned char>(npix_ * 3, &r.hd_bgr[k]);
        r.h_depth[k] = own_.pinned<float>(npix_, &r.hd_depth[k]);
      }
      r.done = own_.event();
      r.cast = own_.event();
      renders_.push_back(r);
    }
    DR_HIP(hipStreamSynchronize(int_stream_));
  }
  ~FusionEngine() {  // the device idle before the growable scratch goes; own_ (declared first, so released last) frees the rest
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
  }

  // tsdf_volume.cu:515-598
  void integrate_scan_async(const uint8_t *bgr, const float *depth, const float *pose16) {
    if (!bgr || !depth || !pose16) fail(DR_ERR_ARG, "IntegrateScanAsync: null argument");
    expect(kIntegrate, "Please call the functions like Integration -> RenderAsync -> GetRenderResults.");
    if (st_radius_ <= 0.0f && !store_.empty()) fail(DR_ERR_PROTOCOL, "IntegrateScanAsync: %zu blocks are in the host store while streaming is off; bring them back with drf_stream_in_region first", store_.size());
    next_ = kRender; loaded_ = false;
    DR_HIP(hipSetDevice(device_));
    const float depth_bound = st_radius_ > 0.0f ? max_valid_depth(depth, npix_, o_.min_sensor_depth, o_.max_sensor_depth) : 0.0f;
    scan_between_streaming(pose16, depth_bound, [&] {
      memcpy(h_bgr_in_, bgr, npix_ * 3);
      memcpy(h_depth_in_, depth, npix_ * 4);
      DR_HIP(hipMemcpyAsync(d_bgr_in_, h_bgr_in_, npix_ * 3, hipMemcpyHostToDevice, int_stream_));
      DR_HIP(hipMemcpyAsync(d_depth_in_, h_depth_in_, npix_ * 4, hipMemcpyHostToDevice, int_stream_));
      // the ray-casts read the volume; their result copies do not (the reference waits for the copies, tsdf_volume.cu:553-556)
      enqueue_scan(d_bgr_in_, d_depth_in_, pose16, true);
    });
  }
  // One scan: the previous scan's use of the pinned buffers awaited, blocks streamed in before and out after, int_done_ behind it
  template <class Enqueue> void scan_between_streaming(const float *pose16, float depth_bound, Enqueue enqueue) {
    DR_HIP(hipEventSynchronize(int_done_));
    if (st_radius_ > 0.0f) stream_before_scan(pose16, depth_bound);
    enqueue();
    if (st_radius_ > 0.0f) stream_after_scan(pose16);
    DR_HIP(hipEventRecord(int_done_, int_stream_));
  }
  // The product's ray-cast: the flag counter cleared, the two-round-trip sampler (SAMPLER 0: round 2's, parity build), the literal pass
  // for the pixels it flagged.  The staging is a trailing pack as in the kernels: none = resident, one RenderStage = staged, a
  // RenderBand behind it = one depth band of a staged render (the flag counter is cleared before the first band only).
  template <int SAMPLER, class... SG>
  void raycast_pass(hipStream_t st, unsigned char *d_bgr, float *d_depth, int *d_flag, const Mat &P, bool zero_flag, const SG &...stage) {
    constexpr bool STAGED = sizeof...(SG) != 0, BANDED = sizeof...(SG) == 2;
    const dim3 grid(8 * cdiv(cdiv((int)npix_, 64), 8)), block(64);
    if (zero_flag) hipLaunchKernelGGL(k_zero_int, dim3(1), dim3(1), 0, st, d_flag);
    FusionDev dv = d_;
    if (raycast_no_skip_) dv.super[0] = nullptr;  // DR_RAYCAST_NO_SKIP=1: every sample is looked up (A/B and parity hook)
    if (d_.fast_div) hipLaunchKernelGGL((k_raycast2<true, false, SAMPLER, STAGED, BANDED>), grid, block, 0, st, dv, P, d_bgr, d_depth, d_flag, (unsigned long long *)nullptr, stage...);
    else hipLaunchKernelGGL((k_raycast2<false, false, SAMPLER, STAGED, BANDED>), grid, block, 0, st, dv, P, d_bgr, d_depth, d_flag, (unsigned long long *)nullptr, stage...);
    hipLaunchKernelGGL((k_raycast_fix<STAGED, BANDED>), dim3(512), dim3(64), 0, st, d_, P, d_bgr, d_depth, d_flag, stage...);
  }
  // sg: the host blocks staged for this render (map scope with stored blocks in reach), nullptr = the resident kernels;
  // band: this launch is one depth band of the render (sg is then that band's staging)
  void launch_raycast(hipStream_t st, unsigned char *d_bgr, float *d_depth, int *d_flag, const Mat &P, const RenderStage *sg = nullptr,
                      const RenderBand *band = nullptr) {
#ifdef DR_PARITY_HOOKS  // the superseded generations have no staged form (render_async refuses them)
    const dim3 grid(8 * cdiv(cdiv((int)npix_, 64), 8)), block(64);
    if (raycast_v1_) { hipLaunchKernelGGL(k_raycast, grid, block, 0, st, d_, P, d_bgr, d_depth); return; }
    if (raycast_stats_ && d_.fast_div) {  // DR_RAYCAST_STATS=1: a synchronous, counting launch of the same loop (prints to stderr)
      hipLaunchKernelGGL(k_zero_int, dim3(1), dim3(1), 0, st, d_flag);
      FusionDev dv = d_;
      if (raycast_no_skip_) dv.super[0] = nullptr;
      if (!d_rstats_) d_rstats_ = own_.device<unsigned long long>(32);
      DR_HIP(hipMemsetAsync(d_rstats_, 0, 32 * 8, st));
      hipLaunchKernelGGL((k_raycast2<true, true>), grid, block, 0, st, dv, P, d_bgr, d_depth, d_flag, d_rstats_);
      unsigned long long h[32];
      DR_HIP(hipMemcpyAsync(h, d_rstats_, sizeof h, hipMemcpyDeviceToHost, st));
      DR_HIP(hipStreamSynchronize(st));
      fprintf(stderr, "raycast stats: waves %llu  iterations/lane %.1f  longest ray %llu  mean wave-longest %.1f | per lane: missing-block samples %.1f, full samples %.1f, skip events %.2f (%.1f steps)\n  wave-longest histogram (x16):",
              h[7], (double)h[0] / (64.0 * h[7]), h[1], (double)h[2] / h[7], (double)h[3] / (64.0 * h[7]), (double)h[6] / (64.0 * h[7]), (double)h[4] / (64.0 * h[7]), (double)h[5] / (64.0 * h[7]));
      for (int i = 0; i < 24; ++i) fprintf(stderr, " %llu", h[8 + i]);
      fprintf(stderr, "\n");
      hipLaunchKernelGGL(k_raycast_fix<false>, dim3(512), dim3(64), 0, st, d_, P, d_bgr, d_depth, d_flag);
      return;
    }
    if (raycast_sampler_ == 0) return raycast_pass<0>(st, d_bgr, d_depth, d_flag, P, true);  // DR_RAYCAST_SAMPLER=0: the four-stage sampler of round 2
#endif
    if (band) raycast_pass<1>(st, d_bgr, d_depth, d_flag, P, band->first != 0, *sg, *band);
    else if (sg) raycast_pass<1>(st, d_bgr, d_depth, d_flag, P, true, *sg);
    else raycast_pass<1>(st, d_bgr, d_depth, d_flag, P, true);
  }
  // One render on its stream, behind the scan: ray-cast (sg: the staged host blocks it also reads, behind their staging), `cast`,
  // hand-off to the host (k_publish; DR_RENDER_D2H=copy, parity build: the two hipMemcpyAsync of round 2), `done`.
  // timing: three events around the ray-cast and the hand-off (bench_sequence).
  // band: one depth band of the render -- z_hi and `first` given, the stream's state filled in here; the hand-off follows the
  // last band only (`cast` is recorded behind every band: the staging stream waits for it before it takes the band's flags back).
  void submit_render(Render &r, const Mat &P, const RenderStage *sg, hipEvent_t *timing = nullptr, const RenderBand *band = nullptr, bool last = true) {
    if (!band || band->first) DR_HIP(hipStreamWaitEvent(r.stream, int_done_, 0));
    if (sg) rs_.wait_ready(r.stream);
    if (timing) DR_HIP(hipEventRecord(timing[0], r.stream));
    if (band) {
      if (!r.d_band) r.d_band = own_.device<RayState>(npix_);
      RenderBand b = *band;
      b.state = r.d_band;
      launch_raycast(r.stream, r.d_bgr, r.d_depth, r.d_flag, P, sg, &b);
    } else
      launch_raycast(r.stream, r.d_bgr, r.d_depth, r.d_flag, P, sg);
    if (timing) DR_HIP(hipEventRecord(timing[1], r.stream));
    DR_HIP(hipEventRecord(r.cast, r.stream));
    if (!last) return;
    if (render_copy_) {
      DR_HIP(hipMemcpyAsync(r.h_bgr[free_slot_], r.d_bgr, npix_ * 3, hipMemcpyDeviceToHost, r.stream));
      DR_HIP(hipMemcpyAsync(r.h_depth[free_slot_], r.d_depth, npix_ * 4, hipMemcpyDeviceToHost, r.stream));
    } else
      hipLaunchKernelGGL(k_publish, dim3(128), dim3(256), 0, r.stream, (const unsigned char *)r.d_depth, (unsigned char *)r.hd_depth[free_slot_], npix_ * 4,
                         (const unsigned char *)r.d_bgr, r.hd_bgr[free_slot_], npix_ * 3);
    if (timing) DR_HIP(hipEventRecord(timing[2], r.stream));
    DR_HIP(hipEventRecord(r.done, r.stream));
  }
  // tsdf_volume.cu:634-700
  void render_async(const float *const *poses, int n) {
    // (a map that was loaded or merged may be rendered before its next scan: drf_load_map, drf_merge_map)
    if (!(loaded_ && next_ == kIntegrate)) expect(kRender, "Please call the functions like IntegrateScanAsync -> RenderAsync -> GetRenderResult.");
    if (n != (int)renders_.size()) fail(DR_ERR_PROTOCOL, "Can only render exactly as many poses as streams. Streams: %zu, Poses: %d.", renders_.size(), n);
    DR_HIP(hipSetDevice(device_));
    // map scope: the stored blocks these poses can read, decided before anything changes (DR_ERR_CAPACITY leaves all as it was)
    RenderStagePlan plan;
    RenderBandPlan bands;
    bool waited = false;
    if (render_scope_ == DRF_RENDER_MAP) {
      for (int i = 0; i < n; ++i) if (!poses[i]) fail(DR_ERR_ARG, "RenderAsync: null pose");
      plan_render_call("RenderAsync", poses, n, plan, bands, waited);
    }
    next_ = kGetRender;
    free_slot_ ^= 1;  // write into the buffers NOT handed out by the last GetRenderResult
    const PassStats ps = render_passes(plan, bands, renders_.data(), poses, n, true);
    render_stats_[0] = plan.keys.size(); render_stats_[1] = ps.total * (size_t)(8 + 4096);
    render_stats_[2] = (uint64_t)plan.whole; render_stats_[3] = waited ? 1 : 0;
    band_stats_[0] = ps.staged ? ps.passes : 0; band_stats_[1] = ps.largest; band_stats_[2] = ps.total; band_stats_[3] = bands.ok ? 1 : 0;
  }
  // What a map-scope render of these poses stages (drf_render_async, and drf_track_frame for its model): the union of the stored
  // blocks in reach, or depth bands of it, or DR_ERR_CAPACITY before anything changes.
  void plan_render_call(const char *who, const float *const *poses, int n, RenderStagePlan &plan, RenderBandPlan &bands, bool &waited) {
    plan = plan_render(poses, n, waited);
    if (!render_stage_fits(plan, rs_capacity())) {
      // depth bands (drf_set_render_bands): the union may exceed the staging as long as every band fits it
      if (render_bands_ >= 2) bands = plan_render_bands(store_, o_, poses, n, rs_capacity(), render_bands_);
      if (!bands.ok)
        fail(DR_ERR_CAPACITY, "%s: the poses can read %zu stored blocks, the render staging holds %zu (drf_set_render_scope%s)", who, plan.keys.size(), rs_capacity(),
             render_bands_ >= 2 ? "; no plan of depth bands within drf_set_render_bands either" : "");
    }
#ifdef DR_PARITY_HOOKS
    if (!plan.keys.empty() && (raycast_v1_ || raycast_stats_ || raycast_sampler_ == 0))
      fail(DR_ERR_UNSUPPORTED, "%s: the superseded ray-cast generations have no staged form (DRF_RENDER_MAP with stored blocks in reach)", who);
#endif
  }
  // The planned render on the n streams of rs, pose i on rs[i]; handoff: the result goes to the host behind the last pass
  // (drf_render_async), otherwise it stays in rs[i]'s device buffers (drf_track_frame's model).
  struct PassStats { size_t passes, largest, total; bool staged; };
  PassStats render_passes(const RenderStagePlan &plan, const RenderBandPlan &bands, Render *rs, const float *const *poses, int n, bool handoff) {
    const bool staged = !plan.keys.empty();  // nothing to stage: exactly the resident launches
    // One pass stages the union; a banded render one depth band after the other.  The two slots of rs_ alternate, so band j + 1 is
    // packed and copied while band j ray-casts; all render streams take a band together and share its staging.
    const size_t passes = bands.ok ? bands.keys.size() : 1;
    size_t largest = 0, total = 0;
    for (size_t j = 0; j < passes; ++j) {
      const std::vector<unsigned long long> &keys = bands.ok ? bands.keys[j] : plan.keys;
      largest = std::max(largest, keys.size());
      total += keys.size();
    }
    if (bands.ok) ensure_render_staging(largest);  // (grown once, before the first band is in flight)
    for (size_t j = 0; j < passes; ++j) {
      RenderStage sg{};
      if (staged) sg = stage_render(bands.ok ? bands.keys[j] : plan.keys);
      RenderBand band{};
      band.z_hi = bands.ok ? bands.z[j + 1] : 0.0f;
      band.first = j == 0;
      for (int i = 0; i < n; ++i) {
        Mat P; memcpy(P.m, poses[i], 64);
        submit_render(rs[i], P, staged ? &sg : nullptr, nullptr, bands.ok ? &band : nullptr, handoff && j + 1 == passes);
      }
      if (staged) {  // behind every ray-cast that read the slot: its flags go back to zero
        for (int i = 0; i < n; ++i) rs_.wait_for(rs[i].cast);
        hipLaunchKernelGGL(k_rs_clear, dim3(cdiv(sg.n, 256)), dim3(256), 0, rs_.stream(), sg.keys, sg.n, rs_super_[rs_.slot()][0], rs_super_[rs_.slot()][1]);
        DR_HIP(hipGetLastError());  // (per band: the launches of its ray-casts included)
      }
    }
    return PassStats{passes, largest, total, staged};
  }
  // Depth bands of map-scope renders: max_passes 0 or 1 = off (the default), 2..64 = a RenderAsync whose union exceeds the
  // staging may run in up to that many bands.
  void set_render_bands(int max_passes) {
    if (max_passes < 0 || max_passes > 64) fail(DR_ERR_ARG, "drf_set_render_bands: max_passes %d is not within 0..64", max_passes);
    if (next_ == kGetRender) fail(DR_ERR_PROTOCOL, "drf_set_render_bands: a render is pending, call GetRenderResult first");
    render_bands_ = max_passes;
  }
  void render_band_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_render_band_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = band_stats_[i];
  }
  // DRF_RENDER_RESIDENT: renders read the pool (the default); DRF_RENDER_MAP: the pool and the host store together.
  // stage_capacity_blocks bounds the staging (0 = min(num_blocks, kStageBlocks)).
  void set_render_scope(int scope, size_t stage_capacity_blocks) {
    if (scope != DRF_RENDER_RESIDENT && scope != DRF_RENDER_MAP) fail(DR_ERR_ARG, "drf_set_render_scope: unknown scope %d", scope);
    if (next_ == kGetRender) fail(DR_ERR_PROTOCOL, "drf_set_render_scope: a render is pending, call GetRenderResult first");
    render_scope_ = scope;
    rs_cap_req_ = stage_capacity_blocks;
  }
  void render_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_render_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = render_stats_[i];
  }
  // tsdf_volume.cu:702-737
  void get_render_result(uint8_t **bgr, float **depth, int n) {
    expect(kGetRender, "Please call the functions in a loop: IntegrateScanAsync -> RenderAsync -> GetRenderResult.");
    if (n != (int)renders_.size()) fail(DR_ERR_ARG, "GetRenderResult: expected %zu outputs", renders_.size());
    next_ = kIntegrate;
    DR_HIP(hipSetDevice(device_));
    for (int i = 0; i < n; ++i) {
      DR_HIP(hipEventSynchronize(renders_[i].done));
      bgr[i] = renders_[i].h_bgr[free_slot_];
      depth[i] = renders_[i].h_depth[free_slot_];
    }
    check_device_flags();
  }
  // Device-resident result of render stream i (the buffers GetRenderResult copies from): valid from GetRenderResult
  // until the next RenderAsync.  Lets a consumer on the same GPU (the coarse tracker's dense-depth hand-off) skip the
  // D2H + H2D round trip.
  void get_render_device(int i, const uint8_t **d_bgr, const float **d_depth) {
    if (i < 0 || i >= (int)renders_.size()) fail(DR_ERR_ARG, "get_render_device: stream %d of %zu", i, renders_.size());
    if (next_ != kIntegrate) fail(DR_ERR_PROTOCOL, "get_render_device: call after GetRenderResult");
    if (d_bgr) *d_bgr = renders_[i].d_bgr;
    if (d_depth) *d_depth = renders_[i].d_depth;
  }
  // Test hook: the page-locked host copies of the last (back = 0) and the second-to-last (back = 1) ray-cast of render stream i that
  // bench_sequence wrote -- the second-to-last one ran BESIDE the allocation of the last scan (enqueue_scan), which is what a test of
  // that overlap has to look at.
  void bench_render_host(int i, int back, const uint8_t **bgr, const float **depth) {
    no_bench_while_streaming("drf_bench_render_host");
    if (i < 0 || i >= (int)renders_.size() || back < 0 || back > 1) fail(DR_ERR_ARG, "bench_render_host: stream %d of %zu, back %d", i, renders_.size(), back);
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipDeviceSynchronize());
    const int slot = free_slot_ ^ back;
    if (bgr) *bgr = renders_[i].h_bgr[slot];
    if (depth) *depth = renders_[i].h_depth[slot];
  }
  void synchronize() {
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipDeviceSynchronize());
    check_device_flags();
  }
  void stats(uint64_t out[4]) {
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipDeviceSynchronize());
    unsigned long long c[4];
    DR_HIP(hipMemcpy(c, d_.cnt, 32, hipMemcpyDeviceToHost));
    out[0] = (uint64_t)pool_blocks(); out[1] = c[3]; out[2] = c[1]; out[3] = c[2];
  }
  // blocks k_integrate has read since the engine was created (one 4 KB read each, whether or not any voxel of the block was updated): with
  // `updated_total` this gives the kernel's HBM bytes exactly -- 4096 x visited + 8 x updated -- for the counter calibration in DESIGN.md
  uint64_t visited_blocks() {
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipDeviceSynchronize());
    unsigned long long v = 0;
    DR_HIP(hipMemcpy(&v, d_.cnt + 4, 8, hipMemcpyDeviceToHost));
    return v;
  }
  void export_blocks(int max_blocks, int32_t *coords, uint8_t *voxels, int *n) {
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipDeviceSynchronize());
    const int na = std::min(pool_blocks(), max_blocks);
    std::vector<unsigned long long> keys(na);
    DR_HIP(hipMemcpy(keys.data(), d_.blk_key, (size_t)na * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < na; ++i) unpack_key_host(keys[i], coords + 3 * i);
    DR_HIP(hipMemcpy(voxels, d_.vox, (size_t)na * 4096, hipMemcpyDeviceToHost));
    if (n) *n = na;
  }
  void fast_div_status(int *enabled, unsigned long long *mismatches) const { if (enabled) *enabled = d_.fast_div; if (mismatches) *mismatches = fast_div_mismatches_; }
  void test_combine(size_t n, const uint8_t *a, const uint8_t *b, int max_weight, uint8_t *out) {
    DR_HIP(hipSetDevice(device_));
    DeviceBuf<Voxel> da, db, dout;
    da.reserve(n, int_stream_); db.reserve(n, int_stream_); dout.reserve(n, int_stream_);
    DR_HIP(hipMemcpy(da.get(), a, n * 8, hipMemcpyHostToDevice));
    DR_HIP(hipMemcpy(db.get(), b, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_combine, dim3(2048), dim3(256), 0, int_stream_, da.get(), db.get(), dout.get(), n, max_weight);
    DR_HIP(hipStreamSynchronize(int_stream_));
    DR_HIP(hipMemcpy(out, dout.get(), n * 8, hipMemcpyDeviceToHost));
  }
  // ---- marching cubes: TsdfVolume::ExtractMeshAsync / GetMeshSync (tsdf_volume.cu:759-838) ----
  void extract_mesh_async(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "ExtractMeshAsync: null argument");
    expect(kIntegrate, "Please call this functions after GetRenderResult.");
    if (mesh_pending_) fail(DR_ERR_PROTOCOL, "mesh_extractor should be NULL (fetch the previous mesh with GetMeshSync first)");
    launch_extraction(lower, upper);
    mesh_pending_ = true;
  }
  size_t mesh_num_triangles() {  // blocks until the pending extraction is done; does not consume it
    if (!mesh_pending_) fail(DR_ERR_PROTOCOL, "mesh_extractor should not be NULL (did you call ExtractMeshAsync before)?");
    if (mesh_pending_update_) fail(DR_ERR_PROTOCOL, "GetMeshSync: the pending extraction is a mesh update, fetch it with drf_get_mesh_update_sync");
    return finish_mesh();
  }
  // vert / cols hold num_max vertices (3 floats each).  The reference compares num_max with the TRIANGLE count
  // (tsdf_volume.cu:796) and would overrun for meshes above num_max / 3 triangles; here the vertex count is checked.
  void get_mesh_sync(size_t num_max, size_t *num, float *vert, float *cols) {
    expect(kIntegrate, "Please call this functions after GetRenderResult.");
    if (!num || !vert || !cols) fail(DR_ERR_ARG, "GetMeshSync: null argument");
    const size_t ntri = mesh_num_triangles();
    if (num_max < 3 * ntri) fail(DR_ERR_CAPACITY, "Did not provide enough storage for mesh (%zu vertices > %zu).", 3 * ntri, num_max);
    fetch_mesh(ntri, vert, cols);
    *num = 3 * ntri;  // 1 triangle = 3 vert (tsdf_volume.cu:800)
    mesh_pending_ = false;
  }
  // DrFusion::SaveMeshToFile (dr_fusion.cpp:74-93): synchronous extraction, then Mesh::SaveToFile(filename, bgr=true)
  // (mesh.cu:24-66): one "v x y z r g b" line per vertex, one "f i i+1 i+2" line per triangle.
  void save_mesh(const char *filename, const float *lower, const float *upper) {
    if (!filename || !lower || !upper) fail(DR_ERR_ARG, "SaveMeshToFile: null argument");
    if (mesh_pending_) fail(DR_ERR_PROTOCOL, "SaveMeshToFile: an ExtractMeshAsync is pending, call GetMeshSync first");
    launch_extraction(lower, upper);
    const size_t ntri = finish_mesh();
    std::vector<float> v(ntri * 9), c(ntri * 9);
    fetch_mesh(ntri, v.data(), c.data());
    FILE *f = fopen(filename, "w");
    if (!f) fail(DR_ERR_IO, "SaveMeshToFile: cannot open %s", filename);
    for (size_t i = 0; i < ntri * 3; ++i)
      fprintf(f, "v %g %g %g %g %g %g\n", v[3 * i], v[3 * i + 1], v[3 * i + 2], c[3 * i], c[3 * i + 1], c[3 * i + 2]);
    for (size_t i = 1; i <= ntri * 3; i += 3) fprintf(f, "f %zu %zu %zu\n", i, i + 1, i + 2);
    if (fclose(f) != 0) fail(DR_ERR_IO, "SaveMeshToFile: write to %s failed", filename);
  }
  // DRF_MESH_RESIDENT: the pool only (the default); DRF_MESH_MAP: the pool and the host store together
  void set_mesh_scope(int scope) {
    if (scope != DRF_MESH_RESIDENT && scope != DRF_MESH_MAP) fail(DR_ERR_ARG, "drf_set_mesh_scope: unknown scope %d", scope);
    if (mesh_pending_) fail(DR_ERR_PROTOCOL, "drf_set_mesh_scope: an extraction is pending, call GetMeshSync first");
    mesh_scope_ = scope;
  }
  // last extraction: blocks meshed (workgroups of each pass), host blocks uploaded (once per chunk that stages them), chunks
  void mesh_stats(uint64_t out[3]) const {
    if (!out) fail(DR_ERR_ARG, "drf_mesh_stats: null argument");
    for (int i = 0; i < 3; ++i) out[i] = mesh_stats_[i];
  }
  // ---- incremental mesh: an extraction that lists only the blocks whose triangles may have changed since the baseline
  // (the last update fetched); no reference counterpart.  DESIGN.md §7c "Incremental mesh".
  void extract_mesh_update_async(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_extract_mesh_update_async: null argument");
    expect(kIntegrate, "Please call this functions after GetRenderResult.");
    if (mesh_pending_) fail(DR_ERR_PROTOCOL, "drf_extract_mesh_update_async: an extraction is pending, fetch it first");
    settle();  // in either scope: what the host store holds decides below
    if (mesh_scope_ == DRF_MESH_RESIDENT && !store_.empty())
      fail(DR_ERR_PROTOCOL, "drf_extract_mesh_update_async: %zu blocks are in the host store; the resident view changes by eviction, which an update does not track (use DRF_MESH_MAP)", store_.size());
    MeshUpdate next;
    next.valid = true;
    // a round-trip mismatch writes a block that is not on the visible list (k_integrate)
    DR_HIP(hipMemcpy(&next.redirects, d_.cnt + 2, 8, hipMemcpyDeviceToHost));
    memcpy(next.box, lower, 12); memcpy(next.box + 3, upper, 12);
    next.full = !mu_base_.valid || mu_force_full_ || mu_overflow_ || memcmp(next.box, mu_base_.box, 24) != 0 || next.redirects != mu_base_.redirects;
    mu_next_ = next;  // (before the launch, which may throw: mu_next_ is read only while mesh_pending_update_ is set)
    if (store_.empty()) launch_mesh_update(lower, upper);
    else launch_mesh_map(lower, upper, true);
    // launched: the scans recorded so far belong to this update, later ones to the next
    mu_force_full_ = false; mu_overflow_ = false;
    mu_poses_.clear();
    mesh_pending_ = mesh_pending_update_ = true;
  }
  void mesh_update_size(size_t *nblk, size_t *ntri, int *full) {
    if (!nblk || !ntri || !full) fail(DR_ERR_ARG, "drf_mesh_update_size: null argument");
    if (!mesh_pending_ || !mesh_pending_update_) fail(DR_ERR_PROTOCOL, "drf_mesh_update_size: no mesh update is pending");
    *ntri = finish_mesh(); *nblk = mu_next_.nblk; *full = mu_next_.full ? 1 : 0;
  }
  void get_mesh_update_sync(size_t max_blocks, size_t num_max, size_t *nblk, int32_t *coords, uint64_t *first, size_t *num, float *vert,
                            float *cols, int *full) {
    if (!nblk || !coords || !first || !num || !vert || !cols || !full) fail(DR_ERR_ARG, "drf_get_mesh_update_sync: null argument");
    if (!mesh_pending_ || !mesh_pending_update_) fail(DR_ERR_PROTOCOL, "drf_get_mesh_update_sync: no mesh update is pending");
    const size_t ntri = finish_mesh(), nb = mu_next_.nblk;
    if (max_blocks < nb) fail(DR_ERR_CAPACITY, "Did not provide enough storage for the patch table (%zu blocks > %zu).", nb, max_blocks);
    if (num_max < 3 * ntri) fail(DR_ERR_CAPACITY, "Did not provide enough storage for mesh (%zu vertices > %zu).", 3 * ntri, num_max);
    first[0] = 0;
    if (nb > 0) {
      DR_HIP(hipMemcpy(coords, mu_coords_.get(), nb * 12, hipMemcpyDeviceToHost));
      DR_HIP(hipMemcpy(first, mu_first_.get(), (nb + 1) * 8, hipMemcpyDeviceToHost));
      fetch_mesh(ntri, vert, cols);
    }
    *nblk = nb; *num = 3 * ntri; *full = mu_next_.full ? 1 : 0;
    mu_base_ = mu_next_;  // the baseline advances: this box, the voxel state at the launch
    mesh_pending_ = mesh_pending_update_ = false;
  }
  void mesh_update_reset() { mu_force_full_ = true; }
  // last update launched: blocks in scope, blocks meshed again, scans folded in, full
  void mesh_update_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_mesh_update_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = mu_stats_[i];
  }

  // bench path: inputs already resident in HBM
  void integrate_device(const void *d_bgr, const void *d_depth, const float *pose16) {
    DR_HIP(hipSetDevice(device_));
    if (st_radius_ > 0.0f) {  // the depths are on the device: bound the scan by max_sensor_depth
      if (!d_bgr || !d_depth || !pose16) fail(DR_ERR_ARG, "drf_integrate_device: null argument");
      return scan_between_streaming(pose16, o_.max_sensor_depth, [&] { enqueue_scan((const unsigned char *)d_bgr, (const float *)d_depth, pose16); });
    }
    if (!store_.empty()) fail(DR_ERR_PROTOCOL, "drf_integrate_device: blocks are in the host store while streaming is off");
    enqueue_scan((const unsigned char *)d_bgr, (const float *)d_depth, pose16);
  }
  void no_bench_while_streaming(const char *what) {
    if (st_radius_ > 0.0f || !store_.empty()) fail(DR_ERR_UNSUPPORTED, "%s: not available while streaming is on or the host store holds blocks", what);
  }
  void bench_integrate(const void *d_bgr, const void *d_depth, const float *poses, int nscans, float *ms, float *kernel_ms) {
    no_bench_while_streaming("drf_bench_integrate");
    DR_HIP(hipSetDevice(device_));
    std::vector<hipEvent_t> ev(2 * (size_t)nscans + 2);
    for (auto &e : ev) DR_HIP(hipEventCreate(&e));
    DR_HIP(hipEventRecord(ev[0], int_stream_));
    for (int s = 0; s < nscans; ++s) {
      kernel_events_[0] = ev[2 + 2 * s]; kernel_events_[1] = ev[3 + 2 * s];
      enqueue_scan((const unsigned char *)d_bgr + (size_t)s * npix_ * 3, (const float *)d_depth + (size_t)s * npix_, poses + 16 * s);
    }
    kernel_events_[0] = kernel_events_[1] = nullptr;
    DR_HIP(hipEventRecord(ev[1], int_stream_));
    DR_HIP(hipStreamSynchronize(int_stream_));
    float t = 0, k = 0;
    DR_HIP(hipEventElapsedTime(&t, ev[0], ev[1]));
    for (int s = 0; s < nscans; ++s) { float q = 0; DR_HIP(hipEventElapsedTime(&q, ev[2 + 2 * s], ev[3 + 2 * s])); k += q; }
    for (auto &e : ev) (void)hipEventDestroy(e);
    if (ms) *ms = t;
    if (kernel_ms) *kernel_ms = k;
    check_device_flags();
  }

  // BASELINE configs[3] loop (dr_debug_example.cpp:78-162: GetRenderResult(k-1) / IntegrateScanAsync(k) / RenderAsync(k) per
  // frame, map growing) over `n` frames whose inputs are resident in HBM: allocate + integrate on the integration stream,
  // then -- render != 0 -- one ray-cast per render stream from the frame's own pose with the D2H of its result into the
  // pinned double buffers, ordered by the same events as the operator path.  ms[0] = first allocate .. last copy
  // (hipEvents), ms[1..4] = sums of the allocate / integrate / ray-cast / D2H intervals, ms[5] = host wall clock.
  void bench_sequence(const void *d_bgr, const void *d_depth, const float *poses, int n, int render, float ms[6]) {
    no_bench_while_streaming("drf_bench_sequence");
    if (!d_bgr || !d_depth || !poses || !ms || n <= 0) fail(DR_ERR_ARG, "bench_sequence: bad argument");
    expect(kIntegrate, "bench_sequence starts where IntegrateScanAsync may be called.");
    DR_HIP(hipSetDevice(device_));
    const int nr = render ? (int)renders_.size() : 0;
    const size_t per = 4 + (size_t)3 * nr;
    std::vector<hipEvent_t> ev(per * n);
    for (auto &e : ev) DR_HIP(hipEventCreate(&e));
    DR_HIP(hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < n; ++s) {
      hipEvent_t *e = &ev[per * s];
      DR_HIP(hipEventRecord(e[0], int_stream_));
      kernel_events_[0] = e[1]; kernel_events_[1] = e[2]; kernel_events_[2] = e[3];
      // (the voxel update waits for the previous frame's ray-casts inside enqueue_scan; allocation, commit and cull run beside them)
      enqueue_scan((const unsigned char *)d_bgr + (size_t)s * npix_ * 3, (const float *)d_depth + (size_t)s * npix_, poses + 16 * s, true);
      kernel_events_[0] = kernel_events_[1] = kernel_events_[2] = nullptr;
      DR_HIP(hipEventRecord(int_done_, int_stream_));
      free_slot_ ^= 1;
      for (int i = 0; i < nr; ++i) {
        Mat P; memcpy(P.m, poses + 16 * s, 64);
        submit_render(renders_[i], P, nullptr, e + 4 + 3 * i);
      }
    }
    DR_HIP(hipDeviceSynchronize());
    ms[5] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; k < 5; ++k) ms[k] = 0.f;
    float q = 0.f;
    hipEvent_t last = nr ? ev[per * (n - 1) + 6 + 3 * (nr - 1)] : ev[per * (n - 1) + 2];
    DR_HIP(hipEventElapsedTime(&ms[0], ev[0], last));
    for (int s = 0; s < n; ++s) {
      hipEvent_t *e = &ev[per * s];
      DR_HIP(hipEventElapsedTime(&q, e[0], e[3])); ms[1] += q;  // allocate + commit + cull (may run beside the previous frame's ray-cast)
      DR_HIP(hipEventElapsedTime(&q, e[1], e[2])); ms[2] += q;  // k_integrate alone
      for (int i = 0; i < nr; ++i) {
        DR_HIP(hipEventElapsedTime(&q, e[4 + 3 * i], e[5 + 3 * i])); ms[3] += q;
        DR_HIP(hipEventElapsedTime(&q, e[5 + 3 * i], e[6 + 3 * i])); ms[4] += q;
      }
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    check_device_flags();
  }

  // ---- streaming: a bounded device pool plus a host store for the rest of the map (DESIGN.md "Streaming voxel blocks") ----
  void set_streaming(float radius, size_t host_capacity_blocks) {
    if (!(radius >= 0.0f) || !std::isfinite(radius)) fail(DR_ERR_ARG, "drf_set_streaming: radius must be finite and >= 0 (got %g)", radius);
    const float rmin = streaming_min_radius(o_);
    if (radius > 0.0f && radius < rmin) fail(DR_ERR_ARG, "drf_set_streaming: radius %g is below drf_streaming_min_radius = %g", radius, rmin);
    settle();
    if (!store_.empty()) fail(DR_ERR_PROTOCOL, "drf_set_streaming: the host store holds %zu blocks; bring them back with drf_stream_in_region first", store_.size());
    if (radius > 0.0f) ensure_staging();
    st_radius_ = radius;
    st_host_cap_ = host_capacity_blocks ? host_capacity_blocks : (size_t)-1;
    reach_.reset();
    // blocks integrated before now are bounded by nothing the host knows: the first scan runs the selection pass
    const double origin[3] = {0.0, 0.0, 0.0};
    if (radius > 0.0f) reach_.push(origin, HUGE_VAL);
  }
  void stream_out_region(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_stream_out_region: null argument");
    expect(kIntegrate, "drf_stream_out_region: call it where IntegrateScanAsync may be called.");
    settle();
    ensure_staging();
    F3 lo, hi, p{0.f, 0.f, 0.f};
    lo.x = lower[0]; lo.y = lower[1]; lo.z = lower[2]; hi.x = upper[0]; hi.y = upper[1]; hi.z = upper[2];
    // count first: a region that does not fit in the host store moves nothing
    launch_eviction(p, 0.0f, lo, hi, 1, 0);
    DR_HIP(hipStreamSynchronize(int_stream_));
    ev_pending_ = false;
    const size_t want = (size_t)sd_.h_out[1];
    if (want > host_free()) fail(DR_ERR_CAPACITY, "drf_stream_out_region: %zu blocks do not fit in the host store (%zu free)", want, host_free());
    for (;;) {
      launch_eviction(p, 0.0f, lo, hi, 1, st_cap_);
      DR_HIP(hipStreamSynchronize(int_stream_));
      const bool more = sd_.h_out[1] > sd_.h_out[0];
      fold_evicted();
      if (!more) break;
    }
  }
  void stream_in_region(const float *lower, const float *upper) {
    if (!lower || !upper) fail(DR_ERR_ARG, "drf_stream_in_region: null argument");
    expect(kIntegrate, "drf_stream_in_region: call it where IntegrateScanAsync may be called.");
    settle();
    std::vector<unsigned long long> keys;
    double bl[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, bh[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    store_.for_each([&](unsigned long long k, const uint8_t *) {
      int c[3]; unpack_key_host(k, c);
      for (int a = 0; a < 3; ++a) {
        const float org = blk_origin_host(c[a], o_.voxel_size);
        if (!(org >= lower[a] && org <= upper[a])) return;
      }
      keys.push_back(k);
      for (int a = 0; a < 3; ++a) { bl[a] = std::min(bl[a], blk_centre_host(c[a], o_.voxel_size)); bh[a] = std::max(bh[a], blk_centre_host(c[a], o_.voxel_size)); }
    });
    if (keys.empty()) return;
    upload(keys);  // checks the pool's free room before anything moves
    DR_HIP(hipStreamSynchronize(int_stream_));
    if (st_radius_ > 0.0f) {  // the ball around the uploaded centres bounds them for the selection skip
      double c[3], r = 0.0;
      for (int a = 0; a < 3; ++a) { c[a] = 0.5 * (bl[a] + bh[a]); r += (bh[a] - bl[a]) * (bh[a] - bl[a]); }
      reach_.push(c, 0.5 * std::sqrt(r) + o_.voxel_size);
    }
  }
  // out: resident blocks, blocks in the host store, blocks streamed out / in (totals), bytes moved, last scan's streaming time (us)
  void streaming_stats(uint64_t out[6]) {
    settle();
    out[0] = (uint64_t)pool_blocks(); out[1] = store_.size(); out[2] = st_out_total_; out[3] = st_in_total_;
    out[4] = 4096 * (st_out_total_ + st_in_total_); out[5] = (uint64_t)std::llround(st_last_us_);
  }
  void export_host_blocks(int max_blocks, int32_t *coords, uint8_t *voxels, int *n) {
    if (max_blocks < 0 || (max_blocks > 0 && (!coords || !voxels))) fail(DR_ERR_ARG, "drf_export_host_blocks: bad argument");
    settle();
    int i = 0;
    store_.for_each([&](unsigned long long k, const uint8_t *v) {
      if (i >= max_blocks) return;
      unpack_key_host(k, coords + 3 * i);
      memcpy(voxels + (size_t)i * 4096, v, 4096);
      ++i;
    });
    if (n) *n = i;
  }

  // ---- the map file (include/dr_mi355x.h "map files"; DESIGN.md §7c "Saving and loading the map") ----
  // Resident and stored blocks merged in ascending key order, chunk by chunk: k_map_gather writes a chunk's resident blocks
  // straight into one of two pinned buffers while the host copies the stored ones into their positions of it, appends the
  // other buffer to the file and folds it into the checksum.  Folds pending evictions first; beyond that nothing changes.
  void save_map(const char *path, size_t chunk_blocks) {
    if (!path) fail(DR_ERR_ARG, "drf_save_map: null argument");
    expect(kIntegrate, "drf_save_map: call it where IntegrateScanAsync may be called.");
    settle();
    const int nres = pool_blocks();
    std::vector<unsigned long long> res((size_t)nres);
    sort_resident(nres, res);
    const std::vector<unsigned long long> sto = store_.sorted_keys();
    const size_t n = res.size() + sto.size();
    std::vector<unsigned long long> keys;
    std::vector<unsigned char> stored;
    keys.reserve(n); stored.reserve(n);
    const BlockRange all{{INT_MIN, INT_MIN, INT_MIN}, {INT_MAX, INT_MAX, INT_MAX}};
    for_each_in_range(res, sto, all, [&](unsigned long long key, bool st) { keys.push_back(key); stored.push_back(st ? 1 : 0); });
    const size_t chunk = mio_.chunk(chunk_blocks, n), nc = (n + chunk - 1) / chunk;
    // per chunk the resident blocks rb[c] .. rb[c + 1] of the sorted pairs; each one's position within its chunk
    std::vector<size_t> rb(nc + 1, 0);
    std::vector<int> dst;
    dst.reserve((size_t)nres);
    for (size_t i = 0; i < n; ++i)
      if (!stored[i]) { ++rb[i / chunk + 1]; dst.push_back((int)(i % chunk)); }
    for (size_t c = 0; c < nc; ++c) rb[c + 1] += rb[c];
    if (nres > 0) DR_HIP(hipMemcpy(mio_.dst.get(), dst.data(), (size_t)nres * 4, hipMemcpyHostToDevice));
    mio_.ensure(chunk);
    std::string err;
    MapWriter w;
    if (!w.open(path, o_.voxel_size, keys.data(), n, err)) fail(DR_ERR_IO, "drf_save_map: %s", err.c_str());
    mio_.write_chunks(
        "drf_save_map", w, n, chunk,
        [&](size_t c) {  // chunk c's resident blocks into the current buffer; nothing is launched for none
          const int m = (int)(rb[c + 1] - rb[c]);
          if (m == 0) return;
          hipLaunchKernelGGL(k_map_gather, dim3(std::min(cdiv(m, 4), 1024)), dim3(256), 0, int_stream_, d_.vox, mio_.slot.get() + rb[c], mio_.dst.get() + rb[c], m,
                             (uint4 *)mio_.pair.dev());
          DR_HIP(hipGetLastError());
        },
        [&](size_t c, unsigned char *h) {  // and the stored ones, while that kernel runs
          const size_t b = c * chunk, m = std::min(chunk, n - b);
          for (size_t i = 0; i < m; ++i)
            if (stored[b + i]) memcpy(h + i * 4096, store_.get(keys[b + i]), 4096);
        });
  }
  // The file validated as a whole first, then its blocks placed: into the pool in the keys' order (streaming off; k_in_place
  // reads one pinned buffer while the host reads the file into the other) or into the host store (streaming on).  A failure
  // leaves the map empty.
  void load_map(const char *path, size_t chunk_blocks) {
    if (!path) fail(DR_ERR_ARG, "drf_load_map: null argument");
    expect(kIntegrate, "drf_load_map: call it where IntegrateScanAsync may be called.");
    const bool pending = ev_pending_;
    settle();
    const int nres = pool_blocks();
    if (pending || nres != 0 || !store_.empty())
      fail(DR_ERR_PROTOCOL, "drf_load_map: the map is not empty (%d resident blocks, %zu in the host store%s)", nres, store_.size(), pending ? ", an eviction was pending" : "");
    std::string err;
    MapReader rd;
    mio_.open_reader("drf_load_map", path, rd);
    const uint64_t n = rd.blocks();
    const bool to_store = st_radius_ > 0.0f;
    if (to_store ? n > (uint64_t)st_host_cap_ : n > (uint64_t)o_.num_blocks)
      fail(DR_ERR_CAPACITY, "drf_load_map: %llu blocks do not fit in the %s (%llu)", (unsigned long long)n, to_store ? "host store" : "pool",
           (unsigned long long)(to_store ? st_host_cap_ : (size_t)o_.num_blocks));
    mu_force_full_ = true;
    if (n == 0) { loaded_ = true; return; }
    const std::vector<unsigned long long> &keys = rd.keys();
    const size_t chunk = mio_.chunk(chunk_blocks, (size_t)n);
    mio_.ensure(chunk);
    bool ok;
    if (to_store) {  // the next scan's stream_before_scan brings in what lies within the radius
      ok = mio_.read_chunks(rd, chunk, err, [&](size_t b, size_t m, const unsigned char *h, const unsigned char *) {
        for (size_t i = 0; i < m; ++i) store_.put(keys[b + i], h + i * 4096);
      });
    } else {  // k_in_place reads one pinned buffer while the host reads the file into the other
      mio_.keys.reserve((size_t)n, int_stream_);
      DR_HIP(hipMemcpy(mio_.keys.get(), keys.data(), (size_t)n * 8, hipMemcpyHostToDevice));
      for (auto &r : renders_) DR_HIP(hipStreamWaitEvent(int_stream_, r.cast, 0));  // blocks are added
      ok = mio_.read_chunks(rd, chunk, err, [&](size_t b, size_t m, const unsigned char *, const unsigned char *d) {
        hipLaunchKernelGGL(k_in_place, dim3(std::min(cdiv((int)m, 4), 1024)), dim3(256), 0, int_stream_, d_, mio_.keys.get() + b, (const uint4 *)d, (int)m);
        hipLaunchKernelGGL(k_in_finish, dim3(1), dim3(64), 0, int_stream_, d_.n_alloc, (int)m);
        DR_HIP(hipGetLastError());
      });
      DR_HIP(hipStreamSynchronize(int_stream_));
    }
    if (!ok) {
      clear_map();
      fail(DR_ERR_IO, "drf_load_map: %s", err.c_str());
    }
    loaded_ = true;
  }

  // A map file merged into the map (the rule: fusion_host.h merge_voxel).  The file validated and every block classified against
  // the map (plan_merge) before anything changes; then chunk by chunk through the two pinned buffers: k_map_merge combines the
  // blocks whose key is resident in place, k_in_place_at appends the new ones (streaming off) while the host combines the
  // chunk's stored blocks into the store, puts the new ones there (streaming on) and reads the next chunk.  A file that changes
  // under the second pass leaves a mixture of merged and untouched blocks (DR_ERR_IO; merge_stats tells how far it got).
  void merge_map(const char *path, size_t chunk_blocks) {
    if (!path) fail(DR_ERR_ARG, "drf_merge_map: null argument");
    expect(kIntegrate, "drf_merge_map: call it where IntegrateScanAsync may be called.");
    settle();
    std::string err;
    MapReader rd;
    mio_.open_reader("drf_merge_map", path, rd);
    const size_t n = (size_t)rd.blocks();
    const std::vector<unsigned long long> &keys = rd.keys();
    const int nres = pool_blocks();
    std::vector<unsigned long long> res((size_t)nres);
    std::vector<int> slots((size_t)nres);
    sort_resident(nres, res);
    if (nres > 0) DR_HIP(hipMemcpy(slots.data(), mio_.slot.get(), (size_t)nres * 4, hipMemcpyDeviceToHost));
    const size_t chunk = mio_.chunk(chunk_blocks, n);
    const MergePlan p = plan_merge(res, slots, store_.sorted_keys(), keys, chunk);
    const bool to_store = st_radius_ > 0.0f;
    const size_t n_add = p.add_key.size(), n_res = p.res_slot.size();
    if (to_store ? store_.size() + n_add > st_host_cap_ : (size_t)nres + n_add > (size_t)o_.num_blocks)
      fail(DR_ERR_CAPACITY, "drf_merge_map: %zu new blocks do not fit in the %s (%zu of %llu in use)", n_add, to_store ? "host store" : "pool",
           to_store ? store_.size() : (size_t)nres, (unsigned long long)(to_store ? st_host_cap_ : (size_t)o_.num_blocks));
    for (auto &v : mg_stats_) v = 0;
    mg_stats_[0] = n;
    mu_force_full_ = true;
    if (n == 0) { loaded_ = true; return; }
    mio_.ensure(chunk);
    // the per-chunk index lists, in the sort's buffers (their contents are on the host now)
    const size_t n_dev = to_store ? 0 : n_add;
    mio_.slot_in.reserve(std::max<size_t>(n_res, 1), int_stream_); mio_.slot.reserve(std::max<size_t>(n_res, 1), int_stream_);
    mio_.dst.reserve(std::max<size_t>(n_dev, 1), int_stream_); mio_.keys.reserve(std::max<size_t>(n_dev, 1), int_stream_);
    mg_counts_.reserve(2, int_stream_);
    if (n_res > 0) {
      DR_HIP(hipMemcpy(mio_.slot_in.get(), p.res_src.data(), n_res * 4, hipMemcpyHostToDevice));
      DR_HIP(hipMemcpy(mio_.slot.get(), p.res_slot.data(), n_res * 4, hipMemcpyHostToDevice));
    }
    if (n_dev > 0) {
      DR_HIP(hipMemcpy(mio_.dst.get(), p.add_src.data(), n_dev * 4, hipMemcpyHostToDevice));
      DR_HIP(hipMemcpy(mio_.keys.get(), p.add_key.data(), n_dev * 8, hipMemcpyHostToDevice));
    }
    DR_HIP(hipMemset(mg_counts_.get(), 0, 16));
    for (auto &r : renders_) DR_HIP(hipStreamWaitEvent(int_stream_, r.cast, 0));  // blocks change
    const unsigned char W = (unsigned char)o_.max_sdf_weight;
    uint64_t host_counts[2] = {0, 0};
    const bool ok = mio_.read_chunks(rd, chunk, err, [&](size_t b, size_t, const unsigned char *h, const unsigned char *d) {
      const size_t c = b / chunk;
      const int mr = (int)(p.rb[c + 1] - p.rb[c]), ma = to_store ? 0 : (int)(p.ab[c + 1] - p.ab[c]);
      if (mr > 0)
        hipLaunchKernelGGL(k_map_merge, dim3(std::min(cdiv(mr, 4), 1024)), dim3(256), 0, int_stream_, d_.vox, mio_.slot_in.get() + p.rb[c], mio_.slot.get() + p.rb[c], mr,
                           (const uint4 *)d, W, mg_counts_.get());
      if (ma > 0) {
        hipLaunchKernelGGL(k_in_place_at, dim3(std::min(cdiv(ma, 4), 1024)), dim3(256), 0, int_stream_, d_, mio_.keys.get() + p.ab[c], mio_.dst.get() + p.ab[c],
                           (const uint4 *)d, ma);
        hipLaunchKernelGGL(k_in_finish, dim3(1), dim3(64), 0, int_stream_, d_.n_alloc, ma);
      }
      if (mr > 0 || ma > 0) DR_HIP(hipGetLastError());
      // the host half of the chunk, from the same buffer, while the kernels read it
      for (size_t i = p.sb[c]; i < p.sb[c + 1]; ++i) merge_block(store_.get_mut(p.sto_key[i]), h + (size_t)p.sto_src[i] * 4096, W, host_counts);
      if (to_store)
        for (size_t i = p.ab[c]; i < p.ab[c + 1]; ++i) store_.put(p.add_key[i], h + (size_t)p.add_src[i] * 4096);
      mg_stats_[1] += p.ab[c + 1] - p.ab[c]; mg_stats_[2] += (uint64_t)mr; mg_stats_[3] += p.sb[c + 1] - p.sb[c];
    });
    DR_HIP(hipStreamSynchronize(int_stream_));
    unsigned long long dev_counts[2];
    DR_HIP(hipMemcpy(dev_counts, mg_counts_.get(), 16, hipMemcpyDeviceToHost));
    mg_stats_[4] = host_counts[0] + dev_counts[0]; mg_stats_[5] = host_counts[1] + dev_counts[1];
    if (!ok) fail(DR_ERR_IO, "drf_merge_map: %s (the blocks merged so far stay merged: drf_merge_stats)", err.c_str());
    loaded_ = true;
  }
  const uint64_t *merge_stats() const { return mg_stats_; }

  // Operations on map files alone (map_ops.h: map_transform, map_align_system, map_align).  The engine lends mio_ -- its device,
  // int_stream_, the pinned pair, voxel_size -- and states where in its call order they may run; its own map is neither read nor changed.
  void transform_map(const char *src, const float *T16, const char *dst, size_t chunk_blocks) {
    map_transform(mio_, src, T16, dst, chunk_blocks, [&] { expect_integrate("drf_transform_map"); });
  }
  const uint64_t *transform_stats() const { return mio_.xf_stats; }
  void align_system(const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, double *sums, uint64_t *counts) {
    map_align_system(mio_, src, ref, T16, opt, sums, counts, [&](const char *who) { expect_integrate(who); });
  }
  // returns what dr_last_error() says after a registration that ran but found no pose (empty otherwise)
  std::string align_map(const char *src, const char *ref, const float *T16, const drf_align_options_t *opt, float *T16_out, drf_align_result_t *res) {
    return map_align(mio_, src, ref, T16, opt, T16_out, res, [&](const char *who) { expect_integrate(who); });
  }
  const uint64_t *align_stats() const { return mio_.al_stats; }

  // ---- a camera pose from a frame: drf_locate_*, drf_track_*, drf_track_colour_*, drf_track_pyramid_* (the rules: pose_host.h;
  // DESIGN.md "Where the frame-pose code lives").  What the families open with, written once.  frame_prologue: the refusals in their one order --
  // the options (bad_option: what the family's resolver returned), the call order, blocks in the host store while streaming is
  // off, the pose, the model pose (the *_system calls of the tracking) -- then pending work settled.
  void frame_prologue(const char *who, const char *bad_option, const float *pose16, const float *model_pose16) {
    if (bad_option) fail(DR_ERR_ARG, "%s: option %s is negative or not finite", who, bad_option);
    expect_integrate(who);
    if (st_radius_ <= 0.0f && !store_.empty())
      fail(DR_ERR_PROTOCOL, "%s: %zu blocks are in the host store while streaming is off; bring them back with drf_stream_in_region first", who, store_.size());
    if (const char *why = transform_pose_fault(pose16)) fail(DR_ERR_ARG, "%s: the pose %s", who, why);
    if (model_pose16)
      if (const char *why = transform_pose_fault(model_pose16)) fail(DR_ERR_ARG, "%s: the model pose %s", who, why);
    settle();  // behind any pending scan; the pinned buffers are idle and every eviction is in the host store
  }
  // the sample grid of a call and what a launch over it needs; max_groups (step = 1) sizes the scratch once for every step
  struct FrameGrid { LocateGrid lg; int total, groups; size_t max_groups; };
  FrameGrid frame_grid(int step) const {
    const LocateGrid lg = locate_grid(o_, step);
    return {lg, (int)locate_positions(lg), (int)locate_groups(lg), (npix_ + 511) / 512};
  }
  // A host image pair, or a depth image alone (d_bgr null), through the scan's pinned input buffers into scratch.  again: the
  // buffers carry this call's frame, which must have left them first.
  void upload_frame(const uint8_t *h_bgr, const float *h_depth, unsigned char *d_bgr, float *d_depth, bool again = false) {
    if (again) DR_HIP(hipStreamSynchronize(int_stream_));
    if (d_bgr) memcpy(h_bgr_in_, h_bgr, npix_ * 3);
    memcpy(h_depth_in_, h_depth, npix_ * 4);
    if (d_bgr) DR_HIP(hipMemcpyAsync(d_bgr, h_bgr_in_, npix_ * 3, hipMemcpyHostToDevice, int_stream_));
    DR_HIP(hipMemcpyAsync(d_depth, h_depth_in_, npix_ * 4, hipMemcpyHostToDevice, int_stream_));
  }

  // A depth frame located in the map this engine holds (the rule: pose_host.h locate_pixel / align_point; DESIGN.md §7c "Locating a
  // depth frame in the map").  The map is read where it lives, through find_block; nothing of it is uploaded, changed or allocated.
  // with_locate does what both calls share -- the prologue, device scratch that is sized once -- and hands body an evaluator:
  // k_map_locate + k_align_fold on int_stream_, 28 doubles and 4 counters back through the pinned pair.
  template <class Body>
  void with_locate(const char *who, const float *h_depth, const void *d_depth, const float *pose16, const drf_locate_options_t *opt, Body &&body) {
    locate_reset();
    LocateOpt lo;
    frame_prologue(who, locate_options(opt, o_.truncation_distance, lo), pose16, nullptr);
    const FrameGrid fg = frame_grid(lo.step);
    const LocateGrid &lg = fg.lg;
    const int total = fg.total, groups = fg.groups;
    double *partial = nullptr;
    unsigned long long *counts = nullptr;
    float *mine = nullptr;  // a host-given depth image
    carve(lc_buf_, int_stream_, [&](Carver &c) {
      partial = c.take<double>(fg.max_groups * 28);
      counts = c.take<unsigned long long>(4);
      mine = c.take<float>(npix_);
    });
    mio_.ensure(1);
    // Map scope (drf_set_locate_scope): the stored blocks an evaluation at the pose can read go through the render's staging, rs_
    // -- no render reads it here: the call is legal only where a scan is, and the device is idle.  A staging serves the poses that
    // follow while locate_stage_serves says so; a pose beyond that selects and stages again.  With an empty store or an empty
    // selection nothing is staged and the resident kernel is launched.
    const bool map_scope = locate_scope_ == DRF_LOCATE_MAP && !store_.empty();
    double slack = locate_stage_slack(o_);
    if (const char *env = hook_env("DR_LOCATE_STAGE_SLACK")) slack = std::min(slack, std::max(0.0, atof(env)) * (double)o_.voxel_size);  // parity hook, in voxels
    std::vector<unsigned long long> keys;  // the selection at sel_pose
    float sel_pose[16];
    RenderStage sg{};
    bool staged = false, selected = false;
    if (map_scope) {  // the refusal: decided at the first pose, before anything is evaluated
      locate_pose16(map_motion(pose16, o_.voxel_size), o_.voxel_size, sel_pose);
      keys = select_locate_blocks(store_, o_, sel_pose);
      if (keys.size() > lc_capacity())
        fail(DR_ERR_CAPACITY, "%s: the pose can read %zu stored blocks, the locate staging holds %zu (drf_set_locate_scope with a larger capacity, or drf_stream_in_region)",
             who, keys.size(), lc_capacity());
    }
    const float *depth = (const float *)d_depth;
    if (h_depth) {
      upload_frame(nullptr, h_depth, nullptr, mine);
      depth = mine;
    }
    lc_stats_[0] = (uint64_t)total; lc_stats_[4] = lc_buf_.capacity(); lc_stats_[5] = store_.size();
    // the slot's flags go back to zero behind the evaluations that read it (they are on int_stream_)
    auto release = [&](bool may_throw) {
      if (!staged) return;
      staged = false;
      hipError_t err = hipEventRecord(rs_.used(), int_stream_);
      if (err == hipSuccess) err = hipStreamWaitEvent(rs_.stream(), rs_.used(), 0);
      if (err == hipSuccess) {
        hipLaunchKernelGGL(k_rs_clear, dim3(cdiv(sg.n, 256)), dim3(256), 0, rs_.stream(), sg.keys, sg.n, rs_super_[rs_.slot()][0], rs_super_[rs_.slot()][1]);
        err = hipGetLastError();
      }
      if (may_throw) DR_HIP(err);
    };
    auto eval = [&](const AlignEval &e, double sums[28], uint64_t c4[4]) {
      if (map_scope) {
        float p16[16];
        locate_pose16(e.m, o_.voxel_size, p16);
        if (selected && !locate_stage_serves(o_, sel_pose, p16, slack)) {
          keys = select_locate_blocks(store_, o_, p16);
          if (keys.size() > lc_capacity())
            fail(DR_ERR_CAPACITY, "%s: a pose of the refinement can read %zu stored blocks, the locate staging holds %zu (drf_set_locate_scope with a larger capacity, or drf_stream_in_region)",
                 who, keys.size(), lc_capacity());
          memcpy(sel_pose, p16, sizeof p16);
          selected = false;
        }
        if (!selected) {
          release(true);
          if (!keys.empty()) {
            sg = stage_render(keys);
            staged = true;
            ++ls_stats_[0]; ls_stats_[1] = std::max<uint64_t>(ls_stats_[1], keys.size()); ls_stats_[2] += keys.size();
          }
          selected = true;
        }
      }
      mio_.evaluate(partial, groups, counts, 4, sums, c4, [&] {
        if (staged) {
          rs_.wait_ready(int_stream_);
          hipLaunchKernelGGL(k_map_locate_staged, dim3(cdiv(groups, 4)), dim3(256), 0, int_stream_, d_, depth, lg, e, groups, total, partial, counts, sg);
        } else {
          hipLaunchKernelGGL(k_map_locate, dim3(cdiv(groups, 4)), dim3(256), 0, int_stream_, d_, depth, lg, e, groups, total, partial, counts);
        }
        DR_HIP(hipGetLastError());
      });
      lc_stats_[1] = c4[0]; lc_stats_[2] = c4[1]; ++lc_stats_[3];
      if (staged) ++ls_stats_[3];
    };
    try {
      body(lo, eval);
    } catch (...) {
      release(false);
      locate_reset();
      throw;
    }
    release(true);
  }
  void locate_system(const char *who, const float *h_depth, const void *d_depth, const float *pose16, const drf_locate_options_t *opt, double *sums,
                     uint64_t *counts) {
    locate_reset();
    if (!(h_depth || d_depth) || !pose16 || !sums || !counts) fail(DR_ERR_ARG, "%s: null argument", who);
    with_locate(who, h_depth, d_depth, pose16, opt, [&](const LocateOpt &lo, auto &eval) {
      double c_src[3];
      locate_centre_src(lo.centre_depth, o_.voxel_size, c_src);
      eval(align_eval(map_motion(pose16, o_.voxel_size), c_src, lo.a, o_.voxel_size), sums, counts);
    });
  }
  // returns what dr_last_error() says after a refinement that ran but found no pose (empty otherwise)
  std::string locate_frame(const char *who, const float *h_depth, const void *d_depth, const float *pose16, const drf_locate_options_t *opt, float *pose16_out,
                           drf_align_result_t *res) {
    locate_reset();
    if (!(h_depth || d_depth) || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    drf_align_result_t r;
    uint64_t c4[4] = {0, 0, 0, 0};
    with_locate(who, h_depth, d_depth, pose16, opt, [&](const LocateOpt &lo, auto &eval) { locate_loop(eval, map_motion(pose16, o_.voxel_size), lo, o_.voxel_size, r, c4); });
    for (int i = 0; i < 16; ++i) pose16_out[i] = (float)r.T[i];
    if (res) *res = r;
    return no_pose_note(std::string(who) + ": the refinement", r,
                        ", " + std::to_string((unsigned long long)c4[2]) + " unobserved, " + std::to_string((unsigned long long)c4[3]) + " outside the band; " +
                            std::to_string(store_.size()) + " blocks are in the host store" +
                            (locate_scope_ == DRF_LOCATE_MAP ? ", " + std::to_string((unsigned long long)ls_stats_[1]) + " of them staged" : std::string()) + ")");
  }
  const uint64_t *locate_stats() const { return lc_stats_; }
  // DRF_LOCATE_RESIDENT: drf_locate_* read the pool (the default); DRF_LOCATE_MAP: the pool and the host store together.
  // stage_capacity_blocks bounds what one evaluation may stage (0 = the render's default); rs_ holds the larger of the two needs.
  void set_locate_scope(int scope, size_t stage_capacity_blocks) {
    if (scope != DRF_LOCATE_RESIDENT && scope != DRF_LOCATE_MAP) fail(DR_ERR_ARG, "drf_set_locate_scope: unknown scope %d", scope);
    if (next_ == kGetRender) fail(DR_ERR_PROTOCOL, "drf_set_locate_scope: a render is pending, call GetRenderResult first");
    locate_scope_ = scope;
    lc_cap_req_ = stage_capacity_blocks;
  }
  void locate_stage_stats(uint64_t out[4]) const {
    if (!out) fail(DR_ERR_ARG, "drf_locate_stage_stats: null argument");
    for (int i = 0; i < 4; ++i) out[i] = ls_stats_[i];
  }

  // A frame tracked against the ray-cast model: by its depth alone (drf_track_*; DESIGN.md §7c "Tracking a depth frame against the
  // ray-cast model"), with the photometric term (drf_track_colour_*; "Tracking with colour"), or coarse to fine (drf_track_reduce,
  // drf_track_pyramid_*; "Tracking coarse to fine").  The rule: pose_host.h track_normal / track_point / track_colour_point /
  // track_loop and track_level_grid / track_reduce_host / track_pyramid_schedule.  One path for the three families (what it
  // guarantees: DESIGN.md "Where the frame-pose code lives").  Every launch is given its level, and level 0 is the single-level
  // call (track_level_grid returns the grid itself), so drf_track_* and drf_track_colour_* are the schedule with one level; colour
  // is a run-time flag.  What differs is the side -- tk_, tc_ or tp_: each family its own scratch, in its own layout, its own
  // statistics and model render, so a call of one family leaves the others' statistics and buffers what they were -- and what each
  // entry does itself: its null arguments, its options, its refusal texts.
  // with_track does what the calls share behind the prologue -- device scratch that is sized once, the frame's intake, the
  // statistics reset when an exception passes -- and hands body the call: the spans and what track_launch_model, track_evaluate
  // (k_track or k_track_colour + k_align_fold on int_stream_; k_align_fold hands back four counters, the photometric terms added
  // leave through a pinned word) and track_render need.  The model's render goes through the engine's one submit (render_passes)
  // on int_stream_ into the scratch; renders_, free_slot_, next_ and the render statistics are not touched.
  struct TrackSide {
    DeviceBuf<unsigned char> buf;             // sized once
    uint64_t stats[8] = {};                   // drf_track_stats / drf_track_colour_stats (the first six), drf_track_pyramid_stats
    uint64_t level[kTrackMaxLevels][4] = {};  // drf_track_pyramid_level_stats
    Render render{};                          // the *_frame call's full-resolution model render: int_stream_ and pointers into buf
    void reset() { memset(stats, 0, sizeof stats); memset(level, 0, sizeof level); }
  };
  struct TrackBufs {  // the spans; a layout leaves null what it does not have
    double *partial; unsigned long long *counts; int *flag; TrackPixel *map;
    float *model, *level, *Ym, *frame, *pyr[kTrackMaxLevels];  // the full-resolution model, its level, Ym, a host-given frame, the frame's levels >= 1
    unsigned char *model_bgr, *level_bgr, *frame_bgr, *pyr_bgr[kTrackMaxLevels];
    unsigned char *render_bgr; RayState *render_band;  // where the model's render puts its colour image and a banded render's ray state
    const float *depth; const unsigned char *bgr;      // the frame at full resolution: the caller's device images, or the spans a host frame went to
  };
  struct TrackCall { const char *who; TrackSide &s; bool colour; FrameGrid fg; TrackBufs b; };
  // The three layouts (DESIGN.md "What the carver guarantees").  What of a render nobody reads once the model kernel runs may lie
  // in the bytes that kernel then overwrites with the model map: a banded render's per-pixel ray state in both single-level
  // layouts, and in the geometric one the colour image too (with colour k_track_model_colour reads it: it has the span model_bgr).
  // The pyramid's is sized for five levels with nothing aliased.
  TrackBufs track_spans(TrackSide &s) {
    TrackBufs b{};
    const size_t max_groups = frame_grid(1).max_groups;
    auto head = [&](Carver &c, size_t counters) {
      b.partial = c.take<double>(max_groups * 28);
      b.counts = c.take<unsigned long long>(counters);  // four that k_align_fold hands back; with colour the fifth (and one unused)
      b.flag = c.take<int>(1);                          // the ray-cast's flag counter
      b.map = c.take<TrackPixel>(npix_, 32);            // the model map
    };
    if (&s == &tk_) {
      carve(s.buf, int_stream_, [&](Carver &c) {
        head(c, 4);
        b.model = c.take<float>(npix_);  // the model's depth: rendered, or a host-given one
        b.frame = c.take<float>(npix_);
        b.render_bgr = (unsigned char *)b.map;
        b.render_band = (RayState *)((unsigned char *)b.map + npix_ * 8);
      });
    } else if (&s == &tc_) {
      carve(s.buf, int_stream_, [&](Carver &c) {
        head(c, 6);
        b.model = c.take<float>(npix_);
        b.Ym = c.take<float>(npix_);
        b.frame = c.take<float>(npix_);
        b.model_bgr = c.take<unsigned char>(npix_ * 3);
        b.frame_bgr = c.take<unsigned char>(npix_ * 3);
        b.render_bgr = b.model_bgr;
        b.render_band = (RayState *)b.map;
      });
    } else {
      auto level_pixels = [&](int L) { return std::max<size_t>(1, (size_t)(o_.width >> L) * (size_t)(o_.height >> L)); };
      carve(s.buf, int_stream_, [&](Carver &c) {
        head(c, 6);
        b.render_band = c.take<RayState>(npix_, 8);
        b.model = c.take<float>(npix_);
        b.level = c.take<float>(level_pixels(1));
        b.Ym = c.take<float>(npix_);
        b.frame = c.take<float>(npix_);
        for (int L = 1; L < kTrackMaxLevels; ++L) b.pyr[L] = c.take<float>(level_pixels(L));
        b.model_bgr = c.take<unsigned char>(npix_ * 3);
        b.level_bgr = c.take<unsigned char>(level_pixels(1) * 3);
        b.frame_bgr = c.take<unsigned char>(npix_ * 3);
        for (int L = 1; L < kTrackMaxLevels; ++L) b.pyr_bgr[L] = c.take<unsigned char>(level_pixels(L) * 3);
        b.render_bgr = b.model_bgr;
      });
    }
    return b;
  }
  // the frame: device images where they lie, or a host pair (without colour: the depth alone) through upload_frame into the spans
  void track_intake(TrackBufs &b, bool colour, const FramePair &frame) {
    b.depth = (const float *)frame.depth;
    b.bgr = (const unsigned char *)frame.bgr;
    if (!frame.on_host) return;
    upload_frame((const uint8_t *)frame.bgr, (const float *)frame.depth, colour ? b.frame_bgr : nullptr, b.frame);
    b.depth = b.frame;
    b.bgr = colour ? b.frame_bgr : nullptr;
  }
  template <class Body>
  void with_track(const char *who, TrackSide &s, bool colour, const FramePair &frame, int step, Body &&body) {
    TrackCall t{who, s, colour, frame_grid(step), track_spans(s)};
    if (colour && !tc_fifth_) tc_fifth_ = own_.pinned<unsigned long long>(1);
    mio_.ensure(1);
    track_intake(t.b, colour, frame);
    s.stats[5] = s.buf.capacity();
    try {
      body(t);
    } catch (...) {
      s.reset();
      throw;
    }
  }
  void launch_reduce(const float *depth, const unsigned char *bgr, int L, float max_jump, float *depth_out, unsigned char *bgr_out) {
    const int WL = o_.width >> L, HL = o_.height >> L;
    const int threads = (WL * HL) << L;  // at most width * height
    hipLaunchKernelGGL(k_track_reduce, dim3(cdiv(threads, 256)), dim3(256), 0, int_stream_, depth, bgr, o_.width, WL, HL, L, max_jump, depth_out, bgr_out);
    DR_HIP(hipGetLastError());
  }
  // level L's model map (with colour: and Ym) from a full-resolution model pair, reduced to the level first above level 0.  The
  // geometric kernels never read bgr_m: in the geometric layout the render's colour image lies in the model map.
  void track_launch_model(const TrackCall &t, const float *depth_m, const unsigned char *bgr_m, int L, const TrackColourOpt &lo) {
    const LocateGrid lg = track_level_grid(t.fg.lg, L);
    if (L > 0) {
      launch_reduce(depth_m, t.colour ? bgr_m : nullptr, L, lo.t.max_jump, t.b.level, t.b.level_bgr);
      depth_m = t.b.level; bgr_m = t.b.level_bgr;
    }
    const int np = lg.W * lg.H;
    if (t.colour) hipLaunchKernelGGL(k_track_model_colour, dim3(cdiv(np, 256)), dim3(256), 0, int_stream_, depth_m, bgr_m, lg, lo.t.max_jump, t.b.map, t.b.Ym);
    else hipLaunchKernelGGL(k_track_model, dim3(cdiv(np, 256)), dim3(256), 0, int_stream_, depth_m, lg, lo.t.max_jump, t.b.map);
    DR_HIP(hipGetLastError());
  }
  // one evaluation of level L against the model map; c[5] with colour, c[4] without
  void track_evaluate(const TrackCall &t, int L, const TrackColourOpt &lo, const AlignEval &e, const float *model_pose16, double sums[28], uint64_t *c) {
    const TrackBufs &b = t.b;
    const LocateGrid lg = track_level_grid(t.fg.lg, L);
    const int total = (int)locate_positions(lg), groups = (int)locate_groups(lg);
    const float *fd = L == 0 ? b.depth : b.pyr[L];
    const unsigned char *fc = L == 0 ? b.bgr : b.pyr_bgr[L];
    const TrackModel tm = track_model(model_pose16, lo.t, o_.voxel_size, b.map);
    mio_.evaluate(b.partial, groups, b.counts, 4, sums, c, [&] {
      if (t.colour) {
        DR_HIP(hipMemsetAsync(b.counts + 4, 0, 8, int_stream_));
        hipLaunchKernelGGL(k_track_colour, dim3(cdiv(groups, 4)), dim3(256), 0, int_stream_, fd, fc, lg, e, tm, track_colour(lo, b.Ym), groups, total, b.partial, b.counts);
        DR_HIP(hipGetLastError());
        DR_HIP(hipMemcpyAsync(tc_fifth_, b.counts + 4, 8, hipMemcpyDeviceToHost, int_stream_));
      } else {
        hipLaunchKernelGGL(k_track, dim3(cdiv(groups, 4)), dim3(256), 0, int_stream_, fd, lg, e, tm, groups, total, b.partial, b.counts);
        DR_HIP(hipGetLastError());
      }
    });
    if (t.colour) c[4] = *tc_fifth_;
  }
  // the model of a *_frame round: the engine's one submit at full resolution into the spans, then level L's model map
  void track_render(const TrackCall &t, int L, const TrackColourOpt &lo, const float *pose16) {
    Render &rd = t.s.render;
    if (!rd.cast) { rd.cast = own_.event(); rd.done = own_.event(); }
    rd.stream = int_stream_;
    rd.d_bgr = t.b.render_bgr;
    rd.d_band = t.b.render_band;
    rd.d_depth = t.b.model;
    rd.d_flag = t.b.flag;
    RenderStagePlan plan;
    RenderBandPlan bands;
    bool waited = false;
    const float *poses[1] = {pose16};
    if (render_scope_ == DRF_RENDER_MAP) plan_render_call(t.who, poses, 1, plan, bands, waited);
    render_passes(plan, bands, &rd, poses, 1, false);
    track_launch_model(t, t.b.model, t.b.model_bgr, L, lo);
  }
  // The body of every *_system call: one evaluation at `level` against a full-resolution model pair the caller gives, n counters
  // out.  A host-given model goes through upload_frame into the spans.  A device-given one is read in place by the single-level
  // calls and copied into the spans by the pyramid's: track_launch_model could read that one in place too, but the copy is part
  // of what drf_track_pyramid_system_device enqueues, and stays.
  void track_system_at(const char *who, TrackSide &s, bool colour, int level, const TrackPyramidOpt &po, const FramePair &frame, const FramePair &model,
                       const float *model_pose16, const float *pose16, double *sums, uint64_t *counts, int n) {
    with_track(who, s, colour, frame, po.c.t.step, [&](TrackCall &t) {
      const TrackBufs &b = t.b;
      const TrackColourOpt lo = track_level_options(po, level);
      if (level > 0) launch_reduce(b.depth, b.bgr, level, lo.t.max_jump, b.pyr[level], b.pyr_bgr[level]);
      const float *depth_m = b.model;
      const unsigned char *bgr_m = b.model_bgr;
      if (model.on_host) {
        upload_frame((const uint8_t *)model.bgr, (const float *)model.depth, colour ? b.model_bgr : nullptr, b.model, true);
      } else if (&s == &tp_) {
        DR_HIP(hipMemcpyAsync(b.model, model.depth, npix_ * 4, hipMemcpyDeviceToDevice, int_stream_));
        if (colour) DR_HIP(hipMemcpyAsync(b.model_bgr, model.bgr, npix_ * 3, hipMemcpyDeviceToDevice, int_stream_));
      } else {
        depth_m = (const float *)model.depth; bgr_m = (const unsigned char *)model.bgr;
      }
      track_launch_model(t, depth_m, bgr_m, level, lo);
      double c_src[3];
      locate_centre_src(lo.t.centre_depth, o_.voxel_size, c_src);
      uint64_t c[5] = {0, 0, 0, 0, 0};
      track_evaluate(t, level, lo, align_eval(map_motion(pose16, o_.voxel_size), c_src, lo.t.a, o_.voxel_size), model_pose16, sums, c);
      for (int i = 0; i < n; ++i) counts[i] = c[i];
      s.stats[0] = (uint64_t)locate_positions(track_level_grid(t.fg.lg, level)); s.stats[1] = c[0]; s.stats[2] = c[1]; s.stats[3] = 1; s.stats[6] = 1;
      s.level[level][2] = 1; s.level[level][3] = c[1];
    });
  }
  // The body of every *_frame call: the frame reduced once to every level above 0, then track_pyramid_schedule over track_loop;
  // po.levels = 1 is the single-level call.  r: level 0's result; last: the counters of its last evaluation.
  void track_levels(const char *who, TrackSide &s, bool colour, const TrackPyramidOpt &po, const FramePair &frame, const float *pose16, drf_align_result_t &r,
                    uint64_t last[5]) {
    with_track(who, s, colour, frame, po.c.t.step, [&](TrackCall &t) {
      for (int L = 1; L < po.levels; ++L) launch_reduce(t.b.depth, t.b.bgr, L, track_level_options(po, L).t.max_jump, t.b.pyr[L], t.b.pyr_bgr[L]);
      track_pyramid_schedule([&](int L, const float *p16, const TrackColourOpt &lo, drf_align_result_t &lr, uint64_t *lc, uint64_t *st2) {
        auto render = [&](const float *p) { track_render(t, L, lo, p); };
        auto eval = [&](const AlignEval &e, const float *mp16, double sums[28], uint64_t *c) { track_evaluate(t, L, lo, e, mp16, sums, c); };
        if (colour) track_loop<5>(render, eval, p16, lo.t, o_.voxel_size, lr, lc, st2);
        else track_loop<4>(render, eval, p16, lo.t, o_.voxel_size, lr, lc, st2);
      }, t.fg.lg, pose16, po, r, s.stats, s.level, last);
    });
  }
  // hands out the pose and returns what dr_last_error() says after a tracking that ran but found no pose (empty otherwise)
  std::string track_note(const char *who, const TrackSide &s, const drf_align_result_t &r, const uint64_t last[5], const std::string &own, float *pose16_out,
                         drf_align_result_t *res) {
    for (int i = 0; i < 16; ++i) pose16_out[i] = (float)r.T[i];
    if (res) *res = r;
    return no_pose_note(std::string(who) + ": the tracking", r,
                        ", " + std::to_string((unsigned long long)last[2]) + " unassociated, " + std::to_string((unsigned long long)last[3]) + " rejected" + own +
                            std::to_string((unsigned long long)s.stats[4]) + " renders; " + std::to_string(store_.size()) + " blocks are in the host store)");
  }
  // The single-level families: Options is drf_track_options_t (geometric: every bgr is null) or drf_track_colour_options_t.
  static const char *track_options_of(const drf_track_options_t *u, float voxel_size, TrackColourOpt &o) { o.photo_weight = 0.0f; return track_options(u, voxel_size, o.t); }
  static const char *track_options_of(const drf_track_colour_options_t *u, float voxel_size, TrackColourOpt &o) { return track_colour_options(u, voxel_size, o); }
  template <class Options>
  void track_system(const char *who, const FramePair &frame, const FramePair &model, const float *model_pose16, const float *pose16, const Options *opt, double *sums,
                    uint64_t *counts) {
    constexpr bool colour = std::is_same<Options, drf_track_colour_options_t>::value;
    TrackSide &s = colour ? tc_ : tk_;
    s.reset();
    if (!frame.has(colour) || !model.has(colour) || !model_pose16 || !pose16 || !sums || !counts) fail(DR_ERR_ARG, "%s: null argument", who);
    TrackPyramidOpt po{{}, 1, 0};
    frame_prologue(who, track_options_of(opt, o_.voxel_size, po.c), pose16, model_pose16);
    track_system_at(who, s, colour, 0, po, frame, model, model_pose16, pose16, sums, counts, colour ? 5 : 4);
  }
  template <class Options>
  std::string track_frame(const char *who, const FramePair &frame, const float *pose16, const Options *opt, float *pose16_out, drf_align_result_t *res) {
    constexpr bool colour = std::is_same<Options, drf_track_colour_options_t>::value;
    TrackSide &s = colour ? tc_ : tk_;
    s.reset();
    if (!frame.has(colour) || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    TrackPyramidOpt po{{}, 1, 0};
    frame_prologue(who, track_options_of(opt, o_.voxel_size, po.c), pose16, nullptr);
    drf_align_result_t r;
    uint64_t last[5] = {0, 0, 0, 0, 0};
    track_levels(who, s, colour, po, frame, pose16, r, last);
    return track_note(who, s, r, last, colour ? ", " + std::to_string((unsigned long long)last[4]) + " with a colour term; " : std::string("; "), pose16_out, res);
  }
  const uint64_t *track_stats() const { return tk_.stats; }
  const uint64_t *track_colour_stats() const { return tc_.stats; }

  // The pyramid family: colour is decided by the images given (bgr null: the geometric kernels).
  // level null: drf_track_pyramid_frame; otherwise the level of a drf_track_pyramid_system, judged with the options.
  TrackPyramidOpt track_pyramid_resolve(const char *who, const drf_track_pyramid_options_t *opt, const int *level) {
    TrackPyramidOpt po;
    if (const char *bad = track_pyramid_options(opt, o_.voxel_size, o_.width, o_.height, po))
      fail(DR_ERR_ARG, "%s: option %s is negative, not finite or out of range (levels <= %d, every level at least %d pixels on a side)", who, bad, kTrackMaxLevels,
           kTrackMinLevelSide);
    if (level && !track_level_fits(o_.width, o_.height, *level))
      fail(DR_ERR_ARG, "%s: level %d is outside 0..%d or below %d pixels on a side of the %dx%d camera", who, *level, kTrackMaxLevels - 1, kTrackMinLevelSide, o_.height,
           o_.width);
    return po;
  }
  // the reduction alone: a host pair through the scratch, or device images in place
  void track_reduce(const char *who, int level, float max_jump, const FramePair &in, void *bgr_out, void *depth_out) {
    tp_.reset();
    if (!in.depth || !depth_out || (in.bgr && !bgr_out)) fail(DR_ERR_ARG, "%s: null argument", who);
    if (!(max_jump >= 0.0f) || !std::isfinite(max_jump)) fail(DR_ERR_ARG, "%s: option max_jump is negative or not finite", who);
    if (!track_level_fits(o_.width, o_.height, level))
      fail(DR_ERR_ARG, "%s: level %d is outside 0..%d or below %d pixels on a side of the %dx%d camera", who, level, kTrackMaxLevels - 1, kTrackMinLevelSide, o_.height,
           o_.width);
    expect_integrate(who);
    settle();
    if (in.on_host) {
      const size_t nl = (size_t)(o_.width >> level) * (size_t)(o_.height >> level);
      TrackBufs b = track_spans(tp_);
      track_intake(b, in.bgr != nullptr, in);
      launch_reduce(b.depth, b.bgr, level, max_jump, b.model, b.model_bgr);  // the model's full-resolution spans hold any level
      DR_HIP(hipMemcpyAsync(depth_out, b.model, nl * 4, hipMemcpyDeviceToHost, int_stream_));
      if (in.bgr) DR_HIP(hipMemcpyAsync(bgr_out, b.model_bgr, nl * 3, hipMemcpyDeviceToHost, int_stream_));
    } else {
      launch_reduce((const float *)in.depth, (const unsigned char *)in.bgr, level, max_jump, (float *)depth_out, (unsigned char *)bgr_out);
    }
    DR_HIP(hipStreamSynchronize(int_stream_));
    tp_.stats[5] = tp_.buf.capacity();
  }
  // one evaluation at `level` (without colour counts[4] = 0)
  void track_pyramid_system(const char *who, int level, const FramePair &frame, const FramePair &model, const float *model_pose16, const float *pose16,
                            const drf_track_pyramid_options_t *opt, double *sums, uint64_t *counts) {
    tp_.reset();
    const bool colour = frame.bgr != nullptr;
    if (!frame.depth || !model.has(colour) || !model_pose16 || !pose16 || !sums || !counts) fail(DR_ERR_ARG, "%s: null argument", who);
    const TrackPyramidOpt po = track_pyramid_resolve(who, opt, &level);
    frame_prologue(who, nullptr, pose16, model_pose16);
    track_system_at(who, tp_, colour, level, po, frame, model, model_pose16, pose16, sums, counts, 5);
  }
  std::string track_pyramid_frame(const char *who, const FramePair &frame, const float *pose16, const drf_track_pyramid_options_t *opt, float *pose16_out,
                                  drf_align_result_t *res) {
    tp_.reset();
    if (!frame.depth || !pose16 || !pose16_out) fail(DR_ERR_ARG, "%s: null argument", who);
    const TrackPyramidOpt po = track_pyramid_resolve(who, opt, nullptr);
    frame_prologue(who, nullptr, pose16, nullptr);
    drf_align_result_t r;
    uint64_t last[5] = {0, 0, 0, 0, 0};
    track_levels(who, tp_, frame.bgr != nullptr, po, frame, pose16, r, last);
    return track_note(who, tp_, r, last,
                      "; " + std::to_string((unsigned long long)tp_.stats[6]) + " levels, " + std::to_string((unsigned long long)tp_.stats[7]) + " abandoned, ", pose16_out, res);
  }
  const uint64_t *track_pyramid_stats() const { return tp_.stats; }
  const uint64_t *track_pyramid_level_stats(int level) const {
    if (level < 0 || level >= kTrackMaxLevels) fail(DR_ERR_ARG, "drf_track_pyramid_level_stats: level %d is outside 0..%d", level, kTrackMaxLevels - 1);
    return tp_.level[level];
  }

 private:
  enum Next { kIntegrate, kRender, kGetRender };
  static constexpr int kStageBlocks = 8192;  // blocks per eviction chain / per stream-in launch (32 MiB of pinned staging each way)
  size_t host_free() const { return st_host_cap_ - std::min(st_host_cap_, store_.size()); }
  int pool_blocks() {  // blocks in the pool; the count lives on the device
    int na = 0;
    DR_HIP(hipMemcpy(&na, d_.n_alloc, 4, hipMemcpyDeviceToHost));
    return std::min(na, o_.num_blocks);
  }
  // the resident order: (blk_key, slot) pairs sorted by key, as mesh_tables sorts the keys -- the keys to res, keys and slots
  // left in mio_.keys / mio_.slot (drf_save_map, drf_merge_map)
  void sort_resident(int nres, std::vector<unsigned long long> &res) {
    if (nres <= 0) return;
    std::vector<int> iota((size_t)nres);
    for (int i = 0; i < nres; ++i) iota[i] = i;
    mio_.keys.reserve((size_t)nres, int_stream_); mio_.slot_in.reserve((size_t)nres, int_stream_);
    mio_.slot.reserve((size_t)nres, int_stream_); mio_.dst.reserve((size_t)nres, int_stream_);
    DR_HIP(hipMemcpy(mio_.slot_in.get(), iota.data(), (size_t)nres * 4, hipMemcpyHostToDevice));
    size_t tb = 0;
    DR_HIP(rocprim::radix_sort_pairs(nullptr, tb, d_.blk_key, mio_.keys.get(), mio_.slot_in.get(), mio_.slot.get(), (size_t)nres, 0, 63, int_stream_));
    mio_.tmp.reserve(std::max<size_t>(tb, 256), int_stream_);  // (never null: a null scratch is rocprim's size query)
    tb = mio_.tmp.capacity();
    DR_HIP(rocprim::radix_sort_pairs(mio_.tmp.get(), tb, d_.blk_key, mio_.keys.get(), mio_.slot_in.get(), mio_.slot.get(), (size_t)nres, 0, 63, int_stream_));
    DR_HIP(hipMemcpyAsync(res.data(), mio_.keys.get(), (size_t)nres * 8, hipMemcpyDeviceToHost, int_stream_));
    DR_HIP(hipStreamSynchronize(int_stream_));
  }
  // a load that failed half way: pool, block index and host store as a new engine has them (the counters were not touched)
  void clear_map() {
    store_ = HostBlockStore();
    const int placed = pool_blocks();
    if (placed == 0) return;
    const size_t cap = (size_t)d_.cmask + 1;
    DR_HIP(hipMemsetAsync(d_.vals, 0xFF, cap * sizeof(int), int_stream_));
    hipLaunchKernelGGL(k_fill_keys, dim3(1024), dim3(256), 0, int_stream_, d_.keys, cap);
    DR_HIP(hipMemsetAsync(d_.vox, 0, (size_t)placed * 4096, int_stream_));
    for (int l = 0; l < kSuperLevels; ++l) DR_HIP(hipMemsetAsync(d_.super[l], 0, (size_t)1 << (3 * (kGridBits - kSuperShift[l])), int_stream_));
    DR_HIP(hipMemsetAsync(d_.present, 0, ((size_t)1 << (3 * kPresentBits - 5)) * sizeof(unsigned), int_stream_));
    DR_HIP(hipMemsetAsync(d_.grid, 0, ((size_t)1 << (3 * kGridBits)) * sizeof(int), int_stream_));
    DR_HIP(hipMemsetAsync(d_.n_alloc, 0, 4 * sizeof(int), int_stream_));
    DR_HIP(hipStreamSynchronize(int_stream_));
  }
  // every pending eviction folded into the host store, the device idle
  void settle() {
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipDeviceSynchronize());
    fold_evicted();
  }
  void ensure_staging() {
    if (st_cap_) return;
    st_cap_ = std::min(o_.num_blocks, kStageBlocks);
    sd_.ctl = own_.device<int>(8);
    DR_HIP(hipMemset(sd_.ctl, 0, 32));
    sd_.list = own_.device<int>(st_cap_);
    sd_.mv_dst = own_.device<int>(st_cap_);
    sd_.mv_src = own_.device<int>(st_cap_);
    h_ev_keys_ = own_.pinned<unsigned long long>(st_cap_, &sd_.h_keys);
    h_ev_vox_ = (uint8_t *)own_.pinned<uint4>((size_t)st_cap_ * 256, &sd_.h_vox);
    sd_.h_out = own_.pinned<int>(4);
    memset(sd_.h_out, 0, 16);
    h_in_keys_ = own_.pinned<unsigned long long>(st_cap_, &hd_in_keys_);
    h_in_vox_ = own_.pinned<uint8_t>((size_t)st_cap_ * 4096, &hd_in_vox_);
    for (auto &e : st_ev_) e = own_.event(hipEventDefault);
  }
  // Enqueue the eviction chain on int_stream_ behind every render stream's last ray-cast (blocks move).  box = 0: blocks whose
  // centre lies beyond sqrt(r2) of p; box = 1: blocks whose origin lies in [lo, hi].  cap = 0 only counts (sd_.h_out[1]).
  void launch_eviction(F3 p, float r2, F3 lo, F3 hi, int box, int cap) {
    for (auto &r : renders_) DR_HIP(hipStreamWaitEvent(int_stream_, r.cast, 0));
    StreamDev s = sd_;
    s.cap = cap;
    const int g = 512;
    hipLaunchKernelGGL(k_ev_select, dim3(g), dim3(256), 0, int_stream_, d_, s, p, r2, lo, hi, box);
    if (cap > 0) {
      hipLaunchKernelGGL(k_ev_gather, dim3(g), dim3(256), 0, int_stream_, d_, s);
      hipLaunchKernelGGL(k_ev_pair, dim3(cdiv(cap, 256)), dim3(256), 0, int_stream_, d_, s);
      hipLaunchKernelGGL(k_ev_move, dim3(g), dim3(256), 0, int_stream_, d_, s);
      hipLaunchKernelGGL(k_ev_zero_tail, dim3(g), dim3(256), 0, int_stream_, d_, s);
      hipLaunchKernelGGL(k_ev_clear, dim3(1024), dim3(256), 0, int_stream_, d_, s, d_.cmask + 1u);
      hipLaunchKernelGGL(k_ev_reindex, dim3(g), dim3(256), 0, int_stream_, d_, s);
    }
    hipLaunchKernelGGL(k_ev_finish, dim3(1), dim3(64), 0, int_stream_, d_, s);
    DR_HIP(hipGetLastError());
    ev_pending_ = cap > 0;
  }
  // the blocks the last eviction chain gathered -> host store (int_stream_ must be idle)
  void fold_evicted() {
    if (st_scan_done_) {  // device time of the last scan's stream-in and eviction launches (0 if it had none)
      float a = 0.f, b = 0.f;
      if (st_timed_ & 1) DR_HIP(hipEventElapsedTime(&a, st_ev_[0], st_ev_[1]));
      if (st_timed_ & 2) DR_HIP(hipEventElapsedTime(&b, st_ev_[2], st_ev_[3]));
      st_last_us_ = 1000.0 * (a + b);
      st_timed_ = 0;
      st_scan_done_ = false;
    }
    if (!ev_pending_) return;
    ev_pending_ = false;
    const int m = sd_.h_out[0];
    for (int i = 0; i < m; ++i) store_.put(h_ev_keys_[i], h_ev_vox_ + (size_t)i * 4096);
    st_out_total_ += (uint64_t)m;
    // the automatic pass took every block beyond radius + hysteresis: what is resident now lies within the largest distance it
    // saw among the blocks that stayed (plus a voxel for the fp32 distance) of its centre
    if (ev_auto_ && sd_.h_out[1] == m) {
      float kept2;
      memcpy(&kept2, &sd_.h_out[3], 4);
      const double r = std::min((double)st_radius_ + hysteresis(), std::sqrt((double)kept2) + o_.voxel_size);
      reach_.reset();
      reach_.push(ev_p_, r);
    }
    ev_auto_ = false;
  }
  // n stored blocks as the staging kernels read them: their keys to kdst, their voxels (4096 bytes each, in the keys' order) to vdst
  void pack_stored(const unsigned long long *keys, size_t n, void *kdst, unsigned char *vdst) const {
    memcpy(kdst, keys, n * 8);
    for (size_t k = 0; k < n; ++k) memcpy(vdst + k * 4096, store_.get(keys[k]), 4096);
  }
  // slots of an open-addressing table over n staged blocks: a power of two, at least twice their number
  static size_t stage_table_slots(size_t n) { size_t s = 1024; while (s < 2 * n) s <<= 1; return s; }
  // stored blocks -> the end of the pool (behind every render stream's last ray-cast).  DR_ERR_CAPACITY before anything moves
  // if they do not fit.
  void upload(const std::vector<unsigned long long> &keys) {
    ensure_staging();
    const int na = pool_blocks();
    if ((size_t)na + keys.size() > (size_t)o_.num_blocks)
      fail(DR_ERR_CAPACITY, "stream-in of %zu blocks does not fit in the pool (%d of num_blocks=%d in use)", keys.size(), na, o_.num_blocks);
    for (auto &r : renders_) DR_HIP(hipStreamWaitEvent(int_stream_, r.cast, 0));
    for (size_t b = 0; b < keys.size(); b += st_cap_) {
      if (b) DR_HIP(hipStreamSynchronize(int_stream_));  // the pinned upload is reused
      const int n = (int)std::min(keys.size() - b, (size_t)st_cap_);
      pack_stored(keys.data() + b, (size_t)n, h_in_keys_, h_in_vox_);
      for (int i = 0; i < n; ++i) store_.erase(keys[b + i]);
      hipLaunchKernelGGL(k_in_place, dim3(std::min(cdiv(n, 4), 1024)), dim3(256), 0, int_stream_, d_, hd_in_keys_, (const uint4 *)hd_in_vox_, n);
      hipLaunchKernelGGL(k_in_finish, dim3(1), dim3(64), 0, int_stream_, d_.n_alloc, n);
      DR_HIP(hipGetLastError());
    }
    st_in_total_ += keys.size();
  }
  double hysteresis() const { return (double)kBS * o_.voxel_size; }  // one block edge
  // Automatic mode, before k_allocate: fold the previous scan's evictions, bring back every stored block whose centre lies
  // within the radius of this scan's camera centre.  No launch and no wait when nothing comes in.
  void stream_before_scan(const float *pose16, float depth_bound) {
    DR_HIP(hipStreamSynchronize(int_stream_));
    fold_evicted();
    double p[3];
    camera_centre(pose16, p);
    std::vector<unsigned long long> in;
    store_.query_sphere(p, st_radius_, o_.voxel_size, in);
    double r = stream_reach(o_, depth_bound);
    if (!in.empty()) {
      DR_HIP(hipEventRecord(st_ev_[0], int_stream_));
      upload(in);
      DR_HIP(hipEventRecord(st_ev_[1], int_stream_));
      st_timed_ |= 1;
      r = std::max(r, (double)st_radius_);
    }
    reach_.add(p, r);
  }
  // After the scan: select resident blocks beyond radius + hysteresis, unless the host can tell that there are none -- every
  // block centre lies in one of the reach balls, so if none of them reaches beyond radius + hysteresis of p nothing is launched.
  void stream_after_scan(const float *pose16) {
    double p[3];
    camera_centre(pose16, p);
    const double lim = (double)st_radius_ + hysteresis();
    const int cap = (int)std::min((size_t)st_cap_, host_free());
    st_scan_done_ = true;
    if (reach_.farthest(p) <= lim || cap == 0) return;
    F3 pf; pf.x = (float)p[0]; pf.y = (float)p[1]; pf.z = (float)p[2];
    const float r2 = (float)(lim * lim);
    DR_HIP(hipEventRecord(st_ev_[2], int_stream_));
    launch_eviction(pf, r2, pf, pf, 0, cap);
    DR_HIP(hipEventRecord(st_ev_[3], int_stream_));
    st_timed_ |= 2;
    ev_auto_ = true;
    memcpy(ev_p_, p, sizeof p);
  }
  // ---- the render scope (DRF_RENDER_MAP; DESIGN.md §7c "Rendering the whole map") ----
  size_t rs_capacity() const { return rs_cap_req_ ? rs_cap_req_ : (size_t)std::min(o_.num_blocks, kStageBlocks); }
  size_t lc_capacity() const { return lc_cap_req_ ? lc_cap_req_ : (size_t)std::min(o_.num_blocks, kStageBlocks); }
  void locate_reset() {
    for (auto &v : lc_stats_) v = 0;
    for (auto &v : ls_stats_) v = 0;
  }
  // The union of stored blocks the poses can read.  Blocks the last scan's eviction chain gathered are not in the store yet: only
  // a pose that could reach one (render_needs_fold) waits for the scan and folds them first.
  RenderStagePlan plan_render(const float *const *poses, int n, bool &waited) {
    if (ev_pending_) {
      bool far = !ev_auto_;
      for (int i = 0; i < n && !far; ++i) far = render_needs_fold(o_, poses[i], ev_p_, (double)st_radius_);
      if (far) {
        DR_HIP(hipEventSynchronize(int_done_));
        fold_evicted();
        waited = true;
      }
    }
    return plan_render_stage(store_, o_, poses, n);
  }
  // rs_ carries [keys | voxels]; each of its two slots has a table and staged superblock flags of its own.  Everything that touches a
  // slot on the device is ordered on rs_'s stream: copy, table clear, k_rs_build, and -- behind the cast events of the renders that
  // read it -- k_rs_clear.
  void ensure_render_staging(size_t n) {
    if (!rs_.stream()) {
      rs_.open(own_);
      for (auto &f : rs_super_)
        for (int l = 0; l < kSuperLevels; ++l) f[l] = own_.device<unsigned char>((size_t)1 << (3 * (kGridBits - kSuperShift[l])), rs_.stream());
    }
    if (n <= rs_blocks_) return;
    const size_t cap = locate_scope_ == DRF_LOCATE_MAP ? std::max(rs_capacity(), lc_capacity()) : rs_capacity();  // the larger need of its two users
    const size_t want = std::min(cap, std::max(2 * rs_blocks_, (n + 1023) & ~(size_t)1023));
    DR_HIP(hipDeviceSynchronize());  // no copy or kernel reads the old allocations
    rs_.reserve((want + 1) * 8 + want * 4096);
    for (auto &t : rs_table_) t.reserve(stage_table_slots(want), rs_.stream());
    rs_blocks_ = want;
  }
  RenderStage stage_render(const std::vector<unsigned long long> &keys) {
    const size_t n = keys.size(), nk = (n + 1) & ~(size_t)1;  // voxels start 16-byte aligned
    ensure_render_staging(n);
    unsigned char *h = rs_.next();
    pack_stored(keys.data(), n, h, h + nk * 8);
    if (nk > n) memset(h + n * 8, 0xFF, 8);
    RenderStage sg{};
    sg.keys = (const unsigned long long *)rs_.dev();
    sg.vox = (const Voxel *)(rs_.dev() + nk * 8);
    sg.table = rs_table_[rs_.slot()].get(); sg.tmask = (unsigned)(stage_table_slots(n) - 1);
    sg.super[0] = rs_super_[rs_.slot()][0]; sg.super[1] = rs_super_[rs_.slot()][1];
    sg.n = (int)n;
    for (size_t k = 0; k < n; ++k) {
      int c[3]; unpack_key_host(keys[k], c);
      constexpr int G = 1 << (kGridBits - 1);
      for (int a = 0; a < 3; ++a) if (c[a] < -G || c[a] >= G) sg.far = 1;
    }
    rs_.copy(nk * 8 + n * 4096);
    DR_HIP(hipMemsetAsync(rs_table_[rs_.slot()].get(), 0, ((size_t)sg.tmask + 1) * 8, rs_.stream()));
    hipLaunchKernelGGL(k_rs_build, dim3(cdiv(sg.n, 256)), dim3(256), 0, rs_.stream(), sg.keys, sg.n, rs_table_[rs_.slot()].get(), sg.tmask,
                       rs_super_[rs_.slot()][0], rs_super_[rs_.slot()][1]);
    DR_HIP(hipGetLastError());
    rs_.record_ready();
    return sg;
  }
  void expect(Next want, const char *msg) {
    static const char *names[] = {"IntegrateScanAsync", "RenderAsync", "GetRenderResult"};
    if (next_ != want) fail(DR_ERR_PROTOCOL, "%s You should have called %s", msg, names[next_]);
  }
  void expect_integrate(const char *who) { expect(kIntegrate, (std::string(who) + ": call it where IntegrateScanAsync may be called.").c_str()); }
  // allocate -> integrate on int_stream_, no host round trip: the number of allocated blocks lives on the
  // device, so the integrate grid is fixed (a few workgroups per CU) and strides over [0, *n_alloc).
  // wait_renders: order the voxel UPDATE behind the ray-casts of the previous scan (they read the voxels).  The allocation pass, the
  // commit and the cull of this scan do not wait: they only turn absent blocks into present, EMPTY ones (zero voxels, weight 0), write
  // the per-pixel records and the visible list -- a ray that meets such a block mid-flight takes the same step as through an absent one
  // (weight 0 either way; the empty-space skip is conservative in both states), so a ray-cast of scan k that runs beside the allocation
  // of scan k + 1 returns the same image bit for bit, and a quarter of the scan (0.08 of 0.46 ms at 5 mm) leaves the critical path.
  void enqueue_scan(const unsigned char *d_bgr, const float *d_depth, const float *pose16, bool wait_renders = false) {
    Mat T, Ti;
    memcpy(T.m, pose16, 64);
    inverse4_host(T.m, Ti.m);
    record_scan_pose(Ti);
    hipLaunchKernelGGL(k_allocate, dim3(cdiv((int)npix_, 256)), dim3(256), 0, int_stream_, d_, d_bgr, d_depth, T);
    hipLaunchKernelGGL(k_alloc_commit, dim3(64), dim3(256), 0, int_stream_, d_);
    hipLaunchKernelGGL(k_cull, dim3(512), dim3(256), 0, int_stream_, d_, Ti);
    if (kernel_events_[2]) DR_HIP(hipEventRecord(kernel_events_[2], int_stream_));  // timing hook: end of allocate + commit + cull
    if (wait_renders) for (auto &r : renders_) DR_HIP(hipStreamWaitEvent(int_stream_, r.cast, 0));
    if (kernel_events_[0]) DR_HIP(hipEventRecord(kernel_events_[0], int_stream_));  // timing hooks: [0]..[1] brackets k_integrate alone
    hipLaunchKernelGGL(k_integrate, dim3(integrate_grid_), dim3(256), 0, int_stream_, d_, d_bgr, d_depth, T, Ti);
    if (kernel_events_[1]) DR_HIP(hipEventRecord(kernel_events_[1], int_stream_));
    hipLaunchKernelGGL(k_fold_counter, dim3(1), dim3(256), 0, int_stream_, d_.cnt, d_.req_count, d_.wg_upd, integrate_grid_);
    DR_HIP(hipGetLastError());
  }
  // ---- the mesh pass, shared by every extraction ----
  void mesh_empty() {
    DR_HIP(hipMemsetAsync(mesh_total_, 0, 8, int_stream_));
    DR_HIP(hipEventRecord(mesh_done_ev(), int_stream_));
  }
  // Prologue of every extraction (int_stream_ idle): the lattice into a.n, the statistics cleared; returns the pool's block count.
  // Nothing is launched yet: the caller enqueues the empty result (mesh_empty) or goes on with mesh_tables.
  int mesh_begin(const float *lower, const float *upper, McArgs &a) {
    for (int k = 0; k < 3; ++k) {  // lattice cells per axis (ExtractMeshKernel, mesh_extractor.cu:241-245)
      a.n[k] = f2i_host(fabsf(lower[k] - upper[k]) / o_.voxel_size);
      if (a.n[k] > (1 << 22))
        fail(DR_ERR_ARG, "ExtractMesh: %d lattice cells along axis %d (box too large for voxel_size %g)", a.n[k], k, o_.voxel_size);
    }
    if (!mesh_total_) mesh_total_ = own_.device<unsigned long long>(1);
    mesh_stats_[0] = mesh_stats_[1] = mesh_stats_[2] = 0;
    return pool_blocks();
  }
  static bool box_empty(const McArgs &a) { return a.n[0] <= 0 || a.n[1] <= 0 || a.n[2] <= 0; }
  // The axis tables, the per-block arrays and the 20 M-triangle output (allocated with the first extraction), then k_mc_axes and
  // the pool's nblk keys sorted into mesh_keys_.  The box is not empty.
  void mesh_tables(const float *lower, McArgs &a, int nblk) {
    const float vs = o_.voxel_size;
    mesh_axis_.reserve((size_t)a.n[0] + a.n[1] + a.n[2], int_stream_);
    if (!mesh_keys_) {
      mesh_keys_ = own_.device<unsigned long long>(o_.num_blocks);
      mesh_counts_ = own_.device<unsigned>(o_.num_blocks);
      mesh_offsets_ = own_.device<unsigned>(o_.num_blocks);
      size_t t1 = 0, t2 = 0;
      DR_HIP(rocprim::radix_sort_keys(nullptr, t1, d_.blk_key, mesh_keys_, (size_t)o_.num_blocks, 0, 63, int_stream_));
      DR_HIP(rocprim::exclusive_scan(nullptr, t2, mesh_counts_, mesh_offsets_, 0u, (size_t)o_.num_blocks, rocprim::plus<unsigned>(), int_stream_));
      mesh_tmp_.reserve(std::max(t1, t2), int_stream_);
      // the reference's MeshExtractor::Init(20000000, ...) (tsdf_volume.cu:776): 72 B per triangle, 1.44 GB of HBM
      mesh_vert_ = own_.device<float>((size_t)kMeshMaxTriangles * 9);
      mesh_cols_ = own_.device<float>((size_t)kMeshMaxTriangles * 9);
    }
    McAxis *p = mesh_axis_.get();
    for (int k = 0; k < 3; ++k) {
      hipLaunchKernelGGL(k_mc_axes, dim3(cdiv(a.n[k], 256)), dim3(256), 0, int_stream_, p, a.n[k], lower[k], vs);
      a.ax[k] = p;
      p += a.n[k];
    }
    a.counts = mesh_counts_; a.offsets = mesh_offsets_;
    a.vert = mesh_vert_; a.cols = mesh_cols_; a.cap_tri = kMeshMaxTriangles;
    size_t tb = mesh_tmp_.capacity();
    if (nblk > 0) DR_HIP(rocprim::radix_sort_keys(mesh_tmp_.get(), tb, d_.blk_key, mesh_keys_, (size_t)nblk, 0, 63, int_stream_));
  }
  // Count, scan, emit for the blocks a.sorted_keys[0, a.nblk).  Resident form: the result is these triangles (k_mc_total).
  // STAGED (one chunk of the map pass): emitted at the running total a.base, which then advances.
  // table: rows [row0, row0 + a.nblk) of the mesh update's patch table.
  template <bool STAGED> void mesh_pass(const McArgs &a, bool table, size_t row0 = 0) {
    const dim3 grid((unsigned)a.nblk), block(256);
    hipLaunchKernelGGL((k_mc_cells<false, STAGED>), grid, block, 0, int_stream_, d_, a);
    size_t tb = mesh_tmp_.capacity();
    DR_HIP(rocprim::exclusive_scan(mesh_tmp_.get(), tb, mesh_counts_, mesh_offsets_, 0u, (size_t)a.nblk, rocprim::plus<unsigned>(), int_stream_));
    hipLaunchKernelGGL((k_mc_cells<true, STAGED>), grid, block, 0, int_stream_, d_, a);
    if (!STAGED) hipLaunchKernelGGL(k_mc_total, dim3(1), dim3(1), 0, int_stream_, mesh_counts_, mesh_offsets_, a.nblk, mesh_total_);
    if (table)
      hipLaunchKernelGGL(k_mu_table, dim3(cdiv(a.nblk + 1, 256)), dim3(256), 0, int_stream_, a.sorted_keys, a.nblk, mesh_counts_, mesh_offsets_,
                         a.base, row0, mu_coords_.get(), mu_first_.get());
    if (STAGED) hipLaunchKernelGGL(k_mc_advance, dim3(1), dim3(1), 0, int_stream_, mesh_counts_, mesh_offsets_, a.nblk, mesh_total_);
  }
  // the extraction is enqueued: blocks meshed, host blocks uploaded (once per chunk that stages them), chunks
  void mesh_end(size_t blocks, size_t uploads, size_t chunks) {
    DR_HIP(hipGetLastError());
    DR_HIP(hipEventRecord(mesh_done_ev(), int_stream_));
    mesh_stats_[0] = blocks; mesh_stats_[1] = uploads; mesh_stats_[2] = chunks;
  }
  // DRF_MESH_MAP folds pending evictions first; with an empty host store it is the resident pass
  void launch_extraction(const float *lower, const float *upper) {
    if (mesh_scope_ == DRF_MESH_MAP) {
      settle();
      if (!store_.empty()) return launch_mesh_map(lower, upper);
    }
    launch_mesh(lower, upper);
  }
  // Enqueue the whole extraction on int_stream_ (after the last integration, before the next one).
  void launch_mesh(const float *lower, const float *upper) {
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipStreamSynchronize(int_stream_));  // the block count lives on the device
    McArgs a{};
    const int nblk = mesh_begin(lower, upper, a);
    if (box_empty(a) || nblk <= 0) return mesh_empty();
    mesh_tables(lower, a, nblk);
    a.sorted_keys = mesh_keys_; a.nblk = nblk;
    mesh_pass<false>(a, false);
    mesh_end((size_t)nblk, 0, 1);
  }
  // ---- mesh update: selection and the resident form ----
  // every entry point that integrates comes through enqueue_scan.  A pose that is not a finite rigid motion (the reach bound
  // assumes one) or one scan too many makes the next update full.
  void record_scan_pose(const Mat &Ti) {
    const bool rigid = pose_is_rigid(Ti.m);  // (fusion_host.h: the one statement of the rule, shared with the render scope)
    if (!rigid || mu_poses_.size() == (size_t)DRF_MESH_UPDATE_MAX_SCANS) { mu_overflow_ = true; return; }
    MuPose p;
    memcpy(p.m, Ti.m, 48);
    mu_poses_.push_back(p);
  }
  // Blocks of keys[0, n) (device, ascending) to mesh again after the recorded scans, compacted in order into mu_sel_; returns
  // their number (one 4-byte read back: the mesh kernels' grid).
  int mu_select(const unsigned long long *keys, int n) {
    mu_flags_.reserve((size_t)n, int_stream_); mu_pos_.reserve((size_t)n, int_stream_); mu_sel_.reserve((size_t)n, int_stream_);
    if (!mu_nsel_) mu_nsel_ = own_.device<int>(1);
    size_t tb = 0;  // scan scratch for n items (the mesh path's is sized for the pool; a map's scope may be longer)
    DR_HIP(rocprim::exclusive_scan(nullptr, tb, mesh_counts_, mesh_offsets_, 0u, (size_t)n, rocprim::plus<unsigned>(), int_stream_));
    mesh_tmp_.reserve(tb, int_stream_);
    MuArgs m{};
    m.keys = keys; m.n = n; m.nposes = (int)mu_poses_.size(); m.reach2 = mesh_update_reach2(o_); m.flags = mu_flags_.get();
    memcpy(m.Ti, mu_poses_.data(), mu_poses_.size() * sizeof(MuPose));
    hipLaunchKernelGGL(k_mu_select, dim3(cdiv(n, 256)), dim3(256), 0, int_stream_, o_, m);
    tb = mesh_tmp_.capacity();
    DR_HIP(rocprim::exclusive_scan(mesh_tmp_.get(), tb, mu_flags_.get(), mu_pos_.get(), 0u, (size_t)n, rocprim::plus<unsigned>(), int_stream_));
    hipLaunchKernelGGL(k_mu_compact, dim3(cdiv(n, 256)), dim3(256), 0, int_stream_, keys, mu_flags_.get(), mu_pos_.get(), n, mu_sel_.get(), mu_nsel_);
    DR_HIP(hipGetLastError());
    int nsel = 0;
    DR_HIP(hipMemcpyAsync(&nsel, mu_nsel_, 4, hipMemcpyDeviceToHost, int_stream_));
    DR_HIP(hipStreamSynchronize(int_stream_));
    return std::max(0, std::min(nsel, n));
  }
  void mu_table_reserve(size_t nblk) { mu_coords_.reserve(3 * nblk, int_stream_); mu_first_.reserve(nblk + 1, int_stream_); }
  // The resident pass of launch_mesh over the selected blocks only (all of them when mu_next_.full), plus the patch table.
  void launch_mesh_update(const float *lower, const float *upper) {
    McArgs a{};
    const int nblk = mesh_begin(lower, upper, a);
    mu_stats_[0] = (uint64_t)std::max(nblk, 0); mu_stats_[1] = 0; mu_stats_[2] = mu_poses_.size(); mu_stats_[3] = mu_next_.full;
    if (box_empty(a) || nblk <= 0 || (!mu_next_.full && mu_poses_.empty())) return mesh_empty();
    mesh_tables(lower, a, nblk);
    a.sorted_keys = mesh_keys_; a.nblk = nblk;
    if (!mu_next_.full) { a.nblk = mu_select(mesh_keys_, nblk); a.sorted_keys = mu_sel_.get(); }
    if (a.nblk == 0) return mesh_empty();
    mu_table_reserve((size_t)a.nblk);
    mesh_pass<false>(a, true);
    mesh_end((size_t)a.nblk, 0, 1);
    mu_stats_[1] = (uint64_t)a.nblk; mu_next_.nblk = (size_t)a.nblk;
  }
  // ---- the map pass (DRF_MESH_MAP with blocks in the host store; DESIGN.md §7c "Meshing the whole map") ----
  // Global order = ascending key over resident and stored blocks, as the resident pass orders the pool.  The merged list is cut
  // into chunks (plan_mesh_chunks); a chunk's keys and the stored blocks it stages are packed into pinned memory and copied to
  // one of two device buffers on a copy stream, so that packing and copying chunk k + 1 overlap the kernels of chunk k.  Per chunk:
  // mesh_pass at the running base (mesh_total_).  Neither the pool nor the host store changes.
  int ms_own_cap() const { return std::min(o_.num_blocks, kStageBlocks); }
  int ms_stage_cap() const { return std::max(ms_own_cap(), 27); }  // one block's 27 neighbours always fit
  // update: the mesh-update form (drf_extract_mesh_update_async) -- only the blocks the selection kernel keeps (all of the scope
  // when mu_next_.full) are planned into chunks, staged and meshed, and each chunk adds its rows to the patch table.
  void launch_mesh_map(const float *lower, const float *upper, bool update = false) {
    McArgs a{};
    const int nblk = mesh_begin(lower, upper, a);
    if (update) { mu_stats_[0] = mu_stats_[1] = 0; mu_stats_[2] = mu_poses_.size(); mu_stats_[3] = mu_next_.full; }
    if (box_empty(a)) return mesh_empty();  // (an empty pool is no reason: the host store holds blocks)
    mesh_tables(lower, a, nblk);
    std::vector<unsigned long long> res(std::max(nblk, 0));
    if (nblk > 0) DR_HIP(hipMemcpyAsync(res.data(), mesh_keys_, (size_t)nblk * 8, hipMemcpyDeviceToHost, int_stream_));
    const std::vector<unsigned long long> sto = store_.sorted_keys();
    const BlockRange range = lattice_block_range(lower, a.n, o_.voxel_size);
    DR_HIP(hipStreamSynchronize(int_stream_));
    // update: the scope is the merged list within the range; the selection kernel runs over it and the survivors come back
    std::vector<unsigned long long> picked;
    if (update) {
      picked.reserve(res.size() + sto.size());
      for_each_in_range(res, sto, range, [&](unsigned long long key, bool) { picked.push_back(key); });
      mu_stats_[0] = picked.size();
      if (picked.empty() || (!mu_next_.full && mu_poses_.empty())) return mesh_empty();
      if (picked.size() > (size_t)INT_MAX) fail(DR_ERR_CAPACITY, "mesh update: %zu blocks in scope", picked.size());
      if (!mu_next_.full) {
        mu_scope_.reserve(picked.size(), int_stream_);
        DR_HIP(hipMemcpyAsync(mu_scope_.get(), picked.data(), picked.size() * 8, hipMemcpyHostToDevice, int_stream_));
        const int nsel = mu_select(mu_scope_.get(), (int)picked.size());
        if (nsel == 0) return mesh_empty();
        picked.resize((size_t)nsel);
        DR_HIP(hipMemcpy(picked.data(), mu_sel_.get(), (size_t)nsel * 8, hipMemcpyDeviceToHost));
      }
      mu_table_reserve(picked.size());
    }
    const MeshPlan plan = plan_mesh_chunks(res, sto, store_, range, (size_t)ms_own_cap(), (size_t)ms_stage_cap(), update ? &picked : nullptr);
    DR_HIP(hipMemsetAsync(mesh_total_, 0, 8, int_stream_));
    if (plan.chunks() > 0 && !ms_.stream()) {
      ms_.open(own_);
      ms_.reserve((size_t)ms_own_cap() * 8 + (size_t)ms_stage_cap() * (8 + 4096));
    }
    a.base = mesh_total_;
    for (size_t ch = 0; ch < plan.chunks(); ++ch) {
      const size_t no = plan.ob[ch + 1] - plan.ob[ch], ns = plan.sb[ch + 1] - plan.sb[ch];
      unsigned char *h = ms_.next();  // the copy of chunk ch - 2 has left this pinned buffer
      memcpy(h, plan.own.data() + plan.ob[ch], no * 8);
      pack_stored(plan.stg.data() + plan.sb[ch], ns, h + no * 8, h + (no + ns) * 8);
      ms_.wait_for(ms_.used());  // the kernels of chunk ch - 2 have read this device buffer
      ms_.copy((no + ns) * 8 + ns * 4096);
      ms_.record_ready();
      ms_.wait_ready(int_stream_);
      const unsigned long long *dk = (const unsigned long long *)ms_.dev();
      a.sorted_keys = dk; a.nblk = (int)no;
      a.st_keys = dk + no; a.st_n = (int)ns; a.st_vox = (const Voxel *)(dk + no + ns);
      mesh_pass<true>(a, update, plan.ob[ch]);
      DR_HIP(hipEventRecord(ms_.used(), int_stream_));
    }
    mesh_end(plan.own.size(), plan.stg.size(), plan.chunks());
    if (update) { mu_stats_[1] = plan.own.size(); mu_next_.nblk = plan.own.size(); }
  }
  hipEvent_t mesh_done_ev() {
    if (!mesh_done_) mesh_done_ = own_.event();
    return mesh_done_;
  }
  void fetch_mesh(size_t ntri, float *vert, float *cols) {
    DR_HIP(hipMemcpy(vert, mesh_vert_, ntri * 36, hipMemcpyDeviceToHost));
    DR_HIP(hipMemcpy(cols, mesh_cols_, ntri * 36, hipMemcpyDeviceToHost));
  }
  size_t finish_mesh() {
    DR_HIP(hipSetDevice(device_));
    DR_HIP(hipEventSynchronize(mesh_done_ev()));
    unsigned long long t = 0;
    DR_HIP(hipMemcpy(&t, mesh_total_, 8, hipMemcpyDeviceToHost));
    if (t > kMeshMaxTriangles) fail(DR_ERR_CAPACITY, "Triangles limit reached! (%llu > %u)", t, kMeshMaxTriangles);
    return (size_t)t;
  }
  // Correctly rounded reciprocals of the three per-engine divisors, each checked against IEEE division over all 2^32
  // dividends (see div_exact); DR_FUSION_IEEE_DIV=1 forces the IEEE sequences (A/B and fallback testing).
  static float rcp_rn(float b) { return (float)(1.0 / (double)b); }  // double rounding cannot bite: 1/b is never within 2^-49 of a float midpoint
  void setup_fast_div() {
    d_.vs_rcp = rcp_rn(o_.voxel_size); d_.fx_rcp = rcp_rn(o_.fx); d_.fy_rcp = rcp_rn(o_.fy);
    d_.fast_div = 0;
    if (hook_env("DR_FUSION_IEEE_DIV")) return;
    DeviceBuf<unsigned long long> counter;  // freed when the check is done
    counter.reserve(1, int_stream_);
    unsigned long long *bad = counter.get(), h = 0;
    DR_HIP(hipMemsetAsync(bad, 0, 8, int_stream_));
    const float b[3] = {o_.voxel_size, o_.fx, o_.fy}, y[3] = {d_.vs_rcp, d_.fx_rcp, d_.fy_rcp};
    for (int k = 0; k < 3; ++k)
      if (b[k] > 0.0f && b[k] < 1e30f) hipLaunchKernelGGL(k_verify_fast_div, dim3(4096), dim3(256), 0, int_stream_, b[k], y[k], bad);
      else h = 1;
    DR_HIP(hipMemcpyAsync(&fast_div_mismatches_, bad, 8, hipMemcpyDeviceToHost, int_stream_));
    DR_HIP(hipStreamSynchronize(int_stream_));
    fast_div_mismatches_ += h;
    d_.fast_div = fast_div_mismatches_ == 0 ? 1 : 0;
  }
  void check_device_flags() {
    int f[4];
    DR_HIP(hipMemcpy(f, d_.n_alloc, 16, hipMemcpyDeviceToHost));
    if (f[1] || f[2]) fail(DR_ERR_CAPACITY, "DrFusion: block pool exhausted (num_blocks=%d) or block coordinate out of range", o_.num_blocks);
  }

  HipOwner own_;  // first: released after every other member
  int device_;
  drf_options_t o_;
  FusionDev d_{};
  size_t npix_ = 0;
  hipStream_t int_stream_ = nullptr;
  hipEvent_t int_done_ = nullptr;
  hipEvent_t kernel_events_[3] = {nullptr, nullptr, nullptr};
  unsigned char *d_bgr_in_ = nullptr, *h_bgr_in_ = nullptr;
  float *d_depth_in_ = nullptr, *h_depth_in_ = nullptr;
  int integrate_grid_ = 4096;
  unsigned long long fast_div_mismatches_ = 0;
  // switches, read once here.  Product: the empty-space skip's A/B switch (a run-time flag of the same kernel) and DR_FUSION_IEEE_DIV (the
  // IEEE-division instances are the product's fallback when the exact fast division fails its check).  Parity build (-DDR_PARITY_HOOKS):
  // the superseded generations -- the literal ray-caster, round 2's four-stage sampler, copy-engine result transfers, statistics.
  bool raycast_no_skip_ = hook_env("DR_RAYCAST_NO_SKIP") != nullptr;
#ifdef DR_PARITY_HOOKS
  bool raycast_v1_ = hook_env("DR_RAYCAST_V1") != nullptr;
  int raycast_sampler_ = hook_env("DR_RAYCAST_SAMPLER") ? std::max(0, std::min(1, atoi(hook_env("DR_RAYCAST_SAMPLER")))) : (getenv("DR_RAYCAST_UNSTAGED") ? 0 : 1);
  bool render_copy_ = hook_env("DR_RENDER_D2H") && !strcmp(hook_env("DR_RENDER_D2H"), "copy");
  bool raycast_stats_ = hook_env("DR_RAYCAST_STATS") != nullptr;     // measuring hook: iteration statistics of k_raycast2 on stderr
  unsigned long long *d_rstats_ = nullptr;
#else
  static constexpr bool render_copy_ = false;
#endif
  std::vector<Render> renders_;
  int free_slot_ = 0;
  Next next_ = kIntegrate;
  bool loaded_ = false;  // the map came from drf_load_map / drf_merge_map and no scan followed yet: RenderAsync is legal where IntegrateScanAsync is
  // mesh extraction state (allocated with the first ExtractMeshAsync)
  static constexpr unsigned kMeshMaxTriangles = 20000000;
  bool mesh_pending_ = false;
  hipEvent_t mesh_done_ = nullptr;
  DeviceBuf<McAxis> mesh_axis_;
  DeviceBuf<unsigned char> mesh_tmp_;  // radix sort / scan scratch
  unsigned long long *mesh_keys_ = nullptr, *mesh_total_ = nullptr;
  unsigned *mesh_counts_ = nullptr, *mesh_offsets_ = nullptr;
  float *mesh_vert_ = nullptr, *mesh_cols_ = nullptr;
  int mesh_scope_ = DRF_MESH_RESIDENT;
  uint64_t mesh_stats_[3] = {0, 0, 0};
  // mesh update (incremental mesh).  mu_base_ = the baseline, i.e. the last update fetched: its box, the round-trip redirect
  // count at its launch; mu_next_ = the pending update, which becomes the baseline when it is fetched; mu_poses_ = Ti of the
  // scans since the last update was LAUNCHED (they belong to the next one).  Device scratch grows with the scope.
  struct MeshUpdate {
    bool valid = false, full = false;
    float box[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long redirects = 0; size_t nblk = 0;  // nblk: rows of its patch table
  };
  bool mesh_pending_update_ = false;
  bool mu_force_full_ = false, mu_overflow_ = false;
  MeshUpdate mu_base_, mu_next_;
  std::vector<MuPose> mu_poses_;
  uint64_t mu_stats_[4] = {0, 0, 0, 0};
  DeviceBuf<unsigned> mu_flags_, mu_pos_;
  DeviceBuf<unsigned long long> mu_sel_, mu_scope_, mu_first_;
  DeviceBuf<int> mu_coords_;
  int *mu_nsel_ = nullptr;
  // map pass staging (opened by the first map-scope extraction that meets a non-empty host store): own keys + staged keys + staged voxels
  BlockStaging ms_;
  // render scope: staging opened by the first map-scope render that has stored blocks in reach, grown up to rs_capacity()
  BlockStaging rs_;
  DeviceBuf<unsigned long long> rs_table_[2];  // per slot of rs_: the open-addressing table and the two staged superblock flag arrays
  unsigned char *rs_super_[2][2] = {};
  int render_scope_ = DRF_RENDER_RESIDENT;
  size_t rs_cap_req_ = 0, rs_blocks_ = 0;
  uint64_t render_stats_[4] = {0, 0, 0, 0};
  int render_bands_ = 0;  // drf_set_render_bands
  uint64_t band_stats_[4] = {0, 0, 0, 0};
  // streaming state (staging allocated with the first drf_set_streaming / region call)
  float st_radius_ = 0.0f;                  // 0 = off
  size_t st_host_cap_ = (size_t)-1;         // host store capacity in blocks
  HostBlockStore store_;
  int st_cap_ = 0;                          // staging capacity in blocks (0 = not allocated)
  StreamDev sd_{};
  unsigned long long *h_ev_keys_ = nullptr, *h_in_keys_ = nullptr, *hd_in_keys_ = nullptr;
  uint8_t *h_ev_vox_ = nullptr, *h_in_vox_ = nullptr, *hd_in_vox_ = nullptr;
  hipEvent_t st_ev_[4] = {nullptr, nullptr, nullptr, nullptr};  // [0..1] stream-in, [2..3] eviction of the last scan
  int st_timed_ = 0;
  bool st_scan_done_ = false;
  double st_last_us_ = 0.0;
  bool ev_pending_ = false, ev_auto_ = false;  // an eviction chain awaits folding; it was the automatic one (centre ev_p_)
  double ev_p_[3] = {0.0, 0.0, 0.0};
  ReachBalls reach_;  // balls that hold every block centre of the map
  uint64_t st_out_total_ = 0, st_in_total_ = 0;
  // map file transport (map_ops.h; allocated with the first use): two pinned chunk buffers, the sorted (key, slot) pairs
  MapIo mio_;
  DeviceBuf<unsigned long long> mg_counts_;  // drf_merge_map: voxels of case 2 and case 3 counted by k_map_merge
  uint64_t mg_stats_[6] = {0, 0, 0, 0, 0, 0};  // drf_merge_stats
  DeviceBuf<unsigned char> lc_buf_;            // drf_locate_*: partial sums, counters and a host-given depth image (sized once)
  uint64_t lc_stats_[6] = {0, 0, 0, 0, 0, 0};  // drf_locate_stats
  TrackSide tk_, tc_, tp_;                     // drf_track_*, drf_track_colour_*, drf_track_reduce / drf_track_pyramid_*: each its own scratch, statistics and model render (with_track)
  unsigned long long *tc_fifth_ = nullptr;     // pinned: the fifth counter of an evaluation with colour
  int locate_scope_ = DRF_LOCATE_RESIDENT;     // drf_set_locate_scope
  size_t lc_cap_req_ = 0;
  uint64_t ls_stats_[4] = {0, 0, 0, 0};        // drf_locate_stage_stats
};

}  // namespace dr

// ==================================================================== C ABI
using dr::guarded;
struct drf_s {
  std::unique_ptr<dr::FusionEngine> e;
};
// every C-ABI entry point goes through this: a NULL handle is an argument error, not a crash
static inline dr::FusionEngine *eng(drf_s *h) {
  if (!h || !h->e) dr::fail(DR_ERR_ARG, "NULL handle");
  return h->e.get();
}
// A search for a pose (drf_align_map, drf_*_frame): DEGENERATE and LOST are results, not failures -- DR_OK, with the reason, the note
// call() returns, where a failure's message would be.
template <class Call>
static int guarded_note(Call &&call) {
  std::string note;
  const int rc = guarded([&] { note = call(); });
  if (rc == DR_OK && !note.empty()) dr::last_error_slot() = note;
  return rc;
}
// the six statistics of an operation's last call, through the engine's getter
static int stats6(drf_s *h, const char *who, uint64_t *out, const uint64_t *(dr::FusionEngine::*get)() const) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "%s: null argument", who);
    const uint64_t *s = (eng(h)->*get)();
    for (int i = 0; i < 6; ++i) out[i] = s[i];
  });
}

extern "C" {

int drf_create(const drf_options_t *opt, int device, drf_t **out) {
  return guarded([&] {
    if (!opt || !out) dr::fail(DR_ERR_ARG, "drf_create: null argument");
    auto *h = new drf_s();
    try { h->e.reset(new dr::FusionEngine(*opt, device)); } catch (...) { delete h; throw; }
    *out = h;
  });
}
void drf_destroy(drf_t *h) { delete h; }
int drf_integrate_scan_async(drf_t *h, const uint8_t *bgr, const float *depth, const float *pose16) {
  return guarded([&] { eng(h)->integrate_scan_async(bgr, depth, pose16); });
}
int drf_render_async(drf_t *h, const float *const *poses16, int n) { return guarded([&] { eng(h)->render_async(poses16, n); }); }
int drf_get_render_result(drf_t *h, uint8_t **bgr, float **depth, int n) { return guarded([&] { eng(h)->get_render_result(bgr, depth, n); }); }
int drf_extract_mesh_async(drf_t *h, const float *lower, const float *upper) {
  return guarded([&] { eng(h)->extract_mesh_async(lower, upper); });
}
int drf_get_mesh_sync(drf_t *h, size_t num_max, size_t *num, float *vert, float *cols) {
  return guarded([&] { eng(h)->get_mesh_sync(num_max, num, vert, cols); });
}
int drf_mesh_num_triangles(drf_t *h, size_t *ntri) {
  return guarded([&] { if (!ntri) dr::fail(DR_ERR_ARG, "drf_mesh_num_triangles: null argument"); *ntri = eng(h)->mesh_num_triangles(); });
}
int drf_save_mesh(drf_t *h, const char *filename, const float *lower, const float *upper) {
  return guarded([&] { eng(h)->save_mesh(filename, lower, upper); });
}
int drf_get_render_device(drf_t *h, int stream, const uint8_t **d_bgr, const float **d_depth) {
  return guarded([&] { eng(h)->get_render_device(stream, d_bgr, d_depth); });
}
int drf_synchronize(drf_t *h) { return guarded([&] { eng(h)->synchronize(); }); }
int drf_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->stats(out); }); }
int drf_export_blocks(drf_t *h, int max_blocks, int32_t *coords, uint8_t *voxels, int *n) {
  return guarded([&] { eng(h)->export_blocks(max_blocks, coords, voxels, n); });
}
int drf_fast_div_status(drf_t *h, int *enabled, uint64_t *mismatches) {
  return guarded([&] { unsigned long long m = 0; eng(h)->fast_div_status(enabled, &m); if (mismatches) *mismatches = m; });
}
int drf_test_combine(drf_t *h, size_t n, const uint8_t *a, const uint8_t *b, int max_weight, uint8_t *out) {
  return guarded([&] { if (!a || !b || !out) dr::fail(DR_ERR_ARG, "drf_test_combine: null argument"); eng(h)->test_combine(n, a, b, max_weight, out); });
}
int drf_integrate_device(drf_t *h, const void *d_bgr, const void *d_depth, const float *pose16) {
  return guarded([&] { eng(h)->integrate_device(d_bgr, d_depth, pose16); });
}
int dr_device_alloc(int device, size_t bytes, void **dptr) {
  return guarded([&] { DR_HIP(hipSetDevice(device)); DR_HIP(dr::device_alloc(dptr, bytes, "dr_device_alloc")); });
}
int dr_device_free(void *dptr) { return guarded([&] { DR_HIP(dr::device_free(dptr)); }); }
// The guarded allocator's switch and its check (dr_common.h, guard_host.h): parity build only.
int dr_guard_set(size_t guard_bytes) {
  return guarded([&] {
#ifndef DR_PARITY_HOOKS
    (void)guard_bytes;
    dr::fail(DR_ERR_UNSUPPORTED, "dr_guard_set: guarded allocation is built into the parity library (libdr_mi355x_hooks.so, -DDR_PARITY_HOOKS) only");
#else
    if (guard_bytes % dr::guard::kGranule) dr::fail(DR_ERR_ARG, "dr_guard_set: the guard size must be a multiple of %zu bytes (0: off)", dr::guard::kGranule);
    dr::guard::Registry &r = dr::guard::registry();
    std::lock_guard<std::mutex> lk(r.mu);
    r.guard_bytes = guard_bytes;
#endif
  });
}
int dr_guard_check(uint64_t out[4], char *report, size_t cap) {
  return guarded([&] {
#ifndef DR_PARITY_HOOKS
    (void)out; (void)report; (void)cap;
    dr::fail(DR_ERR_UNSUPPORTED, "dr_guard_check: guarded allocation is built into the parity library (libdr_mi355x_hooks.so, -DDR_PARITY_HOOKS) only");
#else
    if (!out) dr::fail(DR_ERR_ARG, "dr_guard_check: null argument");
    dr::guard::Registry &r = dr::guard::registry();
    std::lock_guard<std::mutex> lk(r.mu);
    std::vector<dr::guard::Violation> all = r.sticky;
    uint64_t bytes = 0;
    if (!r.live.empty()) DR_HIP(hipDeviceSynchronize());
    for (auto &kv : r.live) { dr::guard::scan_entry(kv.first, kv.second, all); bytes += kv.second.bytes; }
    out[0] = r.live.size(); out[1] = r.since_clear; out[2] = all.size(); out[3] = bytes;
    dr::guard::report(all, report, cap);
#endif
  });
}
int dr_guard_clear(void) {
  return guarded([&] {
#ifndef DR_PARITY_HOOKS
    dr::fail(DR_ERR_UNSUPPORTED, "dr_guard_clear: guarded allocation is built into the parity library (libdr_mi355x_hooks.so, -DDR_PARITY_HOOKS) only");
#else
    dr::guard::Registry &r = dr::guard::registry();
    std::lock_guard<std::mutex> lk(r.mu);
    r.sticky.clear();
    r.since_clear = 0;
#endif
  });
}
int dr_memcpy_h2d(void *dptr, const void *src, size_t bytes) { return guarded([&] { DR_HIP(hipMemcpy(dptr, src, bytes, hipMemcpyHostToDevice)); }); }
int dr_memcpy_d2d(void *dst, const void *src, size_t bytes) {
  // a device-to-device hipMemcpy may return before the copy has run, and the engines' streams are non-blocking:
  // synchronise so that whatever the caller enqueues next (on any stream) sees the data
  return guarded([&] {
    hipPointerAttribute_t at;  // synchronise the device that owns the destination, not whichever is current on this thread --
    int prev = -1;             // and leave the caller's current device as it was (a helper must not move a host thread between GPUs)
    (void)hipGetDevice(&prev);
    const bool moved = hipPointerGetAttributes(&at, dst) == hipSuccess && at.device != prev;
    if (moved) DR_HIP(hipSetDevice(at.device));
    const hipError_t e1 = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice);
    const hipError_t e2 = e1 == hipSuccess ? hipDeviceSynchronize() : e1;
    if (moved && prev >= 0) (void)hipSetDevice(prev);
    DR_HIP(e2);
  });
}
int dr_memcpy_d2h(void *dst, const void *dptr, size_t bytes) { return guarded([&] { DR_HIP(hipMemcpy(dst, dptr, bytes, hipMemcpyDeviceToHost)); }); }
int drf_bench_sequence(drf_t *h, const void *d_bgr, const void *d_depth, const float *poses16, int nframes, int render, float ms[6]) {
  return guarded([&] { eng(h)->bench_sequence(d_bgr, d_depth, poses16, nframes, render, ms); });
}
int drf_visited_blocks(drf_t *h, uint64_t *total) {
  return guarded([&] { if (!total) dr::fail(DR_ERR_ARG, "drf_visited_blocks: null pointer"); *total = eng(h)->visited_blocks(); });
}
int drf_bench_render_host(drf_t *h, int stream, int back, const uint8_t **bgr, const float **depth) {
  return guarded([&] { eng(h)->bench_render_host(stream, back, bgr, depth); });
}
int drf_bench_integrate(drf_t *h, const void *d_bgr, const void *d_depth, const float *poses16, int nscans, float *ms, float *kernel_ms) {
  return guarded([&] { eng(h)->bench_integrate(d_bgr, d_depth, poses16, nscans, ms, kernel_ms); });
}
int drf_streaming_min_radius(const drf_options_t *o, float *radius) {
  return guarded([&] {
    if (!o || !radius) dr::fail(DR_ERR_ARG, "drf_streaming_min_radius: null argument");
    if (!dr::stream_options_ok(*o)) dr::fail(DR_ERR_ARG, "drf_streaming_min_radius: invalid options (voxel_size, fx, fy, max_sensor_depth must be > 0, width and height > 0)");
    *radius = dr::streaming_min_radius(*o);
  });
}
int drf_set_streaming(drf_t *h, float radius, size_t host_capacity_blocks) {
  return guarded([&] { eng(h)->set_streaming(radius, host_capacity_blocks); });
}
int drf_stream_out_region(drf_t *h, const float lower[3], const float upper[3]) {
  return guarded([&] { eng(h)->stream_out_region(lower, upper); });
}
int drf_stream_in_region(drf_t *h, const float lower[3], const float upper[3]) {
  return guarded([&] { eng(h)->stream_in_region(lower, upper); });
}
int drf_streaming_stats(drf_t *h, uint64_t out[6]) {
  return guarded([&] { if (!out) dr::fail(DR_ERR_ARG, "drf_streaming_stats: null argument"); eng(h)->streaming_stats(out); });
}
int drf_export_host_blocks(drf_t *h, int max_blocks, int32_t *coords, uint8_t *voxels, int *n) {
  return guarded([&] { eng(h)->export_host_blocks(max_blocks, coords, voxels, n); });
}
int drf_map_info(const char *path, float *voxel_size, uint64_t *n_blocks) {
  return guarded([&] {
    if (!path || !voxel_size || !n_blocks) dr::fail(DR_ERR_ARG, "drf_map_info: null argument");
    std::string err;
    if (!dr::map_file_info(path, voxel_size, n_blocks, err)) dr::fail(DR_ERR_IO, "drf_map_info: %s", err.c_str());
  });
}
int drf_save_map(drf_t *h, const char *path, size_t chunk_blocks) { return guarded([&] { eng(h)->save_map(path, chunk_blocks); }); }
int drf_load_map(drf_t *h, const char *path, size_t chunk_blocks) { return guarded([&] { eng(h)->load_map(path, chunk_blocks); }); }
int drf_merge_map(drf_t *h, const char *path, size_t chunk_blocks) { return guarded([&] { eng(h)->merge_map(path, chunk_blocks); }); }
int drf_merge_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_merge_stats", out, &dr::FusionEngine::merge_stats); }
int drf_transform_map(drf_t *h, const char *src_path, const float T16[16], const char *dst_path, size_t chunk_blocks) {
  return guarded([&] { eng(h)->transform_map(src_path, T16, dst_path, chunk_blocks); });
}
int drf_transform_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_transform_stats", out, &dr::FusionEngine::transform_stats); }
int drf_align_system(drf_t *h, const char *src_path, const char *ref_path, const float T16[16], const drf_align_options_t *opt, double sums[28],
                     uint64_t counts[3]) {
  return guarded([&] { eng(h)->align_system(src_path, ref_path, T16, opt, sums, counts); });
}
int drf_align_map(drf_t *h, const char *src_path, const char *ref_path, const float T_init16[16], const drf_align_options_t *opt, float T16_out[16],
                  drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->align_map(src_path, ref_path, T_init16, opt, T16_out, res); });
}
int drf_align_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_align_stats", out, &dr::FusionEngine::align_stats); }
int drf_locate_system(drf_t *h, const float *depth, const float pose16[16], const drf_locate_options_t *opt, double sums[28], uint64_t counts[4]) {
  return guarded([&] { eng(h)->locate_system("drf_locate_system", depth, nullptr, pose16, opt, sums, counts); });
}
int drf_locate_system_device(drf_t *h, const void *d_depth, const float pose16[16], const drf_locate_options_t *opt, double sums[28], uint64_t counts[4]) {
  return guarded([&] { eng(h)->locate_system("drf_locate_system_device", nullptr, d_depth, pose16, opt, sums, counts); });
}
int drf_locate_frame(drf_t *h, const float *depth, const float pose_init16[16], const drf_locate_options_t *opt, float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->locate_frame("drf_locate_frame", depth, nullptr, pose_init16, opt, pose16_out, res); });
}
int drf_locate_frame_device(drf_t *h, const void *d_depth, const float pose_init16[16], const drf_locate_options_t *opt, float pose16_out[16],
                            drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->locate_frame("drf_locate_frame_device", nullptr, d_depth, pose_init16, opt, pose16_out, res); });
}
int drf_locate_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_locate_stats", out, &dr::FusionEngine::locate_stats); }
using dr::FramePair;
int drf_track_system(drf_t *h, const float *depth, const float *model_depth, const float model_pose16[16], const float pose16[16], const drf_track_options_t *opt,
                     double sums[28], uint64_t counts[4]) {
  return guarded([&] {
    eng(h)->track_system("drf_track_system", FramePair::host(nullptr, depth), FramePair::host(nullptr, model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_system_device(drf_t *h, const void *d_depth, const void *d_model_depth, const float model_pose16[16], const float pose16[16],
                            const drf_track_options_t *opt, double sums[28], uint64_t counts[4]) {
  return guarded([&] {
    eng(h)->track_system("drf_track_system_device", FramePair::device(nullptr, d_depth), FramePair::device(nullptr, d_model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_frame(drf_t *h, const float *depth, const float pose_init16[16], const drf_track_options_t *opt, float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_frame("drf_track_frame", FramePair::host(nullptr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_frame_device(drf_t *h, const void *d_depth, const float pose_init16[16], const drf_track_options_t *opt, float pose16_out[16],
                           drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_frame("drf_track_frame_device", FramePair::device(nullptr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_track_stats", out, &dr::FusionEngine::track_stats); }
int drf_track_colour_system(drf_t *h, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth, const float model_pose16[16],
                            const float pose16[16], const drf_track_colour_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track_system("drf_track_colour_system", FramePair::host(bgr, depth), FramePair::host(model_bgr, model_depth), model_pose16, pose16, opt, sums, counts);
  });
}
int drf_track_colour_system_device(drf_t *h, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth, const float model_pose16[16],
                                   const float pose16[16], const drf_track_colour_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track_system("drf_track_colour_system_device", FramePair::device(d_bgr, d_depth), FramePair::device(d_model_bgr, d_model_depth), model_pose16, pose16, opt, sums,
                         counts);
  });
}
int drf_track_colour_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_colour_options_t *opt, float pose16_out[16],
                           drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_frame("drf_track_colour_frame", FramePair::host(bgr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_colour_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_colour_options_t *opt,
                                  float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_frame("drf_track_colour_frame_device", FramePair::device(d_bgr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_colour_stats(drf_t *h, uint64_t out[6]) { return stats6(h, "drf_track_colour_stats", out, &dr::FusionEngine::track_colour_stats); }
int drf_track_reduce(drf_t *h, int level, float max_jump, const uint8_t *bgr, const float *depth, uint8_t *bgr_out, float *depth_out) {
  return guarded([&] { eng(h)->track_reduce("drf_track_reduce", level, max_jump, FramePair::host(bgr, depth), bgr_out, depth_out); });
}
int drf_track_reduce_device(drf_t *h, int level, float max_jump, const void *d_bgr, const void *d_depth, void *d_bgr_out, void *d_depth_out) {
  return guarded([&] { eng(h)->track_reduce("drf_track_reduce_device", level, max_jump, FramePair::device(d_bgr, d_depth), d_bgr_out, d_depth_out); });
}
int drf_track_pyramid_system(drf_t *h, int level, const uint8_t *bgr, const float *depth, const uint8_t *model_bgr, const float *model_depth,
                             const float model_pose16[16], const float pose16[16], const drf_track_pyramid_options_t *opt, double sums[28], uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track_pyramid_system("drf_track_pyramid_system", level, FramePair::host(bgr, depth), FramePair::host(model_bgr, model_depth), model_pose16, pose16, opt, sums,
                                 counts);
  });
}
int drf_track_pyramid_system_device(drf_t *h, int level, const void *d_bgr, const void *d_depth, const void *d_model_bgr, const void *d_model_depth,
                                    const float model_pose16[16], const float pose16[16], const drf_track_pyramid_options_t *opt, double sums[28],
                                    uint64_t counts[5]) {
  return guarded([&] {
    eng(h)->track_pyramid_system("drf_track_pyramid_system_device", level, FramePair::device(d_bgr, d_depth), FramePair::device(d_model_bgr, d_model_depth), model_pose16,
                                 pose16, opt, sums, counts);
  });
}
int drf_track_pyramid_frame(drf_t *h, const uint8_t *bgr, const float *depth, const float pose_init16[16], const drf_track_pyramid_options_t *opt,
                            float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_pyramid_frame("drf_track_pyramid_frame", FramePair::host(bgr, depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_pyramid_frame_device(drf_t *h, const void *d_bgr, const void *d_depth, const float pose_init16[16], const drf_track_pyramid_options_t *opt,
                                   float pose16_out[16], drf_align_result_t *res) {
  return guarded_note([&] { return eng(h)->track_pyramid_frame("drf_track_pyramid_frame_device", FramePair::device(d_bgr, d_depth), pose_init16, opt, pose16_out, res); });
}
int drf_track_pyramid_stats(drf_t *h, uint64_t out[8]) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "drf_track_pyramid_stats: null argument");
    const uint64_t *s = eng(h)->track_pyramid_stats();
    for (int i = 0; i < 8; ++i) out[i] = s[i];
  });
}
int drf_track_pyramid_level_stats(drf_t *h, int level, uint64_t out[4]) {
  return guarded([&] {
    if (!out) dr::fail(DR_ERR_ARG, "drf_track_pyramid_level_stats: null argument");
    const uint64_t *s = eng(h)->track_pyramid_level_stats(level);
    for (int i = 0; i < 4; ++i) out[i] = s[i];
  });
}
int drf_set_locate_scope(drf_t *h, int scope, size_t stage_capacity_blocks) { return guarded([&] { eng(h)->set_locate_scope(scope, stage_capacity_blocks); }); }
int drf_locate_stage_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->locate_stage_stats(out); }); }
int drf_set_render_scope(drf_t *h, int scope, size_t stage_capacity_blocks) { return guarded([&] { eng(h)->set_render_scope(scope, stage_capacity_blocks); }); }
int drf_render_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->render_stats(out); }); }
int drf_set_render_bands(drf_t *h, int max_passes) { return guarded([&] { eng(h)->set_render_bands(max_passes); }); }
int drf_render_band_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->render_band_stats(out); }); }
int drf_set_mesh_scope(drf_t *h, int scope) { return guarded([&] { eng(h)->set_mesh_scope(scope); }); }
int drf_mesh_stats(drf_t *h, uint64_t out[3]) { return guarded([&] { eng(h)->mesh_stats(out); }); }
int drf_extract_mesh_update_async(drf_t *h, const float *lower, const float *upper) {
  return guarded([&] { eng(h)->extract_mesh_update_async(lower, upper); });
}
int drf_mesh_update_size(drf_t *h, size_t *nblk, size_t *ntri, int *full) { return guarded([&] { eng(h)->mesh_update_size(nblk, ntri, full); }); }
int drf_get_mesh_update_sync(drf_t *h, size_t max_blocks, size_t num_max, size_t *nblk, int32_t *coords, uint64_t *first, size_t *num,
                             float *vert, float *cols, int *full) {
  return guarded([&] { eng(h)->get_mesh_update_sync(max_blocks, num_max, nblk, coords, first, num, vert, cols, full); });
}
int drf_mesh_update_reset(drf_t *h) { return guarded([&] { eng(h)->mesh_update_reset(); }); }
int drf_mesh_update_stats(drf_t *h, uint64_t out[4]) { return guarded([&] { eng(h)->mesh_update_stats(out); }); }

}  // extern "C"
