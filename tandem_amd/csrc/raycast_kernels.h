// The ray-cast of DrFusion (included by dr_fusion.hip after volume_kernels.h; launched by render_ops.h): k_raycast2 + k_raycast_fix (k_raycast: the
// literal form, parity build), resident and STAGED.  The STAGED form ray-casts the whole streamed map
// (drf_set_render_scope(DRF_RENDER_MAP); DESIGN.md §7c "Rendering the whole map"):
// The host selects the stored blocks a RenderAsync can read (fusion_host.h: select_render_blocks), packs their keys (ascending)
// and voxels into a staging buffer, and k_rs_build derives from the keys what the kernels look blocks up with:
//   * staged superblock flags at the two levels of FusionDev::super (32^3 and 8^3 blocks of the dense grid): 1 = some staged
//     block lies inside.  Zero answers "not staged" after ONE cached byte load whose address depends on the sample position
//     only, so it is issued with the grid loads of round trip 1 -- a miss in a region without staged blocks costs nothing more;
//   * an open-addressing table over the staged blocks of the dense grid, at least twice their number of slots, one 8-byte
//     word per slot: (grid cell + 1) << 32 | staged index, 0 = empty.  One load per probe, consulted only where the level-1
//     flag is set.
// k_rs_clear takes the flags back with the same keys once every ray-cast that read the buffer is done (the table is cleared
// with a memset before it is built).  Staged blocks outside the dense grid (|coordinate| >= 256) are served by the literal
// pass alone, through a binary search of the keys.
#pragma once
#include <type_traits>

namespace dr {

// IEEE division, or the exact three-instruction division by a per-engine constant (div_exact) where it passed its check
template <bool FAST>
__device__ inline float div_by(float a, float b, float y) { return FAST ? div_exact(a, b, y) : a / b; }

// ---- the staging of a map-scope render: types and look-ups (STAGED = true: blocks absent from the pool resolve among the host blocks staged for the render) ----
struct RenderStage {  // passed by value to the STAGED kernels
  const unsigned long long *keys;   // [n] ascending packed block coordinates
  const Voxel *vox;                 // [n * 512]
  const unsigned long long *table;  // [tmask + 1]
  const unsigned char *super[2];    // staged flags, indexed like FusionDev::super
  unsigned tmask;
  int n;
  int far;                          // 1: some staged block lies outside the dense grid
};
struct NoStage {};  // STAGED = false: nothing is passed and nothing is read
template <bool STAGED> using StageArg = std::conditional_t<STAGED, RenderStage, NoStage>;

__device__ inline bool stage_far(const NoStage &) { return false; }
__device__ inline bool stage_far(const RenderStage &s) { return s.far != 0; }
// hazard (b): a superblock may be skipped only if no staged block lies in it either
template <int L> __device__ inline bool stage_super_empty(const NoStage &, unsigned) { return true; }
template <int L> __device__ inline bool stage_super_empty(const RenderStage &s, unsigned cell) { return s.super[L][super_index<kSuperShift[L]>(cell)] == 0; }
// the kernels take the staging as a parameter pack: empty for the resident form
__device__ inline NoStage stage_arg() { return {}; }
__device__ inline const RenderStage &stage_arg(const RenderStage &s) { return s; }

// ---- depth bands (BANDED = true; drf_set_render_bands, DESIGN.md §7c "Rendering beyond the staging"): a map-scope render whose
// staged blocks exceed the staging runs in passes over consecutive slabs of camera depth, each with its own staging.  A ray
// pauses at the end of a slab and resumes in the next pass from the `cur` it stored, so `cur` takes the additions of the
// one-pass loop in the same order.  Per pixel and render stream: `cur` and where the ray stands.
enum : unsigned {
  kRayPending = 0,       // in the fast loop; cur = the next sample
  kRayFinal = 1,         // depth and colour are written
  kRayLiteral = 2,       // handed to k_raycast_fix (bail); cur = the sample that bailed, not consumed yet
  kRayLiteralColour = 3  // the loop hit, the colour sample at cur bailed: k_raycast_fix takes that sample alone
};
struct RayState { float cur; unsigned status; };  // one 8-byte load and store per pixel and pass, outside the ray loop
struct RenderBand {  // passed by value behind the RenderStage
  RayState *state;   // [height * width] of this render stream
  float z_hi;        // this pass samples cur < min(max_sensor_depth, z_hi)
  int first;         // 1: the first pass -- every ray starts at cur = 0, nothing is read from state
};
struct NoBand {};
template <bool BANDED> using BandArg = std::conditional_t<BANDED, RenderBand, NoBand>;
__device__ inline const RenderStage &stage_arg(const RenderStage &s, const RenderBand &) { return s; }
__device__ inline NoBand band_arg() { return {}; }
__device__ inline NoBand band_arg(const RenderStage &) { return {}; }
__device__ inline const RenderBand &band_arg(const RenderStage &, const RenderBand &b) { return b; }
// where the ray loop of a pass ends
__device__ inline float band_limit(float max_depth, const NoBand &) { return max_depth; }
__device__ inline float band_limit(float max_depth, const RenderBand &b) { return fminf(max_depth, b.z_hi); }

__device__ inline unsigned stage_hash(unsigned cell) {
  unsigned h = cell * 0x9E3779B1u;
  return h ^ (h >> 15);
}
// staged index of dense-grid cell `cell`, -1 if it is not staged
__device__ inline int stage_find_cell(const RenderStage &sg, unsigned cell) {
  unsigned s = stage_hash(cell) & sg.tmask;
  for (unsigned probe = 0; probe <= sg.tmask; ++probe) {
    const unsigned long long e = sg.table[s];
    if (e == 0) return -1;
    if ((unsigned)(e >> 32) == cell + 1u) return (int)(unsigned)e;
    s = (s + 1) & sg.tmask;
  }
  return -1;
}

// One lane per staged key: flags and table entry of the keys inside the dense grid.
__global__ __launch_bounds__(256) void k_rs_build(const unsigned long long *__restrict__ keys, int n, unsigned long long *table, unsigned tmask,
                                                  unsigned char *super0, unsigned char *super1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned cell;
  if (!grid_index(unpack_key(keys[i]), cell)) return;
  super0[super_index<kSuperShift[0]>(cell)] = 1;  // plain stores: every writer writes the same value
  super1[super_index<kSuperShift[1]>(cell)] = 1;
  const unsigned long long e = ((unsigned long long)(cell + 1u) << 32) | (unsigned)i;
  unsigned s = stage_hash(cell) & tmask;
  for (unsigned probe = 0; probe <= tmask; ++probe) {  // keys are distinct and the table holds >= 2 n slots: a free one exists
    if (atomicCAS(&table[s], 0ull, e) == 0ull) return;
    s = (s + 1) & tmask;
  }
}
__global__ __launch_bounds__(256) void k_rs_clear(const unsigned long long *__restrict__ keys, int n, unsigned char *super0, unsigned char *super1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned cell;
  if (!grid_index(unpack_key(keys[i]), cell)) return;
  super0[super_index<kSuperShift[0]>(cell)] = 0;
  super1[super_index<kSuperShift[1]>(cell)] = 0;
}

// Pool first, then staging: the voxels of dense-grid cell `cell`, whose grid word is g (<= 0: not in the pool) and whose
// staged level-1 flag is `flag`; nullptr if the block exists in neither.
__device__ inline const Voxel *stage_resolve(const FusionDev &d, const RenderStage &sg, unsigned cell, int g, unsigned char flag) {
  if (g > 0) return d.vox + (size_t)(g - 1) * 512;
  if (flag) {
    const int s = stage_find_cell(sg, cell);
    if (s >= 0) return sg.vox + (size_t)s * 512;
  }
  return nullptr;
}

// interp_voxel2 (below) over pool and staging: the same arithmetic in the same order, the same two round trips.  Round
// trip 1 carries the nine staged flags beside the nine grid words; a pool miss under a set flag probes the table (only near
// staged blocks); the voxel loads of staged blocks are the loads of round trip 2, from the other base address.
template <bool FAST, bool COLOUR>
__device__ inline Voxel interp_voxel2_staged(const FusionDev &d, const RenderStage &sg, F3 pos, bool far_blocks, bool &bail, int *empty_cell) {
  const float vs = d.o.voxel_size, hv = vs / 2.0f, y = d.vs_rcp;
  Voxel zero; zero.sdf = 0.f; zero.c[0] = zero.c[1] = zero.c[2] = 0; zero.weight = 0;
  const float qx = div_by<FAST>(pos.x, vs, y), qy = div_by<FAST>(pos.y, vs, y), qz = div_by<FAST>(pos.z, vs, y);
  const int g0x = f2i(qx + signf_(pos.x) * 0.5f), g0y = f2i(qy + signf_(pos.y) * 0.5f), g0z = f2i(qz + signf_(pos.z) * 0.5f);
  const float pdx = pos.x - hv, pdy = pos.y - hv, pdz = pos.z - hv;
  int gx[2], gy[2], gz[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float ax = pdx + (j ? vs : 0.0f), ay = pdy + (j ? vs : 0.0f), az = pdz + (j ? vs : 0.0f);
    gx[j] = f2i(div_by<FAST>(ax, vs, y) + signf_(ax) * 0.5f);
    gy[j] = f2i(div_by<FAST>(ay, vs, y) + signf_(ay) * 0.5f);
    gz[j] = f2i(div_by<FAST>(az, vs, y) + signf_(az) * 0.5f);
  }
  // ---- round trip 1: nine grid words and nine staged flags ----
  auto cell_of = [&](int x, int yy, int z, bool &ok) { I3 p; p.x = x; p.y = yy; p.z = z; unsigned idx = 0; ok = grid_index(p, idx); return ok ? idx : 0u; };
  bool ok0, okc[8];
  const unsigned i0 = cell_of(g0x >> 3, g0y >> 3, g0z >> 3, ok0);
  unsigned ic[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) ic[c] = cell_of(gx[c & 1] >> 3, gy[(c >> 1) & 1] >> 3, gz[(c >> 2) & 1] >> 3, okc[c]);
  const int w0 = d.grid[i0];
  const unsigned char f0 = sg.super[1][super_index<kSuperShift[1]>(i0)];
  int wc[8];
  unsigned char fc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) { wc[c] = d.grid[ic[c]]; fc[c] = sg.super[1][super_index<kSuperShift[1]>(ic[c])]; }
  if (!ok0 && far_blocks) bail = true;
  const Voxel *p0 = ok0 ? stage_resolve(d, sg, i0, w0, f0) : nullptr;
  if (empty_cell) *empty_cell = (!p0 && ok0) ? (int)i0 : -1;
  if (!p0) return zero;  // (weight 0: the corner look-ups above were speculative)
  const Voxel *pc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) pc[c] = !okc[c] ? nullptr : (ic[c] == i0 ? p0 : stage_resolve(d, sg, ic[c], wc[c], fc[c]));
  // ---- round trip 2: the centre voxel and the eight corners ----
  const Voxel8 t0 = *reinterpret_cast<const Voxel8 *>(p0 + (((g0x & 7) << 6) | ((g0y & 7) << 3) | (g0z & 7)));
  Voxel8 tc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int local = ((gx[c & 1] & 7) << 6) | ((gy[(c >> 1) & 1] & 7) << 3) | (gz[(c >> 2) & 1] & 7);
    tc[c] = *reinterpret_cast<const Voxel8 *>((pc[c] ? pc[c] : p0) + local);
  }
  const Voxel v0 = unpack_voxel(t0.lo, t0.hi);
  if (v0.weight == 0) return v0;
#pragma unroll
  for (int c = 0; c < 8; ++c) if (!okc[c] && far_blocks) bail = true;
  const float wx = qx - floorf(qx), wy = qy - floorf(qy), wz = qz - floorf(qz);
  float dist = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
  const int order[8] = {0, 1, 2, 4, 3, 6, 5, 7};  // the reference's corner order: 000 100 010 001 110 011 101 111
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = order[k];
    const float a = (c & 1) ? wx : (1.0f - wx), b = (c & 2) ? wy : (1.0f - wy), cc = (c & 4) ? wz : (1.0f - wz);
    const float wt = a * b * cc;
    Voxel cvx = unpack_voxel(tc[c].lo, tc[c].hi);
    if (!pc[c]) cvx = zero;
    const Voxel &src = cvx.weight == 0 ? v0 : cvx;
    dist += wt * src.sdf;
    if (COLOUR) {
      cx = cx + (float)src.c[0] * wt;
      cy = cy + (float)src.c[1] * wt;
      cz = cz + (float)src.c[2] * wt;
    }
  }
  Voxel v;
  v.c[0] = f2u8(cx); v.c[1] = f2u8(cy); v.c[2] = f2u8(cz);
  v.weight = v0.weight;
  v.sdf = dist;
  return v;
}

template <bool STAGED = false>
__device__ inline Voxel get_voxel(const FusionDev &d, F3 p, const StageArg<STAGED> &sg = {}) {  // tsdf_volume.cu:147-160
  Voxel z; z.sdf = 0.f; z.c[0] = z.c[1] = z.c[2] = 0; z.weight = 0;
  I3 blk; int local;
  world_to_block_local(d.o, p, blk, local);
  const int b = find_block(d, blk);
  if constexpr (STAGED) {  // the literal pass resolves through the pool, then the staging
    const int s = b < 0 ? find_sorted_key(sg.keys, sg.n, blk) : -1;  // any staged block, inside the dense grid or not
    if (b < 0 && s < 0) return z;
    return *(b >= 0 ? d.vox + (size_t)b * (kBS * kBS * kBS) + local : sg.vox + (size_t)s * (kBS * kBS * kBS) + local);
  }
  if (b < 0) return z;
  return d.vox[(size_t)b * (kBS * kBS * kBS) + local];
}

template <bool STAGED = false>
__device__ inline Voxel get_interpolated_voxel(const FusionDev &d, F3 pos, const StageArg<STAGED> &sg = {}) {  // tsdf_volume.cu:161-289
  const Voxel v0 = get_voxel<STAGED>(d, pos, sg);
  if (v0.weight == 0) return v0;
  const float vs = d.o.voxel_size, hv = vs / 2.0f;
  F3 pd; pd.x = pos.x - hv; pd.y = pos.y - hv; pd.z = pos.z - hv;
  F3 vp; vp.x = pos.x / vs; vp.y = pos.y / vs; vp.z = pos.z / vs;
  F3 w; w.x = vp.x - floorf(vp.x); w.y = vp.y - floorf(vp.y); w.z = vp.z - floorf(vp.z);
  float dist = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
  Voxel v = v0;
  // corner order of the reference: 000 100 010 001 110 011 101 111
  const int order[8] = {0, 1, 2, 4, 3, 6, 5, 7};  // bit0 = x, bit1 = y, bit2 = z
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = order[k];
    F3 q; q.x = pd.x + ((c & 1) ? vs : 0.0f); q.y = pd.y + ((c & 2) ? vs : 0.0f); q.z = pd.z + ((c & 4) ? vs : 0.0f);
    v = get_voxel<STAGED>(d, q, sg);
    const float a = (c & 1) ? w.x : (1.0f - w.x), b = (c & 2) ? w.y : (1.0f - w.y), cc = (c & 4) ? w.z : (1.0f - w.z);
    const float wt = a * b * cc;
    const Voxel &src = v.weight == 0 ? v0 : v;
    dist += wt * src.sdf;
    cx = cx + (float)src.c[0] * wt;
    cy = cy + (float)src.c[1] * wt;
    cz = cz + (float)src.c[2] * wt;
  }
  v.c[0] = f2u8(cx); v.c[1] = f2u8(cy); v.c[2] = f2u8(cz);
  v.weight = v0.weight;
  v.sdf = dist;
  return v;
}

#ifdef DR_PARITY_HOOKS  // the literal first generation as a whole-image kernel (DR_RAYCAST_V1); k_raycast_fix below is its per-pixel form
__global__ __launch_bounds__(64) void k_raycast(const FusionDev d, const Mat pose, unsigned char *__restrict__ bgr,
                                                float *__restrict__ depth_out) {
  const drf_options_t &o = d.o;
  const int size = o.height * o.width;
  // One wave = one 8x8 pixel tile (a row of 64 pixels fans out over ~6 voxel blocks at 2 m, a tile over 1-2, and
  // PMC showed 4.5 GB of L2 misses per 640x480 render with row-wise waves); tiles are dealt to the 8 XCDs in bands of
  // rows so that neighbouring tiles share an L2.  Sizes that are not multiples of 8 keep the row-wise order.
  const bool tiled = (o.width % 8 == 0) && (o.height % 8 == 0) && blockDim.x == 64;
  const int ntile = tiled ? size / 64 : 0, per_xcd = (ntile + 7) >> 3;
  for (int w0 = blockIdx.x; w0 < (tiled ? 8 * per_xcd : (size + 63) / 64); w0 += gridDim.x) {
    int i;
    if (tiled) {
      const int t = (w0 & 7) * per_xcd + (w0 >> 3);
      if (t >= ntile) continue;
      const int tw = o.width / 8, tx = t % tw, ty = t / tw;
      i = (ty * 8 + (threadIdx.x >> 3)) * o.width + tx * 8 + (threadIdx.x & 7);
    } else {
      i = w0 * 64 + threadIdx.x;
      if (i >= size) continue;
    }
    float cur = 0.f;
    while (cur < o.max_sensor_depth) {
      const Voxel v = get_interpolated_voxel(d, xform(pose, point3d(o, i, cur)));
      if (v.weight == 0) cur += o.truncation_distance; else cur += v.sdf;
      if (v.weight != 0 && v.sdf < o.voxel_size) break;
    }
    if (cur < o.max_sensor_depth) {
      const Voxel v = get_interpolated_voxel(d, xform(pose, point3d(o, i, cur)));
      bgr[3 * i] = v.c[0]; bgr[3 * i + 1] = v.c[1]; bgr[3 * i + 2] = v.c[2];
      depth_out[i] = cur;
    } else {
      bgr[3 * i] = bgr[3 * i + 1] = bgr[3 * i + 2] = 0;
      depth_out[i] = 0.0f;
    }
  }
}

#endif  // DR_PARITY_HOOKS

// ---- ray-cast, second generation: same arithmetic, a fraction of the instructions and of the dependent loads ----
// What GetInterpolatedVoxel costs when it is written out literally (above): 9 GetVoxel calls = 27 IEEE divisions by
// voxel_size + 3 for the weights, and 9 block look-ups, each a probe chain into the hash table -- per sphere-tracing step,
// ~100 steps per pixel.  Here:
//   * every division by voxel_size / fx / fy is div_exact (3 instructions, verified equal to the IEEE quotient);
//   * the 8 dual-grid corners differ per axis in ONE of two coordinates, so 6 voxel coordinates are computed, not 24
//     (each coordinate goes through exactly the expression the reference evaluates for it);
//   * blocks are looked up in the dense grid (one load), once per distinct block of the 2x2x2 corner set (almost
//     always one) and shared with the centre voxel's look-up; the 8 corner loads are then independent of each other;
//   * colour is only interpolated for the final sample of a ray.

// Block look-up of the fast ray-caster: dense grid only.  A coordinate outside the grid is absent if the table holds no
// block at all (d.n_alloc[3] counts table inserts; the usual case), otherwise the pixel bails out to the literal pass.
__device__ inline int find_block_xyz(const FusionDev &d, int x, int y, int z, bool far_blocks, bool &bail) {
  I3 p; p.x = x; p.y = y; p.z = z;
  unsigned idx;
  if (grid_index(p, idx)) return d.grid[idx] - 1;
  if (far_blocks) bail = true;
  return -1;
}

template <bool FAST, bool COLOUR>
__device__ inline Voxel interp_voxel(const FusionDev &d, F3 pos, bool far_blocks, bool &bail, int *empty_cell = nullptr) {  // == get_interpolated_voxel(d, pos), tsdf_volume.cu:161-289
  const float vs = d.o.voxel_size, hv = vs / 2.0f, y = d.vs_rcp;
  Voxel zero; zero.sdf = 0.f; zero.c[0] = zero.c[1] = zero.c[2] = 0; zero.weight = 0;
  // GetVoxel(position): WorldToGlobalVoxel (tsdf_volume.cu:109-113), then block = floor(g / 8), local = g mod 8
  const float qx = div_by<FAST>(pos.x, vs, y), qy = div_by<FAST>(pos.y, vs, y), qz = div_by<FAST>(pos.z, vs, y);
  const int g0x = f2i(qx + signf_(pos.x) * 0.5f), g0y = f2i(qy + signf_(pos.y) * 0.5f), g0z = f2i(qz + signf_(pos.z) * 0.5f);
  const int c0x = g0x >> 3, c0y = g0y >> 3, c0z = g0z >> 3;
  const int b0 = find_block_xyz(d, c0x, c0y, c0z, far_blocks, bail);
  if (empty_cell) {  // dense-grid cell of the centre voxel's block when that block does not exist (else -1)
    I3 c; c.x = c0x; c.y = c0y; c.z = c0z;
    unsigned ci;
    *empty_cell = (b0 < 0 && grid_index(c, ci)) ? (int)ci : -1;
  }
  Voxel v0 = zero;
  if (b0 >= 0) v0 = load_voxel(d.vox + (size_t)b0 * 512 + (((g0x & 7) << 6) | ((g0y & 7) << 3) | (g0z & 7)));
  if (v0.weight == 0) return v0;
  const float pdx = pos.x - hv, pdy = pos.y - hv, pdz = pos.z - hv;
  const float wx = qx - floorf(qx), wy = qy - floorf(qy), wz = qz - floorf(qz);  // voxel_position = position / voxel_size is q
  // per-axis corner coordinates: pos_dual + 0.0f and pos_dual + voxel_size
  int gx[2], gy[2], gz[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float ax = pdx + (j ? vs : 0.0f), ay = pdy + (j ? vs : 0.0f), az = pdz + (j ? vs : 0.0f);
    gx[j] = f2i(div_by<FAST>(ax, vs, y) + signf_(ax) * 0.5f);
    gy[j] = f2i(div_by<FAST>(ay, vs, y) + signf_(ay) * 0.5f);
    gz[j] = f2i(div_by<FAST>(az, vs, y) + signf_(az) * 0.5f);
  }
  const int bx0 = gx[0] >> 3, bx1 = gx[1] >> 3, by0 = gy[0] >> 3, by1 = gy[1] >> 3, bz0 = gz[0] >> 3, bz1 = gz[1] >> 3;
  auto look = [&](int x, int yy, int z) { return (x == c0x && yy == c0y && z == c0z) ? b0 : find_block_xyz(d, x, yy, z, far_blocks, bail); };
  int P[8];  // pool block of corner c (bit0 = x, bit1 = y, bit2 = z)
  P[0] = look(bx0, by0, bz0);
  P[1] = bx1 == bx0 ? P[0] : look(bx1, by0, bz0);
  P[2] = by1 == by0 ? P[0] : look(bx0, by1, bz0);
  P[3] = bx1 == bx0 ? P[2] : (by1 == by0 ? P[1] : look(bx1, by1, bz0));
  P[4] = bz1 == bz0 ? P[0] : look(bx0, by0, bz1);
  P[5] = bz1 == bz0 ? P[1] : (bx1 == bx0 ? P[4] : look(bx1, by0, bz1));
  P[6] = bz1 == bz0 ? P[2] : (by1 == by0 ? P[4] : look(bx0, by1, bz1));
  P[7] = bz1 == bz0 ? P[3] : (bx1 == bx0 ? P[6] : (by1 == by0 ? P[5] : look(bx1, by1, bz1)));
  Voxel cv[8];
  // The two z-corners of an (x, y) pair are neighbours in memory (z is the fastest voxel index) whenever they lie in the
  // same block: one 16-byte load then brings both -- 4 gathers per sample instead of 8 for 7 lanes in 8.
  if (bz1 == bz0 && gz[1] == gz[0] + 1) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int local = ((gx[c & 1] & 7) << 6) | ((gy[(c >> 1) & 1] & 7) << 3) | (gz[0] & 7);
      cv[c] = zero; cv[c | 4] = zero;
      if (P[c] >= 0) {
        const Voxel16 t = *reinterpret_cast<const Voxel16 *>(d.vox + (size_t)P[c] * 512 + local);
        cv[c] = unpack_voxel(t.a, t.b); cv[c | 4] = unpack_voxel(t.c, t.d);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int local = ((gx[c & 1] & 7) << 6) | ((gy[(c >> 1) & 1] & 7) << 3) | (gz[(c >> 2) & 1] & 7);
      cv[c] = zero;
      if (P[c] >= 0) cv[c] = load_voxel(d.vox + (size_t)P[c] * 512 + local);
    }
  }
  float dist = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
  const int order[8] = {0, 1, 2, 4, 3, 6, 5, 7};  // the reference's corner order: 000 100 010 001 110 011 101 111
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = order[k];
    const float a = (c & 1) ? wx : (1.0f - wx), b = (c & 2) ? wy : (1.0f - wy), cc = (c & 4) ? wz : (1.0f - wz);
    const float wt = a * b * cc;
    const Voxel &src = cv[c].weight == 0 ? v0 : cv[c];
    dist += wt * src.sdf;
    if (COLOUR) {
      cx = cx + (float)src.c[0] * wt;
      cy = cy + (float)src.c[1] * wt;
      cz = cz + (float)src.c[2] * wt;
    }
  }
  Voxel v;
  v.c[0] = f2u8(cx); v.c[1] = f2u8(cy); v.c[2] = f2u8(cz);
  v.weight = v0.weight;
  v.sdf = dist;
  return v;
}
// interp_voxel in TWO memory round trips.  The statistics of the bench loop (DR_RAYCAST_STATS, r3): a ray takes ~62
// samples, 52 of them inside allocated, carved space (the reference allocates every block between the camera and the
// surface), and all lanes of a wave need about the same number -- the kernel is a chain of dependent gathers, each as slow
// as the slowest of a wave's 64 lanes (some lane always misses L2).  interp_voxel has four dependent stages per sample
// (centre block -> centre voxel -> neighbour blocks -> corner voxels); here every block look-up (centre + the 2x2x2 corner
// blocks, computed from the position alone) is issued at once, then every voxel load (centre + 8 corners, unconditional
// 8-byte loads from a clamped address, masked afterwards) at once.  Same values, same arithmetic, same result.
// STAGED = true (map-scope renders): interp_voxel2_staged above -- the same two round trips over pool and staging.
template <bool FAST, bool COLOUR, bool STAGED = false>
__device__ inline Voxel interp_voxel2(const FusionDev &d, F3 pos, bool far_blocks, bool &bail, int *empty_cell = nullptr, const StageArg<STAGED> &sg = {}) {
  if constexpr (STAGED) return interp_voxel2_staged<FAST, COLOUR>(d, sg, pos, far_blocks, bail, empty_cell);
  const float vs = d.o.voxel_size, hv = vs / 2.0f, y = d.vs_rcp;
  Voxel zero; zero.sdf = 0.f; zero.c[0] = zero.c[1] = zero.c[2] = 0; zero.weight = 0;
  const float qx = div_by<FAST>(pos.x, vs, y), qy = div_by<FAST>(pos.y, vs, y), qz = div_by<FAST>(pos.z, vs, y);
  const int g0x = f2i(qx + signf_(pos.x) * 0.5f), g0y = f2i(qy + signf_(pos.y) * 0.5f), g0z = f2i(qz + signf_(pos.z) * 0.5f);
  const float pdx = pos.x - hv, pdy = pos.y - hv, pdz = pos.z - hv;
  int gx[2], gy[2], gz[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float ax = pdx + (j ? vs : 0.0f), ay = pdy + (j ? vs : 0.0f), az = pdz + (j ? vs : 0.0f);
    gx[j] = f2i(div_by<FAST>(ax, vs, y) + signf_(ax) * 0.5f);
    gy[j] = f2i(div_by<FAST>(ay, vs, y) + signf_(ay) * 0.5f);
    gz[j] = f2i(div_by<FAST>(az, vs, y) + signf_(az) * 0.5f);
  }
  // ---- round trip 1: nine block look-ups (identical addresses coalesce in the load unit) ----
  auto cell_of = [&](int x, int yy, int z, bool &ok) { I3 p; p.x = x; p.y = yy; p.z = z; unsigned idx = 0; ok = grid_index(p, idx); return ok ? idx : 0u; };
  bool ok0, okc[8];
  const unsigned i0 = cell_of(g0x >> 3, g0y >> 3, g0z >> 3, ok0);
  unsigned ic[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) ic[c] = cell_of(gx[c & 1] >> 3, gy[(c >> 1) & 1] >> 3, gz[(c >> 2) & 1] >> 3, okc[c]);
  int b0 = d.grid[i0];
  int P[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) P[c] = d.grid[ic[c]];
  b0 = ok0 ? b0 - 1 : -1;
  if (!ok0 && far_blocks) bail = true;
  if (empty_cell) *empty_cell = (b0 < 0 && ok0) ? (int)i0 : -1;
  if (b0 < 0) return zero;  // (weight 0: the corner look-ups above were speculative)
#pragma unroll
  for (int c = 0; c < 8; ++c) P[c] = okc[c] ? P[c] - 1 : -1;
  // ---- round trip 2: the centre voxel and the eight corners ----
  const Voxel8 t0 = *reinterpret_cast<const Voxel8 *>(d.vox + (size_t)b0 * 512 + (((g0x & 7) << 6) | ((g0y & 7) << 3) | (g0z & 7)));
  Voxel8 tc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int local = ((gx[c & 1] & 7) << 6) | ((gy[(c >> 1) & 1] & 7) << 3) | (gz[(c >> 2) & 1] & 7);
    tc[c] = *reinterpret_cast<const Voxel8 *>(d.vox + (size_t)(P[c] >= 0 ? P[c] : b0) * 512 + local);
  }
  const Voxel v0 = unpack_voxel(t0.lo, t0.hi);
  if (v0.weight == 0) return v0;
  // the far-block bail of the literal order: a corner outside the dense grid only matters once the centre voxel has weight
#pragma unroll
  for (int c = 0; c < 8; ++c) if (!okc[c] && far_blocks) bail = true;
  const float wx = qx - floorf(qx), wy = qy - floorf(qy), wz = qz - floorf(qz);
  float dist = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
  const int order[8] = {0, 1, 2, 4, 3, 6, 5, 7};  // the reference's corner order: 000 100 010 001 110 011 101 111
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = order[k];
    const float a = (c & 1) ? wx : (1.0f - wx), b = (c & 2) ? wy : (1.0f - wy), cc = (c & 4) ? wz : (1.0f - wz);
    const float wt = a * b * cc;
    Voxel cvx = unpack_voxel(tc[c].lo, tc[c].hi);
    if (P[c] < 0) cvx = zero;
    const Voxel &src = cvx.weight == 0 ? v0 : cvx;
    dist += wt * src.sdf;
    if (COLOUR) {
      cx = cx + (float)src.c[0] * wt;
      cy = cy + (float)src.c[1] * wt;
      cz = cz + (float)src.c[2] * wt;
    }
  }
  Voxel v;
  v.c[0] = f2u8(cx); v.c[1] = f2u8(cy); v.c[2] = f2u8(cz);
  v.weight = v0.weight;
  v.sdf = dist;
  return v;
}
// Round 4 measured two more samplers against this one on the bench map (profiles/r04_experiments.txt, 2) and removed both: PAIRED
// gathers (one 8-byte load for the two grid cells and one 16-byte load for the two voxels of a z-corner pair: 4 + 4 gathers, half of
// them not naturally aligned) and the centre voxel SELECTED from the eight corners instead of fetched (8 + 8 gathers, 14 more selects):
// 0.43 ms per render against 0.34 for this sampler.  The kernel is bound by the L1's tag path (PMC, r3: 131.6 M line accesses per
// render, 20 per gather instruction -- the 64 rays of a tile sit in 64 different z-columns of a block), and neither variant lowers the
// number of distinct lines a sample touches; both add instructions.
// Pixels are flagged for the literal pass (k_raycast_fix) with depth -1 when a sample leaves the range div_exact was
// verified on, or needs a block outside the dense grid while the table is not empty.  Neither happens in a room-sized map.
// How many further samples q + j * trunc * dir (j = 1..k) stay inside the superblock of `cell`, shrunk by one voxel on
// every side.  Approximate float arithmetic on purpose: it only has to be conservative (the margin is 5 mm against
// errors of ~1e-5 m), the samples' own positions are never used.
template <int SH>
__device__ inline int skip_steps(unsigned cell, F3 q, F3 dirw, F3 inv_dir, float vs, float inv_trunc) {
  constexpr int H = 1 << (kGridBits - 1);
  constexpr unsigned M = (1u << kGridBits) - 1, SM = ~((1u << SH) - 1u);
  constexpr float hi_off = (float)(kBS << SH) - 1.5f;  // the superblock's n = 8 << SH voxels cover [(g - 0.5) vs, (g + n - 0.5) vs)
  const float gx = (float)((int)(((cell >> (2 * kGridBits)) & SM) - H) * kBS);
  const float gy = (float)((int)((((cell >> kGridBits) & M) & SM) - H) * kBS);
  const float gz = (float)((int)(((cell & M) & SM) - H) * kBS);
  float t = 1e30f;
  if (dirw.x != 0.f) t = fminf(t, ((gx + (dirw.x > 0.f ? hi_off : 0.5f)) * vs - q.x) * inv_dir.x);
  if (dirw.y != 0.f) t = fminf(t, ((gy + (dirw.y > 0.f ? hi_off : 0.5f)) * vs - q.y) * inv_dir.y);
  if (dirw.z != 0.f) t = fminf(t, ((gz + (dirw.z > 0.f ? hi_off : 0.5f)) * vs - q.z) * inv_dir.z);
  return (int)fminf(t * inv_trunc - 0.5f, 256.f);
}
// STATS (DR_RAYCAST_STATS=1, a measuring build of the same loop): per-launch totals of the ray loop in st[] --
// [0] lane iterations, [1] longest ray, [2] sum over waves of their longest ray (what the wave pays), [3] samples whose
// centre block does not exist, [4] skip events, [5] skipped steps, [6] samples with weight != 0, [7] waves, [8..] histogram
// of the waves' longest rays in buckets of 16 iterations.
// SAMPLER: 1 = interp_voxel2 (9 + 9 gathers in two round trips; the product's), 0 = interp_voxel (round 2's four stages; parity build)
// STAGED: the map-scope form -- look-ups fall through to the staged host blocks, a superblock is skipped
// only if neither the pool nor the staging holds a block in it, and a staged block outside the dense grid sends the pixel to the
// literal pass like a table block does.  The product's sampler only.
// The staging is a trailing parameter PACK -- one RenderStage when STAGED, nothing otherwise -- so that the resident instances keep
// their kernel arguments, and with them their instructions, exactly.
// BANDED: one depth band of a staged render (above) -- a RenderBand follows the RenderStage in the pack.  The loop and the
// empty-space skip stop at the band's far side: the staged superblock flags describe this pass's blocks only, so a skip is
// proven only below z_hi (stopping early and resuming by sampling gives the same `cur` sequence).  A ray that hits takes its
// colour sample in the same pass and is final; a ray that neither hit nor left the depth range stores `cur` and stays pending;
// a ray that bails becomes literal at the sample that bailed and is k_raycast_fix's from then on.
template <bool FAST, bool STATS = false, int SAMPLER = 1, bool STAGED = false, bool BANDED = false, class... SG>
__global__ __launch_bounds__(64) void k_raycast2(const FusionDev d, const Mat pose, unsigned char *__restrict__ bgr,
                                                 float *__restrict__ depth_out, int *__restrict__ n_flagged, unsigned long long *st,
                                                 const SG... stage) {
  static_assert(!STAGED || (SAMPLER == 1 && !STATS), "the staged ray-cast exists for the product's sampler");
  static_assert(!BANDED || STAGED, "bands exist for the staged form");
  static_assert(sizeof...(SG) == (STAGED ? 1 : 0) + (BANDED ? 1 : 0), "one RenderStage for the staged form, a RenderBand behind it for the banded one");
  const StageArg<STAGED> &sg = stage_arg(stage...);
  const BandArg<BANDED> &band = band_arg(stage...);
  const drf_options_t &o = d.o;
  const int size = o.height * o.width;
  const float z_end = band_limit(o.max_sensor_depth, band);
  const bool far_blocks = d.n_alloc[3] != 0 || stage_far(sg);
  // one wave = one 8x8 pixel tile, tiles dealt to the 8 XCDs in bands of rows (see k_raycast)
  const bool tiled = (o.width % 8 == 0) && (o.height % 8 == 0) && blockDim.x == 64;
  const int ntile = tiled ? size / 64 : 0, per_xcd = (ntile + 7) >> 3;
  for (int w0 = blockIdx.x; w0 < (tiled ? 8 * per_xcd : (size + 63) / 64); w0 += gridDim.x) {
    int i;
    if (tiled) {
      const int t = (w0 & 7) * per_xcd + (w0 >> 3);
      if (t >= ntile) continue;
      const int tw = o.width / 8, tx = t % tw, ty = t / tw;
      i = (ty * 8 + (threadIdx.x >> 3)) * o.width + tx * 8 + (threadIdx.x & 7);
    } else {
      i = w0 * 64 + threadIdx.x;
      if (i >= size) continue;
    }
    // GetPoint3d(i, cur, sensor) (utils.h:93-101): x = (u - cx) * z / fx, the pixel part is constant along the ray
    const int pv = i / o.width, pu = i - o.width * pv;
    const float ucx = (float)pu - o.cx, vcy = (float)pv - o.cy;
    bool bail = false;
    auto sample_pos = [&](float cur) {
      F3 p;
      p.z = cur;
      const float tx = ucx * cur, ty = vcy * cur;
      p.x = div_by<FAST>(tx, o.fx, d.fx_rcp);
      p.y = div_by<FAST>(ty, o.fy, d.fy_rcp);
      const F3 q = xform(pose, p);
      if (FAST && !(in_fast_range(q.x) && in_fast_range(q.y) && in_fast_range(q.z) && in_fast_range(tx) && in_fast_range(ty))) bail = true;
      return q;
    };
    // Empty-space skip.  A sample whose centre voxel lies in a block that does not exist returns weight 0 and the ray
    // advances by the truncation distance (2 cm at TANDEM's settings: ~150 look-ups across a room).  d.super[] marks the
    // superblocks (32^3 and 8^3 blocks) of the dense grid that hold any block at all; while the ray stays inside an empty one
    // (shrunk by a voxel on every side: three orders of magnitude above the float error of the approximate ray used
    // here) every sample is known to return weight 0, so `cur` takes the same sequence of float additions -- the
    // result is bit-identical -- without transforming, dividing or loading anything.  DR_RAYCAST_NO_SKIP=1 turns it off.
    F3 dirw, inv_dir;
    {
      const float lx = ucx / o.fx, ly = vcy / o.fy;
      dirw.x = pose.m[0] * lx + pose.m[1] * ly + pose.m[2];
      dirw.y = pose.m[4] * lx + pose.m[5] * ly + pose.m[6];
      dirw.z = pose.m[8] * lx + pose.m[9] * ly + pose.m[10];
      inv_dir.x = 1.0f / dirw.x; inv_dir.y = 1.0f / dirw.y; inv_dir.z = 1.0f / dirw.z;
    }
    const float inv_trunc = 1.0f / o.truncation_distance, vs = o.voxel_size;
    float cur = 0.f;
    bool hit = false;  // (BANDED: the loop ended at a surface, not at the band's far side)
    if constexpr (BANDED) {
      if (!band.first) {
        const RayState s = band.state[i];
        if (s.status != kRayPending) continue;  // final, or the literal pass's
        cur = s.cur;
      }
    }
    unsigned n_it = 0, n_miss = 0, n_skip = 0, n_skipped = 0, n_full = 0;
    while (cur < z_end) {
      const F3 q = sample_pos(cur);
      int cell = -1;
      const Voxel v = SAMPLER == 1 ? interp_voxel2<FAST, false, STAGED>(d, q, far_blocks, bail, (STAGED || d.super[0]) ? &cell : nullptr, sg)
                                   : interp_voxel<FAST, false>(d, q, far_blocks, bail, d.super[0] ? &cell : nullptr);
      if (STAGED && !d.super[0]) cell = -1;  // (the staged sampler always reports the cell: its pointer stays a plain local)
      if (bail) break;
      if (STATS) { ++n_it; n_miss += cell >= 0; n_full += v.weight != 0; }
      if (v.weight == 0) {
        cur += o.truncation_distance;
        if (cell >= 0) {
          int k = 0;
          if (d.super[0][super_index<kSuperShift[0]>((unsigned)cell)] == 0 && stage_super_empty<0>(sg, (unsigned)cell)) k = skip_steps<kSuperShift[0]>((unsigned)cell, q, dirw, inv_dir, vs, inv_trunc);
          else if (d.super[1][super_index<kSuperShift[1]>((unsigned)cell)] == 0 && stage_super_empty<1>(sg, (unsigned)cell)) k = skip_steps<kSuperShift[1]>((unsigned)cell, q, dirw, inv_dir, vs, inv_trunc);
          if (STATS && k > 0) { ++n_skip; n_skipped += k; }
          for (; k > 0 && cur < z_end; --k) cur += o.truncation_distance;
        }
      } else cur += v.sdf;
      if (v.weight != 0 && v.sdf < o.voxel_size) { hit = true; break; }
    }
    if (STATS) {
      unsigned mx = n_it, sum = n_it, sm = n_miss, ss = n_skip, sk = n_skipped, sf = n_full;
      for (int off = 32; off; off >>= 1) {
        mx = max(mx, (unsigned)__shfl_xor((int)mx, off)); sum += __shfl_xor((int)sum, off); sm += __shfl_xor((int)sm, off);
        ss += __shfl_xor((int)ss, off); sk += __shfl_xor((int)sk, off); sf += __shfl_xor((int)sf, off);
      }
      if (threadIdx.x == 0) {
        atomicAdd(&st[0], (unsigned long long)sum); atomicMax(&st[1], (unsigned long long)mx); atomicAdd(&st[2], (unsigned long long)mx);
        atomicAdd(&st[3], (unsigned long long)sm); atomicAdd(&st[4], (unsigned long long)ss); atomicAdd(&st[5], (unsigned long long)sk);
        atomicAdd(&st[6], (unsigned long long)sf); atomicAdd(&st[7], 1ull); atomicAdd(&st[8 + min(mx / 16u, 23u)], 1ull);
      }
    }
    if constexpr (BANDED) {
      RayState s;
      s.cur = cur;
      s.status = kRayLiteral;
      if (!bail) {
        s.status = kRayPending;
        if (hit && cur < o.max_sensor_depth) {
          const F3 qf = sample_pos(cur);
          const Voxel v = interp_voxel2<FAST, true, STAGED>(d, qf, far_blocks, bail, nullptr, sg);
          if (bail) s.status = kRayLiteralColour;
          else {
            bgr[3 * i] = v.c[0]; bgr[3 * i + 1] = v.c[1]; bgr[3 * i + 2] = v.c[2];
            depth_out[i] = cur;
            s.status = kRayFinal;
          }
        } else if (hit || !(cur < o.max_sensor_depth)) {
          bgr[3 * i] = bgr[3 * i + 1] = bgr[3 * i + 2] = 0;
          depth_out[i] = 0.0f;
          s.status = kRayFinal;
        }
      }
      band.state[i] = s;
      if (bail) atomicAdd(n_flagged, 1);
      continue;
    }
    if (!bail && cur < o.max_sensor_depth) {
      const F3 qf = sample_pos(cur);
      const Voxel v = SAMPLER == 1 ? interp_voxel2<FAST, true, STAGED>(d, qf, far_blocks, bail, nullptr, sg) : interp_voxel<FAST, true>(d, qf, far_blocks, bail);
      bgr[3 * i] = v.c[0]; bgr[3 * i + 1] = v.c[1]; bgr[3 * i + 2] = v.c[2];
      depth_out[i] = cur;
    } else {
      bgr[3 * i] = bgr[3 * i + 1] = bgr[3 * i + 2] = 0;
      depth_out[i] = 0.0f;
    }
    if (bail) { depth_out[i] = -1.0f; atomicAdd(n_flagged, 1); }
  }
}
// The literal ray-caster for the pixels k_raycast2 flagged; exits at once when there are none.
// BANDED: the literal rays of this and of earlier passes (n_flagged counts them over the whole render) go on from their stored
// `cur` to the band's far side; the fast sampler and this one agree bit for bit on every sample that does not bail.
template <bool STAGED = false, bool BANDED = false, class... SG>
__global__ __launch_bounds__(64) void k_raycast_fix(const FusionDev d, const Mat pose, unsigned char *__restrict__ bgr,
                                                    float *__restrict__ depth_out, int *__restrict__ n_flagged, const SG... stage) {
  static_assert(!BANDED || STAGED, "bands exist for the staged form");
  static_assert(sizeof...(SG) == (STAGED ? 1 : 0) + (BANDED ? 1 : 0), "one RenderStage for the staged form, a RenderBand behind it for the banded one");
  const StageArg<STAGED> &sg = stage_arg(stage...);
  const BandArg<BANDED> &band = band_arg(stage...);
  if (*n_flagged == 0) return;
  const drf_options_t &o = d.o;
  const int size = o.height * o.width;
  const float z_end = band_limit(o.max_sensor_depth, band);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < size; i += gridDim.x * blockDim.x) {
    float cur = 0.f;
    bool hit = false;
    if constexpr (BANDED) {
      const RayState s = band.state[i];  // (written by this pass's k_raycast2 or an earlier pass: never stale)
      if (s.status != kRayLiteral && s.status != kRayLiteralColour) continue;
      cur = s.cur;
      hit = s.status == kRayLiteralColour;
    } else {
      if (!(depth_out[i] == -1.0f)) continue;
    }
    while (!hit && cur < z_end) {
      const Voxel v = get_interpolated_voxel<STAGED>(d, xform(pose, point3d(o, i, cur)), sg);
      if (v.weight == 0) cur += o.truncation_distance; else cur += v.sdf;
      if (v.weight != 0 && v.sdf < o.voxel_size) { hit = true; break; }
    }
    if constexpr (BANDED) {
      if (!hit && cur < o.max_sensor_depth) {  // the band's far side: literal in the next pass as well
        RayState s;
        s.cur = cur; s.status = kRayLiteral;
        band.state[i] = s;
        continue;
      }
      RayState s;
      s.cur = cur; s.status = kRayFinal;
      band.state[i] = s;
    }
    if (cur < o.max_sensor_depth) {
      const Voxel v = get_interpolated_voxel<STAGED>(d, xform(pose, point3d(o, i, cur)), sg);
      bgr[3 * i] = v.c[0]; bgr[3 * i + 1] = v.c[1]; bgr[3 * i + 2] = v.c[2];
      depth_out[i] = cur;
    } else {
      bgr[3 * i] = bgr[3 * i + 1] = bgr[3 * i + 2] = 0;
      depth_out[i] = 0.0f;
    }
  }
}

}  // namespace dr
