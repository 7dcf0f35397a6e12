// Ray-casting the whole streamed map (drf_set_render_scope(DRF_RENDER_MAP); DESIGN.md §7c "Rendering the whole map"): the
// staged form of the ray-cast kernels.  Included by dr_fusion.hip in front of its ray-cast section.
//
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
// the literal pass: any staged block, inside the dense grid or not
__device__ inline int stage_find_sorted(const RenderStage &sg, I3 p) {
  const int B = 1 << 20;  // pack_key, by value
  if (p.x < -B || p.x >= B || p.y < -B || p.y >= B || p.z < -B || p.z >= B) return -1;
  const unsigned long long key = ((unsigned long long)(unsigned)(p.x + B) << 42) | ((unsigned long long)(unsigned)(p.y + B) << 21) | (unsigned long long)(unsigned)(p.z + B);
  int lo = 0, hi = sg.n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (sg.keys[mid] < key) lo = mid + 1; else hi = mid; }
  return lo < sg.n && sg.keys[lo] == key ? lo : -1;
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

template <bool FAST> __device__ inline float div_by(float a, float b, float y);  // dr_fusion.hip, ray-cast section

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

// interp_voxel2 (dr_fusion.hip) over pool and staging: the same arithmetic in the same order, the same two round trips.  Round
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

}  // namespace dr
