// locate_kernels.h -- drf_locate_system / drf_locate_frame on the device: one evaluation of the localisation's Gauss-Newton system
// (the rule: pose_host.h locate_pixel / align_point; DESIGN.md §7c "Locating a depth frame in the map").  Included by
// dr_fusion.hip inside namespace dr, behind align_kernels.h, whose k_align_fold folds the groups; launched by pose_ops.h.  k_map_locate reads the pool;
// k_map_locate_staged reads the pool and the stored blocks staged for the call (drf_set_locate_scope(DRF_LOCATE_MAP)), through
// the RenderStage of raycast_kernels.h.

// The engine's live map as align_point's fetch: the voxel at lattice point (x, y, z) through find_block -- the dense grid (one
// load) or the far-block table -- an absent block, one only requested, or one outside the key range reading as weight 0.  The
// eight corners of a sample almost always share one block: the first corner's block is resolved (or taken from the sample before,
// neighbouring pixels mostly land in the same block) and kept, and a later corner looks a block up only when it crosses a face.
// Voxels are read as the 8-byte loads the engine uses everywhere (Voxel8).
struct LocateFetch {
  const FusionDev &d;
  int bx = 0, by = 0, bz = 0, pool = -1;  // the block kept
  bool have = false;
  int corner = 0;  // corners fetched for the current sample
  __device__ LocateFetch(const FusionDev &dev) : d(dev) {}
  __device__ void operator()(int x, int y, int z, uint32_t v[2]) {
    const int cx = x >> 3, cy = y >> 3, cz = z >> 3;  // arithmetic shift = floor division by 8
    int p;
    if (have && cx == bx && cy == by && cz == bz) p = pool;
    else {
      I3 c; c.x = cx; c.y = cy; c.z = cz;
      p = find_block(d, c);
      if (corner == 0) { bx = cx; by = cy; bz = cz; pool = p; have = true; }
    }
    ++corner;
    v[0] = 0; v[1] = 0;
    if (p < 0) return;
    const Voxel8 t = *reinterpret_cast<const Voxel8 *>(d.vox + (size_t)p * 512 + (size_t)(((x & 7) << 6) | ((y & 7) << 3) | (z & 7)));
    v[0] = t.lo; v[1] = t.hi;
  }
};

// The same fetch over pool and staging (drf_set_locate_scope(DRF_LOCATE_MAP); DESIGN.md §7c "Locating in the whole map"): the pool
// first, as find_block resolves it; on a miss inside the dense grid the staged level-1 flag (one cached byte) and, only where it is
// set, the staging's table; on a miss outside the grid a binary search of the ascending keys, only if some staged block lies there.
// What is kept from corner to corner and from sample to sample is the block's base pointer -- pool or staging, or null -- so a
// staged block costs its look-up once, as a pool block does.  The voxel load is the same Voxel8 load from the other base address.
struct LocateFetchStaged {
  const FusionDev &d;
  const RenderStage &sg;
  int bx = 0, by = 0, bz = 0;
  const Voxel *base = nullptr;  // the block kept (null: it exists in neither)
  bool have = false;
  int corner = 0;
  __device__ LocateFetchStaged(const FusionDev &dev, const RenderStage &stage) : d(dev), sg(stage) {}
  __device__ const Voxel *resolve(I3 c) const {
    unsigned cell;
    if (grid_index(c, cell)) {  // find_block's grid word and the staged flag in one round trip: both addresses depend on the cell only
      const int g = d.grid[cell];
      const unsigned char flag = sg.super[1][super_index<kSuperShift[1]>(cell)];
      return stage_resolve(d, sg, cell, g, flag);
    }
    const int p = find_block_table(d, c);  // (find_block outside the dense grid)
    if (p >= 0) return d.vox + (size_t)p * 512;
    const int s = sg.far ? find_sorted_key(sg.keys, sg.n, c) : -1;
    return s >= 0 ? sg.vox + (size_t)s * 512 : nullptr;
  }
  __device__ void operator()(int x, int y, int z, uint32_t v[2]) {
    const int cx = x >> 3, cy = y >> 3, cz = z >> 3;
    const Voxel *p;
    if (have && cx == bx && cy == by && cz == bz) p = base;
    else {
      I3 c; c.x = cx; c.y = cy; c.z = cz;
      p = resolve(c);
      if (corner == 0) { bx = cx; by = cy; bz = cz; base = p; have = true; }
    }
    ++corner;
    v[0] = 0; v[1] = 0;
    if (!p) return;
    const Voxel8 t = *reinterpret_cast<const Voxel8 *>(p + (size_t)(((x & 7) << 6) | ((y & 7) << 3) | (z & 7)));
    v[0] = t.lo; v[1] = t.hi;
  }
};

// One wave per group i in [0, groups) of 512 grid positions (no grid stride; the four waves of a workgroup share nothing), lane l on
// positions 512 i + l + 64 k, k = 0..7: consecutive lanes on consecutive positions, which for step = 1 are consecutive pixels of a
// row -- the depth loads coalesce.  A group without a sample (the sky, a masked border) does no look-up and writes 28 zeros, which
// is what the sums of nothing are.  The 28 sums live in registers (align_point's loops are unrolled; the loop over k is not, so
// that the register count stays where k_map_align's is); the wave's butterfly x = x + shfl_xor(x, off), off = 32..1, leaves the
// group's sums in every lane and lane 0 writes them to partial[i].  counts += {samples, valid, unobserved, outside}: integers, one
// atomic each per wave.  The map is only read.
__global__ __launch_bounds__(256) void k_map_locate(const FusionDev d, const float *__restrict__ depth, const LocateGrid lg, const AlignEval e, int groups,
                                                    int total, double *__restrict__ partial, unsigned long long *__restrict__ counts) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= groups) return;
  bool mine = false;  // one of this lane's 8 positions is a sample
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int n = 512 * i + lane + 64 * k;
    if (n < total) mine = mine || locate_is_sample(lg, depth[locate_offset(lg, n)]);
  }
  if (!__any(mine)) {  // wave-uniform
    if (lane < 28) partial[(size_t)i * 28 + lane] = 0.0;
    return;
  }
  double acc[28];
#pragma unroll
  for (int c = 0; c < 28; ++c) acc[c] = 0.0;
  unsigned ns = 0, nv = 0, nu = 0;
  LocateFetch fetch(d);
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const int n = 512 * i + lane + 64 * k;
    double g[3];
    if (n >= total || !locate_pixel(lg, e.vs, n, depth, g)) continue;
    ++ns;
    fetch.corner = 0;
    const int r = align_point<true>(e, g[0], g[1], g[2], 0.0f, fetch, acc);
    nv += r == 1 ? 1u : 0u;
    nu += r == 0 ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 28; ++c) acc[c] = acc[c] + __shfl_xor(acc[c], off);
    ns += __shfl_xor(ns, off); nv += __shfl_xor(nv, off); nu += __shfl_xor(nu, off);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 28; ++c) partial[(size_t)i * 28 + c] = acc[c];
    atomicAdd(&counts[0], (unsigned long long)ns);
    if (nv) atomicAdd(&counts[1], (unsigned long long)nv);
    if (nu) atomicAdd(&counts[2], (unsigned long long)nu);
    if (ns - nv - nu) atomicAdd(&counts[3], (unsigned long long)(ns - nv - nu));
  }
}
// The map-scope form, a second kernel: the same wave over LocateFetchStaged, the staging behind the resident kernel's arguments.
// The text is repeated, not shared: the resident kernel routed through a common inlined body compiles to other instructions (123
// VGPRs against 121), and it is held to the ones it had.  What differs is the fetch and nothing else.
__global__ __launch_bounds__(256) void k_map_locate_staged(const FusionDev d, const float *__restrict__ depth, const LocateGrid lg, const AlignEval e, int groups,
                                                           int total, double *__restrict__ partial, unsigned long long *__restrict__ counts, const RenderStage sg) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= groups) return;
  bool mine = false;  // one of this lane's 8 positions is a sample
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int n = 512 * i + lane + 64 * k;
    if (n < total) mine = mine || locate_is_sample(lg, depth[locate_offset(lg, n)]);
  }
  if (!__any(mine)) {  // wave-uniform
    if (lane < 28) partial[(size_t)i * 28 + lane] = 0.0;
    return;
  }
  double acc[28];
#pragma unroll
  for (int c = 0; c < 28; ++c) acc[c] = 0.0;
  unsigned ns = 0, nv = 0, nu = 0;
  LocateFetchStaged fetch(d, sg);
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const int n = 512 * i + lane + 64 * k;
    double g[3];
    if (n >= total || !locate_pixel(lg, e.vs, n, depth, g)) continue;
    ++ns;
    fetch.corner = 0;
    const int r = align_point<true>(e, g[0], g[1], g[2], 0.0f, fetch, acc);
    nv += r == 1 ? 1u : 0u;
    nu += r == 0 ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 28; ++c) acc[c] = acc[c] + __shfl_xor(acc[c], off);
    ns += __shfl_xor(ns, off); nv += __shfl_xor(nv, off); nu += __shfl_xor(nu, off);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 28; ++c) partial[(size_t)i * 28 + c] = acc[c];
    atomicAdd(&counts[0], (unsigned long long)ns);
    if (nv) atomicAdd(&counts[1], (unsigned long long)nv);
    if (nu) atomicAdd(&counts[2], (unsigned long long)nu);
    if (ns - nv - nu) atomicAdd(&counts[3], (unsigned long long)(ns - nv - nu));
  }
}
