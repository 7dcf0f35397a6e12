// Incremental mesh ("mesh update", DESIGN.md §7c "Incremental mesh"): which blocks of a sorted key list must be meshed
// again after the scans recorded since the baseline, and the patch table that names the blocks of the result.  Included
// by dr_fusion.hip after mesh_kernels.h; launched by mesh_ops.h.  No reference counterpart.
//
// A block's voxels can differ from the baseline only if k_cull's test (cull_block_visible, the same device function)
// holds for its coordinates under the pose of a recorded scan; the update bound (a written voxel has vd < sd + trunc,
// sd <= max_sensor_depth * rho) cuts off the far end of the frustum.  A block's triangles depend on the 27 blocks around
// it, so a block is selected iff the test holds for one of those 27.  A superset is safe (the block is meshed again and
// comes back unchanged); a subset is not.
#pragma once

namespace dr {

struct MuArgs {  // (MuPose: fusion_host.h, with the ledger that records them)
  const unsigned long long *keys;  // [n] ascending packed keys of the scope
  int n;
  int nposes;                      // <= DRF_MESH_UPDATE_MAX_SCANS
  float reach2;                    // square of the update reach for a block origin in the camera frame (host, mu_reach)
  unsigned *flags;                 // [n] 1 = mesh again
  MuPose Ti[DRF_MESH_UPDATE_MAX_SCANS];
};

// One lane per block of the scope; poses are wave-uniform kernel arguments (scalar loads), 27 x nposes tests at most.
__global__ __launch_bounds__(256) void k_mu_select(const drf_options_t o, const MuArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const I3 P = unpack_key(a.keys[i]);
  bool hit = false;
  for (int s = 0; s < a.nposes && !hit; ++s) {
    Mat T;
#pragma unroll
    for (int j = 0; j < 12; ++j) T.m[j] = a.Ti[s].m[j];
    T.m[12] = T.m[13] = T.m[14] = 0.0f; T.m[15] = 1.0f;
    for (int k = 0; k < 27 && !hit; ++k) {
      I3 Q; Q.x = P.x + k / 9 - 1; Q.y = P.y + (k / 3) % 3 - 1; Q.z = P.z + k % 3 - 1;
      F3 pc;
      const bool vis = cull_block_visible(o, Q, T, pc);
      hit = vis && pc.x * pc.x + pc.y * pc.y + pc.z * pc.z < a.reach2;
    }
  }
  a.flags[i] = hit ? 1u : 0u;
}

// pos = exclusive scan of flags: the survivors keep their order
__global__ __launch_bounds__(256) void k_mu_compact(const unsigned long long *keys, const unsigned *flags, const unsigned *pos, int n,
                                                    unsigned long long *out, int *n_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) out[pos[i]] = keys[i];
  if (i == n - 1) *n_out = (int)(pos[i] + flags[i]);
}

// Patch table rows [row0, row0 + nblk] of one pass over `keys` (nblk > 0): block coordinates and first triangle row; the
// row behind the last block holds the running total, which the next chunk's first row overwrites with the same value.
__global__ __launch_bounds__(256) void k_mu_table(const unsigned long long *keys, int nblk, const unsigned *counts, const unsigned *offsets,
                                                  const unsigned long long *base, size_t row0, int *coords, unsigned long long *first) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nblk) return;
  const unsigned long long b = base ? *base : 0ull;
  if (i == nblk) { first[row0 + i] = b + offsets[nblk - 1] + counts[nblk - 1]; return; }
  const I3 P = unpack_key(keys[i]);
  int *c = coords + 3 * (row0 + i);
  c[0] = P.x; c[1] = P.y; c[2] = P.z;
  first[row0 + i] = b + offsets[i];
}

}  // namespace dr
