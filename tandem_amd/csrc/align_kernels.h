// align_kernels.h -- drf_align_system / drf_align_map on the device: one evaluation of the registration's Gauss-Newton system
// (the rule: pose_host.h align_voxel; DESIGN.md §7c "Registering two maps").  Included by dr_fusion.hip inside namespace dr, behind
// stream_kernels.h, whose table search (xf_find) and block look-up (XfFetch) the reference map is read through.

// One wave per source block i in [0, n_src) of the ascending key table (no grid stride: the workgroup's four waves meet at one
// barrier), lane l on voxels 2 (l + 64 k) and the next, k = 0..3: k_map_transform's lane-to-voxel map, here the summation order.
// The image q = R g + tv of a source block is a rotated 7-voxel cube and its trilinear corners add one voxel: at most 7 sqrt(3) + 1
// voxels along an axis, so it spans at most 3 reference blocks per axis.  27 lanes resolve those from nb0 = floor(min over the
// block's 8 corner voxels of q) >> 3 on, one binary search each in the reference's key table, into LDS; a corner outside them
// (an R that drifted from orthogonal during the iterations could produce one) searches the table itself.  A block without a sample
// -- far from the surface, most of a map -- does no search and no gather and writes 28 zeros, which is what the sums of nothing
// are.  The 28 sums live in registers (align_voxel's loops are unrolled; the loop over k is not, and re-reads its uint4 so that no
// voxel is indexed by k); the wave's butterfly x = x + shfl_xor(x, off), off = 32..1, leaves the block's sums in every lane and lane
// 0 writes them to partial[i].  counts += {samples, valid, invalid}: integers, one atomic each per wave.
__global__ __launch_bounds__(256) void k_map_align(const unsigned long long *__restrict__ src_keys, const uint4 *__restrict__ src_vox, int n_src,
                                                   const unsigned long long *__restrict__ ref_keys, const uint2 *__restrict__ ref_vox, int n_ref,
                                                   const AlignEval e, double *__restrict__ partial, unsigned long long *__restrict__ counts) {
  __shared__ int s_near[4][27];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  const bool live = i < n_src;
  int blk[3] = {0, 0, 0};
  XfFetch fetch;
  fetch.keys = ref_keys; fetch.vox = ref_vox; fetch.near = s_near[wave]; fetch.n = n_ref;
  fetch.nb0[0] = fetch.nb0[1] = fetch.nb0[2] = 0;
  bool mine = false;  // one of this lane's 8 voxels is a sample
  if (live) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 p = src_vox[(size_t)i * 256 + lane + 64 * k];
      const uint32_t a[2] = {p.x, p.y}, b[2] = {p.z, p.w};
      mine = mine || align_is_sample(a, e) || align_is_sample(b, e);
    }
  }
  const bool work = __any(mine);  // wave-uniform (a wave that is not live has no sample)
  if (work) {
    const unsigned long long key = src_keys[i];
    blk[0] = (int)((key >> 42) & 0x1fffff) - (1 << 20);
    blk[1] = (int)((key >> 21) & 0x1fffff) - (1 << 20);
    blk[2] = (int)(key & 0x1fffff) - (1 << 20);
    double lo[3] = {1073741824.0, 1073741824.0, 1073741824.0};
    for (int c = 0; c < 8; ++c) {
      const double g0 = (double)(blk[0] * 8 + ((c & 4) ? 7 : 0)), g1 = (double)(blk[1] * 8 + ((c & 2) ? 7 : 0)), g2 = (double)(blk[2] * 8 + ((c & 1) ? 7 : 0));
      for (int k = 0; k < 3; ++k) {
        const double q = ((e.m.R[3 * k] * g0 + e.m.R[3 * k + 1] * g1) + e.m.R[3 * k + 2] * g2) + e.m.tv[k];
        lo[k] = q < lo[k] ? q : lo[k];
      }
    }
    for (int k = 0; k < 3; ++k) {
      const double c = lo[k] > -1073741824.0 ? lo[k] : -1073741824.0;  // (beyond it align_voxel reads nothing)
      fetch.nb0[k] = (int)floor(c) >> 3;
    }
    if (lane < 27) s_near[wave][lane] = xf_find(ref_keys, n_ref, fetch.nb0[0] + lane / 9, fetch.nb0[1] + (lane / 3) % 3, fetch.nb0[2] + lane % 3);
  }
  __syncthreads();
  if (!live) return;
  if (!work) {
    if (lane < 28) partial[(size_t)i * 28 + lane] = 0.0;
    return;
  }
  double acc[28];
#pragma unroll
  for (int c = 0; c < 28; ++c) acc[c] = 0.0;
  unsigned ns = 0, nv = 0;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int v = 2 * (lane + 64 * k);  // voxels v and v + 1: neighbours along z
    const uint4 p = src_vox[(size_t)i * 256 + lane + 64 * k];
    const int gx = blk[0] * 8 + (v >> 6), gy = blk[1] * 8 + ((v >> 3) & 7), gz = blk[2] * 8 + (v & 7);
    const uint32_t a[2] = {p.x, p.y}, b[2] = {p.z, p.w};
    if (align_is_sample(a, e)) {
      ++ns;
      nv += align_voxel(e, gx, gy, gz, __uint_as_float(p.x), fetch, acc) ? 1u : 0u;
    }
    if (align_is_sample(b, e)) {
      ++ns;
      nv += align_voxel(e, gx, gy, gz + 1, __uint_as_float(p.z), fetch, acc) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 28; ++c) acc[c] = acc[c] + __shfl_xor(acc[c], off);
    ns += __shfl_xor(ns, off); nv += __shfl_xor(nv, off);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 28; ++c) partial[(size_t)i * 28 + c] = acc[c];
    atomicAdd(&counts[0], (unsigned long long)ns);
    if (nv) atomicAdd(&counts[1], (unsigned long long)nv);
    if (ns - nv) atomicAdd(&counts[2], (unsigned long long)(ns - nv));
  }
}

// The fold over blocks: workgroup c = one wave = component c of 28.  Lane l adds partial[l], partial[l + 64], ... in ascending order
// from +0.0, then the same butterfly.  out (a pinned buffer the host reads after the stream's synchronisation) receives the 28 sums
// and, behind them, four counters (the registration uses three, its fourth stays 0; k_map_locate all four).
__global__ __launch_bounds__(64) void k_align_fold(const double *__restrict__ partial, int n, const unsigned long long *__restrict__ counts,
                                                   double *__restrict__ out) {
  const int lane = threadIdx.x, c = blockIdx.x;
  double x = 0.0;
  for (int i = lane; i < n; i += 64) x = x + partial[(size_t)i * 28 + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = x + __shfl_xor(x, off);
  if (lane == 0) out[c] = x;
  if (c == 0 && lane < 4) reinterpret_cast<unsigned long long *>(out + 28)[lane] = counts[lane];
}
