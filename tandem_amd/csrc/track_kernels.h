// track_kernels.h -- drf_track_system / drf_track_frame on the device: the model map of one render and one evaluation of the
// tracking's Gauss-Newton system (the rule: pose_host.h track_normal / track_point; DESIGN.md §7c "Tracking a depth frame against
// the ray-cast model").  Included by dr_fusion.hip inside namespace dr, behind locate_kernels.h; launched by pose_ops.h; k_align_fold folds the groups.

// One lane per pixel of the model depth image: the pixel's normal and depth as one 16-byte element, once per render, so that an
// evaluation gathers one aligned element per sample instead of five depths.  A border pixel reads nothing but writes its zeros.
__global__ __launch_bounds__(256) void k_track_model(const float *__restrict__ Dm, const LocateGrid lg, float max_jump, TrackPixel *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= lg.W * lg.H) return;
  const int v = i / lg.W, u = i - v * lg.W;
  out[i] = track_normal(lg, max_jump, Dm, u, v);
}

// k_map_locate's shape: one wave per group i in [0, groups) of 512 grid positions, four per workgroup that share nothing (no LDS,
// no barrier), lane l on positions 512 i + l + 64 k, k = 0..7 -- consecutive lanes on consecutive pixels of a row, the frame's depth
// loads coalesce.  A group without a sample writes 28 zeros and gathers nothing.  The 28 sums live in registers (align_accumulate's
// loops are unrolled; the loop over k is not); the butterfly leaves the group's sums in every lane and lane 0 writes partial[i].
// counts += {samples, valid, unassociated, rejected}: integers, one atomic each per wave.  The model map is only read: one
// 16-byte load per associated sample, at an address that depends on the sample's projection.
__global__ __launch_bounds__(256) void k_track(const float *__restrict__ depth, const LocateGrid lg, const AlignEval e, const TrackModel t, int groups, int total,
                                               double *__restrict__ partial, unsigned long long *__restrict__ counts) {
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
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const int n = 512 * i + lane + 64 * k;
    double g[3];
    if (n >= total || !locate_pixel(lg, e.vs, n, depth, g)) continue;
    ++ns;
    const int r = track_point(e, t, lg, g[0], g[1], g[2], acc);
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
