// track_exposure_kernels.h -- drf_track_exposure_system / drf_track_exposure_frame on the device: one evaluation of the 8 x 8 system
// of pose, gain and offset, and the fold of its 45-wide rows (the rule: pose_host.h track_exposure_point / exposure_accumulate;
// DESIGN.md §7c "Tracking under a change of exposure").  Included by dr_fusion.hip inside namespace dr, behind
// track_pyramid_kernels.h; launched by pose_ops.h.  The model map and Ym are k_track_model_colour's, the levels k_track_reduce's.

// k_track_colour's shape: one wave per group of 512 grid positions, four per workgroup, no LDS, no barrier, a wave-uniform early-out
// for a group without a sample, the loop over k not unrolled, one integer atomic per wave and counter.  45 doubles in registers
// are 90 VGPRs where k_track_colour holds 56, so its bound of 128 cannot hold: two waves per SIMD are asked for (256 VGPRs), and
// the compiler's report says what it took, without scratch.  align_accumulate stands once in the instruction stream
// (the two terms are trips of one loop), exposure_accumulate once behind it.  Lane 0 writes the group's 45 partial sums with
// plain vector stores.  counts += {samples, valid, unassociated, rejected, photometric terms added}.
__global__ __launch_bounds__(256, 2) void k_track_exposure(const float *__restrict__ depth, const unsigned char *__restrict__ bgr, const LocateGrid lg, const AlignEval e,
                                                        const TrackModel t, const TrackColour tc, const TrackExposure x, int groups, int total,
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
    if (lane < 45) partial[(size_t)i * 45 + lane] = 0.0;
    return;
  }
  double acc[45];
#pragma unroll
  for (int c = 0; c < 45; ++c) acc[c] = 0.0;
  unsigned packed = 0;  // a lane has at most 8 of each: samples | valid << 8 | unassociated << 16 | photometric << 24, one register in the loop
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const int n = 512 * i + lane + 64 * k;
    double g[3];
    if (n >= total || !locate_pixel(lg, e.vs, n, depth, g)) continue;
    const int r = track_exposure_point(e, t, tc, x, lg, g[0], g[1], g[2], track_intensity(bgr + 3 * locate_offset(lg, n)), acc);
    packed += 1u + ((r & 1) ? 0x100u : 0u) + (r == 0 ? 0x10000u : 0u) + (r == 3 ? 0x1000000u : 0u);
  }
  unsigned ns = packed & 255u, nv = (packed >> 8) & 255u, nu = (packed >> 16) & 255u, np = packed >> 24;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 45; ++c) acc[c] = acc[c] + __shfl_xor(acc[c], off);
    ns += __shfl_xor(ns, off); nv += __shfl_xor(nv, off); nu += __shfl_xor(nu, off); np += __shfl_xor(np, off);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 45; ++c) partial[(size_t)i * 45 + c] = acc[c];
    atomicAdd(&counts[0], (unsigned long long)ns);
    if (nv) atomicAdd(&counts[1], (unsigned long long)nv);
    if (nu) atomicAdd(&counts[2], (unsigned long long)nu);
    if (ns - nv - nu) atomicAdd(&counts[3], (unsigned long long)(ns - nv - nu));
    if (np) atomicAdd(&counts[4], (unsigned long long)np);
  }
}

// The fold over groups for 45-wide rows, by k_align_fold's rule: workgroup c = one wave = component c of 45.  Lane l adds
// partial[l], partial[l + 64], ... in ascending order from +0.0, then the butterfly.  out (the pinned pair's current slot, which the
// host reads after the stream's synchronisation) receives the 45 sums and, behind them, the five counters: 400 bytes.
__global__ __launch_bounds__(64) void k_exposure_fold(const double *__restrict__ partial, int n, const unsigned long long *__restrict__ counts,
                                                      double *__restrict__ out) {
  const int lane = threadIdx.x, c = blockIdx.x;
  double x = 0.0;
  for (int i = lane; i < n; i += 64) x = x + partial[(size_t)i * 45 + c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = x + __shfl_xor(x, off);
  if (lane == 0) out[c] = x;
  if (c == 0 && lane < 5) reinterpret_cast<unsigned long long *>(out + 45)[lane] = counts[lane];
}
