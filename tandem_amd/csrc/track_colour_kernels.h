// track_colour_kernels.h -- drf_track_colour_system / drf_track_colour_frame on the device: the model map and the model intensity
// map of one render, and one evaluation of the system with the photometric term (the rule: pose_host.h track_model_intensity /
// track_photo_term / track_colour_point; DESIGN.md §7c "Tracking with colour").  Included by dr_fusion.hip inside namespace dr,
// behind track_kernels.h; launched by pose_ops.h; k_align_fold folds the groups.

// One lane per pixel: k_track_model's element, and the pixel's intensity from its three colour bytes where that element is valid.
__global__ __launch_bounds__(256) void k_track_model_colour(const float *__restrict__ Dm, const unsigned char *__restrict__ Cm, const LocateGrid lg, float max_jump,
                                                            TrackPixel *__restrict__ out, float *__restrict__ Ym) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= lg.W * lg.H) return;
  const int v = i / lg.W, u = i - v * lg.W;
  const TrackPixel p = track_normal(lg, max_jump, Dm, u, v);
  out[i] = p;
  Ym[i] = track_model_intensity(p, Cm + 3 * (size_t)i);
}

// k_track's shape: one wave per group of 512 grid positions, four per workgroup, no LDS, no barrier, a wave-uniform early-out for
// a group without a sample, 28 doubles in registers with the loop over k not unrolled, one integer atomic per wave and counter.
// Per valid sample: the 16-byte model-map gather, two 8-byte gathers of Ym (rows v0 and v0 + 1), and the frame's three colour
// bytes next to its depth, at an address consecutive lanes share a row of.  align_accumulate stands once in the instruction
// stream: track_colour_point runs its two terms as trips of one loop.  Four waves per SIMD are asked for (128 VGPRs): the kernel
// needs k_track's 120 and the second term's (r, n), which fits without scratch once the four per-lane counters share a register.
// counts += {samples, valid, unassociated, rejected, photometric terms added}.
__global__ __launch_bounds__(256, 4) void k_track_colour(const float *__restrict__ depth, const unsigned char *__restrict__ bgr, const LocateGrid lg, const AlignEval e,
                                                      const TrackModel t, const TrackColour tc, int groups, int total, double *__restrict__ partial,
                                                      unsigned long long *__restrict__ counts) {
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
  unsigned packed = 0;  // a lane has at most 8 of each: samples | valid << 8 | unassociated << 16 | photometric << 24, one register in the loop
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {
    const int n = 512 * i + lane + 64 * k;
    double g[3];
    if (n >= total || !locate_pixel(lg, e.vs, n, depth, g)) continue;
    const int r = track_colour_point(e, t, tc, lg, g[0], g[1], g[2], track_intensity(bgr + 3 * locate_offset(lg, n)), acc);
    packed += 1u + ((r & 1) ? 0x100u : 0u) + (r == 0 ? 0x10000u : 0u) + (r == 3 ? 0x1000000u : 0u);
  }
  unsigned ns = packed & 255u, nv = (packed >> 8) & 255u, nu = (packed >> 16) & 255u, np = packed >> 24;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 28; ++c) acc[c] = acc[c] + __shfl_xor(acc[c], off);
    ns += __shfl_xor(ns, off); nv += __shfl_xor(nv, off); nu += __shfl_xor(nu, off); np += __shfl_xor(np, off);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 28; ++c) partial[(size_t)i * 28 + c] = acc[c];
    atomicAdd(&counts[0], (unsigned long long)ns);
    if (nv) atomicAdd(&counts[1], (unsigned long long)nv);
    if (nu) atomicAdd(&counts[2], (unsigned long long)nu);
    if (ns - nv - nu) atomicAdd(&counts[3], (unsigned long long)(ns - nv - nu));
    if (np) atomicAdd(&counts[4], (unsigned long long)np);
  }
}
