// track_pyramid_kernels.h -- drf_track_reduce / drf_track_pyramid_* on the device: the reduction of a (bgr, depth) pair to level L of
// the image pyramid (the rule: pose_host.h track_reduce_host and its pieces; DESIGN.md §7c "Tracking coarse to fine").  The level's
// model map and evaluation are launches of k_track_model(_colour) and k_track(_colour) with the level's LocateGrid.  Included by
// dr_fusion.hip inside namespace dr, behind track_colour_kernels.h; launched by pose_ops.h.

// One lane per full-resolution pixel that a level pixel covers: thread t holds column i = t mod s of level pixel p = t / s
// (s = 2^L <= 16 divides 64, so a block's row never leaves its wave), p = v W_L + u over the level image.  A wave therefore covers
// 64 / s level pixels, and in every pass over the block's rows its lanes read one row-contiguous span of 64 floats (and 192 colour
// bytes) -- broken only where the span crosses the level row's end, and the dropped remainder columns and rows are never read.
// Two passes over the s rows of the block: the smallest valid depth (a min butterfly over the s lanes), then the sums -- the
// rule's butterfly t = t + t[i ^ off] across the lanes per row, the rows added in ascending order; the integer count and colour
// sums are folded once at the end.  The second pass reads what the first one brought into the cache.  No LDS, no scratch, no early
// return (a tail lane beyond W_L H_L reads nothing and holds an invalid pixel, so every shuffle sees 64 live lanes); lane i = 0
// stores the level pixel.  bgr null: the depth alone.
__global__ __launch_bounds__(256) void k_track_reduce(const float *__restrict__ depth, const unsigned char *__restrict__ bgr, int W, int WL, int HL, int L, float max_jump,
                                                      float *__restrict__ depth_out, unsigned char *__restrict__ bgr_out) {
  const int s = 1 << L;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int p = t >> L, i = t & (s - 1);
  const bool live = p < WL * HL;
  const int v = live ? p / WL : 0, u = live ? p - v * WL : 0;
  const size_t at = (size_t)(v * s) * (size_t)W + (size_t)(u * s + i);
  float z0 = 0.0f;
  bool any = false;  // z0 is the smallest valid depth so far
  for (int r = 0; r < s; ++r) {
    const float z = live ? depth[at + (size_t)r * W] : 0.0f;
    if (track_reduce_valid(z)) { z0 = any && z0 < z ? z0 : z; any = true; }
  }
  for (int off = s >> 1; off > 0; off >>= 1) {
    const float zo = __shfl_xor(z0, off);
    const bool ao = __shfl_xor(any ? 1 : 0, off) != 0;
    if (ao) { z0 = any && z0 < zo ? z0 : zo; any = true; }
  }
  int n = 0, c0 = 0, c1 = 0, c2 = 0;
  float S = 0.0f;
  for (int r = 0; r < s; ++r) {
    const size_t px = at + (size_t)r * W;
    const float z = live && any ? depth[px] : 0.0f;
    const bool acc = any && track_reduce_accepted(z, z0, max_jump);
    float row = acc ? z : 0.0f;
    if (acc) {
      ++n;
      if (bgr) { c0 += bgr[3 * px]; c1 += bgr[3 * px + 1]; c2 += bgr[3 * px + 2]; }
    }
    for (int off = s >> 1; off > 0; off >>= 1) row = row + __shfl_xor(row, off);
    S = r == 0 ? row : S + row;
  }
  for (int off = s >> 1; off > 0; off >>= 1) {
    n += __shfl_xor(n, off);
    c0 += __shfl_xor(c0, off); c1 += __shfl_xor(c1, off); c2 += __shfl_xor(c2, off);
  }
  if (!live || i != 0) return;
  const bool keep = any && 2 * n >= s * s;
  depth_out[p] = keep ? S / (float)n : 0.0f;
  if (bgr) {
    bgr_out[3 * (size_t)p] = keep ? track_reduce_colour(c0, n) : (unsigned char)0;
    bgr_out[3 * (size_t)p + 1] = keep ? track_reduce_colour(c1, n) : (unsigned char)0;
    bgr_out[3 * (size_t)p + 2] = keep ? track_reduce_colour(c2, n) : (unsigned char)0;
  }
}
