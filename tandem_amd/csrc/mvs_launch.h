// mvs_launch.h -- one launcher per kernel family of mvs_kernels.h (the convolution, k_fn_front, k_fn_head3 and k_tail have theirs next to their kernels).
// A launcher takes the family's argument struct and a stream; where a family has several instances it asks the choice function of mvs_host.h
// (choose_costvol / choose_prob / choose_regress) which one -- the same call names the instance in drm_profile.  Grids and LDS sizes are computed here
// and nowhere else.  The parity build (-DDR_PARITY_HOOKS) contains the superseded generations; in the product a choice that names one is an error.
#pragma once
#include <atomic>

#include "mvs_kernels.h"

namespace dr {

// ------------------------------------------------------------------ small launches
struct PreprocessArgs { const uint8_t *bgr; float4 *img; const float *lut; size_t npix; };
inline void launch_preprocess(const PreprocessArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(k_preprocess, dim3((unsigned)((a.npix + 255) / 256)), dim3(256), 0, st, a.bgr, a.img, a.lut, a.npix);
}
inline void launch_cache_io(const CacheIoArgs &io, int V, hipStream_t st) { hipLaunchKernelGGL(k_cache_io, dim3(32, V), dim3(256), 0, st, io); }
// out: the first logical pixel of a (V, H, W, 8) tensor with a zero border of `pad` pixels; T: the border correction (compose_out3)
struct BorderFixArgs { float *out; const float *T; int V, H, W, pad; };
inline void launch_out3_border(const BorderFixArgs &a, hipStream_t st) {
  const int per = 2 * (a.H + a.W) - 4, n = a.V * per * 8;
  const int rs = (a.W + 2 * a.pad) * 8;
  hipLaunchKernelGGL(k_out3_border, dim3(cdiv(n, 256)), dim3(256), 0, st, a.out, a.T, a.V, a.H, a.W, rs, (size_t)(a.H + 2 * a.pad) * rs);
}
// x: (V, H, W, cin); w, bias: the 1x1 layer cin -> 32; coarse: (V, H / 2, W / 2, 32), added nearest-upsampled.  cin names the instance (8 is the one there is).
struct SkipUpArgs { const float *x, *w, *bias, *coarse; float *out; int V, H, W, cin; };
inline void launch_skip_up([[maybe_unused]] const SkipUpArgs &a, [[maybe_unused]] hipStream_t st) {
#ifdef DR_PARITY_HOOKS
  const size_t npix = (size_t)a.V * a.H * a.W;
  const dim3 grid((unsigned)std::min<size_t>((npix + 31) / 32, 8192));
  hipLaunchKernelGGL(k_skip_up<8>, grid, dim3(256), 0, st, a.x, a.w, a.bias, a.coarse, a.out, a.V, a.H, a.W);
#endif  // (the product plans no SKIPUP op: MvsPlanBuilder::add_skip)
}

// The four result maps of a window go to the pinned host block in ONE kernel (16-byte stores over PCIe) instead of four
// copy-engine transfers: 4 x (launch + completion latency) is most of the time those take for 1.2 MB each.
__global__ __launch_bounds__(256) void k_publish4(const float4 *__restrict__ a, const float4 *__restrict__ b, const float4 *__restrict__ c,
                                                  const float4 *__restrict__ d, float4 *__restrict__ host, size_t n4) {
  const size_t nt = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < 4 * n4; i += nt) {
    const size_t k = i / n4, j = i - k * n4;
    host[i] = (k == 0 ? a : (k == 1 ? b : (k == 2 ? c : d)))[j];
  }
}
// n4: float4s per map (H and W are multiples of 32: whole float4s)
inline void launch_publish4(const float *a, const float *b, const float *c, const float *d, float *host_dev, size_t n4, hipStream_t st) {
  hipLaunchKernelGGL(k_publish4, dim3(256), dim3(256), 0, st, (const float4 *)a, (const float4 *)b, (const float4 *)c, (const float4 *)d, (float4 *)host_dev, n4);
}

// ------------------------------------------------------------------ cost volume
inline CostVolShape costvol_shape(const CostVolArgs &a) { return {a.V, a.h, a.w, a.planes.D, a.dchunk, a.fpad, a.view_aggregation}; }

template <int C, int DCH>
inline void launch_costvol5(const CostVolChoice &k, const CostVolArgs &b, const CostVolArgs &b4, dim3 grid, dim3 grid4, hipStream_t st) {
#ifdef DR_PARITY_HOOKS
  if (!k.b) hipLaunchKernelGGL((k_costvol5<C, DCH, 0, 1>), grid, dim3(256), 0, st, b);
  else if (k.c == 4) hipLaunchKernelGGL((k_costvol5<C, DCH, 1, 4>), grid4, dim3(256), 0, st, b4);
  else hipLaunchKernelGGL((k_costvol5<C, DCH, 1, 1>), grid, dim3(256), 0, st, b);
#else
  hipLaunchKernelGGL((k_costvol5<C, DCH, 1, 4>), grid4, dim3(256), 0, st, b4);
#endif
}

inline void launch_costvol(const CostVolArgs &a, const MvsSwitches &sw, int stage, hipStream_t st) {
  const CostVolChoice k = choose_costvol(costvol_shape(a), sw, stage);
  const int C = k.C;
  CostVolArgs b = a;
  b.gz = cdiv(a.planes.D, a.dchunk);
  b.abl = sw.cv5_abl;
  if (k.family == CostVolChoice::V1) {
#ifdef DR_PARITY_HOOKS
    const int cpl = k.a, pxb = 256 / (C / cpl);
    b.gx = cdiv(a.w, pxb); b.nwg = b.gx * b.gz * a.h;
    const dim3 grid1(8 * cdiv(b.nwg, 8));
    if (C == 32 && cpl == 8) hipLaunchKernelGGL((k_costvol<32, 8>), grid1, dim3(256), 0, st, b);
    else if (C == 32) hipLaunchKernelGGL((k_costvol<32, 4>), grid1, dim3(256), 0, st, b);
    else if (C == 16 && cpl == 8) hipLaunchKernelGGL((k_costvol<16, 8>), grid1, dim3(256), 0, st, b);
    else if (C == 16) hipLaunchKernelGGL((k_costvol<16, 4>), grid1, dim3(256), 0, st, b);
    else hipLaunchKernelGGL((k_costvol<8, 4>), grid1, dim3(256), 0, st, b);
    return;
#else
    fail(DR_ERR_UNSUPPORTED, "k_costvol (unpadded feature maps) is built into the parity library only");
#endif
  }
  // bordered feature maps: 4 channels per lane, no per-tap validity logic
  b.gx = cdiv(a.w, 1024 / C); b.nwg = b.gx * b.gz * a.h;
  const dim3 grid(8 * cdiv(b.nwg, 8));
  if (k.family == CostVolChoice::V4) {
#ifdef DR_PARITY_HOOKS
    const int dch = k.a, tw = C == 8 ? 16 : 8, th = (1024 / C) / tw;
    const bool sp8 = k.b == 8;
    CostVolArgs c4 = a;
    c4.gx = a.w / tw; c4.gz = a.planes.D / dch; c4.nwg = c4.gx * (a.h / th) * c4.gz;
    const dim3 g4(8 * cdiv(c4.nwg, 8));
    if (C == 32 && dch == 8) hipLaunchKernelGGL((k_costvol4<32, 8, 4>), g4, dim3(256), 0, st, c4);
    else if (C == 32) hipLaunchKernelGGL((k_costvol4<32, 4, 4>), g4, dim3(256), 0, st, c4);
    else if (C == 16 && sp8) hipLaunchKernelGGL((k_costvol4<16, 8, 8>), g4, dim3(256), 0, st, c4);
    else if (C == 16 && dch == 8) hipLaunchKernelGGL((k_costvol4<16, 8, 4>), g4, dim3(256), 0, st, c4);
    else if (C == 16) hipLaunchKernelGGL((k_costvol4<16, 4, 4>), g4, dim3(256), 0, st, c4);
    else if (sp8) hipLaunchKernelGGL((k_costvol4<8, 8, 8>), g4, dim3(256), 0, st, c4);
    else if (dch == 8) hipLaunchKernelGGL((k_costvol4<8, 8, 4>), g4, dim3(256), 0, st, c4);
    else hipLaunchKernelGGL((k_costvol4<8, 4, 4>), g4, dim3(256), 0, st, c4);
#else
    fail(DR_ERR_UNSUPPORTED, "k_costvol4 is built into the parity library only");
#endif
  } else if (k.family == CostVolChoice::V5) {  // view-outer / plane-inner sweep, the chunk's planes accumulate in registers (bit-identical to k_costvol3)
    const bool d8 = k.a == 8;
    CostVolArgs b4 = b;  // the four-row tile: x segments of a quarter of the pixels, four rows per workgroup
    b4.gx = cdiv(a.w, 256 / C); b4.nwg = b4.gx * b4.gz * cdiv(a.h, 4);
    const dim3 grid4(8 * cdiv(b4.nwg, 8));
    if (C == 32 && d8) launch_costvol5<32, 8>(k, b, b4, grid, grid4, st);
    else if (C == 32) launch_costvol5<32, 4>(k, b, b4, grid, grid4, st);
    else if (C == 16 && d8) launch_costvol5<16, 8>(k, b, b4, grid, grid4, st);
    else if (C == 16) launch_costvol5<16, 4>(k, b, b4, grid, grid4, st);
    else if (d8) launch_costvol5<8, 8>(k, b, b4, grid, grid4, st);
    else launch_costvol5<8, 4>(k, b, b4, grid, grid4, st);
  } else {
    const bool v3 = k.family == CostVolChoice::V3;
    if (v3 && C == 32) hipLaunchKernelGGL((k_costvol3<32>), grid, dim3(256), 0, st, b);
    else if (v3 && C == 16) hipLaunchKernelGGL((k_costvol3<16>), grid, dim3(256), 0, st, b);
    else if (v3) hipLaunchKernelGGL((k_costvol3<8>), grid, dim3(256), 0, st, b);
    else if (C == 32) hipLaunchKernelGGL((k_costvol2<32>), grid, dim3(256), 0, st, b);
    else if (C == 16) hipLaunchKernelGGL((k_costvol2<16>), grid, dim3(256), 0, st, b);
    else hipLaunchKernelGGL((k_costvol2<8>), grid, dim3(256), 0, st, b);
  }
}

// ------------------------------------------------------------------ prob head, regression
struct ProbArgs {
  const float *x, *wt;  // conv11's output (D,h,w,8); the weights as [tap][cin] (prob_taps).  x == nullptr: the stage has no PROB op (a TAIL or CONV op writes its logits)
  float *out;           // logits (D,h,w)
  int D, h, w;
};
inline ProbShape prob_shape(const ProbArgs &o) { return {o.D, o.h, o.w}; }

// rg: the stage's regression, which k_prob2_regress runs in the same launch where choose_prob says so (the stage's REGRESS op then launches nothing)
inline void launch_prob(const ProbArgs &o, const RegressArgs &rg, const MvsSwitches &sw, int stage, hipStream_t st) {
  const ProbChoice k = choose_prob(prob_shape(o), sw, stage);
  if (k.family == ProbChoice::GATHER) {
#ifdef DR_PARITY_HOOKS
    const int zchunk = k.zchunk, pb = sw.prob_block, xo = k.n;
    dim3 grid(cdiv(o.h * (o.w / xo), pb), cdiv(o.D, zchunk));
    int gz = 0, nwg = 0;
    if (!sw.prob_launch_order) {  // XCD-band workgroup order (A/B hook: the plain 2-D launch order)
      gz = (int)grid.y; nwg = (int)(grid.x * grid.y);
      grid = dim3(8 * cdiv(nwg, 8));
    }
    if (xo == 4) hipLaunchKernelGGL(k_prob<4>, grid, dim3(pb), 0, st, o.x, o.wt, o.out, o.D, o.h, o.w, zchunk, gz, nwg);
    else if (xo == 2) hipLaunchKernelGGL(k_prob<2>, grid, dim3(pb), 0, st, o.x, o.wt, o.out, o.D, o.h, o.w, zchunk, gz, nwg);
    else hipLaunchKernelGGL(k_prob<1>, grid, dim3(pb), 0, st, o.x, o.wt, o.out, o.D, o.h, o.w, zchunk, gz, nwg);
    return;
#else
    fail(DR_ERR_UNSUPPORTED, "k_prob is built into the parity library only");
#endif
  }
  const int NR = k.family == ProbChoice::STAGED ? k.n : 1, zc = k.zchunk;
  const int gxp = cdiv(o.w, kProbTX), gyp = cdiv(o.h, kProbTY * NR), gzp = cdiv(o.D, zc), nw = gxp * gyp * gzp;
  const dim3 grid(8 * cdiv(nw, 8));
  const size_t pl = prob2_lds_bytes(NR);
  if (k.family == ProbChoice::STAGED_REGRESS)
    hipLaunchKernelGGL(k_prob2_regress<8>, grid, dim3(256), pl, st, o.x, o.wt, o.out, o.h, o.w, gxp, gyp, nw, rg);
  else if (NR == 4) {
    static std::atomic<int> big{0};
    if (!big.load()) { DR_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_prob2<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); big.store(1); }
    hipLaunchKernelGGL(k_prob2<4>, grid, dim3(256), pl, st, o.x, o.wt, o.out, o.D, o.h, o.w, zc, gxp, gyp, gzp, nw);
  } else if (NR == 2) hipLaunchKernelGGL(k_prob2<2>, grid, dim3(256), pl, st, o.x, o.wt, o.out, o.D, o.h, o.w, zc, gxp, gyp, gzp, nw);
  else hipLaunchKernelGGL(k_prob2<1>, grid, dim3(256), pl, st, o.x, o.wt, o.out, o.D, o.h, o.w, zc, gxp, gyp, gzp, nw);
}

inline void launch_regress(const RegressArgs &r, const MvsSwitches &sw, hipStream_t st) {
  const dim3 grid(cdiv(r.h * r.w, 256)), block(256);
  const int D = choose_regress(r.planes.D, sw);
  if (D == 48) hipLaunchKernelGGL(k_regress_r<48>, grid, block, 0, st, r);
  else if (D == 32) hipLaunchKernelGGL(k_regress_r<32>, grid, block, 0, st, r);
  else if (D == 8) hipLaunchKernelGGL(k_regress_r<8>, grid, block, 0, st, r);
  else if (D == 4) hipLaunchKernelGGL(k_regress_r<4>, grid, block, 0, st, r);
  else hipLaunchKernelGGL(k_regress, grid, block, 0, st, r);
}

// ------------------------------------------------------------------ edge filter (exact radix-select quantile: edge, three histogram levels, apply)
struct FilterArgs {
  const float *depth3, *conf3;  // stage 3's maps
  float *edge, *depth, *conf;   // the edge measure; the filtered result
  unsigned *state, *hist;       // four 4-word select states; one 2048-bin histogram per level
  int n, H, W;                  // n = H * W
  int hist_blocks;              // workgroups of a histogram level (MvsSwitches::hist_blocks)
  bool fused;                   // the scans run as the prologue of the kernels that follow them (MvsSwitches::filter_fused)
};
// the three levels of the select: key bits [21, 32), [10, 21), [0, 10)
constexpr int kSelectShift[3] = {21, 10, 0}, kSelectBits[3] = {11, 11, 10};
inline void launch_edge(const FilterArgs &f, unsigned rank, hipStream_t st) {
  if (f.fused) hipLaunchKernelGGL(k_edge2, dim3(cdiv(f.n, 256)), dim3(256), 0, st, f.depth3, f.edge, f.H, f.W, f.state, f.hist, rank);
  else hipLaunchKernelGGL(k_edge, dim3(cdiv(f.n, 256)), dim3(256), 0, st, f.depth3, f.edge, f.H, f.W, f.state, rank);
}
// level 0..2 of the select, over that level's key bits; the fused form of levels 1 and 2 first scans the level before
inline void launch_hist(const FilterArgs &f, int level, hipStream_t st) {
  const dim3 grid(std::min(cdiv(f.n, 256), f.hist_blocks));
  const int shift = kSelectShift[level], bits = kSelectBits[level];
  if (f.fused && level > 0)
    hipLaunchKernelGGL(k_hist_s, grid, dim3(256), 0, st, f.edge, f.n, kSelectShift[level - 1], kSelectBits[level - 1], shift, bits, level, f.state, f.hist);
  else hipLaunchKernelGGL(k_hist, grid, dim3(256), 0, st, f.edge, f.n, shift, bits, f.state, f.hist);
}
inline void launch_scan(const FilterArgs &f, int level, hipStream_t st) {
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(256), 0, st, f.state, f.hist, kSelectShift[level], kSelectBits[level]);
}
// (the fused form first scans the last level)
inline void launch_apply(const FilterArgs &f, hipStream_t st) {
  if (f.fused) hipLaunchKernelGGL(k_apply_s, dim3(cdiv(f.n, 256)), dim3(256), 0, st, f.edge, f.state, f.hist, kSelectShift[2], kSelectBits[2], f.depth3, f.conf3, f.depth, f.conf, f.n);
  else hipLaunchKernelGGL(k_apply, dim3(cdiv(f.n, 256)), dim3(256), 0, st, f.edge, f.state, f.depth3, f.conf3, f.depth, f.conf, f.n);
}

}  // namespace dr
