// conv_plan.h -- the host half of the convolution kernels (conv_mfma.h and its companions): the logical layer description, the kernel-argument
// structs, the list of template instances of every kernel family, and the planner that turns a layer into packed weights, tap tables, a tile plan
// and a launch.  Plain C++17 over dr_host.h and march_plan.h, no HIP header: g++ compiles it alone for the CPU tests (tests/test_conv_plan_host.py,
// tests/cpp/tuned_rows.cpp) and tools/dump_plans.cpp.  plan_conv is a list of named steps over one record (ConvPlanner); the arena that receives
// the planner's small arrays is a template parameter (HostArena here, DeviceArena in conv_mfma.h).
#pragma once
#include <algorithm>
#include <cmath>

#include "dr_host.h"
#include "march_plan.h"

#if !defined(__HIPCC__)
// The plan structs name two HIP types: float4 (only as a pointee) and dim3.  Stand-ins for a host-only compile, as march_plan.h guards DR_HD.
struct float4 { float x, y, z, w; };
struct dim3 {
  unsigned x, y, z;
  constexpr dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
#endif

namespace dr {

struct ConvClass {  // one output-parity class of a launch (plain convs have exactly one)
  int NU;        // K chunks per channel pass
  int tap_base;  // offset into tapoff[]
  int w_base;    // offset into wpk[] (float4 units)
  int ooz, ooy, oox;
};

struct ConvArgs {
  const float *in;
  float *out;
  const float4 *wpk;
  const float *scale, *bias, *add;
  const int *tapoff;
  const ConvClass *cls;
  int inD, inH, inW, inC;
  int outD, outH, outW, outC;
  int nPD, nPH, nPW;
  int sz, sy, sx, pz, py, px;
  int omz, omy, omx;
  int TZ, TY, TXT, TZI, TYI, TXI;
  int npass, ctTot, rows_valid, relu, add_mode, addH, addW;
  int par_rows, par_map;    // transposed layers: rows per output parity (= Cout) and 3 bits (z,y,x) per parity; 0 otherwise
  unsigned magicX, magicY;  // ceil(2^32 / TXI), ceil(2^32 / TYI): exact division of tile positions (< 2^16)
  int nuMax;                // max K chunks per pass over the classes (sizes the LDS weight area)
  int tilesD, tilesH, tilesW;
  // FZ instances: the input tensor is never materialised -- the staging step computes it from FeatureNet's skip pair,
  // in[v][y][x][c] = (W1 . fz_x[v][y][x][0..FZ) + fz_b)[c] + fz_coarse[v][y/2][x/2][c]   (module.py:517-529)
  const float *fz_x, *fz_w, *fz_b, *fz_coarse;
  // k_conv_a (persistent, LDS-DMA staged) only:
  int pass_stride;      // input elements between the channel slices of two passes: CI (the slices interleave inside a position's record) or, for an
                        // input stored as consecutive (D,H,W,CI) sub-tensors (stage 1's cost volume), the size of one sub-tensor
  const float *zero16;  // 16 zero bytes: the source of every staged element outside the tensor
  int a_slots;          // 16-byte LDS slots per tile buffer (multiple of 512)
  int a_wbufs;          // weight buffers: npass when all passes fit (each fetched once per workgroup), else 2 (one per pass in flight)
  int class_loop;       // k_conv, single-pass transposed layers: > 0 = the number of parity classes ONE workgroup walks on its staged tile (grid.y = 1), see k_conv
};

constexpr int kConvThreads = 256;
constexpr size_t kConvMaxLds = 160 * 1024;  // gfx950: 160 KiB LDS per CU, one workgroup may take all of it

enum ConvMode { CONV_NORMAL = 0, CONV_XPAIR = 1, CONV_X8 = 2 };

struct ConvLayer {  // logical description (torch semantics)
  int Cin = 0, Cout = 0;
  int kd = 1, kh = 1, kw = 1;
  int sd = 1, sh = 1, sw = 1;
  bool transposed = false;          // ConvTranspose3d(k=3, pad=1, output_padding = stride-1)
  int up2 = 0;                      // 1 + py: Conv2d(k=3, pad=1) applied to the nearest x2 upsampling (in H and W) of the input,
                                    // which is given at HALF resolution and never upsampled in memory; this launch produces the output rows 2Y + py.  Output
                                    // pixel (2Y+py, 2X+px) reads 2 x 2 input pixels, the kernel rows / columns that fall on the same input
                                    // pixel summed (weight (Cout,Cin,1,3,3)); both px are rows of the launch (2 * Cout rows)
  const float *weight = nullptr;    // (Cout,Cin,kd,kh,kw) or transposed (Cin,Cout,kd,kh,kw)
  std::vector<float> scale, bias;   // per Cout (folded BN / conv bias); empty -> 1 / 0
  bool relu = false;
  int out_pad = 0;                  // the output tensor carries a border of this many pixels in H and W (`out` points at its first interior pixel)
};

struct ConvFuse {  // FeatureNet skip pair fused into the staging step of the layer that consumes it (device pointers)
  const float *x, *w, *b, *coarse;
  int cin;  // channels of x (8)
};

// The kernel family of a plan.  The values are the codes of conv_tuned.h's last column (tools/tune_conv.sh writes them) and of the planner's candidates.
enum ConvFamily {
  CONV_FAM_TILE = 0,       // k_conv (4 waves, one tile per workgroup; k_conv_c / k_conv_b are launch forms of it)
  CONV_FAM_ASYNC = 1,      // k_conv_a (persistent, LDS-DMA staged, 8 waves)
  CONV_FAM_MARCH = 2,      // k_conv_m marching along z / over 2-D tiles
  CONV_FAM_ROWMARCH = 3,   // k_conv_m marching down the rows of a 2-D layer
  CONV_FAM_WINO = 4,       // k_conv_w (k_conv with the y axis in Winograd F(2,3) form)
  CONV_FAM_WINOMARCH = 5,  // the Winograd form on k_conv_m (3-D layers)
};

struct ConvLaunch {
  ConvArgs args;
  int ci, ct, pt, fz = 0;
  int async = 0;  // 1: k_conv_a (persistent, LDS-DMA staged, 512 threads); 2: k_conv_m (marching, 8 consumer + 2 producer waves); 4: k_conv_w -- what
                  // launch_conv dispatches on; march.rm / march.wino tell k_conv_m's three families apart (conv_family())
  MarchArgs march{};
  int nup = 0;    // k_conv_m: K chunks per input plane
  int ncw = 8;    // k_conv_m: consumer waves (8 or 12)
  int bf3 = 0;    // 1: k_conv_b (bf16 x 3 operands; wpk holds hi / lo bf16 fragments, 32-wide K chunks)
  dim3 grid;
  size_t lds_bytes;
  double flops;  // useful (algorithmic) flops of this launch
};

inline ConvFamily conv_family(const ConvLaunch &c) {
  if (c.async == 2) return c.march.rm ? CONV_FAM_ROWMARCH : (c.march.wino ? CONV_FAM_WINOMARCH : CONV_FAM_MARCH);
  return c.async == 4 ? CONV_FAM_WINO : (c.async ? CONV_FAM_ASYNC : CONV_FAM_TILE);
}
// the family as drm_profile, drm_autotune and DR_CONV_PRINT print it in front of <CI,CT,PT> (the tile kernel has no prefix)
inline const char *conv_family_name(ConvFamily f) {
  static const char *const names[] = {"", "async", "march", "rowmarch", "wino", "winomarch"};
  return names[f];
}
// the kernel template that runs the family
inline const char *conv_family_kernel(ConvFamily f) {
  static const char *const names[] = {"k_conv", "k_conv_a", "k_conv_m", "k_conv_m", "k_conv_w", "k_conv_m"};
  return names[f];
}

struct DimTaps {               // per-axis decomposition of one parity class
  std::vector<int> t, off;     // kernel index, input offset (>= 0)
  int s = 1, p = 0, om = 1, oo = 0, npos = 0;
  int par = -1;                // transposed stride-2 axis split into classes: the output parity this class produces (-1: not split)
};

// Per-axis tap lists.  Normal conv: in = pos*s - pad + t.  Transposed stride 1: out[o] = sum_t x[o+1-t] w[t].
// Transposed stride 2 (k=3, pad=1, output_padding=1):  out[2m] = x[m] w[1];  out[2m+1] = x[m] w[2] + x[m+1] w[0].
// All 2^d output parities of a position m read the same 2^d input neighbourhood, so the layer runs as ONE stride-1
// convolution with a 2-wide kernel per strided axis and npar*Cout output rows (row = parity*Cout + channel, zero
// weight where a parity does not use an offset); the epilogue scatters row groups to out[2m + parity].
inline int parity_kernel_index(int parity, int off) {  // -1: this (parity, offset) pair carries no weight
  if (parity == 0) return off == 0 ? 1 : -1;
  return off == 0 ? 2 : 0;
}
// A strided transposed axis comes in two forms.  DENSE: both parities are output ROWS of one class (offsets {0,1}, zero weight
// where parity 0 does not use offset 1) -- one class, but a quarter of the products per axis are multiplications by zero.
// SPLIT: one class per parity (parity 0: offset 0 only; parity 1: offsets 0 and 1) -- no zero products, half the rows.
// An up2 axis (ConvLayer::up2): output 2m + par of the 3-tap kernel over the upsampled signal reads input {m-1, m} (par 0: kernel
// index 0 | indices 1 and 2 summed) or {m, m+1} (par 1: indices 0 and 1 summed | index 2); offsets are relative to m - 1 (pad 1).
inline std::vector<DimTaps> axis_classes_up2(int in_size, bool split) {
  std::vector<DimTaps> r;
  if (!split) { DimTaps d; d.t = {0, 1, 2}; d.off = {0, 1, 2}; d.p = 1; d.om = 2; d.npos = in_size; r.push_back(d); return r; }
  DimTaps e; e.t = {0, 1}; e.off = {0, 1}; e.p = 1; e.om = 2; e.oo = 0; e.npos = in_size; e.par = 0; r.push_back(e);
  DimTaps o; o.t = {1, 2}; o.off = {1, 2}; o.p = 1; o.om = 2; o.oo = 1; o.npos = in_size; o.par = 1; r.push_back(o);
  return r;
}
// kernel indices that (parity, input offset) of an up2 axis sums; returns the count (0: the pair carries no weight)
inline int up2_kernel_set(int parity, int off, int (&k)[2]) {
  if (parity == 0) { if (off == 0) { k[0] = 0; return 1; } if (off == 1) { k[0] = 1; k[1] = 2; return 2; } return 0; }
  if (off == 1) { k[0] = 0; k[1] = 1; return 2; }
  if (off == 2) { k[0] = 2; return 1; }
  return 0;
}
// Taps that can only ever read padding are dropped: on an axis of extent 1 a 3-tap stride-1 kernel touches the tensor through its centre tap
// alone (stage 3's conv6 runs on a depth of 1: two thirds of its products were multiplications by staged zeros), a stride-2 kernel on an axis of
// extent 2 through two of its three taps (conv5), a transposed stride-2 axis of extent 1 never reads x[m + 1] (conv7).  The remaining offsets are
// shifted so that the smallest is 0 (the padding shrinks with them): the halo a tile stages shrinks too.
inline void prune_taps(DimTaps &d, int in_size) {
  std::vector<int> t, off;
  for (size_t i = 0; i < d.t.size(); ++i) {
    bool used = false;
    for (int pos = 0; pos < d.npos && !used; ++pos) { const int x = pos * d.s - d.p + d.off[i]; used = x >= 0 && x < in_size; }
    if (used) { t.push_back(d.t[i]); off.push_back(d.off[i]); }
  }
  if (t.empty() || t.size() == d.t.size()) return;
  const int mo = *std::min_element(off.begin(), off.end());
  for (int &o : off) o -= mo;
  d.p -= mo;
  d.t = t; d.off = off;
}
// (prune: the planner asks for it on the DEPTH axis only -- the in-plane axes of every layer are far longer than their kernels, and the row march /
// Winograd forms are written for exactly three y taps; DR_CONV_NO_TAP_PRUNE, parity build, turns it off: ConvPolicy)
inline std::vector<DimTaps> axis_classes(int k, int s, bool transposed, int in_size, bool split = false, bool prune = false) {
  std::vector<DimTaps> r;
  if (!transposed) {
    DimTaps d;
    for (int t = 0; t < k; ++t) { d.t.push_back(t); d.off.push_back(t); }
    d.s = s; d.p = k / 2; d.npos = (in_size + 2 * (k / 2) - k) / s + 1;
    r.push_back(d);
  } else if (k == 1) {
    DimTaps d; d.t = {0}; d.off = {0}; d.npos = in_size; r.push_back(d);
  } else if (s == 1) {
    DimTaps d;
    for (int t = 0; t < k; ++t) { d.t.push_back(t); d.off.push_back(2 - t); }
    d.p = 1; d.npos = in_size;
    r.push_back(d);
  } else if (!split) {
    // dense parity form: input offsets {0,1}; which kernel index a (parity, offset) pair selects is resolved when the
    // weights are packed (parity_kernel_index), the two parities of this axis become separate output ROWS
    DimTaps d; d.t = {0, 1}; d.off = {0, 1}; d.om = 2; d.oo = 0; d.npos = in_size; r.push_back(d);
  } else {
    DimTaps e; e.t = {0}; e.off = {0}; e.om = 2; e.oo = 0; e.npos = in_size; e.par = 0; r.push_back(e);
    DimTaps o; o.t = {0, 1}; o.off = {0, 1}; o.om = 2; o.oo = 1; o.npos = in_size; o.par = 1; r.push_back(o);
  }
  if (prune)
    for (DimTaps &d : r) prune_taps(d, in_size);
  return r;
}

struct ConvPlanOut {
  std::vector<ConvLaunch> launches;
  int outD, outH, outW;
  int ncand = 0;  // feasible (CI, PT, CT, tile) candidates the planner ranked
};

// The planner's arena for a process without a device (CPU tests, tools/dump_plans.cpp): the "uploads" stay in host memory, and the size of
// each is kept so that a check can tell whether an offset of the plan lies inside its array.
struct HostArena {
  std::vector<void *> ptrs;
  std::vector<size_t> bytes;  // of upload i
  int *err_flag = nullptr;    // what MarchArgs::err receives (see DeviceArena)
  template <class T>
  T *upload(const std::vector<T> &h) {
    T *d = static_cast<T *>(malloc(std::max<size_t>(h.size() * sizeof(T), 16)));
    memcpy(d, h.data(), h.size() * sizeof(T));
    ptrs.push_back(d);
    bytes.push_back(h.size() * sizeof(T));
    return d;
  }
  HostArena() = default;
  HostArena(const HostArena &) = delete;
  HostArena &operator=(const HostArena &) = delete;
  ~HostArena() { for (void *p : ptrs) free(p); }
};

// Measured-best plans for known layer shapes (tools/tune_conv.sh -> conv_tuned.h); anything else uses the cost model.
struct ConvTuned {
  int Cin, Cout, kd, kh, kw, sd, sh, sw, transposed, mode, inD, inH, inW;  // layer signature
  int ci, ct, pt, tz, ty, txt;                                              // plan: channel pass, row tiles, position tiles per wave, tile shape (txt in 16s)
  int async_;                                                               // the plan's ConvFamily
};
#include "conv_tuned.h"

// ---- the template instances of every kernel family: ONE list each, from which the planner's predicate (here) and launch_conv's dispatcher
// (conv_mfma.h) both expand ----
// k_conv (CI, CT, PT)
#define DR_CONV_INSTANCES(X)                                                                   \
  X(4, 1, 4) X(4, 1, 1) X(8, 1, 4) X(8, 1, 1) X(8, 2, 4) X(8, 2, 1) X(8, 4, 4) X(8, 4, 1)      \
  X(16, 1, 4) X(16, 1, 1) X(16, 2, 4) X(16, 2, 1) X(16, 4, 4) X(16, 4, 1)
// k_conv_b (parity build): k_conv's without the 4-channel pass
#define DR_CONV_B_INSTANCES(X)                                                                 \
  X(8, 1, 4) X(8, 1, 1) X(8, 2, 4) X(8, 2, 1) X(8, 4, 4) X(8, 4, 1)                            \
  X(16, 1, 4) X(16, 1, 1) X(16, 2, 4) X(16, 2, 1) X(16, 4, 4) X(16, 4, 1)
// k_conv_c, the class-loop form
#define DR_CONV_C_INSTANCES(X) X(8, 1, 4) X(8, 1, 1) X(8, 2, 4) X(8, 2, 1) X(16, 1, 4) X(16, 1, 1) X(16, 2, 4) X(16, 2, 1)
// k_conv_a.  PT = 1 (round 4): 128-position tiles, for the layers whose halo (stride 2, 5 x 5) does not fit twice at 256
#define DR_CONV_A_INSTANCES(X)                                                                 \
  X(4, 1, 4) X(4, 1, 2)                                                                        \
  X(8, 1, 4) X(8, 1, 2) X(8, 1, 1) X(8, 2, 4) X(8, 2, 2) X(8, 2, 1)                            \
  X(16, 1, 4) X(16, 1, 2) X(16, 1, 1) X(16, 2, 4) X(16, 2, 2) X(16, 2, 1)
// k_conv_w: 16-channel passes with one or two row tiles, 8-channel passes (Cin = 8) with one
// (PT = 4 needs more than 256 registers: 64 accumulators + two operand sets of 80)
#define DR_CONV_W_INSTANCES(X) X(16, 1, 1) X(16, 1, 2) X(16, 2, 1) X(16, 2, 2) X(8, 1, 1) X(8, 1, 2)
// k_conv_m instances (CI, NUP, CT, PT, consumer waves).  3-D layers: NUP = 6 (8 channels, XPAIR), 12 (16 channels, XPAIR), 9 (16 channels);
// row march of 2-D layers: NUP = 2 (8 channels, XPAIR), 4 (16 channels, XPAIR), 3 (16 channels).  CT = 2 with PT = 4 needs more than the
// 168 registers three waves per SIMD leave; twelve consumer waves leave 128 each.
#define DR_MARCH_INSTANCES(X)                                                                                         \
  X(8, 6, 1, 2, 8) X(8, 6, 1, 4, 8) X(8, 6, 1, 1, 12) X(8, 6, 1, 2, 12)                                               \
  X(16, 12, 1, 2, 8) X(16, 12, 1, 4, 8) X(16, 12, 1, 1, 12) X(16, 12, 1, 2, 12)                                       \
  X(16, 9, 1, 2, 8) X(16, 9, 1, 4, 8) X(16, 9, 1, 1, 12) X(16, 9, 1, 2, 12) X(16, 9, 2, 2, 8)                         \
  X(8, 2, 1, 1, 8) X(8, 2, 1, 2, 8) X(8, 2, 1, 4, 8) X(8, 2, 1, 1, 10) X(8, 2, 1, 2, 10)                              \
  X(16, 4, 1, 1, 8) X(16, 4, 1, 2, 8) X(16, 4, 1, 4, 8) X(16, 4, 1, 1, 10) X(16, 4, 1, 2, 10)                         \
  X(16, 3, 1, 1, 8) X(16, 3, 1, 2, 8) X(16, 3, 1, 4, 8) X(16, 3, 1, 1, 10) X(16, 3, 1, 2, 10)                         \
  X(16, 3, 2, 1, 8) X(16, 3, 2, 2, 8) X(16, 3, 2, 1, 10) X(16, 3, 2, 2, 10)
// the Winograd form of the 3-D instances (march_consumer_w): one position tile (16 x by a row pair) per wave
#define DR_MARCH_W_INSTANCES(X) X(8, 6, 1, 1, 8) X(16, 12, 1, 1, 8) X(16, 9, 1, 1, 8)  // (twelve consumer waves leave 128 registers: the two operand sets spill)

#define DR_X3(CI_, CT_, PT_) if (ci == CI_ && ct == CT_ && pt == PT_) return true;
#define DR_X5(CI_, NUP_, CT_, PT_, NCW_) if (ci == CI_ && nup == NUP_ && ct == CT_ && pt == PT_ && ncw == NCW_) return true;
inline bool conv_instance_exists(int ci, int ct, int pt) { DR_CONV_INSTANCES(DR_X3) return false; }
inline bool conv_b_instance_exists(int ci, int ct, int pt) { DR_CONV_B_INSTANCES(DR_X3) return false; }
inline bool conv_c_instance_exists(int ci, int ct, int pt) { DR_CONV_C_INSTANCES(DR_X3) return false; }
inline bool conv_a_instance_exists(int ci, int ct, int pt) { DR_CONV_A_INSTANCES(DR_X3) return false; }
inline bool conv_w_instance_exists(int ci, int ct, int pt) { DR_CONV_W_INSTANCES(DR_X3) return false; }
inline bool conv_m_instance_exists(int ci, int nup, int ct, int pt, int ncw, bool wino = false) {
  if (wino) { DR_MARCH_W_INSTANCES(DR_X5) return false; }
  DR_MARCH_INSTANCES(DR_X5)
  return false;
}
#undef DR_X3
#undef DR_X5
// whether a launch's instance is in its family's list (the fused-skip forms of the parity build are dispatched by hand: launch_conv)
inline bool conv_launch_instance_exists(const ConvLaunch &c) {
  switch (conv_family(c)) {
    case CONV_FAM_TILE: return c.bf3 ? conv_b_instance_exists(c.ci, c.ct, c.pt) : (c.args.class_loop > 0 ? conv_c_instance_exists(c.ci, c.ct, c.pt) : conv_instance_exists(c.ci, c.ct, c.pt));
    case CONV_FAM_ASYNC: return conv_a_instance_exists(c.ci, c.ct, c.pt);
    case CONV_FAM_WINO: return conv_w_instance_exists(c.ci, c.ct, c.pt);
    default: return conv_m_instance_exists(c.ci, c.nup, c.ct, c.pt, c.ncw, c.march.wino != 0);
  }
}

// rocprofv3's spelling of the launch's kernel instance (drm_profile prints it)
inline void conv_instance_name(const ConvLaunch &c, char *kn, size_t n) {
  if (c.async == 2) snprintf(kn, n, "k_conv_m<%d,%d,%d,%d,%d,%d,%d>", c.ci, c.nup, c.ct, c.pt, c.fz, c.ncw, c.march.wino);
  else if (c.async || c.bf3 || c.args.class_loop > 0)
    snprintf(kn, n, "%s<%d,%d,%d>", c.async ? conv_family_kernel(conv_family(c)) : (c.bf3 ? "k_conv_b" : "k_conv_c"), c.ci, c.ct, c.pt);
  else snprintf(kn, n, "k_conv<%d,%d,%d,%d>", c.ci, c.ct, c.pt, c.fz);
}

// Opt-in precision mode (DR_CONV_BF16X3=1, parity build): every layer with Cin % 8 == 0 runs on k_conv_b -- k_conv's data flow on the bf16 matrix cores
// with both operands split into two bf16 terms and the three leading products accumulated in fp32 (conv_bf3.h has the numerics).
inline int conv_bf3_policy() {
  const char *e = hook_env("DR_CONV_BF16X3");
  return e && atoi(e) > 0 ? 1 : 0;
}
// What the environment says about planning, read ONCE at the top of plan_conv: nothing below it calls getenv.  The first five are the product's
// switches ("Environment switches"); the rest exist in the parity build only (hook_env) and keep their defaults in the product.
struct ConvPolicy {
  int async = 2;     // DR_CONV_ASYNC: which kernel family the planner may use: 0 = k_conv only, 1 = k_conv_a only (falls back to k_conv when no async plan
                     // fits), 2 = both, ranked together (A/B hook)
  int march = 1;     // DR_CONV_MARCH: 0 = never plan k_conv_m, 1 = rank it with the other families (default), 2 = prefer it wherever it applies (A/B hook)
  int rowmarch = 1;  // DR_CONV_ROWMARCH: the same for the row march of 2-D layers (0 = never, 1 = ranked, 2 = preferred)
  int wino = 1;      // DR_CONV_WINO: 0 = never plan k_conv_w, 1 = rank it with the other families (default), 2 = prefer it wherever it applies (A/B hook, tests)
  bool no_tuned = false;  // DR_CONV_NO_TUNED: the cost model's ranking as it is, no conv_tuned.h row applied
  int bf3 = 0;            // conv_bf3_policy()
  // Form of a stride-2 transposed layer (see axis_classes): 0 = every strided axis dense (8 * Cout rows, 27 of 64 products useful),
  // 1 = x dense, z and y split (2 * Cout rows in 4 classes, 3 of 4 useful), 2 = every axis split (Cout rows in 8 classes, all
  // useful).  Default by measurement at 640x480 (profiles/r03_experiments.txt): conv11 (Cout 8) 0.076 / 0.073 / 0.126 ms, conv9 (Cout 16)
  // 0.039 / 0.030 / 0.034, conv7 (Cout 32) 0.0265 / 0.0233 / 0.0221 for forms 0 / 1 / 2.  DR_DECONV_FORM overrides (A/B hook).
  int deconv_form = -1;   // -1: by Cout
  // Order in which an instance of the Winograd form walks its range: 2 = scatter (march_consumer_ws: every input plane read and transformed
  // once), 1 = gather (march_consumer_w).  DR_MARCH_W_ORDER forces one order on every instance (parity build only: the side-by-side tests and A/Bs).
  int march_w_order = 2;
  int march_pdepth = 0;   // DR_MARCH_PDEPTH: loads each producer wave keeps in flight, 1..4 (0: by form; A/B hook)
  bool no_tap_prune = false, no_class_loop = false, no_pipe = false;  // DR_CONV_NO_TAP_PRUNE, DR_CONV_NO_CLASS_LOOP, DR_CONV_NO_PIPE (A/B)
  bool march_any_tile = false;  // DR_MARCH_ANY_TILE: tiles more than twice the layer as well -- the unit tests run the kernel on layers of a few rows
  bool fz_no_march = false;     // DR_FZ_NO_MARCH: the fused skip on the tile kernel only
};
inline ConvPolicy conv_policy() {
  ConvPolicy p;
  if (const char *e = getenv("DR_CONV_ASYNC")) p.async = atoi(e);
  if (const char *e = getenv("DR_CONV_MARCH")) p.march = atoi(e);
  if (const char *e = getenv("DR_CONV_ROWMARCH")) p.rowmarch = atoi(e);
  if (const char *e = getenv("DR_CONV_WINO")) p.wino = atoi(e);
  p.no_tuned = getenv("DR_CONV_NO_TUNED") != nullptr;
  p.bf3 = conv_bf3_policy();
  if (const char *e = hook_env("DR_DECONV_FORM")) p.deconv_form = std::max(0, std::min(2, atoi(e)));
  if (const char *e = hook_env("DR_MARCH_W_ORDER")) p.march_w_order = atoi(e) == 1 ? 1 : 2;
  if (const char *e = hook_env("DR_MARCH_PDEPTH")) p.march_pdepth = std::max(1, std::min(4, atoi(e)));
  p.no_tap_prune = hook_env("DR_CONV_NO_TAP_PRUNE") != nullptr;
  p.no_class_loop = hook_env("DR_CONV_NO_CLASS_LOOP") != nullptr;
  p.no_pipe = hook_env("DR_CONV_NO_PIPE") != nullptr;
  p.march_any_tile = hook_env("DR_MARCH_ANY_TILE") != nullptr;
  p.fz_no_march = hook_env("DR_FZ_NO_MARCH") != nullptr;
  return p;
}

struct MarchShape {  // derived geometry of a k_conv_m candidate
  int nup, npi, npo, ns, tyi, txi, np, ps, r, ncw;
  size_t wbytes, lds_bytes;
  long long steps;
  int grid;
  bool ok;
};
// rm (row march of a 2-D layer): KZ is the layer's kd (1), ntp the x taps of ONE row, nPD the images, nPH the rows; ty must be 1.
// wino (march_consumer_w; KZ = 3 only): ty counts row PAIRS, nPH the pairs of the layer, ntp the taps of one plane as the DIRECT form has them (3 rows x the x taps)
inline MarchShape march_shape(int KZ, int ntp, int Cin, int ci, int ct, int pt, int ty, int txt, int SX, int exy, int exx, int nPD, int nPH, int nPW, int CTtot,
                              bool rm = false, bool wino = false) {
  MarchShape m{};
  const int tpc = 16 / ci;
  if (Cin % ci || ntp % tpc || CTtot % ct || (ty * txt) % pt || (rm && (ty != 1 || KZ != 1)) || (wino && (KZ != 3 || rm || (ntp / 3) % tpc))) return m;
  m.ncw = ty * txt / pt;  // one wave per PT position tiles
  m.nup = ntp / tpc;      // (Winograd form: the same count -- three raw kernel rows per chunk of x taps)
  if (!conv_m_instance_exists(ci, m.nup, ct, pt, m.ncw, wino)) return m;
  const int npass = Cin / ci, kz = rm ? 3 : KZ;
  if (npass > 2) return m;
  m.npi = KZ == 1 ? npass : 1; m.npo = KZ == 1 ? 1 : npass; m.ns = kz * m.npi;
  m.tyi = rm ? 1 : (wino ? 2 * ty + 2 : ty - 1 + exy); m.txi = (txt * 16 - 1) * SX + exx; m.np = m.tyi * m.txi;
  if (m.np >= 65536) return m;
  m.ps = cdiv(((m.np + 15) & ~15) * (ci / 4), 128) * 128;
  if (m.ps / 128 > kMarchMaxIt) return m;
  m.wbytes = (size_t)m.ns * m.nup * ct * 1024;
  const size_t fixed = m.wbytes + kMarchFlagInts * 4;
  if (fixed >= kConvMaxLds) return m;
  // ring: the planes a step reads, plus what the producers may fetch ahead (rows are small: two whole rows ahead when they fit)
  const int rmin = kz == 3 ? 3 * m.npi : m.npi + 1, rmax = rm ? 5 * m.npi : (kz == 3 ? 4 : 2 * m.npi + 2);
  m.r = (int)std::min<size_t>(rmax, (kConvMaxLds - fixed) / ((size_t)m.ps * 16));
  if (m.r < rmin) return m;
  m.lds_bytes = (size_t)m.r * m.ps * 16 + fixed;
  m.steps = (long long)(rm ? 1 : cdiv(nPH, ty)) * cdiv(nPW, txt * 16) * nPD * (rm ? nPH : 1);
  const int split = CTtot / ct;
  m.grid = 8 * cdiv((int)std::min<long long>(m.steps, std::max(8, 256 / split)), 8);
  m.ok = true;
  return m;
}
// Winograd F(2,3) weight transform along one 3-tap axis: point p of (g0, g1, g2)
inline double conv_wino_g(int p, int k) {
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  return G[p][k];
}
inline size_t conv_a_slots(int np, int ci) { return (size_t)cdiv(((np + 1) & ~1) * (ci / 4), 512) * 512; }
inline unsigned short bf16_rne(float f) {  // round to nearest even, as v_cvt_pk_bf16_f32 does
  unsigned u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
inline float bf16_value(unsigned short h) {
  const unsigned u = (unsigned)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// tile shapes (tz, ty, txt) of the tile kernels: 16, 8 (k_conv_w with two position tiles per wave) and 4 position tiles per workgroup
inline constexpr int kConvTiles16[][3] = {{1, 1, 16}, {1, 2, 8}, {1, 4, 4}, {1, 8, 2}, {1, 16, 1}, {2, 1, 8}, {2, 2, 4},
                                          {2, 4, 2}, {2, 8, 1}, {4, 1, 4}, {4, 2, 2}, {4, 4, 1}, {8, 1, 2}, {8, 2, 1}, {16, 1, 1}};
inline constexpr int kConvTiles8[][3] = {{1, 1, 8}, {1, 2, 4}, {1, 4, 2}, {1, 8, 1}, {2, 1, 4}, {2, 2, 2}, {2, 4, 1}, {4, 1, 2}, {4, 2, 1}, {8, 1, 1}};
inline constexpr int kConvTiles4[][3] = {{1, 1, 4}, {1, 2, 2}, {1, 4, 1}, {2, 1, 2}, {2, 2, 1}, {4, 1, 1}};

struct ConvCand {  // one feasible plan: channel pass width, position tiles per wave, row tiles, tile shape, halo tile, family
  double cost;
  int ci, pt, ct, tz, ty, txt, tzi, tyi, txi;
  ConvFamily family;
};

// plan_conv's record: the call's inputs, what the steps share (classes, rows, CTtot, strides, paddings, extents, par_map), the candidates and the
// chosen one.  Every step is a member; plan_conv below is the list of them.
struct ConvPlanner {
  // ---- the call ----
  const ConvLayer &L;
  ConvMode mode;
  const float *in;
  int inD, inH, inW, inC;
  float *out;
  const float *add;
  int add_mode;
  const ConvFuse *fz;
  int in_split;
  ConvPolicy pol;
  bool bf3 = false;
  // ---- geometry(): shared by every step after it ----
  std::vector<DimTaps> cz, cy, cx;
  bool parity_layer = false;
  ConvPlanOut R;
  int rows = 0, rows_valid = 0, outWv = 0, outCv = 0;
  int npar = 1, par_map = 0;  // transposed: parity bits of the strided axes, enumerated (z, y, x) -> par_map holds 3 bits (z<<2|y<<1|x) per parity
  bool strided[3] = {false, false, false}, dense[3] = {false, false, false};  // dense: parity carried by the output rows
  int CTtot = 0, shifts = 1;
  // geometry shared by all parity classes: strides, padding, extents = union over classes
  int SZ = 1, SY = 1, SX = 1, PZ = 0, PY = 0, PX = 0;  // (a k_conv_w plan re-describes the y axis once it is chosen: winograd_y_axis)
  int nPD = 0, nPH = 0, nPW = 0;
  int exz = 0, exy = 0, exx = 0;
  struct Cls { const DimTaps *z, *y, *x; int ntaps; };
  std::vector<Cls> classes;
  int ncls = 0;
  // ---- candidates, rank() ----
  std::vector<ConvCand> cands;
  bool march_ok = false;
  int march_ntp = 0;  // k_conv_m: taps per input plane
  ConvCand k{};       // the chosen one
  int npass = 0, TPC = 0;
  bool wino = false, wino_raw = false;  // wino_raw: the marching kernel derives the transformed weights itself (raw rows g0, g1 / 2, g2)
  // ---- pack() ----
  std::vector<int> tapoff;
  std::vector<float> pk, sc, bi;
  std::vector<ConvClass> cls;
  double flops = 0;

  ConvPlanner(const ConvLayer &L_, ConvMode mode_, const float *in_, int inD_, int inH_, int inW_, int inC_, float *out_, const float *add_, int add_mode_,
              const ConvFuse *fz_, int in_split_)
      : L(L_), mode(mode_), in(in_), inD(inD_), inH(inH_), inW(inW_), inC(inC_), out(out_), add(add_), add_mode(add_mode_), fz(fz_), in_split(in_split_), pol(conv_policy()) {}
  ConvPlanner(const ConvPlanner &) = delete;  // (classes points into cz / cy / cx)

  // Checks the call and derives the layer's parity classes, row layout and the geometry every class shares.
  void geometry() {
    if (L.Cin % 4 != 0 || inC < L.Cin) fail(DR_ERR_ARG, "plan_conv: Cin=%d must be a multiple of 4 (tensor C=%d)", L.Cin, inC);
    const int form = L.transposed ? (pol.deconv_form >= 0 ? pol.deconv_form : (L.Cout >= 32 ? 2 : 1)) : 0;
    if (L.up2 && (L.up2 > 2 || L.transposed || L.kd != 1 || L.kh != 3 || L.kw != 3 || L.sd != 1 || L.sh != 1 || L.sw != 1 || mode != CONV_NORMAL))
      fail(DR_ERR_ARG, "plan_conv: up2 is a plain 3x3 stride-1 2-D layer over the upsampled input");
    cz = axis_classes(L.kd, L.sd, L.transposed, inD, form >= 1, !pol.no_tap_prune);
    cy = axis_classes(L.kh, L.sh, L.transposed, inH, form >= 1);
    cx = axis_classes(L.kw, L.sw, L.transposed, inW, form >= 2);
    if (L.up2) {  // one y parity per launch (a single class: the persistent kernels apply), both x parities as rows
      cy = {axis_classes_up2(inH, true)[L.up2 - 1]};
      cx = axis_classes_up2(inW, false);
    }
    parity_layer = L.transposed || L.up2;
    R.outD = L.transposed ? inD * L.sd : cz[0].npos;
    R.outH = L.transposed ? inH * L.sh : (L.up2 ? 2 * inH : cy[0].npos);
    R.outW = L.transposed ? inW * L.sw : (L.up2 ? 2 * inW : cx[0].npos);
    outWv = R.outW;
    if (mode == CONV_XPAIR) {
      if (L.transposed || L.sw != 1 || L.Cout != 8 || (R.outW & 1)) fail(DR_ERR_ARG, "XPAIR needs Cout=8, stride 1, even W");
      rows = 16; rows_valid = 16; outWv = R.outW / 2; outCv = 16;
    } else if (mode == CONV_X8) {
      if (L.transposed || L.sw != 1 || L.Cout != 1 || (R.outW & 7)) fail(DR_ERR_ARG, "X8 needs Cout=1, stride 1, W%%8==0");
      rows = 16; rows_valid = 8; outWv = R.outW / 8; outCv = 8;
    } else {
      rows = cdiv(L.Cout, 16) * 16; rows_valid = L.Cout; outCv = L.Cout;
      if (L.Cout % 4) fail(DR_ERR_ARG, "plan_conv: Cout=%d must be a multiple of 4", L.Cout);
    }
    strided[0] = L.transposed && L.sd == 2; strided[1] = (L.transposed && L.sh == 2) || L.up2; strided[2] = (L.transposed && L.sw == 2) || L.up2;
    dense[0] = strided[0] && form < 1; dense[1] = strided[1] && form < 1 && !L.up2; dense[2] = strided[2] && (L.up2 || form < 2);
    if (parity_layer) {
      if (mode != CONV_NORMAL) fail(DR_ERR_ARG, "plan_conv: transposed layers use CONV_NORMAL");
      for (int d = 0; d < 3; ++d) if (dense[d]) npar *= 2;
      for (int q = 0; q < npar; ++q) {
        int bits = 0, rem = q;
        for (int d = 2; d >= 0; --d) if (dense[d]) { bits |= (rem & 1) << (2 - d); rem >>= 1; }
        par_map |= bits << (3 * q);
      }
      rows_valid = npar * L.Cout; rows = cdiv(rows_valid, 16) * 16;
    }
    CTtot = rows / 16;
    shifts = mode == CONV_XPAIR ? 2 : (mode == CONV_X8 ? 8 : 1);
    if (shifts > 1) {  // widen the x taps: in = pos*shifts - pad + t', t' in [0, kw + shifts - 1)
      DimTaps &X = cx[0];
      X.t.clear(); X.off.clear();
      for (int t = 0; t < L.kw + shifts - 1; ++t) { X.t.push_back(t); X.off.push_back(t); }
      X.s = shifts; X.npos = outWv;
    }
    SZ = cz[0].s; SY = cy[0].s; SX = cx[0].s; PZ = cz[0].p; PY = cy[0].p; PX = cx[0].p;
    nPD = cz[0].npos; nPH = cy[0].npos; nPW = cx[0].npos;
    for (auto &c : cz) for (int o : c.off) exz = std::max(exz, o + 1);
    for (auto &c : cy) for (int o : c.off) exy = std::max(exy, o + 1);
    for (auto &c : cx) for (int o : c.off) exx = std::max(exx, o + 1);
    for (auto &Z : cz) for (auto &Y : cy) for (auto &X : cx) classes.push_back({&Z, &Y, &X, (int)(Z.t.size() * Y.t.size() * X.t.size())});
    ncls = (int)classes.size();
    bf3 = pol.bf3 && !fz && L.Cin % 8 == 0;  // (the Cin = 4 first layer and the fused-skip form stay on the fp32 kernels)
    if (in_split) {
      if (in_split != 16 || fz || bf3 || L.Cin % 16) fail(DR_ERR_ARG, "plan_conv: a split input has 16-channel sub-tensors and plain fp32 staging");
    }
  }

  // ---- plan: channel pass width CI, position tiles per wave PT, tile shape, output-row split; one generator per family, each with its cost model ----
  int async_policy() const { return (fz || bf3) ? 0 : pol.async; }
  // k_conv_a: 8 waves, 8*pt position tiles per workgroup, two tile buffers
  void cands_async() {
    if (!(async_policy() >= 1 && ncls == 1)) return;
    for (int ci : {16, 8, 4}) {
      if (in_split && ci != in_split) continue;  // a split input only has 16-channel passes
      if (L.Cin % ci || (ci == 4 && L.Cin != 4)) continue;
      const int npass = L.Cin / ci, tpc = 16 / ci, nu = cdiv(classes[0].ntaps, tpc);
      if (npass > 2 && (npass & 1)) continue;  // weight buffers alternate with the pass parity
      for (int pt : {1, 2, 4})
        for (int tz = 1; tz <= 8 * pt; tz *= 2)
          for (int ty = 1; tz * ty <= 8 * pt; ty *= 2) {
            const int txt = 8 * pt / (tz * ty);
            if ((tz > 1 && tz / 2 >= nPD) || (ty > 1 && ty / 2 >= nPH) || (txt > 1 && (txt / 2) * 16 >= nPW)) continue;  // more than half of the tile outside
            const int tzi = (tz - 1) * SZ + exz, tyi = (ty - 1) * SY + exy, txi = (txt * 16 - 1) * SX + exx;
            if ((size_t)tzi * tyi * txi >= 65536) continue;
            const double tiles = (double)cdiv(nPD, tz) * cdiv(nPH, ty) * cdiv(nPW, txt * 16);
            for (int ct : {2, 1}) {
              if (CTtot % ct || !conv_a_instance_exists(ci, ct, pt)) continue;
              const size_t slots = conv_a_slots(tzi * tyi * txi, ci);
              size_t bytes = 2 * slots * 16 + (size_t)npass * nu * ct * 1024 + (size_t)nu * tpc * 4 + 64;  // all passes' weights resident ...
              if (bytes > kConvMaxLds) bytes = 2 * slots * 16 + (size_t)std::min(npass, 2) * nu * ct * 1024 + (size_t)nu * tpc * 4 + 64;  // ... or two in flight
              if (bytes > kConvMaxLds) continue;
              const double wpc = bytes * 2 <= kConvMaxLds ? 2.0 : 1.0, split = CTtot / ct;
              const double mfma_unit = nu * 4.0 * ct * pt * 32.0 * 2.0;  // cycles per SIMD: two waves of the workgroup share it
              const double stage_unit = slots / 4.0;                    // ~64 B/clk/CU from L2
              const double unit = wpc * std::max(mfma_unit, stage_unit) + 700.0;
              // x 1.1: the two families' cost models are not calibrated against each other; an untuned shape only
              // moves to the persistent kernel when its model says so with some margin
              const double cost = 1.1 * std::ceil(tiles * split / (256.0 * wpc)) * npass * unit;
              cands.push_back({cost, ci, pt, ct, tz, ty, txt, tzi, tyi, txi, CONV_FAM_ASYNC});
            }
          }
    }
  }
  // k_conv_m: the stride-1 3x3 / 3x3x3 layers on the marching producer/consumer kernel (conv_march.h)
  // (a fused FeatureNet skip runs on it in exactly one form: 8-channel source, 32 -> 8 XPAIR 3x3 layer, producers compute the tile)
  void cands_march() {
    const bool march_fz_ok = !fz || (fz->cin == 8 && L.Cin == 32 && L.kd == 1 && mode == CONV_XPAIR && !pol.fz_no_march);
    const int march_policy = (march_fz_ok && !bf3) ? pol.march : 0;
    march_ok = march_policy >= 1 && ncls == 1 && !L.transposed && !L.up2 && mode != CONV_X8 && L.kh == 3 && L.kw == 3 && (L.kd == 1 || L.kd == 3) &&
               (int)cz[0].t.size() == L.kd &&  // (a depth axis with pruned taps -- extent 1 or 2 -- stays on the tile kernels)
               SZ == 1 && SY == 1 && L.sw == 1;
    march_ntp = march_ok ? 3 * (int)cx[0].t.size() : 0;
    if (!march_ok) return;
    for (int ci : {16, 8}) {
      if (in_split && ci != in_split) continue;  // a split input only has 16-channel passes
      if (ci == 8 && L.Cin != 8) continue;
      for (int ncw : {8, 12})
      for (int pt : {1, 2, 4})
        for (int ty = 1; ty <= ncw * pt; ++ty) {
          if ((ncw * pt) % ty) continue;
          const int txt = ncw * pt / ty;
          if ((ty > 1 && ty / 2 >= nPH) || (txt > 1 && (txt / 2) * 16 >= nPW)) continue;
          for (int ct : {2, 1}) {
            const MarchShape ms = march_shape(L.kd, march_ntp, L.Cin, ci, ct, pt, ty, txt, SX, exy, exx, nPD, nPH, nPW, CTtot);
            if (!ms.ok || (fz && (ci != 16 || ct != 1 || ncw != 8))) continue;
            const double spw = std::ceil((double)ms.steps / ms.grid);
            const double unit = ms.ns * ms.nup * 4.0 * ct * pt * 32.0 * (ncw / 4) * (ncw == 12 ? 0.94 : 1.0);  // MFMA cycles of a step per SIMD (ncw / 4 consumer waves each; three hide each other's gaps better)
            const double startup = (double)ms.lds_bytes / 16.0 + 3000.0;
            double cost = ms.npo * (spw * unit * 1.02 + startup);
            if (fz) cost *= 1.5;  // measured (r3): with a 3-slot ring and two channel passes per tile the fused-skip producers are the bottleneck (0.24 ms against k_conv's 0.214 at 480 x 640)
            else if (L.kd == 1) cost *= 1.6;  // 2-D layers: one step per tile, the whole halo per step -- measured 1.1-1.25x k_conv_a's time where the model says 0.6x (profiles/r03_experiments.txt, 8)
            if (march_policy >= 2) cost *= 1e-3;
            cands.push_back({cost, ci, pt, ct, 1, ty, txt, L.kd, ms.tyi, ms.txi, CONV_FAM_MARCH});
          }
        }
    }
  }
  // the Winograd form of the marching kernel: 3-D layers, even output height; ty counts row pairs
  void cands_winomarch() {
    const int wino_policy_m = (!fz && !bf3) ? pol.wino : 0;
    if (!(march_ok && wino_policy_m >= 1 && L.kd == 3 && (R.outH & 1) == 0 && R.outH >= 2)) return;
    const int nPHw = R.outH / 2;
    for (int ci : {16, 8}) {
      if (in_split && ci != in_split) continue;  // a split input only has 16-channel passes
      if (ci == 8 && L.Cin != 8) continue;
      for (int ncw : {8})
        for (int ty = 1; ty <= ncw; ++ty) {
          if (ncw % ty) continue;
          const int txt = ncw / ty;
          // (DR_MARCH_ANY_TILE, parity build: tiles more than twice the layer as well -- the unit tests run the kernel on layers of a few rows)
          if (!pol.march_any_tile && ((ty > 1 && ty / 2 >= nPHw) || (txt > 1 && (txt / 2) * 16 >= nPW))) continue;
          const MarchShape ms = march_shape(L.kd, march_ntp, L.Cin, ci, 1, 1, ty, txt, SX, exy, exx, nPD, nPHw, nPW, CTtot, false, true);
          if (!ms.ok) continue;
          const double spw = std::ceil((double)ms.steps / ms.grid);
          const double unit = ms.ns * (ms.nup / 3) * 16.0 * 32.0 * (ncw / 4) * (ncw == 12 ? 0.94 : 1.0);  // MFMA cycles of a step per SIMD: 16 per chunk of x taps and section
          const double startup = (double)ms.lds_bytes / 16.0 + 3000.0;
          double cost = ms.npo * (spw * unit * 1.1 + startup);
          if (wino_policy_m >= 2) cost *= 1e-3 * 0.5;  // (preferred: ahead of k_conv_w's candidates as well)
          cands.push_back({cost, ci, 1, 1, 1, ty, txt, L.kd, ms.tyi, ms.txi, CONV_FAM_WINOMARCH});
        }
    }
  }
  // the row march: 2-D 3x3 stride-1 layers on the same kernel, marching down the rows of each image
  void cands_rowmarch() {
    const bool rowmarch_ok = !fz && !bf3 && pol.rowmarch >= 1 && ncls == 1 && !L.transposed && !L.up2 && mode != CONV_X8 && L.kd == 1 && L.kh == 3 && L.kw == 3 &&
                             SZ == 1 && SY == 1 && L.sw == 1 && !add;
    if (!rowmarch_ok) return;
    const int row_ntp = (int)cx[0].t.size();  // x taps of one row
    for (int ci : {16, 8}) {
      if (in_split && ci != in_split) continue;  // a split input only has 16-channel passes
      if (ci == 8 && L.Cin != 8) continue;
      for (int ncw : {8, 10})
        for (int pt : {1, 2, 4}) {
          const int txt = ncw * pt;
          if (txt > 1 && (txt / 2) * 16 >= nPW) continue;
          for (int ct : {2, 1}) {
            const MarchShape ms = march_shape(L.kd, row_ntp, L.Cin, ci, ct, pt, 1, txt, SX, exy, exx, nPD, nPH, nPW, CTtot, true);
            if (!ms.ok) continue;
            const double spw = std::ceil((double)ms.steps / ms.grid);
            const double waste = (double)cdiv(nPW, txt * 16) * txt * 16 / nPW;  // strips hanging over the end of the row
            const double unit = ms.ns * ms.nup * 4.0 * ct * pt * 32.0 * (ncw / 4.0) + 300.0;  // MFMA cycles of a step per SIMD + the per-step bookkeeping
            const double startup = (double)ms.lds_bytes / 16.0 + 3000.0;
            double cost = (spw * unit * 1.02 + startup) * 1.5;  // measured 1.05-1.15x k_conv_a's time at 6-13 steps per workgroup: the model has no term for the ring fill
            (void)waste;
            if (pol.rowmarch >= 2) cost *= 1e-3;
            cands.push_back({cost, ci, pt, ct, 1, 1, txt, 1, 1, ms.txi, CONV_FAM_ROWMARCH});
          }
        }
    }
  }
  // k_conv_w: k_conv's launch form with the y axis in Winograd F(2,3) form (conv_wino.h).  A position tile is 16 x by one row PAIR:
  // to the tile geometry the layer has stride 2 and a 4-row kernel in y; a K chunk is 4 points x 4 MFMAs per (row tile, position tile).
  void cands_wino() {
    const int wino_policy = (!fz && !bf3) ? pol.wino : 0;
    const bool wino_ok = wino_policy >= 1 && ncls == 1 && !L.transposed && !L.up2 && mode != CONV_X8 && L.kh == 3 && L.sh == 1 && (R.outH & 1) == 0 && R.outH >= 2;
    if (!wino_ok) return;
    const int nPHw = R.outH / 2, ntw = (int)(cz[0].t.size() * cx[0].t.size());
    for (int ci : {16, 8}) {
      if (in_split && ci != in_split) continue;  // a split input only has 16-channel passes
      if (L.Cin % ci || (ci == 8 && L.Cin != 8)) continue;
      const int npass = L.Cin / ci, tpc = 16 / ci, nr = cdiv(ntw, tpc);
      for (int pt : {2, 1}) {
        const int (*cand)[3] = pt == 2 ? kConvTiles8 : kConvTiles4;
        const int ncand = pt == 2 ? 10 : 6;
        for (int k = 0; k < ncand; ++k) {
          const int *c = cand[k];
          if ((c[0] > 1 && c[0] / 2 >= nPD) || (c[1] > 1 && c[1] / 2 >= nPHw) || (c[2] > 1 && (c[2] / 2) * 16 >= nPW)) continue;  // more than half of the tile outside
          const int tzi = (c[0] - 1) * SZ + exz, tyi = (c[1] - 1) * 2 + 4, txi = (c[2] * 16 - 1) * SX + exx;
          if ((size_t)tzi * tyi * txi >= 65536) continue;
          const double tiles = (double)cdiv(nPD, c[0]) * cdiv(nPHw, c[1]) * cdiv(nPW, c[2] * 16);
          for (int ct : {2, 1}) {
            if (CTtot % ct || !conv_w_instance_exists(ci, ct, pt)) continue;
            const size_t bytes = (size_t)tzi * tyi * txi * (ci + 4) * 4 + (size_t)4 * nr * ct * 1024 + (size_t)4 * nr * tpc * 4 + 64;
            if (bytes > kConvMaxLds) continue;
            const int split = CTtot / ct;
            const double waves_simd = ct * pt == 1 ? 4.0 : (ct * pt == 2 ? 3.0 : 2.0);  // register budget of the instance
            const double wg_per_cu = std::max(1.0, std::min({(double)(kConvMaxLds / bytes), waves_simd}));
            const double stage = npass * (((double)tzi * tyi * txi * (ci / 4) + 4.0 * nr * ct * 64.0) / 256.0 * 60.0 + 900.0);
            const double chunk_mfma = 16.0 * ct * pt * 32.0;
            const double n_wg = tiles * split;
            const double mfma_total = n_wg * npass * nr * chunk_mfma, stage_total = n_wg * stage;
            const double lat_wg = npass * nr * chunk_mfma + stage;
            const double waves = std::ceil(n_wg / (256.0 * wg_per_cu));
            const double thr = (mfma_total + stage_total) / 256.0 / (wg_per_cu >= 2 ? 0.8 : 0.5);
            // measured (r4, profiles/r04_winograd.txt): 14-17 % faster than the best direct plan on every 2-D 3x3 layer of both tuned shapes, 5-7 % on the
            // 16- to 64-channel 3-D layers, slower than the marching kernel on the conv0 layers.  The model below overstates the gain (it has no term
            // for the smaller tiles' halo), so an untuned shape moves here with a margin, and a 3-D layer only when a tuned row says so.
            double cost = std::max(thr, waves * lat_wg) * (L.kd == 1 ? 1.25 : 2.5);
            if (wino_policy >= 2) cost *= 1e-3;
            cands.push_back({cost, ci, pt, ct, c[0], c[1], c[2], tzi, tyi, txi, CONV_FAM_WINO});
          }
        }
      }
    }
  }
  // k_conv (and its bf16 x 3 form): every layer; with DR_CONV_ASYNC=1 only where no other family produced a candidate
  void cands_tile() {
    const bool sync_too = async_policy() != 1 || cands.empty();
    if (!sync_too) return;
    for (int ci : {16, 8, 4}) {
      if (in_split && ci != in_split) continue;  // a split input only has 16-channel passes
      if (L.Cin % ci || (ci == 4 && L.Cin != 4)) continue;
      if (fz && ci != 16) continue;  // fused-skip instances exist for 16-channel passes, one row tile
      const int npass = L.Cin / ci, tpc = (bf3 ? 32 : 16) / ci, wkb = bf3 ? 2048 : 1024;  // taps and weight bytes per K chunk (and 16 output rows)
      double chunks = 0;  // K chunks per pass summed over classes
      for (auto &c : classes) chunks += cdiv(c.ntaps, tpc);
      for (int pt : {4, 1}) {
        const int (*cand)[3] = pt == 4 ? kConvTiles16 : kConvTiles4;
        const int ncand = pt == 4 ? 15 : 6;
        for (int k = 0; k < ncand; ++k) {
          const int *c = cand[k];
          const int tzi = (c[0] - 1) * SZ + exz, tyi = (c[1] - 1) * SY + exy, txi = (c[2] * 16 - 1) * SX + exx;
          int nu_max = 0;
          for (auto &cc : classes) nu_max = std::max(nu_max, cdiv(cc.ntaps, tpc));
          const double tiles = (double)cdiv(nPD, c[0]) * cdiv(nPH, c[1]) * cdiv(nPW, c[2] * 16);
          for (int ct : {4, 2, 1}) {
            if (CTtot % ct || !(bf3 ? conv_b_instance_exists(ci, ct, pt) : conv_instance_exists(ci, ct, pt)) || (fz && ct != 1)) continue;
            const size_t bytes = (size_t)tzi * tyi * txi * (ci + 4) * 4 + (size_t)nu_max * ct * wkb + (size_t)nu_max * tpc * 4 + 64;
            if (bytes > kConvMaxLds) continue;
            const int split = CTtot / ct;
            // cost model (cycles): MFMA issue, staging, and a latency floor per chunk; see DESIGN.md
            const double wg_per_cu = std::max(1.0, std::min({(double)(kConvMaxLds / bytes), 8.0, (ct == 4 && pt == 4) ? 5.0 : 8.0}));
            const double stage = npass * (((double)tzi * tyi * txi * (ci / 4) + (chunks / ncls) * ct * 64.0) / 256.0 * 60.0 + 900.0);
            const double chunk_mfma = bf3 ? 3.0 * ct * pt * 16.0 : 4.0 * ct * pt * 32.0;  // (bf3: three 16-cycle MFMAs per 32-wide chunk)
            const double n_wg = tiles * split;  // per class
            const double mfma_total = n_wg * npass * chunks * chunk_mfma, stage_total = n_wg * ncls * stage;
            const double lat_wg = npass * (chunks / ncls) * std::max(chunk_mfma, 160.0) + stage;
            const double waves = std::ceil(n_wg * ncls / (256.0 * wg_per_cu));
            const double thr = (mfma_total + stage_total) / 256.0 / (wg_per_cu >= 2 ? 0.8 : 0.5);
            const double cost = std::max(thr, waves * lat_wg);
            cands.push_back({cost, ci, pt, ct, c[0], c[1], c[2], tzi, tyi, txi, CONV_FAM_TILE});
          }
        }
      }
    }
  }

  // the generation order is part of the ranking (the sort is stable), and the ranks are public: DR_CONV_RANK, the autotuner
  void candidates() {
    cands_async();
    cands_march();
    cands_winomarch();
    cands_rowmarch();
    cands_wino();
    cands_tile();
  }

  // Ranks the candidates (stable: equal costs keep their generation order), applies the tuned table and picks candidate `rank` (clamped).
  void choose(int rank) {
    if (cands.empty()) fail(DR_ERR_ARG, "plan_conv: no kernel instance / tile shape for Cin=%d Cout=%d", L.Cin, L.Cout);
    std::stable_sort(cands.begin(), cands.end(), [](const ConvCand &a, const ConvCand &b) { return a.cost < b.cost; });
    if (!pol.no_tuned) {  // a measured plan for exactly this layer swaps places with the cost model's first choice -- for EVERY rank, so that the
                          // ranks stay a permutation of the candidates (the autotuner used to never time the model's own first choice of a tuned layer)
      for (const ConvTuned &t : kConvTuned) {
        if (t.Cin != L.Cin || t.Cout != L.Cout || t.kd != L.kd || t.kh != L.kh || t.kw != L.kw || t.sd != L.sd || t.sh != L.sh || t.sw != L.sw ||
            t.transposed != (L.transposed ? 1 : (L.up2 ? 1 + L.up2 : 0)) || t.mode != (int)mode + (in_split ? 16 : 0) || t.inD != inD || t.inH != inH || t.inW != inW) continue;
        for (size_t i = 0; i < cands.size(); ++i) {
          const ConvCand &c = cands[i];
          if (c.ci == t.ci && c.ct == t.ct && c.pt == t.pt && c.tz == t.tz && c.ty == t.ty && c.txt == t.txt && (int)c.family == t.async_) { std::swap(cands[0], cands[i]); break; }
        }
        break;
      }
    }
    k = cands[std::min<size_t>(rank < 0 ? 0 : rank, cands.size() - 1)];
    R.ncand = (int)cands.size();
    npass = L.Cin / k.ci; TPC = (bf3 ? 32 : 16) / k.ci;
    wino = k.family == CONV_FAM_WINO || k.family == CONV_FAM_WINOMARCH; wino_raw = k.family == CONV_FAM_WINOMARCH;
    if (wino) {  // the y axis as k_conv_w sees it: positions are row pairs, the tap table carries row 0 only (the kernel adds rows 1..3 itself)
      DimTaps &Y = cy[0];
      Y.t = {0}; Y.off = {0}; Y.s = 2; Y.p = 1; Y.om = 2; Y.oo = 0; Y.npos = R.outH / 2;
      SY = 2; PY = 1; nPH = Y.npos;
      classes[0].ntaps = (int)(cz[0].t.size() * cx[0].t.size());
    }
  }

  float weight_at(int co, int ci, int tz, int ty, int tx) const {
    if (!L.transposed) return L.weight[((((size_t)co * L.Cin + ci) * L.kd + tz) * L.kh + ty) * L.kw + tx];
    return L.weight[((((size_t)ci * L.Cout + co) * L.kd + tz) * L.kh + ty) * L.kw + tx];
  }
  struct ClassTaps { std::vector<int> tz, ty, tx; };  // kernel index per axis of each tap of a class
  // the weight that multiplies input channel `cin` of tap `tap` of class `c` for output row `row` (ky >= 0: that kernel row instead of the tap's)
  float weight_of(const Cls &c, const ClassTaps &T, int tap, int cin, int row, int ky = -1) const {
    const DimTaps &Z = *c.z, &Y = *c.y, &X = *c.x;
    float v = 0.f;
    if (tap < c.ntaps && row < rows_valid) {
      if (L.up2) {  // sum of the kernel entries that fall on this (parity, input offset) pair, per axis
        const int q = row / L.Cout, co = row % L.Cout, bits = (par_map >> (3 * q)) & 7;
        int ky[2], kx[2];
        const int ny = up2_kernel_set(Y.par, T.ty[tap], ky), nx = up2_kernel_set(bits & 1, T.tx[tap], kx);
        double acc = 0;
        for (int iy = 0; iy < ny; ++iy) for (int ix = 0; ix < nx; ++ix) acc += weight_at(co, cin, 0, ky[iy], kx[ix]);
        v = (float)acc;
      } else if (L.transposed) {
        const int q = row / L.Cout, co = row % L.Cout, bits = (par_map >> (3 * q)) & 7;
        const int offs[3] = {T.tz[tap], T.ty[tap], T.tx[tap]};  // for transposed layers DimTaps::t carries the input offset
        int kk[3];
        bool ok = true;
        const int cpar[3] = {Z.par, Y.par, X.par};
        for (int d = 0; d < 3; ++d) {
          if (strided[d]) kk[d] = parity_kernel_index(dense[d] ? (bits >> (2 - d)) & 1 : cpar[d], offs[d]);
          else kk[d] = offs[d];  // stride-1 axis: DimTaps::t is the kernel index already (k == 1 or the 3-tap flip)
          ok = ok && kk[d] >= 0;
        }
        if (ok) v = weight_at(co, cin, kk[0], kk[1], kk[2]);
      } else if (mode == CONV_NORMAL) v = weight_at(row, cin, T.tz[tap], ky >= 0 ? ky : T.ty[tap], T.tx[tap]);
      else {
        const int shift = mode == CONV_XPAIR ? (row >> 3) : row, co = mode == CONV_XPAIR ? (row & 7) : 0;
        const int kx = T.tx[tap] - shift;
        if (kx >= 0 && kx < L.kw) v = weight_at(co, cin, T.tz[tap], ky >= 0 ? ky : T.ty[tap], kx);
      }
    }
    return v;
  }
  // The fp32 layouts are [pass][chunk of taps][sub-chunk][row tile][lane] x 4: one sub-chunk (the plain form), the four Winograd points of k_conv_w
  // (u_p = sum_ky G[p][ky] w[ky], formed in double, rounded once) or the three raw kernel rows g0, g1 / 2, g2 of the marching Winograd form
  // (march_consumer_w forms u1, u2 from them).  Lane (i = l & 15, g = l >> 4) holds K = 16 u + 4 g .. + 3 of row 16 ct + i.
  void pack_class_fp32(const Cls &c, const ClassTaps &T, int NR, size_t w0) {
    const int CI = k.ci, sub = wino_raw ? 3 : (wino ? 4 : 1), NU = sub * NR;
    for (int p = 0; p < npass; ++p) for (int u = 0; u < NR; ++u) for (int s4 = 0; s4 < sub; ++s4) for (int ct = 0; ct < CTtot; ++ct)
      for (int l = 0; l < 64; ++l) for (int s = 0; s < 4; ++s) {
        const int g = l >> 4, i = l & 15, k16 = 4 * g + s;
        const int tap = u * TPC + k16 / CI, cin = p * CI + k16 % CI, row = ct * 16 + i;
        float v;
        if (wino_raw) v = (s4 == 1 ? 0.5f : 1.f) * weight_of(c, T, tap, cin, row, s4);
        else if (wino) {
          double a = 0;
          for (int ky = 0; ky < 3; ++ky) a += conv_wino_g(s4, ky) * (double)weight_of(c, T, tap, cin, row, ky);
          v = (float)a;
        } else v = weight_of(c, T, tap, cin, row);
        pk[w0 + ((((size_t)p * NU + u * sub + s4) * CTtot + ct) * 64 + l) * 4 + s] = v;
      }
  }
  // [pass][chunk][row tile][hi | lo][lane] x 8 bf16: lane (i = l & 15, g = l >> 4) holds K = 32 u + 8 g .. + 7 of row 16 ct + i
  void pack_class_bf3(const Cls &c, const ClassTaps &T, int NU, size_t w0) {
    const int CI = k.ci;
    unsigned short *pb = reinterpret_cast<unsigned short *>(pk.data() + w0);
    for (int p = 0; p < npass; ++p) for (int u = 0; u < NU; ++u) for (int ct = 0; ct < CTtot; ++ct)
      for (int l = 0; l < 64; ++l) for (int s = 0; s < 8; ++s) {
        const int g = l >> 4, i = l & 15, k32 = 8 * g + s;
        const float v = weight_of(c, T, u * TPC + k32 / CI, p * CI + k32 % CI, ct * 16 + i);
        const unsigned short hi = bf16_rne(v), lo = bf16_rne(v - bf16_value(hi));
        const size_t frag = (((size_t)p * NU + u) * CTtot + ct) * 2;
        pb[((frag + 0) * 64 + l) * 8 + s] = hi;
        pb[((frag + 1) * 64 + l) * 8 + s] = lo;
      }
  }
  // The per-row epilogue affine, and class after class the tap tables (LDS position offsets) and packed weights.
  void pack() {
    sc.assign(rows, 1.f); bi.assign(rows, 0.f);
    for (int r = 0; r < rows_valid; ++r) {
      const int c = parity_layer ? r % L.Cout : (mode == CONV_NORMAL ? r : (mode == CONV_XPAIR ? (r & 7) : 0));
      if (!L.scale.empty()) sc[r] = L.scale[c];
      if (!L.bias.empty()) bi[r] = L.bias[c];
    }
    cls.resize(ncls);
    for (int ic = 0; ic < ncls; ++ic) {
      const DimTaps &Z = *classes[ic].z, &Y = *classes[ic].y, &X = *classes[ic].x;
      const int ntz = (int)Z.t.size(), nty = (int)Y.t.size(), ntx = (int)X.t.size(), ntaps = classes[ic].ntaps;
      const int NR = cdiv(ntaps, TPC), NU = wino_raw ? 3 * NR : (wino ? 4 * NR : NR);  // k_conv_w: four weight chunks (one per Winograd point) per chunk of taps; marching form: three (the raw kernel rows)
      cls[ic].NU = NU; cls[ic].tap_base = (int)tapoff.size(); cls[ic].w_base = (int)(pk.size() / 4);
      cls[ic].ooz = Z.oo; cls[ic].ooy = Y.oo; cls[ic].oox = X.oo;
      ClassTaps T;
      T.tz.resize(ntaps); T.ty.resize(ntaps); T.tx.resize(ntaps);
      const size_t t0 = tapoff.size();
      tapoff.resize(t0 + (size_t)NR * TPC, 0);
      {
        int n = 0;
        for (int iz = 0; iz < ntz; ++iz) for (int iy = 0; iy < nty; ++iy) for (int ix = 0; ix < ntx; ++ix, ++n) {
          tapoff[t0 + n] = (Z.off[iz] * k.tyi + Y.off[iy]) * k.txi + X.off[ix];
          T.tz[n] = Z.t[iz]; T.ty[n] = Y.t[iy]; T.tx[n] = X.t[ix];
        }
      }
      const size_t w0 = pk.size();
      pk.resize(w0 + (size_t)npass * NU * CTtot * 64 * 4 * (bf3 ? 2 : 1), 0.f);
      if (bf3) pack_class_bf3(classes[ic], T, NU, w0);
      else pack_class_fp32(classes[ic], T, NR, w0);
      if (L.up2) flops += ic == 0 ? 2.0 * nPD * nPH * nPW * 16.0 * L.Cin * L.Cout : 0.0;  // 4 output pixels x (2 x 2 input pixels) per input position
      else if (L.transposed) flops += ic == 0 ? 2.0 * nPD * nPH * nPW * (double)L.kd * L.kh * L.kw * L.Cin * L.Cout : 0.0;
      else flops += 2.0 * nPD * (wino ? 2 * nPH : nPH) * nPW * (mode == CONV_NORMAL ? 1 : shifts) * (double)ntz * (wino ? 3 : nty) * (mode == CONV_NORMAL ? ntx : L.kw) * L.Cin * L.Cout;  // (algorithmic: the direct form's)
    }
  }

  // Uploads the packed arrays and fills the kernel arguments; the launch it leaves is k_conv's plain form (one workgroup per tile and class).
  template <class Arena>
  void fill_args(ConvLaunch &cl, Arena &arena) {
    const int CI = k.ci, CT = k.ct, TZ = k.tz, TY = k.ty, TXT = k.txt, TZI = k.tzi, TYI = k.tyi, TXI = k.txi, CIS = CI + 4;
    ConvArgs &a = cl.args;
    a.in = in; a.out = out; a.wpk = reinterpret_cast<const float4 *>(arena.upload(pk));
    a.scale = arena.upload(sc); a.bias = arena.upload(bi); a.add = add; a.tapoff = arena.upload(tapoff);
    a.cls = arena.upload(cls);
    a.inD = inD; a.inH = inH; a.inW = inW; a.inC = in_split ? in_split : inC;
    a.pass_stride = in_split ? (int)((size_t)inD * inH * inW * in_split) : CI;
    if (in_split && (size_t)inD * inH * inW * in_split >= (1ull << 31)) fail(DR_ERR_ARG, "plan_conv: split input too large");
    a.outD = R.outD; a.outH = R.outH + 2 * L.out_pad; a.outW = outWv; a.outC = outCv;
    if (L.out_pad) {  // bordered output: only the strides change (the x border is a whole number of XPAIR / X8 output groups or the mode is refused)
      if ((2 * L.out_pad) % shifts) fail(DR_ERR_ARG, "plan_conv: an output border of %d pixels does not fit the %d-wide output groups", L.out_pad, shifts);
      a.outW = outWv + 2 * L.out_pad / shifts;
    }
    a.nPD = nPD; a.nPH = nPH; a.nPW = nPW;
    a.sz = SZ; a.sy = SY; a.sx = SX; a.pz = PZ; a.py = PY; a.px = PX;
    a.omz = cz[0].om; a.omy = cy[0].om; a.omx = cx[0].om;
    a.par_rows = parity_layer ? L.Cout : 0; a.par_map = par_map;
    a.TZ = TZ; a.TY = TY; a.TXT = TXT; a.TZI = TZI; a.TYI = TYI; a.TXI = TXI;
    a.magicX = TXI == 1 ? 0u : (unsigned)((0x100000000ull + TXI - 1) / TXI);
    a.magicY = TYI == 1 ? 0u : (unsigned)((0x100000000ull + TYI - 1) / TYI);
    if ((size_t)TZI * TYI * TXI >= 65536) fail(DR_ERR_ARG, "plan_conv: halo tile too large");
    a.npass = npass; a.ctTot = CTtot; a.rows_valid = rows_valid; a.relu = L.relu ? 1 : 0;
    a.add_mode = add ? add_mode : 0;
    a.addH = R.outH / 2; a.addW = (mode == CONV_NORMAL ? R.outW : outWv) / 2;
    a.tilesD = cdiv(nPD, TZ); a.tilesH = cdiv(nPH, TY); a.tilesW = cdiv(nPW, TXT * 16);
    cl.ci = CI; cl.ct = CT; cl.pt = k.pt;
    a.fz_x = a.fz_w = a.fz_b = a.fz_coarse = nullptr;
    if (fz) {
      if (fz->cin != 8 || L.transposed || SZ != 1 || SY != 1) fail(DR_ERR_ARG, "plan_conv: fused skip needs an 8-channel source and a stride-1 layer");
      a.fz_x = fz->x; a.fz_w = fz->w; a.fz_b = fz->b; a.fz_coarse = fz->coarse; cl.fz = fz->cin;
    }
    cl.grid = dim3(8 * cdiv(a.tilesD * a.tilesH * a.tilesW, 8), ncls, CTtot / CT);
    int nu_max = 0;
    for (auto &c : cls) nu_max = std::max(nu_max, c.NU);
    a.nuMax = nu_max;
    cl.lds_bytes = (size_t)TZI * TYI * TXI * CIS * 4 + (size_t)nu_max * CT * (bf3 ? 2048 : 1024) + (size_t)nu_max * TPC * 4 + 64;
    cl.bf3 = bf3 ? 1 : 0;
    a.zero16 = nullptr; a.a_slots = 0; a.a_wbufs = 1; a.class_loop = 0;
    cl.flops = flops;
  }

  // The tile kernels (k_conv, k_conv_b, k_conv_w): k_conv's class loop and pipelined passes where they apply.
  void finish_tile(ConvLaunch &cl) const {
    const int CI = k.ci, CT = k.ct, PT = k.pt, nu_max = cl.args.nuMax;
    ConvArgs &a = cl.args;
    const bool plain = k.family == CONV_FAM_TILE && !bf3 && !fz;
    // k_conv's class loop (see the kernel): single-pass layers with several parity classes, both weight buffers and every class's tap table next to the tile
    if (plain && ncls > 1 && npass == 1 && conv_c_instance_exists(CI, CT, PT) && !pol.no_class_loop) {
      const size_t with_loop = cl.lds_bytes + (size_t)nu_max * CT * 1024 + (size_t)(ncls - 1) * nu_max * TPC * 4;
      if (with_loop <= kConvMaxLds) {
        a.class_loop = ncls;
        cl.lds_bytes = with_loop;
        cl.grid.y = 1;
      }
    }
    // k_conv with pipelined passes (see the kernel): small multi-pass layers on the one-position-tile instances whose tile is at most 6 loads per lane
    if (plain && PT == 1 && CT <= 2 && npass >= 2 && (size_t)k.tzi * k.tyi * k.txi * (CI / 4) <= 6 * kConvThreads && !pol.no_pipe &&
        cl.lds_bytes + (size_t)nu_max * CT * 1024 <= kConvMaxLds) {
      a.a_wbufs = 2;
      cl.lds_bytes += (size_t)nu_max * CT * 1024;
    }
    if (k.family == CONV_FAM_WINO) cl.async = 4;  // (k_conv's LDS layout and grid: the tile, nuMax weight chunks, the tap table)
  }
  // k_conv_a: two tile buffers, the passes' weights resident or two in flight, a persistent grid
  template <class Arena>
  void finish_async(ConvLaunch &cl, Arena &arena) const {
    const int CI = k.ci, CT = k.ct, nu_max = cl.args.nuMax;
    ConvArgs &a = cl.args;
    cl.async = 1;
    a.zero16 = arena.upload(std::vector<float>(4, 0.f));
    a.a_slots = (int)conv_a_slots(k.tzi * k.tyi * k.txi, CI);
    a.a_wbufs = npass;
    cl.lds_bytes = 2 * (size_t)a.a_slots * 16 + (size_t)a.a_wbufs * nu_max * CT * 1024 + (size_t)nu_max * TPC * 4 + 64;
    if (cl.lds_bytes > kConvMaxLds) {  // the passes' weights do not all fit next to the two tile buffers: two buffers, re-fetched per pass
      a.a_wbufs = std::min(npass, 2);
      cl.lds_bytes = 2 * (size_t)a.a_slots * 16 + (size_t)a.a_wbufs * nu_max * CT * 1024 + (size_t)nu_max * TPC * 4 + 64;
    }
    const int ntiles = a.tilesD * a.tilesH * a.tilesW, split = CTtot / CT;
    const int wpc = cl.lds_bytes * 2 <= kConvMaxLds ? 2 : 1;
    const int want = std::max(1, std::min(ntiles, 256 * wpc / split));
    cl.grid = dim3(8 * cdiv(want, 8), 1, split);
  }
  // k_conv_m in its three forms (march, row march, Winograd march): the in-plane tap table and MarchArgs
  template <class Arena>
  void finish_march(ConvLaunch &cl, Arena &arena) const {
    const int CI = k.ci, CT = k.ct, PT = k.pt, TY = k.ty, TXT = k.txt, TXI = k.txi;
    ConvArgs &a = cl.args;
    const bool rm = k.family == CONV_FAM_ROWMARCH;
    const MarchShape ms = rm ? march_shape(L.kd, (int)cx[0].t.size(), L.Cin, CI, CT, PT, 1, TXT, SX, exy, exx, nPD, nPH, nPW, CTtot, true)
                             : march_shape(L.kd, march_ntp, L.Cin, CI, CT, PT, TY, TXT, SX, exy, exx, nPD, nPH, nPW, CTtot, false, wino_raw);
    if (!ms.ok) fail(DR_ERR_ARG, "plan_conv: inconsistent k_conv_m plan");
    cl.async = 2; cl.nup = ms.nup; cl.ncw = ms.ncw;
    a.zero16 = arena.upload(std::vector<float>(4, 0.f));
    a.a_slots = 0; a.a_wbufs = 0;
    MarchArgs &m = cl.march;
    const int kz = rm ? 3 : L.kd;
    std::vector<int> tap2d((size_t)ms.nup * TPC, 0);
    {
      const DimTaps &Y = *classes[0].y, &X = *classes[0].x;
      int n = 0;
      if (rm) for (size_t ix = 0; ix < X.t.size(); ++ix, ++n) tap2d[n] = X.off[ix];  // the y taps are the sections of the step
      else for (size_t iy = 0; iy < Y.t.size(); ++iy) for (size_t ix = 0; ix < X.t.size(); ++ix, ++n) tap2d[n] = Y.off[iy] * TXI + X.off[ix];
    }
    m.tap2d = arena.upload(tap2d);
    m.geo.KZ = kz; m.geo.NPI = ms.npi; m.geo.Dc = rm ? nPH : (L.kd == 3 ? nPD : 1);
    m.NPO = ms.npo;
    m.colsH = rm ? 1 : cdiv(nPH, TY); m.colsW = cdiv(nPW, TXT * 16);
    m.ncols = (L.kd == 3 ? 1 : nPD) * m.colsH * m.colsW;
    m.R = ms.r; m.PS = ms.ps; m.NP = ms.np; m.nit = ms.ps / 128;
    m.wsec = ms.nup * CT * 64; m.NU = kz * ms.nup;
    m.steps = (int)ms.steps;
    m.ncw = ms.ncw;
    m.rm = rm ? 1 : 0;
    m.wino = wino_raw ? pol.march_w_order : 0;
    const long long iplane = (long long)a.inH * a.inW * a.inC, oplane = (long long)a.outH * a.outW * a.outC;
    if (iplane * std::max(1, a.inD) >= (1ll << 31) || oplane * std::max(1, a.outD) >= (1ll << 31)) fail(DR_ERR_ARG, "plan_conv: tensor too large for k_conv_m's 32-bit strides");
    m.i_sv = L.kd == 3 ? 0 : (int)iplane; m.i_sz = rm ? a.inW * a.inC : (L.kd == 3 ? (int)iplane : 0); m.i_sy = rm ? 0 : a.inW * a.inC;
    m.o_sv = L.kd == 3 ? 0 : (int)oplane; m.o_sz = rm ? a.outW * a.outC : (L.kd == 3 ? (int)oplane : 0); m.o_sy = rm ? 0 : a.outW * a.outC;
    m.inHp = rm ? 1 : a.inH;
    m.err = arena.err_flag;
    m.depth = rm ? 3 : 2;  // loads each producer wave keeps in flight (rows are small and steps short: one more)
    if (pol.march_pdepth) m.depth = pol.march_pdepth;  // A/B hook
    cl.lds_bytes = ms.lds_bytes;
    cl.grid = dim3(ms.grid, 1, CTtot / CT);
  }
};

// in_split: 0 = the input is one (D,H,W,inC) tensor; 16 = it is stored as inC / 16 consecutive (D,H,W,16) sub-tensors (only 16-channel passes apply;
// a tuned row of such a layer carries mode + 16: plans measured in one layout are never applied to the other)
// rank: which candidate of the cost model's ranking to build (0 = its choice); used by the engine's autotuner
template <class Arena>
inline ConvPlanOut plan_conv(const ConvLayer &L, ConvMode mode, const float *in, int inD, int inH, int inW, int inC,
                             float *out, const float *add, int add_mode, Arena &arena, int rank = 0, const ConvFuse *fz = nullptr, int in_split = 0) {
  ConvPlanner P(L, mode, in, inD, inH, inW, inC, out, add, add_mode, fz, in_split);
  P.geometry();
  P.candidates();
  P.choose(rank);
  P.pack();
  ConvLaunch cl{};
  P.fill_args(cl, arena);
  switch (P.k.family) {
    case CONV_FAM_TILE: case CONV_FAM_WINO: P.finish_tile(cl); break;
    case CONV_FAM_ASYNC: P.finish_async(cl, arena); break;
    default: P.finish_march(cl, arena); break;
  }
  P.R.launches.push_back(cl);
  return std::move(P.R);
}

}  // namespace dr
