// conv_mfma.h -- the convolution kernels of the depth pipeline: a tap-table implicit GEMM on
// the fp32 matrix cores of gfx950 (v_mfma_f32_16x16x4_f32, exact fp32 == an fmaf chain), in two launch forms that
// share operand mapping, packed weights, tap tables and epilogue:
//   k_conv<CI,CT,PT,FZ>  4 waves, one tile per workgroup, register-staged halo tile (FZ = 8: the staging step computes
//                        FeatureNet's skip.stage3 + upsample instead of copying a tensor);
//   k_conv_a<CI,CT,PT>   8 waves, persistent over (tile, channel pass) units, halo tiles streamed into a second LDS
//                        buffer by LDS-DMA (global_load_lds_dwordx4) under the K loop of the current unit.
//
// It replaces every dense contraction the reference hands to cuDNN through ATen
// (FeatureNet.forward cva_mvsnet/models/module.py:496-531, CostRegNet.forward module.py:577-600):
// Conv2d 3x3 / 5x5-stride-2 / 1x1, Conv3d 3^3 (stride 1, 2, (1,2,2)) and ConvTranspose3d 3^3
// stride 2 (as ONE stride-1 conv with 8*Cout parity rows), with the eval-mode BatchNorm folded into a per-channel
// scale/bias, ReLU, the UNet residual adds and FeatureNet's nearest-upsample-add fused in the epilogue.
//
// Data layout: channels-last everywhere, tensor = (D|V, H, W, C) fp32.
//
// GEMM mapping (one wave = 64 lanes):
//   A (16 x 4)  = weights : row i = output row (channel), 4 K-values        -> lane (i = l&15, g = l>>4)
//   B (4 x 16)  = inputs  : col j = output position (16 consecutive along W) -> lane (j = l&15, g = l>>4)
//   D (16 x 16) : lane holds rows 4g..4g+3 of column j  => one float4 channels-last store per lane.
// K is the flattened (tap, cin) axis, walked in chunks of 16: each lane fetches ONE float4 (4
// consecutive cin of "its" tap) from the LDS-staged input tile and ONE float4 of pre-packed weights,
// and feeds four back-to-back MFMAs (k-order inside the dot product is free, so lane-group g owns
// K = 16q+4g .. +3).  Taps are a runtime table of LDS offsets, which is what lets the same kernel do
// strided convs, transposed convs (dense parity rows) and the two "shifted-weights" modes:
//   XPAIR: a Cout=8 layer is run as a stride-(1,1,2) conv with a 4-wide kernel and 16 output rows
//          (8 channels x 2 adjacent x) on the output viewed as (D,H,W/2,16): 75 % MFMA row use, not 50 %.
//   X8   : the Cout=1 `prob` layer is run as 8 x-shifts per column on the output viewed as (D,H,W/8,8).
#pragma once
#include <algorithm>
#include <atomic>
#include <functional>

#include "dr_common.h"
#include "conv_plan.h"  // the host half: ConvArgs / ConvLaunch, the instance lists, the planner (plain C++, tested on the CPU)

namespace dr {

typedef float floatx4 __attribute__((ext_vector_type(4)));

// ---- epilogue: folded BN, ReLU, residual / upsample add, one float4 (4 channels) per lane ----
template <int CT>
__device__ inline void conv_load_affine(const ConvArgs &a, int g, int ct0, float4 (&sc)[CT], float4 (&bi)[CT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {  // scale / bias are padded to whole 16-row tiles on the host
    sc[ct] = *reinterpret_cast<const float4 *>(a.scale + (ct0 + ct) * 16 + 4 * g);
    bi[ct] = *reinterpret_cast<const float4 *>(a.bias + (ct0 + ct) * 16 + 4 * g);
  }
}
// The residual / upsample-add operand is FETCHED FOR A GROUP OF UP TO FOUR (position tile, row tile) entries before the first store of the
// group: `add` and `out` may alias (the folded stage-3 head adds in place), so hipcc keeps every load behind the store before it, and the
// per-entry form paid one exposed memory round trip per entry (load, wait, store, load, wait, store ... in the ISA of every add layer).
// ADD = false: the instantiation for layers without a residual operand -- no load and therefore no s_waitcnt vmcnt in it (k_conv_a issues the next
// unit's DMA before it: a counter wait here would wait for those older pieces as well).
template <int CT, int PT, bool ADD = true>
__device__ inline void conv_epilogue(const ConvArgs &a, const ConvClass &cls, floatx4 (&acc)[CT][PT], const float4 (&scv)[CT], const float4 (&biv)[CT],
                                     int wave, int j, int g, int ct0, int pz0, int py0, int px0) {
#ifdef DR_EPILOGUE_PER_ENTRY  // A/B build: the per-entry form
  constexpr int NE = CT * PT, GB = 1;
#else
  constexpr int NE = CT * PT, GB = NE < 4 ? NE : 4;
#endif
#pragma unroll
  for (int e0 = 0; e0 < NE; e0 += GB) {
    size_t obase[GB];
    float4 r[GB];
    bool ok[GB];
#pragma unroll
    for (int k = 0; k < GB; ++k) {
      const int e = e0 + k, pt = e / CT, ct = e - pt * CT;  // (compile-time after unrolling)
      const int tau = wave * PT + pt;
      const int xt = tau % a.TXT, yt = (tau / a.TXT) % a.TY, zt = tau / (a.TXT * a.TY);
      const int qz = pz0 + zt, qy = py0 + yt, qx = px0 + xt * 16 + j;
      const int c0 = (ct0 + ct) * 16 + 4 * g;
      ok[k] = e < NE && qz < a.nPD && qy < a.nPH && qx < a.nPW && c0 < a.rows_valid;
      int oz = qz * a.omz + cls.ooz, oy = qy * a.omy + cls.ooy, ox = qx * a.omx + cls.oox, ch = c0;
      if (a.par_rows) {  // transposed layer: this lane's 4 rows are 4 channels of output parity q
        const int q = c0 / a.par_rows, bits = (a.par_map >> (3 * q)) & 7;
        ch = c0 - q * a.par_rows;
        oz += (bits >> 2) & 1; oy += (bits >> 1) & 1; ox += bits & 1;
      }
      obase[k] = (((size_t)oz * a.outH + oy) * a.outW + ox) * a.outC + ch;
      size_t abase = obase[k];
      if (a.add_mode == 2) abase = (((size_t)oz * a.addH + (oy >> 1)) * a.addW + (ox >> 1)) * a.outC + ch;
      r[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ADD && a.add_mode && ok[k]) r[k] = *reinterpret_cast<const float4 *>(a.add + abase);
    }
#pragma unroll
    for (int k = 0; k < GB; ++k) {
      const int e = e0 + k, pt = e / CT, ct = e - pt * CT;
      if (e >= NE || !ok[k]) continue;
      const float4 sc = scv[ct], bi = biv[ct];
      float4 v;
      v.x = acc[ct][pt][0] * sc.x + bi.x;
      v.y = acc[ct][pt][1] * sc.y + bi.y;
      v.z = acc[ct][pt][2] * sc.z + bi.z;
      v.w = acc[ct][pt][3] * sc.w + bi.w;
      if (a.relu) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      }
      if (ADD && a.add_mode) { v.x += r[k].x; v.y += r[k].y; v.z += r[k].z; v.w += r[k].w; }
      *reinterpret_cast<float4 *>(a.out + obase[k]) = v;
    }
  }
}

// ---- K loop over the chunks of one channel pass, operands of chunk u+1 fetched under the MFMAs of u ----
// Two operand register sets used alternately (the loop is unrolled by two): renaming the prefetched set into the current
// one at the end of every iteration costs 8 v_mov_b64 whose results the next MFMAs have to wait for -- 118 vs 104 TFLOP/s
// (one wave per SIMD) and 138 vs 120-127 (two) in tools/ubench/mfma_lds2.hip, which isolates exactly this loop.
template <int CT, int PT>
__device__ inline void conv_chunk_mfma(const float4 (&av)[CT], const float4 (&bv)[PT], floatx4 (&acc)[CT][PT]) {
  // consecutive MFMAs go to different accumulators (16x16x4: 32-cycle issue, 40-cycle dependent latency)
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct].x, bv[pt].x, acc[ct][pt], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct].y, bv[pt].y, acc[ct][pt], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct].z, bv[pt].z, acc[ct][pt], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct].w, bv[pt].w, acc[ct][pt], 0, 0, 0);
}
template <int CT, int PT>
__device__ inline void conv_chunk_load(const float *lds, const float4 *wp, int toff, int u, const int (&base)[PT], float4 (&av)[CT],
                                       float4 (&bv)[PT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) av[ct] = wp[(u * CT + ct) * 64];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) bv[pt] = *reinterpret_cast<const float4 *>(lds + base[pt] + toff);
}
// Anchor prefetched operands at the END of the MFMA block before them: without a use there hipcc sinks the loads in
// front of their own MFMAs and every chunk eats a full LDS round trip.
template <int CT, int PT>
__device__ inline void conv_chunk_anchor(const float4 (&av)[CT], const float4 (&bv)[PT], int toff) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) asm volatile("" ::"v"(av[ct].x), "v"(av[ct].y), "v"(av[ct].z), "v"(av[ct].w));
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) asm volatile("" ::"v"(bv[pt].x), "v"(bv[pt].y), "v"(bv[pt].z), "v"(bv[pt].w));
  asm volatile("" ::"v"(toff));
}
template <int CT, int PT>
__device__ inline void conv_kloop(const float *lds, const float4 *wl, const int *tp, int TPC, int NU, int lane, const int (&base)[PT],
                                  floatx4 (&acc)[CT][PT]) {
  const float4 *wp = wl + lane;
  float4 a0[CT], b0[PT], a1[CT], b1[PT];
  // the tap offset of a chunk is itself an LDS read: it is fetched one chunk before the operands that need it
  int tA = tp[0], tB = tp[min(1, NU - 1) * TPC];
  conv_chunk_load<CT, PT>(lds, wp, tA, 0, base, a0, b0);
  int u = 0;
  for (; u + 1 < NU; u += 2) {
    // sched_barrier: the operand reads of the NEXT chunk are issued before the MFMAs of this one and waited for after them
    conv_chunk_load<CT, PT>(lds, wp, tB, u + 1, base, a1, b1);
    tA = tp[min(u + 2, NU - 1) * TPC];
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_mfma<CT, PT>(a0, b0, acc);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_anchor<CT, PT>(a1, b1, tA);
    conv_chunk_load<CT, PT>(lds, wp, tA, min(u + 2, NU - 1), base, a0, b0);
    tB = tp[min(u + 3, NU - 1) * TPC];
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_mfma<CT, PT>(a1, b1, acc);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_anchor<CT, PT>(a0, b0, tB);
  }
  if (u < NU) conv_chunk_mfma<CT, PT>(a0, b0, acc);  // odd chunk count: set 0 holds the last chunk
}

// The K loop for NARROW waves (CT * PT <= 2: the coarse and strided layers, ~25 launches per forward).  Two things the loop above leaves
// on the table there: (1) a chunk is 4 or 8 MFMAs = 128-256 cycles, about one LDS round trip, so operands fetched ONE chunk ahead arrive
// late -- here they are fetched two chunks ahead (three register sets in rotation, the loop unrolled by three); (2) with a single
// accumulator tile the four MFMAs of a chunk depend on each other (40-cycle dependent latency against a 32-cycle issue interval) --
// here they alternate between two accumulators that are added at the end (k_conv_m does the same, conv_march.h).
// `load(tap offset, chunk, av, bv)` fetches one chunk's operands (k_conv and k_conv_a address their tiles differently).
template <int CT, int PT>
__device__ inline void conv_chunk_mfma2(const float4 (&av)[CT], const float4 (&bv)[PT], floatx4 (&acc)[CT][PT], floatx4 (&acc2)[CT][PT]) {
  if constexpr (CT * PT == 1) {
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0].x, bv[0].x, acc[0][0], 0, 0, 0);
    acc2[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0].y, bv[0].y, acc2[0][0], 0, 0, 0);
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0].z, bv[0].z, acc[0][0], 0, 0, 0);
    acc2[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0].w, bv[0].w, acc2[0][0], 0, 0, 0);
  } else conv_chunk_mfma<CT, PT>(av, bv, acc);
}
template <int CT, int PT, class Load>
__device__ inline void conv_kloop_narrow(const int *tp, int TPC, int NU, floatx4 (&acc)[CT][PT], Load load) {
  float4 a0[CT], b0[PT], a1[CT], b1[PT], a2[CT], b2[PT];
  floatx4 acc2[CT][PT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc2[ct][pt] = floatx4{0.f, 0.f, 0.f, 0.f};
  auto tap = [&](int u) { return tp[min(u, NU - 1) * TPC]; };  // (the tap offset of a chunk is itself an LDS read: fetched a chunk before its operands)
  int t0 = tap(0), t1 = tap(1), t2 = tap(2);
  load(t0, 0, a0, b0);
  load(t1, min(1, NU - 1), a1, b1);
  int u = 0;
  for (; u + 2 < NU; u += 3) {  // invariant: set 0 holds chunk u, set 1 chunk u + 1
    load(t2, u + 2, a2, b2);
    t0 = tap(u + 3);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_mfma2<CT, PT>(a0, b0, acc, acc2);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_anchor<CT, PT>(a1, b1, t0);
    load(t0, min(u + 3, NU - 1), a0, b0);
    t1 = tap(u + 4);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_mfma2<CT, PT>(a1, b1, acc, acc2);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_anchor<CT, PT>(a2, b2, t1);
    load(t1, min(u + 4, NU - 1), a1, b1);
    t2 = tap(u + 5);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_mfma2<CT, PT>(a2, b2, acc, acc2);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_anchor<CT, PT>(a0, b0, t2);
  }
  if (u < NU) conv_chunk_mfma2<CT, PT>(a0, b0, acc, acc2);      // one or two chunks left: sets 0 and 1 hold them
  if (u + 1 < NU) conv_chunk_mfma2<CT, PT>(a1, b1, acc, acc2);
  if constexpr (CT * PT == 1) acc[0][0] += acc2[0][0];
}

// grid = (tiles, parity classes, output-row groups).  PT = position tiles (16 positions each) per wave.
// FZ > 0: fused FeatureNet skip -- the staged tile is computed (1x1 conv of an FZ-channel tensor + bias + nearest
// upsample of the coarser level) instead of copied; the arithmetic is k_skip_up's, so the result is bit-identical to
// running that kernel first and this one on its output.
// One LDS-DMA piece: every lane fetches 16 bytes from its own global address, the wave's 1 KiB lands at LDS byte address
// `lds_dst` (wave-uniform) + lane * 16.  Issued from inline asm on purpose: given the builtin, hipcc orders every later
// LDS read behind the DMA with s_waitcnt vmcnt(0) -- directly in front of the K loop, which serialises the very overlap
// this kernel exists for.  The asm statement is invisible to hipcc's counters; k_conv_a waits for it itself
// (conv_a_wait_dma) before the barrier that publishes the buffer.  M0 is saved and restored around the instruction.
__device__ inline void conv_a_dma16(const void *gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ inline void conv_a_wait_dma() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ inline unsigned conv_a_lds_addr(const void *p) {
  return (unsigned)(unsigned long long)(__attribute__((address_space(3))) const char *)p;
}

// Four waves per SIMD (128 VGPRs) for the one-row-tile instances without the fused skip: they need 129-135 registers when left alone,
// i.e. three workgroups per CU instead of four, and the layers they run (transposed, strided, coarse: a few microseconds of
// work per workgroup between three memory round trips) are bound by exactly that occupancy.  DR_CONV_WAVES3 = the old bound (A/B build).
#ifdef DR_CONV_WAVES3
#define DR_KCONV_MIN_WAVES(CT, FZ) 1
#else
#define DR_KCONV_MIN_WAVES(CT, FZ) ((CT) == 1 && (FZ) == 0 ? 4 : 1)
#endif
// (the body of k_conv and of k_conv_c, its class-loop form: two kernels so that the class loop's code does not sit in the instances that never take it --
// inside one kernel it cost conv9's instance <16,2,4> 25 %, 0.031 -> 0.039 ms, without ever running there)
template <int CI, int CT, int PT, int FZ, bool CL>
__device__ __forceinline__ void conv_tile_body(const ConvArgs &a) {
  extern __shared__ float4 lds4[];
  float *lds = reinterpret_cast<float *>(lds4);
  constexpr int CIS = CI + 4;  // LDS floats per staged position (+4: spreads b128 reads over bank slots)
  constexpr int TPC = 16 / CI; // taps per 16-wide K chunk
  constexpr int C4 = CI / 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const ConvClass cls = a.cls[blockIdx.y];
  const int ct0 = blockIdx.z * CT;

  // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (own L2 each), so XCD k takes the k-th
  // contiguous range of tiles (x fastest, then y, then z): neighbouring tiles, which share their halo, share an L2.
  // grid.x is padded to a multiple of 8 (so that XCD == blockIdx.x % 8 for every row group); surplus workgroups exit.
  const int ntiles = a.tilesD * a.tilesH * a.tilesW, per_xcd = (ntiles + 7) >> 3;
  int b = (int)(blockIdx.x & 7u) * per_xcd + (int)(blockIdx.x >> 3);
  if (b >= ntiles) return;
  const int tw = b % a.tilesW;
  b /= a.tilesW;
  const int th = b % a.tilesH, td = b / a.tilesH;
  const int pz0 = td * a.TZ, py0 = th * a.TY, px0 = tw * a.TXT * 16;
  const int iz0 = pz0 * a.sz - a.pz, iy0 = py0 * a.sy - a.py, ix0 = px0 * a.sx - a.px;

  int base[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int tau = wave * PT + pt;
    const int xt = tau % a.TXT, yt = (tau / a.TXT) % a.TY, zt = tau / (a.TXT * a.TY);
    base[pt] = (((zt * a.sz) * a.TYI + yt * a.sy) * a.TXI + (xt * 16 + j) * a.sx) * CIS + (4 * g) % CI;
  }
  const int sub = (4 * g) / CI;

  floatx4 acc[CT][PT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int NP = a.TZI * a.TYI * a.TXI, NU = cls.NU;
  // tap table of this class -> LDS (pre-multiplied by the position stride) so the K loop has no dependent global load
  float4 *wl = lds4 + ((size_t)NP * CIS) / 4;                           // [NU][CT][64] packed weights of the current pass
  int *tapl = reinterpret_cast<int *>(wl + (size_t)a.nuMax * CT * 64);  // [NU*TPC] tap offsets (floats)
  for (int i = tid; i < NU * TPC; i += kConvThreads) tapl[i] = a.tapoff[cls.tap_base + i] * CIS;
  [[maybe_unused]] const unsigned n_w = (unsigned)NU * CT * 64;
  const int *tp = tapl + sub;
  const unsigned total = (unsigned)NP * C4;
  // PIPELINED PASSES (a.a_wbufs == 2; the planner sets it for the small multi-pass layers: PT = 1, the whole tile in kPipeBatch loads per lane).
  // The coarse UNet levels run 2-4 channel passes of a few microseconds each, and every pass began with a bare round trip to L2 for its tile and
  // its weights (one workgroup per CU or fewer: nobody else covers it).  Here the loads of pass p + 1 -- the tile into registers, the weights by
  // LDS-DMA into the OTHER weight buffer -- are issued before the K loop of pass p and land under it: one exposed round trip per workgroup
  // instead of one per pass.  Same products, same order: bit-identical to the plain loop (DR_CONV_NO_PIPE=1 keeps that one, A/B).
  if constexpr (PT == 1 && CT <= 2 && FZ == 0) {
    if (a.a_wbufs == 2) {
      constexpr int kPipeBatch = 6;
      float4 *wb1 = wl + (size_t)a.nuMax * CT * 64;
      int *tapl2 = reinterpret_cast<int *>(wb1 + (size_t)a.nuMax * CT * 64);  // (the tap table sits behind BOTH weight buffers)
      for (int i = tid; i < NU * TPC; i += kConvThreads) tapl2[i] = a.tapoff[cls.tap_base + i] * CIS;
      const int *tp2 = tapl2 + sub;
      int soff[kPipeBatch], dst[kPipeBatch];  // element offset of this lane's k-th staged float4 inside pass 0's slice (-1: outside the tensor), LDS float index (-1: none)
#pragma unroll
      for (int k = 0; k < kPipeBatch; ++k) {
        const unsigned e = k * kConvThreads + tid;
        const unsigned pos = e / C4, c4 = e - pos * C4;
        const unsigned t = a.magicX ? __umulhi(pos, a.magicX) : pos, x = pos - t * a.TXI;
        const unsigned z = a.magicY ? __umulhi(t, a.magicY) : t, y = t - z * a.TYI;
        const int gz = iz0 + (int)z, gy = iy0 + (int)y, gx = ix0 + (int)x;
        dst[k] = e < total ? (int)(pos * CIS + c4 * 4) : -1;
        soff[k] = (e < total && gz >= 0 && gz < a.inD && gy >= 0 && gy < a.inH && gx >= 0 && gx < a.inW) ? (int)((((size_t)gz * a.inH + gy) * a.inW + gx) * a.inC + c4 * 4) : -1;
      }
      float4 v[kPipeBatch];
      auto issue = [&](int p) {  // weights of pass p -> buffer p & 1 (LDS-DMA), its tile -> registers; nothing is waited for here
        float4 *wb = (p & 1) ? wb1 : wl;
        const float4 *wsrc = a.wpk + cls.w_base + ((size_t)p * NU * a.ctTot + ct0) * 64;
        for (int e = wave; e < NU * CT; e += kConvThreads / 64) {
          const int u = e / CT, ct = e - u * CT;
          conv_a_dma16(wsrc + ((size_t)u * a.ctTot + ct) * 64 + lane, __builtin_amdgcn_readfirstlane(conv_a_lds_addr(wb + (size_t)e * 64)));
        }
#pragma unroll
        for (int k = 0; k < kPipeBatch; ++k) {
          v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (soff[k] >= 0) v[k] = *reinterpret_cast<const float4 *>(a.in + (size_t)soff[k] + (size_t)p * a.pass_stride);
        }
      };
      __builtin_amdgcn_s_setprio(2);
      issue(0);
      for (int p = 0; p < a.npass; ++p) {
#pragma unroll
        for (int k = 0; k < kPipeBatch; ++k)
          if (dst[k] >= 0) *reinterpret_cast<float4 *>(lds + dst[k]) = v[k];
        conv_a_wait_dma();  // (everything in flight belongs to pass p: its tile, consumed just above, and its weights)
        __builtin_amdgcn_s_setprio(0);
        __syncthreads();
        if (p + 1 < a.npass) issue(p + 1);  // in flight across the K loop, which touches neither those registers nor that weight buffer
        const float4 *wp = ((p & 1) ? wb1 : wl) + lane;
        conv_kloop_narrow<CT, PT>(tp2, TPC, NU, acc, [&](int toff, int u, float4 (&av)[CT], float4 (&bv)[PT]) { conv_chunk_load<CT, PT>(lds, wp, toff, u, base, av, bv); });
        __syncthreads();  // everybody has left the tile before pass p + 1 overwrites it
      }
      float4 scv[CT], biv[CT];
      conv_load_affine<CT>(a, g, ct0, scv, biv);
      conv_epilogue<CT, PT>(a, cls, acc, scv, biv, wave, j, g, ct0, pz0, py0, px0);
      return;
    }
  }
  // CLASS LOOP (a.class_loop = number of parity classes; single-pass transposed layers: conv11).  With one class per workgroup a layer like stage 2's conv11 is
  // 4800 workgroups whose life is three dependent round trips (weights + tile, barrier, residual operand) around 1.7 us of MFMA work: 0.072 ms, 0.050 of it with the
  // MFMA loop compiled out (profiles/r06_strided_layers_ablation.txt).  Here a workgroup stages its tile ONCE and walks the classes on it, the NEXT class's weights
  // streaming into the other weight buffer (LDS-DMA) under the current class's MFMA loop and epilogue: one exposed round trip per workgroup instead of one per class.
  // Every class's tap table sits in LDS from the start.  Same tile values, same weights, same chunk order per output: bit-identical to the class-per-workgroup launch.
  if constexpr (CL) {
    {
      const int ncls = a.class_loop, tstride = a.nuMax * TPC;
      float4 *wb1 = wl + (size_t)a.nuMax * CT * 64;
      int *tap_all = reinterpret_cast<int *>(wb1 + (size_t)a.nuMax * CT * 64);  // [ncls][nuMax * TPC], behind both weight buffers
      for (int i = tid; i < ncls * tstride; i += kConvThreads) {
        const int c = i / tstride, k = i - c * tstride;
        tap_all[i] = k < a.cls[c].NU * TPC ? a.tapoff[a.cls[c].tap_base + k] * CIS : 0;
      }
      auto issue_w = [&](int c) {  // class c's packed weights -> buffer c & 1
        const unsigned wb = conv_a_lds_addr(wl) + (unsigned)(c & 1) * (unsigned)a.nuMax * CT * 1024u;  // (LDS byte address; an address-space cast of a SELECTED pointer trips hipcc -O2)
        const float4 *wsrc = a.wpk + a.cls[c].w_base + (size_t)ct0 * 64;
        const int n = a.cls[c].NU * CT;
        for (int e = wave; e < n; e += kConvThreads / 64) {
          const int u = e / CT, ct = e - u * CT;
          conv_a_dma16(wsrc + ((size_t)u * a.ctTot + ct) * 64 + lane, __builtin_amdgcn_readfirstlane(wb + (unsigned)e * 1024u));
        }
      };
      __builtin_amdgcn_s_setprio(2);
      issue_w(0);
      constexpr int kStageBatchC = 12;
      for (unsigned e0 = 0; e0 < total; e0 += kConvThreads * kStageBatchC) {
        float4 v[kStageBatchC];
        int dst[kStageBatchC];
#pragma unroll
        for (int k = 0; k < kStageBatchC; ++k) {
          const unsigned e = e0 + k * kConvThreads + tid;
          const unsigned pos = e / C4, c4 = e - pos * C4;
          const unsigned t = a.magicX ? __umulhi(pos, a.magicX) : pos, x = pos - t * a.TXI;
          const unsigned z = a.magicY ? __umulhi(t, a.magicY) : t, y = t - z * a.TYI;
          const int gz = iz0 + (int)z, gy = iy0 + (int)y, gx = ix0 + (int)x;
          v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          dst[k] = e < total ? (int)(pos * CIS + c4 * 4) : -1;
          if (e < total && gz >= 0 && gz < a.inD && gy >= 0 && gy < a.inH && gx >= 0 && gx < a.inW)
            v[k] = *reinterpret_cast<const float4 *>(a.in + (((size_t)gz * a.inH + gy) * a.inW + gx) * a.inC + c4 * 4);
        }
#pragma unroll
        for (int k = 0; k < kStageBatchC; ++k)
          if (dst[k] >= 0) *reinterpret_cast<float4 *>(lds + dst[k]) = v[k];
      }
      float4 scv[CT], biv[CT];
      conv_load_affine<CT>(a, g, ct0, scv, biv);
      for (int c = 0; c < ncls; ++c) {
        conv_a_wait_dma();  // class c's weights have landed (and, first time round, nothing else of this wave is in flight) ...
        __builtin_amdgcn_s_setprio(0);
        __syncthreads();    // ... everybody's have, the tile and the tap tables are written, and every wave has left the buffer class c + 1 goes into
        if (c + 1 < ncls) issue_w(c + 1);
        const ConvClass cc = a.cls[c];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = floatx4{0.f, 0.f, 0.f, 0.f};
        const float4 *wc = (c & 1) ? wb1 : wl;
        const int *tpc = tap_all + c * tstride + sub;
        if constexpr (CT * PT <= 2) {
          const float4 *wp = wc + lane;
          conv_kloop_narrow<CT, PT>(tpc, TPC, cc.NU, acc, [&](int toff, int u, float4 (&av)[CT], float4 (&bv)[PT]) { conv_chunk_load<CT, PT>(lds, wp, toff, u, base, av, bv); });
        } else conv_kloop<CT, PT>(lds, wc, tpc, TPC, cc.NU, lane, base, acc);
        conv_epilogue<CT, PT>(a, cc, acc, scv, biv, wave, j, g, ct0, pz0, py0, px0);
      }
      return;
    }
  }
  for (int p = 0; p < a.npass; ++p) {
    // Staging waves get issue priority over co-resident workgroups' K loops: the sooner their loads are in flight the
    // sooner this workgroup can feed the MFMA pipe; the K loop of the neighbour fills the remaining issue slots.
    // (The opposite assignment -- priority to the K loop -- measured 6 % slower.)
    __builtin_amdgcn_s_setprio(2);
    // This pass's packed weights go to LDS by LDS-DMA, requested BEFORE the tile is staged: the round trip to L2 for the
    // weights runs beside the tile's instead of after it, and costs no registers.  (For the coarse layers, whose tiles are
    // small and whose weights are 28-110 KB per pass, the weight fetch was half of the staging step.)  The K loop of the
    // previous pass has left `wl` (barrier at the end of the pass); the pieces have landed at conv_a_wait_dma() below.
    const float4 *wsrc = a.wpk + cls.w_base + ((size_t)p * NU * a.ctTot + ct0) * 64;
#ifndef DR_CONV_NO_WEIGHT_DMA
#ifdef DR_ABL_NO_STAGE
    if (a.npass < 0)
#endif
    for (int e = wave; e < NU * CT; e += kConvThreads / 64) {  // piece e = u * CT + ct: 64 lanes x 16 B, contiguous on both sides
      const int u = e / CT, ct = e - u * CT;
      conv_a_dma16(wsrc + ((size_t)u * a.ctTot + ct) * 64 + lane, __builtin_amdgcn_readfirstlane(conv_a_lds_addr(wl + (size_t)e * 64)));
    }
#endif
    // ---- stage CI channels of the input halo tile into LDS (zero outside the tensor).  Loads are issued in
    // batches of kStageBatch per lane BEFORE the first LDS write so their HBM/L2 latencies overlap. ----
    constexpr int kStageBatch = CT >= 4 ? 6 : 12;  // normally the whole stage: one exposed HBM/L2 latency per pass
    if constexpr (FZ > 0) {
      static_assert(FZ == 0 || (C4 == kConvThreads / 64 && FZ % 4 == 0), "one wave per 4-channel group of the pass");
      // wave w produces channels p*CI + 4w .. +3 of every staged position: its 4 x FZ weights are wave-uniform (scalar
      // registers), a lane reads 4*FZ contiguous bytes of x (64 lanes = one contiguous run) and writes one float4.
      const int q = __builtin_amdgcn_readfirstlane(p * C4 + wave);
      float wr[4][FZ];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < FZ; ++c) wr[r][c] = a.fz_w[(4 * q + r) * FZ + c];
      const float4 fb = *reinterpret_cast<const float4 *>(a.fz_b + 4 * q);
#ifndef DR_FZ_BATCH
#define DR_FZ_BATCH 4
#endif
      constexpr int kFB = DR_FZ_BATCH;
      const int Hc = a.inH >> 1, Wc = a.inW >> 1;
      for (int p0 = 0; p0 < NP; p0 += 64 * kFB) {
        float4 xv[kFB][FZ / 4], up[kFB];
        int dst[kFB];
        bool in[kFB];
#pragma unroll
        for (int k = 0; k < kFB; ++k) {
          const unsigned pos = p0 + k * 64 + lane;
          const unsigned t = a.magicX ? __umulhi(pos, a.magicX) : pos, x = pos - t * a.TXI;
          const unsigned z = a.magicY ? __umulhi(t, a.magicY) : t, y = t - z * a.TYI;
          const int gz = iz0 + (int)z, gy = iy0 + (int)y, gx = ix0 + (int)x;
          dst[k] = (int)pos < NP ? (int)(pos * CIS + wave * 4) : -1;
          in[k] = (int)pos < NP && gz >= 0 && gz < a.inD && gy >= 0 && gy < a.inH && gx >= 0 && gx < a.inW;
          up[k] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int c = 0; c < FZ / 4; ++c) xv[k][c] = up[k];
          if (in[k]) {
            const float *xp = a.fz_x + (((size_t)gz * a.inH + gy) * a.inW + gx) * FZ;
#pragma unroll
            for (int c = 0; c < FZ / 4; ++c) xv[k][c] = *reinterpret_cast<const float4 *>(xp + 4 * c);
            up[k] = *reinterpret_cast<const float4 *>(a.fz_coarse + (((size_t)gz * Hc + (gy >> 1)) * Wc + (gx >> 1)) * a.inC + 4 * q);
          }
        }
#pragma unroll
        for (int k = 0; k < kFB; ++k) {
          float acc4[4] = {0.f, 0.f, 0.f, 0.f}, xi[FZ];
#pragma unroll
          for (int c = 0; c < FZ / 4; ++c) { xi[4 * c] = xv[k][c].x; xi[4 * c + 1] = xv[k][c].y; xi[4 * c + 2] = xv[k][c].z; xi[4 * c + 3] = xv[k][c].w; }
#pragma unroll
          for (int sft = 0; sft < 4; ++sft)
#pragma unroll
            for (int gq = 0; gq < FZ / 4; ++gq)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc4[r] = __builtin_fmaf(wr[r][4 * gq + sft], xi[4 * gq + sft], acc4[r]);
          float4 o = make_float4(0.f, 0.f, 0.f, 0.f);  // outside the tensor: the 3x3 layer's zero padding
          if (in[k]) { o.x = (acc4[0] + fb.x) + up[k].x; o.y = (acc4[1] + fb.y) + up[k].y; o.z = (acc4[2] + fb.z) + up[k].z; o.w = (acc4[3] + fb.w) + up[k].w; }
          if (dst[k] >= 0) *reinterpret_cast<float4 *>(lds + dst[k]) = o;
        }
      }
    } else
#ifdef DR_ABL_NO_STAGE
    if (a.npass < 0)  // ablation build: no staging at all (results are garbage)
#endif
    for (unsigned e0 = 0; e0 < total; e0 += kConvThreads * kStageBatch) {
      float4 v[kStageBatch];
      int dst[kStageBatch];
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k) {
        const unsigned e = e0 + k * kConvThreads + tid;
        const unsigned pos = e / C4, c4 = e - pos * C4;
        // exact for pos < 2^16; a divisor of 1 has no 32-bit magic (2^32), the host stores 0 for it
        const unsigned t = a.magicX ? __umulhi(pos, a.magicX) : pos, x = pos - t * a.TXI;
        const unsigned z = a.magicY ? __umulhi(t, a.magicY) : t, y = t - z * a.TYI;
        const int gz = iz0 + (int)z, gy = iy0 + (int)y, gx = ix0 + (int)x;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        dst[k] = e < total ? (int)(pos * CIS + c4 * 4) : -1;
        if (e < total && gz >= 0 && gz < a.inD && gy >= 0 && gy < a.inH && gx >= 0 && gx < a.inW)
          v[k] = *reinterpret_cast<const float4 *>(a.in + (((size_t)gz * a.inH + gy) * a.inW + gx) * a.inC + (size_t)p * a.pass_stride + c4 * 4);
      }
#pragma unroll
      for (int k = 0; k < kStageBatch; ++k)
        if (dst[k] >= 0) *reinterpret_cast<float4 *>(lds + dst[k]) = v[k];
    }
#ifndef DR_CONV_NO_WEIGHT_DMA
    conv_a_wait_dma();
#else
    {  // (A/B build: the weights through registers, after the tile)
      constexpr int kWB = 8;
#ifdef DR_ABL_NO_STAGE
      if (a.npass < 0)
#endif
      for (unsigned e0 = 0; e0 < n_w; e0 += kConvThreads * kWB) {
        float4 v[kWB];
#pragma unroll
        for (int k = 0; k < kWB; ++k) {
          const unsigned e = e0 + k * kConvThreads + tid;  // = (u*CT + ct)*64 + l
          const unsigned u = e / (CT * 64), r = e - u * (CT * 64);
          v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (e < n_w) v[k] = wsrc[(size_t)u * a.ctTot * 64 + r];
        }
#pragma unroll
        for (int k = 0; k < kWB; ++k) {
          const unsigned e = e0 + k * kConvThreads + tid;
          if (e < n_w) wl[e] = v[k];
        }
      }
    }
#endif
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
#ifndef DR_ABL_NO_KLOOP
#ifdef DR_NO_NARROW_KLOOP  // A/B build
    if constexpr (false) {
#else
    if constexpr (CT * PT <= 2) {
#endif
      const float4 *wp = wl + lane;
      conv_kloop_narrow<CT, PT>(tp, TPC, NU, acc, [&](int toff, int u, float4 (&av)[CT], float4 (&bv)[PT]) { conv_chunk_load<CT, PT>(lds, wp, toff, u, base, av, bv); });
    } else conv_kloop<CT, PT>(lds, wl, tp, TPC, NU, lane, base, acc);
#endif
    __syncthreads();
  }

  float4 scv[CT], biv[CT];
  conv_load_affine<CT>(a, g, ct0, scv, biv);
  conv_epilogue<CT, PT>(a, cls, acc, scv, biv, wave, j, g, ct0, pz0, py0, px0);
}
template <int CI, int CT, int PT, int FZ = 0>
__global__ __launch_bounds__(kConvThreads, DR_KCONV_MIN_WAVES(CT, FZ)) void k_conv(const ConvArgs a) {
  conv_tile_body<CI, CT, PT, FZ, false>(a);
}
// k_conv_c: k_conv's CLASS LOOP form (a.class_loop parity classes per workgroup, grid.y = 1), under k_conv's register bound
template <int CI, int CT, int PT>
__global__ __launch_bounds__(kConvThreads, DR_KCONV_MIN_WAVES(CT, 0)) void k_conv_c(const ConvArgs a) {
  conv_tile_body<CI, CT, PT, 0, true>(a);
}

#ifdef DR_PARITY_HOOKS  // the bf16 x 3 precision mode is not fp32 arithmetic and never the product's: its kernel is built into the parity library only
#include "conv_bf3.h"  // k_conv_b: k_conv on the bf16 matrix cores with three-term split operands (DR_CONV_BF16X3=1)
#endif

// ------------------------------------------------------------------------------------------------
// k_conv_a: the same implicit GEMM as a PERSISTENT workgroup whose staging is asynchronous.
//
// k_conv's phases are additive (r2 ablation at s2.conv0: K loop 61 %, staging 24 %, epilogue + launch 11 %; two
// co-resident workgroups run in phase, so they do not hide each other's staging).  Here a workgroup of 8 waves walks a
// list of (tile, channel pass) units; while the MFMAs of unit i run out of LDS buffer i & 1, the halo tile (and, for
// multi-pass layers, the packed weights) of unit i + 1 stream into the other buffer with global_load_lds_dwordx4 --
// no staging registers, no ds_write pass, one barrier per unit.  The LDS-DMA destination is wave-uniform base +
// lane * 16, so the tile is stored unpadded; bank conflicts of the operand reads are avoided by a slot permutation
// applied on the SOURCE side (each lane fetches the element that belongs in its slot) and on the read side
// (tools/ubench/glds_probe.hip: conflict-free for position strides 1 and 2, which is what the layers use).
constexpr int kConvAThreads = 512;

template <int CI>
__host__ __device__ inline int conv_a_unit(int pos, int c4) {  // (position, channel group) -> 16-byte slot
  if constexpr (CI == 4) return pos;
  else if constexpr (CI == 8) return ((pos ^ ((pos >> 3) & 1)) << 1) | c4;
  else return ((pos ^ ((pos >> 3) & 1)) << 2) | (c4 ^ ((pos >> 1) & 3));
}
template <int CI>
__host__ __device__ inline void conv_a_slot(int s, int &pos, int &c4) {  // inverse of conv_a_unit (both xors are involutions)
  if constexpr (CI == 4) { pos = s; c4 = 0; }
  else if constexpr (CI == 8) { const int pp = s >> 1; pos = pp ^ ((pp >> 3) & 1); c4 = s & 1; }
  else { const int pp = s >> 2; pos = pp ^ ((pp >> 3) & 1); c4 = (s & 3) ^ ((pos >> 1) & 3); }
}

template <int CI, int CT>
__device__ inline void conv_a_issue(const ConvArgs &a, float4 *tile, float4 *wbuf, bool with_weights, int NP, int NU, int p, int ct0, int w_base,
                                    int iz0, int iy0, int ix0, int wave, int lane) {
  for (int s0 = wave * 64; s0 < a.a_slots; s0 += kConvAThreads) {  // s0 is wave-uniform
    int pos, c4;
    conv_a_slot<CI>(s0 + lane, pos, c4);
    const unsigned t = a.magicX ? __umulhi((unsigned)pos, a.magicX) : (unsigned)pos, x = pos - t * a.TXI;
    const unsigned z = a.magicY ? __umulhi(t, a.magicY) : t, y = t - z * a.TYI;
    const int gz = iz0 + (int)z, gy = iy0 + (int)y, gx = ix0 + (int)x;
    const float *src = a.zero16;
    if (pos < NP && gz >= 0 && gz < a.inD && gy >= 0 && gy < a.inH && gx >= 0 && gx < a.inW)
      src = a.in + (((size_t)gz * a.inH + gy) * a.inW + gx) * a.inC + (size_t)p * a.pass_stride + c4 * 4;
    conv_a_dma16(src, __builtin_amdgcn_readfirstlane(conv_a_lds_addr(tile + s0)));
  }
  if (with_weights) {  // packed weights of this pass and row group: [u][CT][64] float4, lane-linear as they are in memory
    const float4 *wsrc = a.wpk + w_base + ((size_t)p * NU * a.ctTot + ct0) * 64;
    for (int e0 = wave * 64; e0 < NU * CT * 64; e0 += kConvAThreads) {
      const int u = e0 / (CT * 64), r = e0 - u * (CT * 64);
      conv_a_dma16(wsrc + (size_t)u * a.ctTot * 64 + r + lane, __builtin_amdgcn_readfirstlane(conv_a_lds_addr(wbuf + e0)));
    }
  }
}

template <int CI, int CT, int PT>
__device__ inline void conv_a_load(const float4 *tile, const float4 *wp, int toff, int u, int c4, const int (&bpos)[PT], float4 (&av)[CT], float4 (&bv)[PT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) av[ct] = wp[(u * CT + ct) * 64];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) bv[pt] = tile[conv_a_unit<CI>(bpos[pt] + toff, c4)];
}
template <int CI, int CT, int PT>
__device__ inline void conv_a_kloop(const float4 *tile, const float4 *wl, const int *tp, int TPC, int NU, int lane, int c4, const int (&bpos)[PT],
                                    floatx4 (&acc)[CT][PT]) {
  const float4 *wp = wl + lane;
  float4 a0[CT], b0[PT], a1[CT], b1[PT];
  int tA = tp[0], tB = tp[min(1, NU - 1) * TPC];
  conv_a_load<CI, CT, PT>(tile, wp, tA, 0, c4, bpos, a0, b0);
  int u = 0;
  for (; u + 1 < NU; u += 2) {
    conv_a_load<CI, CT, PT>(tile, wp, tB, u + 1, c4, bpos, a1, b1);
    tA = tp[min(u + 2, NU - 1) * TPC];
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_mfma<CT, PT>(a0, b0, acc);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_anchor<CT, PT>(a1, b1, tA);
    conv_a_load<CI, CT, PT>(tile, wp, tA, min(u + 2, NU - 1), c4, bpos, a0, b0);
    tB = tp[min(u + 3, NU - 1) * TPC];
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_mfma<CT, PT>(a1, b1, acc);
    __builtin_amdgcn_sched_barrier(0);
    conv_chunk_anchor<CT, PT>(a0, b0, tB);
  }
  if (u < NU) conv_chunk_mfma<CT, PT>(a0, b0, acc);
}

// grid = (persistent workgroups (multiple of 8), 1, output-row groups); 8 waves, PT position tiles per wave.
template <int CI, int CT, int PT>
__global__ __launch_bounds__(kConvAThreads) void k_conv_a(const ConvArgs a) {
  extern __shared__ float4 lds4[];
  constexpr int TPC = 16 / CI;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 15, g = lane >> 4;
  const ConvClass cls = a.cls[0];
  const int ct0 = blockIdx.z * CT;
  const int NP = a.TZI * a.TYI * a.TXI, NU = cls.NU, n_w = NU * CT * 64;

  // LDS: [tile 0][tile 1][weights 0][weights 1 (multi-pass layers)][tap table]
  float4 *tile0 = lds4, *tile1 = lds4 + a.a_slots;
  float4 *wb0 = lds4 + 2 * (size_t)a.a_slots;  // weight buffer of pass p: wb0 + (p % a_wbufs) * n_w
  int *tapl = reinterpret_cast<int *>(wb0 + (size_t)a.a_wbufs * n_w);
  for (int i = tid; i < NU * TPC; i += kConvAThreads) tapl[i] = a.tapoff[cls.tap_base + i];
  const int *tp = tapl + (4 * g) / CI;
  const int c4 = ((4 * g) % CI) / 4;

  int bpos[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int tau = wave * PT + pt;
    const int xt = tau % a.TXT, yt = (tau / a.TXT) % a.TY, zt = tau / (a.TXT * a.TY);
    bpos[pt] = ((zt * a.sz) * a.TYI + yt * a.sy) * a.TXI + (xt * 16 + j) * a.sx;
  }

  // this workgroup's tiles: XCD k (= blockIdx.x % 8, own L2) owns the k-th contiguous range of tiles; its workgroups
  // take them round-robin, so at any time an XCD works on neighbouring tiles whose halos overlap in its L2
  const int ntiles = a.tilesD * a.tilesH * a.tilesW, per_xcd = (ntiles + 7) >> 3;
  const int xcd = blockIdx.x & 7, wi = blockIdx.x >> 3, nw = gridDim.x >> 3;
  const int t_lo = xcd * per_xcd, t_hi = min(ntiles, t_lo + per_xcd);
  const int my_tiles = t_lo + wi < t_hi ? (t_hi - t_lo - wi + nw - 1) / nw : 0;
  const int n_units = my_tiles * a.npass;
  auto tile_origin = [&](int k, int &pz0, int &py0, int &px0) {
    int b = t_lo + wi + k * nw;
    const int tw = b % a.tilesW;
    b /= a.tilesW;
    pz0 = (b / a.tilesH) * a.TZ; py0 = (b % a.tilesH) * a.TY; px0 = tw * a.TXT * 16;
  };
  auto issue = [&](int unit) {
    const int k = unit / a.npass, p = unit - k * a.npass;
    int pz0, py0, px0;
    tile_origin(k, pz0, py0, px0);
    // weight buffer = pass % buffers: when every pass has its own buffer it is fetched once per workgroup
    conv_a_issue<CI, CT>(a, (unit & 1) ? tile1 : tile0, wb0 + (size_t)(p % a.a_wbufs) * n_w, unit < a.npass || a.npass > a.a_wbufs, NP, NU, p, ct0, cls.w_base,
                         pz0 * a.sz - a.pz, py0 * a.sy - a.py, px0 * a.sx - a.px, wave, lane);
  };

  floatx4 acc[CT][PT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = floatx4{0.f, 0.f, 0.f, 0.f};

  float4 scv[CT], biv[CT];  // folded BatchNorm of this lane's rows: fetched once, not per tile
  conv_load_affine<CT>(a, g, ct0, scv, biv);
  if (n_units > 0) issue(0);
  int done_tile = -1;  // tile whose accumulators are complete and not yet written
  for (int i = 0; i < n_units; ++i) {
    conv_a_wait_dma();  // this wave's pieces of unit i have landed ...
    __syncthreads();    // ... and so have everybody else's; every wave is done reading the other buffer
    // The next unit's DMA goes out BEFORE the previous tile's epilogue when that epilogue only stores (no residual operand): the round trip to L2 /
    // HBM then runs beside the epilogue as well as the K loop (a stride-2 layer's K loop is 0.7 us against a 2-3 us round trip).  With a residual
    // operand the order stays epilogue first: the DMA is invisible to hipcc's counters, and the vmcnt it puts behind the residual loads would then
    // wait for the (older) DMA pieces too.
#ifndef DR_ABL_NO_STAGE
#ifndef DR_CONV_A_ISSUE_LATE  // (A/B build: always after the epilogue, round 3's order)
    const bool early = a.add_mode == 0;
#else
    const bool early = false;
#endif
    if (early && i + 1 < n_units) issue(i + 1);
#endif
#ifdef DR_ABL_NO_EPI
    if (done_tile >= 0 && a.npass < 0) {
#else
    if (done_tile >= 0) {  // epilogue of the previous tile: its stores retire under the K loop below
#endif
      int pz0, py0, px0;
      tile_origin(done_tile, pz0, py0, px0);
      if (a.add_mode) conv_epilogue<CT, PT, true>(a, cls, acc, scv, biv, wave, j, g, ct0, pz0, py0, px0);
      else conv_epilogue<CT, PT, false>(a, cls, acc, scv, biv, wave, j, g, ct0, pz0, py0, px0);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = floatx4{0.f, 0.f, 0.f, 0.f};
      done_tile = -1;
    }
#ifndef DR_ABL_NO_STAGE
    if (!early && i + 1 < n_units) issue(i + 1);
#endif
#ifndef DR_ABL_NO_KLOOP
#ifdef DR_NO_NARROW_KLOOP
    if constexpr (false) {
#else
    if constexpr (CT * PT <= 2) {
#endif
      const float4 *tile = (i & 1) ? tile1 : tile0, *wp = wb0 + (size_t)((i % a.npass) % a.a_wbufs) * n_w + lane;
      conv_kloop_narrow<CT, PT>(tp, TPC, NU, acc, [&](int toff, int u, float4 (&av)[CT], float4 (&bv)[PT]) { conv_a_load<CI, CT, PT>(tile, wp, toff, u, c4, bpos, av, bv); });
    } else conv_a_kloop<CI, CT, PT>((i & 1) ? tile1 : tile0, wb0 + (size_t)((i % a.npass) % a.a_wbufs) * n_w, tp, TPC, NU, lane, c4, bpos, acc);
#endif
    if ((i + 1) % a.npass == 0) done_tile = i / a.npass;
  }
  if (done_tile >= 0) {
    int pz0, py0, px0;
    tile_origin(done_tile, pz0, py0, px0);
    conv_epilogue<CT, PT>(a, cls, acc, scv, biv, wave, j, g, ct0, pz0, py0, px0);
  }
}

}  // namespace dr
#include "conv_wino.h"   // k_conv_w: k_conv with the y axis of a 3-tap stride-1 layer in Winograd F(2,3) form (two thirds of the MFMAs)
namespace dr {
template <int CI> __host__ __device__ inline int conv_a_unit(int pos, int c4);
}
#include "conv_march.h"  // k_conv_m: marching producer/consumer kernel for the stride-1 3x3 / 3x3x3 layers (and their Winograd form)
namespace dr {

// ------------------------------------------------------------------------------------------------
// Host side: the planner is conv_plan.h; here its device arena and the launches.

struct DeviceArena {  // owns small device buffers created while planning (weights, tables)
  std::vector<void *> ptrs;
  int *err_flag = nullptr;  // where k_conv_m reports a wait that gave up (device-visible memory owned by the caller)
  template <class T>
  T *upload(const std::vector<T> &h) {
    T *d = dalloc<T>(h.size());
    DR_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    ptrs.push_back(d);
    return d;
  }
  ~DeviceArena() { for (void *p : ptrs) dfree(p); }
};

// MaxDynamicSharedMemorySize is a per-device attribute of each kernel: the opt-in is tracked per (device, instance).
inline void conv_allow_big_lds(const void *fn, std::atomic<unsigned long long> &done, size_t lds_bytes) {
  if (lds_bytes <= 64 * 1024) return;
  int dev = 0;
  DR_HIP(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return;
  DR_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kConvMaxLds));
  done.fetch_or(bit, std::memory_order_release);
}
template <int CI, int CT, int PT, int FZ = 0>
inline void launch_conv_inst(const ConvLaunch &c, hipStream_t st) {
  static std::atomic<unsigned long long> done{0};  // bit d: set on device d
  conv_allow_big_lds(reinterpret_cast<const void *>(&k_conv<CI, CT, PT, FZ>), done, c.lds_bytes);
  hipLaunchKernelGGL((k_conv<CI, CT, PT, FZ>), c.grid, dim3(kConvThreads), c.lds_bytes, st, c.args);
}
#ifdef DR_PARITY_HOOKS
template <int CI, int CT, int PT>
inline void launch_conv_b_inst(const ConvLaunch &c, hipStream_t st) {
  static std::atomic<unsigned long long> done{0};
  conv_allow_big_lds(reinterpret_cast<const void *>(&k_conv_b<CI, CT, PT>), done, c.lds_bytes);
  hipLaunchKernelGGL((k_conv_b<CI, CT, PT>), c.grid, dim3(kConvThreads), c.lds_bytes, st, c.args);
}
#endif
template <int CI, int CT, int PT>
inline void launch_conv_c_inst(const ConvLaunch &c, hipStream_t st) {
  static std::atomic<unsigned long long> done{0};
  conv_allow_big_lds(reinterpret_cast<const void *>(&k_conv_c<CI, CT, PT>), done, c.lds_bytes);
  hipLaunchKernelGGL((k_conv_c<CI, CT, PT>), c.grid, dim3(kConvThreads), c.lds_bytes, st, c.args);
}
template <int CI, int CT, int PT>
inline void launch_conv_a_inst(const ConvLaunch &c, hipStream_t st) {
  static std::atomic<unsigned long long> done{0};
  conv_allow_big_lds(reinterpret_cast<const void *>(&k_conv_a<CI, CT, PT>), done, c.lds_bytes);
  hipLaunchKernelGGL((k_conv_a<CI, CT, PT>), c.grid, dim3(kConvAThreads), c.lds_bytes, st, c.args);
}
template <int CI, int CT, int PT>
inline void launch_conv_w_inst(const ConvLaunch &c, hipStream_t st) {
  static std::atomic<unsigned long long> done{0};
  conv_allow_big_lds(reinterpret_cast<const void *>(&k_conv_w<CI, CT, PT>), done, c.lds_bytes);
  hipLaunchKernelGGL((k_conv_w<CI, CT, PT>), c.grid, dim3(kConvThreads), c.lds_bytes, st, c.args);
}
template <int CI, int NUP, int CT, int PT, int FZ = 0, int NCW = 8, int W = 0>
inline void launch_conv_m_inst(const ConvLaunch &c, hipStream_t st) {
  static std::atomic<unsigned long long> done{0};
  conv_allow_big_lds(reinterpret_cast<const void *>(&k_conv_m<CI, NUP, CT, PT, FZ, NCW, W>), done, c.lds_bytes);
  hipLaunchKernelGGL((k_conv_m<CI, NUP, CT, PT, FZ, NCW, W>), c.grid, dim3(64 * (NCW + (FZ ? kMarchFzProducers : kMarchProducers))), c.lds_bytes, st, c.args, c.march);
}
// The dispatcher expands from the instance lists of conv_plan.h, the ones the planner's predicates expand from.
inline void launch_conv(const ConvLaunch &c, hipStream_t st) {
#define DR_LAUNCH3(LAUNCH, CI_, CT_, PT_) if (c.ci == CI_ && c.ct == CT_ && c.pt == PT_) { LAUNCH<CI_, CT_, PT_>(c, st); return; }
#define DR_LAUNCH5(W_, CI_, NUP_, CT_, PT_, NCW_) if (c.ci == CI_ && c.nup == NUP_ && c.ct == CT_ && c.pt == PT_ && c.ncw == NCW_) { launch_conv_m_inst<CI_, NUP_, CT_, PT_, 0, NCW_, W_>(c, st); return; }
#ifndef DR_PARITY_HOOKS
  if (c.bf3) fail(DR_ERR_UNSUPPORTED, "launch_conv: the bf16 x 3 kernel is built with -DDR_PARITY_HOOKS only");
#else
  if (c.bf3) {
    if (!c.async && !c.fz) {
#define DR_X(CI_, CT_, PT_) DR_LAUNCH3(launch_conv_b_inst, CI_, CT_, PT_)
      DR_CONV_B_INSTANCES(DR_X)
#undef DR_X
    }
    fail(DR_ERR_ARG, "launch_conv: no bf16x3 instance CI=%d CT=%d", c.ci, c.ct);
  }
#endif
#ifndef DR_PARITY_HOOKS  // the fused-skip forms (FeatureNet's stage-3 head in its literal order) are instantiated in the parity build only
  if (c.fz) fail(DR_ERR_UNSUPPORTED, "launch_conv: fused-skip kernels are built with -DDR_PARITY_HOOKS only");
#else
  if (c.async == 2 && c.fz) {
    if (c.fz != 8 || c.ci != 16 || c.nup != 12 || c.ct != 1 || c.ncw != 8) fail(DR_ERR_ARG, "launch_conv: no fused-skip marching instance FZ=%d CI=%d NUP=%d CT=%d", c.fz, c.ci, c.nup, c.ct);
    if (c.pt == 4) launch_conv_m_inst<16, 12, 1, 4, 8>(c, st);
    else launch_conv_m_inst<16, 12, 1, 2, 8>(c, st);
    return;
  }
#endif
  if (c.async == 2 && c.march.wino == 2) {
#define DR_X(CI_, NUP_, CT_, PT_, NCW_) DR_LAUNCH5(2, CI_, NUP_, CT_, PT_, NCW_)
    DR_MARCH_W_INSTANCES(DR_X)
#undef DR_X
  }
#ifdef DR_PARITY_HOOKS  // the gather order: superseded on every instance (ConvPolicy::march_w_order), kept for the side-by-side tests
  if (c.async == 2 && c.march.wino) {
#define DR_X(CI_, NUP_, CT_, PT_, NCW_) DR_LAUNCH5(1, CI_, NUP_, CT_, PT_, NCW_)
    DR_MARCH_W_INSTANCES(DR_X)
#undef DR_X
  }
#endif
  if (c.async == 2 && c.march.wino) {
    fail(DR_ERR_ARG, "launch_conv: no Winograd marching instance CI=%d NUP=%d CT=%d PT=%d waves=%d", c.ci, c.nup, c.ct, c.pt, c.ncw);
  }
  if (c.async == 2) {
#define DR_X(CI_, NUP_, CT_, PT_, NCW_) DR_LAUNCH5(0, CI_, NUP_, CT_, PT_, NCW_)
    DR_MARCH_INSTANCES(DR_X)
#undef DR_X
    fail(DR_ERR_ARG, "launch_conv: no marching instance CI=%d NUP=%d CT=%d PT=%d waves=%d", c.ci, c.nup, c.ct, c.pt, c.ncw);
  }
  if (c.async == 4) {
#define DR_X(CI_, CT_, PT_) DR_LAUNCH3(launch_conv_w_inst, CI_, CT_, PT_)
    DR_CONV_W_INSTANCES(DR_X)
#undef DR_X
    fail(DR_ERR_ARG, "launch_conv: no Winograd instance CI=%d CT=%d PT=%d", c.ci, c.ct, c.pt);
  }
  if (c.async) {
    if (c.ci == 4 && c.ct == 1 && c.pt == 1) fail(DR_ERR_ARG, "launch_conv: no async instance CI=4 PT=1");
#define DR_X(CI_, CT_, PT_) DR_LAUNCH3(launch_conv_a_inst, CI_, CT_, PT_)
    DR_CONV_A_INSTANCES(DR_X)
#undef DR_X
    fail(DR_ERR_ARG, "launch_conv: no async instance CI=%d CT=%d PT=%d", c.ci, c.ct, c.pt);
  }
#ifdef DR_PARITY_HOOKS
  if (c.fz) {
    if (c.fz != 8 || c.ci != 16 || c.ct != 1) fail(DR_ERR_ARG, "launch_conv: no fused-skip instance FZ=%d CI=%d CT=%d", c.fz, c.ci, c.ct);
    if (c.pt == 4) launch_conv_inst<16, 1, 4, 8>(c, st);
    else launch_conv_inst<16, 1, 1, 8>(c, st);
    return;
  }
#endif
  if (c.args.class_loop > 0) {
#define DR_X(CI_, CT_, PT_) DR_LAUNCH3(launch_conv_c_inst, CI_, CT_, PT_)
    DR_CONV_C_INSTANCES(DR_X)
#undef DR_X
    fail(DR_ERR_ARG, "launch_conv: no class-loop instance CI=%d CT=%d PT=%d", c.ci, c.ct, c.pt);
  }
#define DR_X(CI_, CT_, PT_) DR_LAUNCH3(launch_conv_inst, CI_, CT_, PT_)
  DR_CONV_INSTANCES(DR_X)
#undef DR_X
#undef DR_LAUNCH3
#undef DR_LAUNCH5
  fail(DR_ERR_ARG, "launch_conv: no instance CI=%d CT=%d", c.ci, c.ct);
}

}  // namespace dr
