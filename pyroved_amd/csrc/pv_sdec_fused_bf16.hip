// pv_sdec_fused_bf16.hip — the fused persistent spatial-decoder forward+backward kernel with the 128x128
// contractions on the bf16 matrix cores in SPLIT precision ("bf16x3"):
//      x = hi + lo  (hi = bf16(x), lo = bf16(x - hi));   a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi   (fp32 accumulate)
// Each product carries ~2^-16 relative error (the dropped lo*lo term and the residual of the split), i.e.
// fp32-class results (the parity tests hold it to the same 1e-4 bar as the f32-MFMA kernel) at 3/16 of the
// f32-input MFMA's matrix time: v_mfma_f32_16x16x32_bf16 does 8x the k of v_mfma_f32_16x16x4_f32 in about half
// the cycles.  Everything outside the two hidden layers' GEMMs (coordinate layer, tanh, logit, likelihood,
// reductions) stays fp32.
//
// Mapping.  One persistent 256-thread workgroup per CU = 4 waves, ONE per SIMD, each with the full 512-register
// budget (the 8-wave / 256-register form of this kernel spilled its persistent accumulators to scratch every
// tile).  A tile is 64 rows: each wave carries one 16-row unit.  As in pv_sdec_fused.hip:
//   * layers are computed transposed, D[j][r] = sum_k W[j][k] h[r][k], so the 16x16 C/D layout of one layer is
//     the B-operand layout of the next: activations stay in registers through forward and dgrad;
//   * a wave owns two 16x128 slices of dW1 and dW2 in accumulators for the whole kernel and the workgroup
//     exchanges (dpre, h) through LDS for the wgrad;
//   * per-workgroup partial gradients are reduced in a fixed order afterwards (no float atomics).
// What the bf16 split changes:
//   * weights live in LDS as bf16 hi and lo images, row-major [128][128] with permuted columns and XOR-swizzled
//     16-byte chunks (pv_fb_layout.h); the
//     forward reads a lane's A operand with one ds_read_b128, the dgrad reads the TRANSPOSED operand from the same
//     image with ds_read_b64_tr_b16 (hardware 4x16 transpose), so one image serves both orientations;
//   * activations are split to (hi, lo) once per tensor (3 VALU per element) and the split feeds both the next
//     contraction and the wgrad exchange;
//   * LDS OVERLAY.  The two layers' weight images fill 128 of the 160 KB, which leaves no room to stage a whole
//     tile's (dpre, h) for the wgrad.  So the staging area of layer 2's wgrad lies OVER W1's images (idle between
//     the forward of layer 1 and the dgrad of layer 1) and that of layer 1's wgrad and of the coordinate layer's
//     reductions OVER W2's images (idle from the dgrad of layer 2 to the next tile's forward of layer 2); the
//     overwritten images come back by LDS-DMA (global_load_lds_dwordx4, no registers, asynchronous) from a
//     pre-split global copy made once per step (pv_fb_prep_kernel), under the dgrad of layer 2 resp. the next
//     tile's coordinate layer + forward of layer 1.  One staging pass per layer then covers all 64 rows: the
//     wgrad contracts 32 rows per v_mfma_f32_16x16x32_bf16 (operands by ds_read_b64_tr_b16; bias gradients ride
//     along as an MFMA against ones) and a tile needs 6 workgroup barriers instead of 24;
//   * column sums that need no other wave's rows (d(wo), and dhz / dWc of the coordinate layer) are wave-local
//     transposes through the wave's own rows of whichever staging area is dead at that moment (fb_colsum).
#include "pv_sdec_fused.h"
#include "pv_fb_layout.h"
#include "pv_sdec_prims.h"
#include "pv_kernels.h"        // PvHeadBwd, pv_head_dz / pv_head_bwd_math: the own-sample epilogue's latent backward
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

typedef int int4_ __attribute__((ext_vector_type(4)));

#define FB_WAVES 4               // waves per workgroup (one per SIMD), one 16-row unit each
#define TILE_UNITS FB_WAVES      // units per workgroup tile
#define TILE_ROWS (TILE_UNITS * FD_UNIT)
#define ST_ARR (TILE_ROWS * LDS2)          // elements of one staging array (64 rows)
#define ST_BYTES (2 * ST_ARR)              // 18,432
// byte offsets in dynamic LDS:  [ weight images and staging areas (FbLds<PREC>) | vectors ... ]
#define FB_TOP_BYTES (4 * IMG_BYTES + 3 * ST_BYTES - IMG_BYTES)   // 153,600: the largest map (three staging arrays over a lo image)
#define BO_VEC FB_TOP_BYTES                // fp32 vectors: Wc0, Wc1, bc, wo, b1, b2 (128 each)
#define BO_INFO (BO_VEC + 6 * FD_H * 4)    // per row of the tile (each wave its own 16): x0[64], x1[64], (fp16 modes) 2^e[64]
#define BO_RED (BO_INFO + 768)
#define BO_CHZ (BO_RED + 256)              // next tile's per-unit inputs, fetched by LDS-DMA a tile ahead:
#define BO_CTP (BO_CHZ + FB_WAVES * FD_H * 4)   //   hz[b] (128 floats), tp[b] (8 of 64 floats), grid rows (16*cd of 64)
#define BO_CGR (BO_CTP + FB_WAVES * 256)
#define BO_TAILV (BO_CGR + FB_WAVES * 256)  // column-parallel tail (H231 build): column-sum vectors [3][128] + per-wave row partials [2][4][16]
#define FB_LDS_BYTES (BO_TAILV + 2048)
#define FB_THREADS (64 * FB_WAVES)
#ifndef FB_GB
#define FB_GB 2                  // output blocks per operand group of the layer loops (8 / FB_GB groups per k-block)
#endif
#define FB_GPM (8 / FB_GB)
#ifndef FB_DGD
#define FB_DGD 1                 // operand prefetch distance (groups) of the dgrad loops
#endif
// ---- precision modes (template parameter PREC) -------------------------------------------------------------------------------
//   FB_P_BF16  plain bf16 operands, one product per contraction (plan.fused = 3 on small problems)
//   FB_P_X3    bf16 hi + lo everywhere, three products (rounds 1-3's fp32-class kernel)
//   FB_P_H221  (round 4) fp16: the WEIGHTS are two exact pieces, activations and dL/dpre ONE piece: forward 2 products, dgrad 2,
//              wgrad 1.  A weight's rounding error is systematic (the same perturbation in every one of the 2e5 rows), an
//              activation's is independent from row to row and averages out of every sum the step forms — so only the weights
//              keep their second piece.  5 product passes instead of 9, no 3-instruction split of every activation, half the
//              staging traffic.
//   FB_P_H223 / H321 / H333   the same with the wgrad (both operands split), the forward (split activations) or everything at
//              three products: the other corners of the error table (scripts/fb_prec_table.py, profiles/r04_fb_prec_table.txt)
// fp16's narrow exponent is dealt with by exact power-of-two scaling, never by a rounding:
//   * weight images hold s W with max |s W| in [1, 2) (pv_fb_layout.h); the forward un-scales inside tanh's own multiply, the
//     backward CARRIES the scales (dgrad outputs are s x larger) and removes them where a gradient leaves the kernel;
//   * a row's dL/dlogit = m 2^e is split: the mantissa m goes down the dgrad chain (every dL/dpre operand is then O(1..2^12)
//     whatever the data's scale or the row's weight), 2^(e + dl_exp) is folded into the row's STAGED activation (h 2^(e+dl_exp),
//     exact) so the wgrad product is unchanged; the bias gradient contracts dL/dpre against that factor (a 9th column block of
//     the staged rows) instead of against ones; per-row results (dL/dpre0) get 2^e back in fp32.
#define FB_P_BF16 0
#define FB_P_X3 1
#define FB_P_H221 2
#define FB_P_H223 3
#define FB_P_H321 4
#define FB_P_H333 5
#define FB_P_H2A1 6              // dgrad of layer 2 with dL/dpre2 split (3 products), the rest as H221
#define FB_P_H2B1 7              // dgrad of layer 1 with dL/dpre1 split
#define FB_P_H231 8              // both dgrads with split dL/dpre
#define FB_P_H131 9              // H231 whose FORWARD contracts the weights' hi piece only (experiment: is the forward's second product needed?)
template <int P> struct FbP {
  static constexpr bool F16 = P >= 2;                          // fp16 pieces, normalised weights, per-row exponent
  static constexpr int WP = P == FB_P_BF16 ? 1 : 2;            // weight pieces (LDS images per layer)
  static constexpr bool FWD_LO = P == FB_P_X3 || P == FB_P_H321 || P == FB_P_H333;   // forward also contracts the activation's lo piece
  static constexpr bool DGR2_LO = P == FB_P_X3 || P == FB_P_H333 || P == FB_P_H2A1 || P == FB_P_H231 || P == FB_P_H131;   // dgrad of layer 2 also contracts dL/dpre2's lo piece
  static constexpr bool DGR1_LO = P == FB_P_X3 || P == FB_P_H333 || P == FB_P_H2B1 || P == FB_P_H231 || P == FB_P_H131;   // dgrad of layer 1: dL/dpre1's
  static constexpr bool FWD_WLO = WP == 2 && P != FB_P_H131;   // the forward contracts the weights' lo piece
  static constexpr bool WG3 = P == FB_P_X3 || P == FB_P_H223 || P == FB_P_H333;      // wgrad: both operands split, three products
  static constexpr bool HL = FWD_LO || WG3;                    // activations carry a lo piece
  static constexpr bool DL2 = DGR2_LO || WG3;                  // dL/dpre2 / dL/dpre1 carry a lo piece
  static constexpr bool DL1 = DGR1_LO || WG3;
  static constexpr bool DL = DL2 || DL1;
  static constexpr bool KEEP_WO = !HL && !DL;                  // registers to keep d(wo) per lane for the whole kernel
  // fp16 modes whose dL/dpre is split anyway stage the lo pieces too, for the BIAS gradients only: db = sum_rows dpre is a
  // column sum whose terms cancel (to 1e-3 of their size on jiVAE's db2) and one 16-bit piece left it at 5.9e-4
  static constexpr bool BIAS_LO = F16 && DL2 && DL1 && !WG3;
};
#define FB_KAPPA 16.0f           // fp16 modes: dL/dpre2 operands are kappa * s_o * mantissa(dL/dlogit) * wo * (1 - h2^2): |.| <= 32

// LDS map of the weight images and the two staging areas (NST arrays each: NAD_D of dL/dpre pieces, then NAD_H of activation pieces).
//   one piece:                  [ W1h | W2h | st2 | st1 ]                      (no overlay, no reloads)
//   two pieces, NST = 4:        [ W1h W1l | gap 8K | W2h W2l ]   st2 over W1h W1l + gap, st1 over gap + W2h W2l
//   two pieces, NST = 2 or 3:   [ W1h | W1l | gap | W2l | W2h ]   st2 over W1l + gap, st1 over gap + W2l: only the lo images
//                               are overwritten and come back by LDS-DMA (32 KB per layer and tile instead of 64)
// Everything from BO_VEC on sits at the same offsets in all modes.
template <int P> struct FbLds {
  static constexpr bool OV = FbP<P>::WP == 2;
  static constexpr int NAD_D = (FbP<P>::WG3 || FbP<P>::BIAS_LO) ? 2 : 1;      // staging arrays of dL/dpre, of the activations
  static constexpr int NAD_H = FbP<P>::WG3 ? 2 : 1;
  static constexpr int NST = NAD_D + NAD_H;
  static constexpr int NOV = NST == 4 ? 2 : 1;                 // images under a staging area
  static constexpr int GAP = OV ? NST * ST_BYTES - NOV * IMG_BYTES : 0;
  static constexpr int W1H = 0;
  static constexpr int W1L = IMG_BYTES;
  static constexpr int W2H = !OV ? IMG_BYTES : (NST == 4 ? 2 * IMG_BYTES + GAP : 3 * IMG_BYTES + GAP);
  static constexpr int W2L = !OV ? 0 : (NST == 4 ? 3 * IMG_BYTES + GAP : 2 * IMG_BYTES + GAP);
  static constexpr int ST2 = !OV ? 2 * IMG_BYTES : (NST == 4 ? 0 : IMG_BYTES);
  static constexpr int ST1 = !OV ? 2 * IMG_BYTES + 2 * ST_BYTES : 2 * IMG_BYTES;
  // what a staging area overwrites: LDS offset, offset in the global image copy (W1h W1l W2h W2l), bytes
  static constexpr int RL1_LDS = NST == 4 ? 0 : IMG_BYTES, RL1_SRC = RL1_LDS, RL_BYTES = NOV * IMG_BYTES;
  static constexpr int RL2_LDS = NST == 4 ? W2H : W2L, RL2_SRC = NST == 4 ? 2 * IMG_BYTES : 3 * IMG_BYTES;
  static_assert(GAP >= 0, "staging overlays");
  static_assert(!OV || (ST2 + NST * ST_BYTES <= 2 * IMG_BYTES + GAP && ST1 + NST * ST_BYTES <= 4 * IMG_BYTES + GAP), "overlay");
  static_assert((OV ? 4 * IMG_BYTES + GAP : 2 * IMG_BYTES + 4 * ST_BYTES) <= BO_VEC, "images and staging end before the vectors");
};
static_assert(IMG_BYTES % (FB_WAVES * 1024) == 0, "image reload: whole 1 KB LDS-DMA pieces per wave");
static_assert(FB_LDS_BYTES <= 160 * 1024, "LDS budget");

// The stage fences of the elementwise phases and layer loops: __builtin_amdgcn_sched_barrier(mask), mask 0 = nothing crosses.
// NOT to be relaxed under the iterative-ILP strategy this file is compiled with (Makefile): masks 0x2 / 0x6 (VALU, SALU may cross)
// measure another 0.9-1.4 % faster there and produce WRONG gradients in the H231 builds (35 parity tests fail; the same masks
// with the default scheduler, and mask 0 with iterative-ILP, pass everything) — profiles/r06l_sched_strategy.txt.
#ifndef FB_FENCE_MASK
#define FB_FENCE_MASK 0
#endif
#ifdef FB_NO_FENCE
#define FB_FENCE() do { } while (0)
#else
#define FB_FENCE() __builtin_amdgcn_sched_barrier(FB_FENCE_MASK)
#endif
// (per group of sites, for the experiment of profiles/r06l_sched_strategy.txt: A forward layer loop, B dgrad layer loop, C tanh stages,
//  D weight-gradient consume loop)
#ifndef FB_FENCE_MASK_A
#define FB_FENCE_MASK_A FB_FENCE_MASK
#endif
#ifndef FB_FENCE_MASK_B
#define FB_FENCE_MASK_B FB_FENCE_MASK
#endif
#ifndef FB_FENCE_MASK_C
#define FB_FENCE_MASK_C FB_FENCE_MASK
#endif
#ifndef FB_FENCE_MASK_D
#define FB_FENCE_MASK_D FB_FENCE_MASK
#endif
#define FB_FENCE_A() __builtin_amdgcn_sched_barrier(FB_FENCE_MASK_A)
#ifndef FB_FENCE_MASK_B1
#define FB_FENCE_MASK_B1 FB_FENCE_MASK_B
#endif
#ifndef FB_FENCE_MASK_B2
#define FB_FENCE_MASK_B2 FB_FENCE_MASK_B
#endif
#define FB_FENCE_B1() __builtin_amdgcn_sched_barrier(FB_FENCE_MASK_B1)      // dgrad loop: between the operand requests and the MFMA group
#define FB_FENCE_B2() __builtin_amdgcn_sched_barrier(FB_FENCE_MASK_B2)      // dgrad loop: behind the MFMA group
#define FB_FENCE_C() __builtin_amdgcn_sched_barrier(FB_FENCE_MASK_C)
#define FB_FENCE_D() __builtin_amdgcn_sched_barrier(FB_FENCE_MASK_D)
// 16-bit operands travel as bf16x4 / bf16x8 bit containers in every mode; F16 picks the instruction that reads them
template <bool F16> __device__ __forceinline__ f32x4 fb_mma(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_, a), __builtin_bit_cast(half8_, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float fb_tanh(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// forward layer of the wave's unit: out = bias + W in (pre-activation on return; times the images' scale in the fp16
// modes, whose bias vector is stored scaled); `in` arrives as 16-bit pieces (hi, and lo where the mode has one) per C/D
// block.  Stream: per k-block m (32 k's) and group of FB_GB output blocks read the weight operands (hi / lo, one group
// ahead) and issue FB_GB MFMAs per product: hi x hi, [hi x lo], [lo x hi] — independent accumulator chains.
template <int P>
__device__ __forceinline__ void fb_layer_fwd(const __bf16* __restrict__ Wh, const __bf16* __restrict__ Wl,
                                             const float* __restrict__ bs, const bf16x4 (&ih)[8],
                                             const bf16x4 (&il)[8], f32x4 (&out)[8], int r, int q, int qs) {
  constexpr bool F16 = FbP<P>::F16, WL = FbP<P>::FWD_WLO, AL = FbP<P>::FWD_LO;
  const bool sw = qs && q >= 2;                          // q-swapped images: this lane's chunk holds [h = 1 | h = 0]
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) out[ob] = *reinterpret_cast<const f32x4*>(bs + 16 * ob + 4 * q);
  // row 16*ob + r, logical chunk 4m + q  ->  physical chunk 4*(m ^ (r&3)) + (q ^ SL[r>>2])
  r |= sd_opaque0();
  const int lbase = r * LDB + 8 * (q ^ fb_sl(r >> 2));
  const __bf16* ah = Wh + lbase;
  const __bf16* al = Wl + lbase;
  int xm[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) xm[m] = 32 * (m ^ (r & 3));
  bf16x8 wh[2][FB_GB], wl[2][FB_GB];
  auto load = [&](int g, bf16x8 (&h)[FB_GB], bf16x8 (&l)[FB_GB]) {
    const int m = g / FB_GPM, op = (g % FB_GPM) * FB_GB;
#pragma unroll
    for (int o = 0; o < FB_GB; ++o) {
      const int off = 16 * (op + o) * LDB + xm[m];
      h[o] = *reinterpret_cast<const bf16x8*>(ah + off);
      if (WL) l[o] = *reinterpret_cast<const bf16x8*>(al + off);
    }
  };
  load(0, wh[0], wl[0]);
#pragma unroll
  for (int g = 0; g < 4 * FB_GPM; ++g) {
    const int m = g / FB_GPM, op = (g % FB_GPM) * FB_GB;
    if (g + 1 < 4 * FB_GPM) load(g + 1, wh[(g + 1) & 1], wl[(g + 1) & 1]);
    FB_FENCE_A();
    const bf16x8 bh = sd_catq(ih[2 * m], ih[2 * m + 1], sw);
    const bf16x8(&h)[FB_GB] = wh[g & 1];
    const bf16x8(&l)[FB_GB] = wl[g & 1];
#pragma unroll
    for (int o = 0; o < FB_GB; ++o) out[op + o] = fb_mma<F16>(h[o], bh, out[op + o]);
    if (AL) {
      const bf16x8 bl = sd_catq(il[2 * m], il[2 * m + 1], sw);
#pragma unroll
      for (int o = 0; o < FB_GB; ++o) out[op + o] = fb_mma<F16>(h[o], bl, out[op + o]);
    }
    if (WL) {
#pragma unroll
      for (int o = 0; o < FB_GB; ++o) out[op + o] = fb_mma<F16>(l[o], bh, out[op + o]);
    }
    FB_FENCE_A();
  }
}

// dgrad of the wave's unit: out[k] = sum_j W[j][k] dp[j]; A = W^T via the transposing LDS read; dp arrives as pieces
template <int P, bool AL>
__device__ __forceinline__ void fb_layer_dgrad(const __bf16* __restrict__ Wh, const __bf16* __restrict__ Wl,
                                               const bf16x4 (&ih)[8], const bf16x4 (&il)[8], f32x4 (&out)[8], int r,
                                               int q, int qs) {
  constexpr bool F16 = FbP<P>::F16, WL = FbP<P>::WP == 2;
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) out[kb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // lane i of 16-lane group q points at W[j0 + i/4][16*kb + 4*(i%4)], j0 = 32m + 4q (+16): after the transpose
  // lane k' holds W[j0 .. j0+3][16*kb + k']
  // (rows j0 + r/4 with j0 = 32m + 4q (+16): swizzle 4*(r>>2) + SL[q]; logical chunk 4*kk + (r&3), kk = kb/2)
  r |= sd_opaque0();
  // (q-swapped images: piece r&3 of column block 2 kk + h sits in half h ^ ((r&3) >> 1))
  const int toff = (4 * q + (r >> 2)) * LDB + 8 * ((r & 3) ^ fb_sl(q));
  const int hs = qs ? 4 * ((r >> 1) & 1) : 0;
  const __bf16* ahx[2] = {Wh + toff + hs, Wh + toff + 4 - hs};
  const __bf16* alx[2] = {Wl + toff + hs, Wl + toff + 4 - hs};
  int xk[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) xk[kk] = 32 * (kk ^ (r >> 2));
  bf16x8 wh[FB_DGD + 1][FB_GB], wl[FB_DGD + 1][FB_GB];      // operands FB_DGD groups ahead (transposing reads are slow)
  auto load = [&](int g, bf16x8 (&h)[FB_GB], bf16x8 (&l)[FB_GB]) {
    const int m = g / FB_GPM, kp = (g % FB_GPM) * FB_GB;
#pragma unroll
    for (int o = 0; o < FB_GB; ++o) {
      const int off = 32 * m * LDB + xk[(kp + o) >> 1];
      const __bf16* ah = ahx[(kp + o) & 1];
      const __bf16* al = alx[(kp + o) & 1];
      h[o] = sd_cat(sd_tr(ah + off), sd_tr(ah + off + 16 * LDB));
      if (WL) l[o] = sd_cat(sd_tr(al + off), sd_tr(al + off + 16 * LDB));
    }
  };
#pragma unroll
  for (int g = 0; g < FB_DGD; ++g) load(g, wh[g], wl[g]);
#pragma unroll
  for (int g = 0; g < 4 * FB_GPM; ++g) {
    const int m = g / FB_GPM, kp = (g % FB_GPM) * FB_GB;
    if (g + FB_DGD < 4 * FB_GPM) load(g + FB_DGD, wh[(g + FB_DGD) % (FB_DGD + 1)], wl[(g + FB_DGD) % (FB_DGD + 1)]);
    FB_FENCE_B1();
    const bf16x8 bh = sd_cat(ih[2 * m], ih[2 * m + 1]);
    const bf16x8(&h)[FB_GB] = wh[g % (FB_DGD + 1)];
    const bf16x8(&l)[FB_GB] = wl[g % (FB_DGD + 1)];
#pragma unroll
    for (int o = 0; o < FB_GB; ++o) out[kp + o] = fb_mma<F16>(h[o], bh, out[kp + o]);
    if (AL) {
      const bf16x8 bl = sd_cat(il[2 * m], il[2 * m + 1]);
#pragma unroll
      for (int o = 0; o < FB_GB; ++o) out[kp + o] = fb_mma<F16>(h[o], bl, out[kp + o]);
    }
    if (WL) {
#pragma unroll
      for (int o = 0; o < FB_GB; ++o) out[kp + o] = fb_mma<F16>(l[o], bh, out[kp + o]);
    }
    FB_FENCE_B2();
  }
}

// Written as STAGES over all 32 values of a lane with scheduling fences in between (round 2): left alone, hipcc walks the
// values two at a time through the dependent chain mul -> exp -> add -> rcp -> fma, and the one wave of a SIMD then pays
// every instruction's latency (~10 cycles each instead of ~6.5; scripts/ubench/valu_rates.hip).
// (sd_tanh8 is this without the leading multiply: its callers' operands arrive pre-scaled by C)
__device__ __forceinline__ void fb_tanh8(f32x4 (&v)[8], float c = SD_C) {       // c: C / (scale carried by v)
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) v[ob] = v[ob] * c;
  FB_FENCE_C();
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[ob][i] = __builtin_amdgcn_exp2f(v[ob][i]);
  FB_FENCE_C();
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) v[ob] = v[ob] + 1.0f;
  FB_FENCE_C();
#pragma unroll
  for (int ob = 0; ob < 8; ++ob)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[ob][i] = __builtin_amdgcn_rcpf(v[ob][i]);
  FB_FENCE_C();
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) v[ob] = 1.0f - 2.0f * v[ob];
  FB_FENCE_C();
}

__device__ __forceinline__ void fb_mul_dtanh(f32x4 (&out)[8], const f32x4 (&h)[8]) {
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) out[kb] = out[kb] * (1.0f - h[kb] * h[kb]);
}

// a unit's rows -> 16-bit pieces per C/D block: hi, and lo = 16-bit(v - hi) where the mode wants it
template <bool F16, bool LO>
__device__ __forceinline__ void fb_presplit(const f32x4 (&v)[8], bf16x4 (&h)[8], bf16x4 (&l)[8]) {
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) {
    if constexpr (F16) {
      const half4_ hh = __builtin_convertvector(v[jb], half4_);
      h[jb] = __builtin_bit_cast(bf16x4, hh);
      if (LO) {
        // lo = fp16(v - hi): the difference is exact, so one mixed-precision fma per value (f16 hi and f32 v in, one rounding into
        // its half of the pair) gives the same bits as cvt, sub, cvt — 4 instructions per four values instead of 10
        typedef unsigned int u32x2_ __attribute__((ext_vector_type(2)));
        const u32x2_ hu = __builtin_bit_cast(u32x2_, hh);
        u32x2_ lu;
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lu[0]) : "v"(hu[0]), "v"(v[jb][0]));
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lu[0]) : "v"(hu[0]), "v"(v[jb][1]));
        asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lu[1]) : "v"(hu[1]), "v"(v[jb][2]));
        asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lu[1]) : "v"(hu[1]), "v"(v[jb][3]));
        l[jb] = __builtin_bit_cast(bf16x4, lu);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (LO) { __bf16 a, b; fb_split(v[jb][i], a, b); h[jb][i] = a; l[jb][i] = b; }
        else h[jb][i] = (__bf16)v[jb][i];
      }
    }
  }
}
__device__ __forceinline__ void fb_zero8(bf16x4 (&h)[8], bf16x4 (&l)[8]) {
  const short4_ z = {0, 0, 0, 0};
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) { h[jb] = __builtin_bit_cast(bf16x4, z); l[jb] = __builtin_bit_cast(bf16x4, z); }
}
// the wave's 16 rows (row = 16 * wave + r) of one staged tensor: hi and lo arrays, row-major [64][LDS2].  Inside
// every 16-column block the four 8-byte pieces are XOR-swizzled by (row>>2)&3: ds_write_b64 is banked mod 32 and
// serviced 16 lanes (16 rows, one q) at a time, and 72-dword rows alone would put rows r and r+4 on the same banks
// (4-way); the transposing reads (sd_stage_toff) undo the swizzle and stay conflict-free.
// (sd_stage_store is the one-array, unscaled form of this; h8_stage_store one array with SCALED)
// SCALED (fp16 modes, the activation operand): every piece times the row's power of two ph (exact), and the row's ph itself
// into column block 8 (the rows' padding) of the hi array: the bias gradient contracts against it (fb_wgrad_consume)
template <bool LO, bool SCALED>
__device__ __forceinline__ void fb_stage_store(__bf16* __restrict__ sh, __bf16* __restrict__ sl, const bf16x4 (&h)[8],
                                               const bf16x4 (&l)[8], int row, int q, half4_ ph = half4_{}) {
  row |= sd_opaque0();
  const int e = row * LDS2 + 4 * (q ^ ((row >> 2) & 3));
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) {
    if constexpr (SCALED) {
      *reinterpret_cast<half4_*>(sh + e + 16 * jb) = __builtin_bit_cast(half4_, h[jb]) * ph;
      if (LO) *reinterpret_cast<half4_*>(sl + e + 16 * jb) = __builtin_bit_cast(half4_, l[jb]) * ph;
    } else {
      *reinterpret_cast<bf16x4*>(sh + e + 16 * jb) = h[jb];
      if (LO) *reinterpret_cast<bf16x4*>(sl + e + 16 * jb) = l[jb];
    }
  }
  if constexpr (SCALED) *reinterpret_cast<half4_*>(sh + e + 16 * 8) = ph;
}

// wgrad of the wave's two 16-row slices (rows 16*(2*wave + s) ..) over the staged tile's 64 rows:
//   dW[j][k] += sum_rows dpre[row][j] h[row][k];   db[j] += sum_rows dpre[row][j]  (MFMA against ones)
// k-step ks contracts rows 32ks .. 32ks+31: lane group q feeds rows 32ks + {4q..4q+3, 16+4q..16+4q+3} of BOTH
// operands (two transposing reads each), which is all the contraction needs.
// (fp16 modes: the bias gradient's second operand is the rows' own factor — column block 8 of the staged activations — the
//  product then being what the weight gradient's is: dpre_n[row][j] * 2^(e_row + dl_exp); BIAS_LO: dL/dpre's lo pieces are
//  staged for this product alone)
// (the 4-wave, per-precision-mode form; w8_wgrad_consume owns one 32 x 64 block per wave with one bf16 piece per operand)
template <int P>
__device__ __forceinline__ void fb_wgrad_consume(const __bf16* st, f32x4 (&accW)[2][8], f32x4 (&accB)[2], int wave,
                                                 int r, int q, int ksteps) {
  constexpr bool F16 = FbP<P>::F16, WG3 = FbP<P>::WG3, AL = WG3 || FbP<P>::BIAS_LO;
  const int toff = sd_stage_toff(r | sd_opaque0(), q);
  const short one = 0x3f80;                           // bf16 1.0
  const short8_ ones_s = {one, one, one, one, one, one, one, one};
  const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_s);
  // two LDS byte addresses (the dpre arrays' and the activation arrays') carry everything that is not a compile-time
  // constant; opaque, so that every read of a k-step is base + immediate — one staging area lies beyond the 16-bit offset
  // field of a ds_read and cost a v_add_u32 per read (pv_sdec_fused_w8.hip: w8_wgrad_consume)
  unsigned la = (unsigned)(size_t)st + 2u * (unsigned)(toff + 32 * wave);
  unsigned lb = (unsigned)(size_t)st + 2u * (unsigned)(FbLds<P>::NAD_D * ST_ARR + toff);
  asm volatile("" : "+v"(la), "+v"(lb));
  constexpr unsigned ROW16 = 2u * 16 * LDS2, ARR = 2u * ST_ARR;
  auto tr_at = [](unsigned addr) {
    const short4_ v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)(size_t)addr);
    return __builtin_bit_cast(bf16x4, v);
  };
  for (int ks = 0; ks < ksteps; ++ks) {
    bf16x8 a_h[2], a_l[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      a_h[s] = sd_cat(tr_at(la + 32u * s), tr_at(la + 32u * s + ROW16));
      if (AL) a_l[s] = sd_cat(tr_at(la + ARR + 32u * s), tr_at(la + ARR + 32u * s + ROW16));
    }
    bf16x8 bh[2][2], bl[2][2];
    auto load = [&](int kp, bf16x8 (&h)[2], bf16x8 (&l)[2]) {
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const unsigned off = 32u * (unsigned)(kp + o);
        h[o] = sd_cat(tr_at(lb + off), tr_at(lb + off + ROW16));
        if (WG3) l[o] = sd_cat(tr_at(lb + ARR + off), tr_at(lb + ARR + off + ROW16));
      }
    };
    load(0, bh[0], bl[0]);
    const bf16x8 bias_b = F16 ? sd_cat(tr_at(lb + 32u * 8), tr_at(lb + 32u * 8 + ROW16)) : ones;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      accB[s] = fb_mma<F16>(a_h[s], bias_b, accB[s]);
      if (AL) accB[s] = fb_mma<F16>(a_l[s], bias_b, accB[s]);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kp = 2 * g;
      if (g + 1 < 4) load(kp + 2, bh[(g + 1) & 1], bl[(g + 1) & 1]);
      FB_FENCE_D();
      const bf16x8(&h)[2] = bh[g & 1];
      const bf16x8(&l)[2] = bl[g & 1];
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int s = 0; s < 2; ++s) accW[s][kp + o] = fb_mma<F16>(a_h[s], h[o], accW[s][kp + o]);
      if (WG3) {
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
          for (int s = 0; s < 2; ++s) accW[s][kp + o] = fb_mma<F16>(a_h[s], l[o], accW[s][kp + o]);
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
          for (int s = 0; s < 2; ++s) accW[s][kp + o] = fb_mma<F16>(a_l[s], h[o], accW[s][kp + o]);
      }
      FB_FENCE_D();
    }
    la += 2 * ROW16; lb += 2 * ROW16;
  }
}

// (the permlane form, as w8_sum_q; x3_sum_q / h8_sum_q are two __shfl_xor)
__device__ __forceinline__ float fb_sum_q(float v) {
  return pv_sum_rows(v);                             // (pv_common.h: v_permlane16/32_swap, the bits of the two shfl_xor sums)
}
// Column sums over a unit's 16 rows of a C/D-layout tensor v (lane (r, q): row r, columns 16*jb + 4q + i), optionally
// also weighted by two per-row scalars: wave-local transpose through LDS.  The wave writes its 16 x 128 fp32 tile
// into `tmp` (its OWN 16 rows of two adjacent staging arrays: 72 + 72 floats per row, which it is about to overwrite
// with its staging anyway), then lane l sums columns 2l, 2l+1 over the rows and adds them into its accumulator slots
// (round 4: the accumulators are two registers each per lane — lane l owns columns 2l, 2l+1 — where they were LDS words updated by
// read-modify-write: 8 KB of LDS freed for the third staging array of the fp16 build).  No workgroup barrier, no cross-lane VALU.
// NWT: 0 plain column sums; 2 also the sums weighted by w1 and by w2; 3 the plain sum weighted by w0 as well (fp16 modes:
// w0 = the row's 2^e, w1 / w2 = 2^e x0 / 2^e x1 — the rows come normalised)
template <int NWT>
__device__ __forceinline__ void fb_colsum(const f32x4 (&v)[8], float* __restrict__ tmp /* &arrA[16*wave][0] */,
                                          float2& acc0, float2& acc1, float2& acc2,
                                          const float* __restrict__ w1, const float* __restrict__ w2, int lane, int r,
                                          int q, const float* __restrict__ w0 = nullptr) {
  // row r: columns 0..63 at tmp[r*72 ..], columns 64..127 at tmp[ST_ARR/2 .. ] (the next array's same row; float units)
  constexpr int HALF = ST_ARR / 2;                       // one bf16 staging array, in floats
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) {
    float* p = tmp + (jb < 4 ? 0 : HALF) + r * (LDS2 / 2) + 16 * (jb & 3) + 4 * q;
    *reinterpret_cast<f32x4*>(p) = v[jb];
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);                    // lgkmcnt(0): the wave's own stores have landed
  const float* c = tmp + (lane < 32 ? 0 : HALF) + 2 * (lane & 31);
  float s0 = 0.0f, s1 = 0.0f, a0 = 0.0f, a1 = 0.0f, b0 = 0.0f, b1 = 0.0f;
  f32x4 wv0[4], wv1[4], wv2[4];                          // the 16 rows' weights: broadcast ds_read_b128
  if (NWT >= 2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wv1[k] = *reinterpret_cast<const f32x4*>(w1 + 4 * k);
      wv2[k] = *reinterpret_cast<const f32x4*>(w2 + 4 * k);
      if (NWT == 3) wv0[k] = *reinterpret_cast<const f32x4*>(w0 + 4 * k);
    }
  }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const float2 x = *reinterpret_cast<const float2*>(c + rr * (LDS2 / 2));
    if (NWT == 3) { const float w = wv0[rr >> 2][rr & 3]; s0 += x.x * w; s1 += x.y * w; }
    else { s0 += x.x; s1 += x.y; }
    if (NWT >= 2) {
      const float u = wv1[rr >> 2][rr & 3], t = wv2[rr >> 2][rr & 3];
      a0 += x.x * u; a1 += x.y * u;
      b0 += x.x * t; b1 += x.y * t;
    }
  }
  acc0.x += s0; acc0.y += s1;
  if (NWT >= 2) {
    acc1.x += a0; acc1.y += a1;
    acc2.x += b0; acc2.y += b1;
  }
}

// ---- column-parallel tail (round 6; the H231 build) --------------------------------------------------------------------------
// At batch 256 a workgroup owns 49 units: twelve full 4-wave tiles and ONE unit more, which row-parallel costs a whole tile's
// dependent chain (1/13 of the launch) for one wave's work.  Here the four waves SHARE that unit, as the 8-wave kernel's tail
// does (pv_sdec_fused_w8.hip): wave w computes the column blocks 2w, 2w + 1 of every layer (a quarter of the matrix and of the
// transcendental instructions) and the waves exchange their 16-bit pieces through LDS.  After an exchange every wave holds the
// unit's whole row set in exactly the registers the row-parallel form keeps, so the weight-gradient staging is the row-parallel
// code run by one wave (wave 0: the 16 rows; wave 1: 16 zero rows — a k-step contracts 32), with the same barriers, LDS overlay
// and image reloads as a full tile.  What differs from the row-parallel arithmetic: sums over a row's 128 columns (the logit,
// the row-local coordinate backward) are four per-wave partial sums added in wave order, and the wave-local column sums
// (d(wo), dL/d(hz), dWc) are 16-lane butterflies — other summation orders of the same fp32 terms.
#ifndef FB_TAIL
#define FB_TAIL 1                // 0: the odd last unit row-parallel, as in rounds 1-5 (A/B builds)
#endif
// LDS of the tail: everything lives in the GAP between the two layers' images (never an image: no reload inside the tail) — one
// 8 KB exchange buffer (halves alternate: h0 | h1, then dpre hi | lo), three COMPACT 16-row staging arrays (the tail's weight
// gradient contracts its 16 rows with v_mfma_f32_16x16x16_f16: no zero rows, no 64-row arrays) and the unit's d(wo) sums; the
// other column sums and the per-wave row partials sit behind the prefetch slots (BO_TAILV)
template <int P> struct FbTailLds {
  using LL = FbLds<P>;
  static constexpr int G0 = 2 * IMG_BYTES;                                       // the gap (W1h | W1l | gap | W2l | W2h)
  static constexpr int E = G0;                                                   // exchange buffer, 2 x 4 KB
  static constexpr int ST_ROWS16 = 16 * LDS2 * 2;                                // bytes of a compact staging array
  static constexpr int SD = E + 8192;                                            // dL/dpre hi, lo
  static constexpr int SA = SD + 2 * ST_ROWS16;                                  // activations (scaled rows + their factor column)
  static constexpr int WOV = SA + ST_ROWS16;                                     // d(wo) column sums [128]
  static constexpr int V = BO_TAILV;                                             // dL/d(hz), dWc0, dWc1 [3][128]
  static constexpr int RP = V + 3 * FD_H * 4;                                    // row partials [2][4][16] (the logit's first, then d0 | d1)
  static_assert(LL::NST == 3 && LL::OV && LL::W1L + IMG_BYTES == G0 && LL::W2L == G0 + LL::GAP, "the tail's LDS map is written for the three-array overlay (H231)");
  static_assert(WOV + FD_H * 4 <= G0 + LL::GAP, "exchange buffer + compact staging + d(wo) fit in the gap");
  static_assert(FB_WAVES * 16 * 36 * 4 <= 2 * ST_ROWS16 && FB_WAVES * 16 * 36 * 4 <= IMG_BYTES, "fb_tail_colsum's transpose buffers");
  static_assert(RP + 2 * 4 * 16 * 4 <= FB_LDS_BYTES && FB_LDS_BYTES <= 160 * 1024, "tail vectors");
};
__device__ __forceinline__ float fb_row16_sum(float v) {       // sum over the 16 lanes of a row (all lanes end with it)
#define FB_DPP_F(X, CTRL) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(X), (CTRL), 0xF, 0xF, false))
  v += FB_DPP_F(v, 0x128);                            // row_ror:8            lane ^ 8
  { const float t = FB_DPP_F(v, 0x141); v += FB_DPP_F(t, 0x1B); }   // lane ^ 4
  v += FB_DPP_F(v, 0x4E);                             // lane ^ 2
  v += FB_DPP_F(v, 0xB1);                             // lane ^ 1
#undef FB_DPP_F
  return v;
}
// Column sums over the unit's 16 rows of the wave's two blocks v (lane (r, q): row r, columns 32 wave + 16 o + 4q + i), weighted
// per row by up to three weight vectors (w[k][row]; null: ones): a wave-local transpose through `tmp` (16 rows x 36 floats of
// this wave's own) — lane l sums column 32 wave + (l & 31) over rows 8 (l >> 5) .. +7, the two halves meet by one half-wave swap.
// A 16-lane DPP butterfly per value (the first cut of this tail) cost 6 dependent VALU per value: 2.4 k cycles for the 24 sums
// of the coordinate layer against ~0.5 k this way.
template <int NW>
__device__ __forceinline__ void fb_tail_colsum(const f32x4 (&v)[2], float* __restrict__ tmp, const float* __restrict__ w0,
                                               const float* __restrict__ w1, const float* __restrict__ w2, int lane, int r, int q,
                                               float (&out)[3]) {
#pragma unroll
  for (int o = 0; o < 2; ++o) *reinterpret_cast<f32x4*>(tmp + r * 36 + 16 * o + 4 * q) = v[o];
  __builtin_amdgcn_s_waitcnt(0xc07f);                    // lgkmcnt(0): the wave's own stores have landed
  const int col = lane & 31, r0 = 8 * (lane >> 5);
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x = tmp[(r0 + k) * 36 + col];
    s0 += w0 ? x * w0[r0 + k] : x;
    if (NW >= 2) s1 += x * w1[r0 + k];
    if (NW >= 3) s2 += x * w2[r0 + k];
  }
  auto meet = [](float a) {
    const unsigned b = __float_as_uint(a);
    auto sw = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  };
  out[0] = meet(s0);
  if (NW >= 2) out[1] = meet(s1);
  if (NW >= 3) out[2] = meet(s2);
}
__device__ __forceinline__ void fb_xchg_put(char* smb, int off, const bf16x4 (&mine)[2], int wave, int lane) {
#pragma unroll
  for (int o = 0; o < 2; ++o) reinterpret_cast<bf16x4*>(smb + off)[(2 * wave + o) * 64 + lane] = mine[o];
}
__device__ __forceinline__ void fb_xchg_get(const char* smb, int off, bf16x4 (&all)[8], int lane) {
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) all[jb] = reinterpret_cast<const bf16x4*>(smb + off)[jb * 64 + lane];
}
// blocks 2 wave, 2 wave + 1 of a forward layer (fb_layer_fwd's arithmetic for two of its eight output blocks)
template <int P>
__device__ __forceinline__ void fb_tail_fwd(const __bf16* __restrict__ Wh, const __bf16* __restrict__ Wl,
                                            const float* __restrict__ bs, const bf16x4 (&ih)[8], f32x4 (&out)[2], int wave,
                                            int r, int q, int qs) {
  constexpr bool F16 = FbP<P>::F16, WL = FbP<P>::FWD_WLO;
  const bool sw = qs && q >= 2;
#pragma unroll
  for (int o = 0; o < 2; ++o) out[o] = *reinterpret_cast<const f32x4*>(bs + 16 * (2 * wave + o) + 4 * q);
  const int lbase = r * LDB + 8 * (q ^ fb_sl(r >> 2)) + 32 * wave * LDB;
  bf16x8 wh[4][2], wl[4][2];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int off = lbase + 16 * o * LDB + 32 * (m ^ (r & 3));
      wh[m][o] = *reinterpret_cast<const bf16x8*>(Wh + off);
      if (WL) wl[m][o] = *reinterpret_cast<const bf16x8*>(Wl + off);
    }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const bf16x8 bh = sd_catq(ih[2 * m], ih[2 * m + 1], sw);
#pragma unroll
    for (int o = 0; o < 2; ++o) out[o] = fb_mma<F16>(wh[m][o], bh, out[o]);
    if (WL) {
#pragma unroll
      for (int o = 0; o < 2; ++o) out[o] = fb_mma<F16>(wl[m][o], bh, out[o]);
    }
  }
}
// blocks 2 wave, 2 wave + 1 of a dgrad layer (fb_layer_dgrad's arithmetic: h x dp_hi, h x dp_lo, l x dp_hi)
template <int P, bool AL>
__device__ __forceinline__ void fb_tail_dgrad(const __bf16* __restrict__ Wh, const __bf16* __restrict__ Wl, const bf16x4 (&ih)[8],
                                              const bf16x4 (&il)[8], f32x4 (&out)[2], int wave, int r, int q, int qs) {
  constexpr bool F16 = FbP<P>::F16, WL = FbP<P>::WP == 2;
  const int hs = qs ? 4 * ((r >> 1) & 1) : 0;
#pragma unroll
  for (int o = 0; o < 2; ++o) out[o] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  // (kb = 2 wave + o: kb >> 1 = wave, kb & 1 = o)
  const int toff = (4 * q + (r >> 2)) * LDB + 8 * ((r & 3) ^ fb_sl(q)) + 32 * (wave ^ (r >> 2));
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    bf16x8 h[2], l[2];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int off = toff + 32 * m * LDB + (o ? 4 - hs : hs);
      h[o] = sd_cat(sd_tr(Wh + off), sd_tr(Wh + off + 16 * LDB));
      if (WL) l[o] = sd_cat(sd_tr(Wl + off), sd_tr(Wl + off + 16 * LDB));
    }
    const bf16x8 bh = sd_cat(ih[2 * m], ih[2 * m + 1]);
#pragma unroll
    for (int o = 0; o < 2; ++o) out[o] = fb_mma<F16>(h[o], bh, out[o]);
    if (AL) {
      const bf16x8 bl = sd_cat(il[2 * m], il[2 * m + 1]);
#pragma unroll
      for (int o = 0; o < 2; ++o) out[o] = fb_mma<F16>(h[o], bl, out[o]);
    }
    if (WL) {
#pragma unroll
      for (int o = 0; o < 2; ++o) out[o] = fb_mma<F16>(l[o], bh, out[o]);
    }
  }
}
// the tail's weight gradient: dW[j][k] += sum over the unit's 16 rows of dpre[row][j] h[row][k] (+ the bias gradient against the
// rows' factor column) from COMPACT staging arrays (dpre hi | dpre lo at sd, activations at sa; fb_stage_store's row layout) with
// the 16-row matrix instruction — fb_wgrad_consume's arithmetic for one half k-step
template <int P>
__device__ __forceinline__ void fb_wgrad_consume16(const __bf16* sd, const __bf16* sa, f32x4 (&accW)[2][8], f32x4 (&accB)[2],
                                                   int wave, int r, int q) {
  static_assert(FbP<P>::F16 && FbP<P>::BIAS_LO && !FbP<P>::WG3, "H231");
  const int toff = sd_stage_toff(r, q);
  auto tr4 = [](const __bf16* p_) { return __builtin_bit_cast(half4_, sd_tr(p_)); };
  half4_ a_h[2], a_l[2];
#pragma unroll
  for (int s_ = 0; s_ < 2; ++s_) {
    a_h[s_] = tr4(sd + toff + 32 * wave + 16 * s_);
    a_l[s_] = tr4(sd + 16 * LDS2 + toff + 32 * wave + 16 * s_);
  }
  const half4_ bias_b = tr4(sa + toff + 16 * 8);
#pragma unroll
  for (int s_ = 0; s_ < 2; ++s_) {
    accB[s_] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_h[s_], bias_b, accB[s_], 0, 0, 0);
    accB[s_] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_l[s_], bias_b, accB[s_], 0, 0, 0);
  }
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) {
    const half4_ b = tr4(sa + toff + 16 * kb);
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_) accW[s_][kb] = __builtin_amdgcn_mfma_f32_16x16x16f16(a_h[s_], b, accW[s_][kb], 0, 0, 0);
  }
}
__device__ __forceinline__ void fb_tanh2(f32x4 (&v)[2], float c) {
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[o][i] = 1.0f - 2.0f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v[o][i] * c) + 1.0f);
}
// two blocks -> fp16 pieces (fb_presplit's arithmetic)
template <bool LO>
__device__ __forceinline__ void fb_presplit2(const f32x4 (&v)[2], bf16x4 (&h)[2], bf16x4 (&l)[2]) {
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const half4_ hh = __builtin_convertvector(v[o], half4_);
    h[o] = __builtin_bit_cast(bf16x4, hh);
    if (LO) {
      typedef unsigned int u32x2_ __attribute__((ext_vector_type(2)));
      const u32x2_ hu = __builtin_bit_cast(u32x2_, hh);
      u32x2_ lu;
      asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lu[0]) : "v"(hu[0]), "v"(v[o][0]));
      asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lu[0]) : "v"(hu[0]), "v"(v[o][1]));
      asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lu[1]) : "v"(hu[1]), "v"(v[o][2]));
      asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lu[1]) : "v"(hu[1]), "v"(v[o][3]));
      l[o] = __builtin_bit_cast(bf16x4, lu);
    }
  }
}

// phase-timing trace (profiling only, enabled by PV_FD_ABLATE bit 256): shader-clock stamps of workgroup 0 /
// wave 0 for its first tiles; read back with pv_debug_read_trace()
__device__ long long fb_trace[256];
#ifdef FB_TRACE
#define FB_STAMP(k)                                                                        \
  do {                                                                                     \
    if ((f.ablate & 256) && g == 0 && tid == 0 && tile_no < 4)                             \
      fb_trace[tile_no * 32 + (k)] = (long long)__builtin_readcyclecounter();              \
  } while (0)
#define FB_KSTAMP(k)                                                                       \
  do {                                                                                     \
    if ((f.ablate & 256) && blockIdx.x == 0 && threadIdx.x == 0)                           \
      fb_trace[200 + (k)] = (long long)__builtin_readcyclecounter();                       \
  } while (0)
#define FB_TSTAMP(k)                                                                       \
  do {                                                                                     \
    if ((f.ablate & 256) && blockIdx.x == 0 && threadIdx.x == 0)                           \
      fb_trace[160 + (k)] = (long long)__builtin_readcyclecounter();                       \
  } while (0)
#else
#define FB_STAMP(k) do { } while (0)     // (the stamps split basic blocks: compiled in only for scripts/gpu_trace.py)
#define FB_KSTAMP(k) do { } while (0)
#define FB_TSTAMP(k) do { } while (0)    // (the column-parallel tail's phases)
#endif

// stand-alone form of the per-step preparation (pv_fb_layout.h); the SVI step runs it inside the encoder's
// first-layer launch instead (pv_encoder.hip)
__global__ __launch_bounds__(256) void pv_fb_prep_kernel(PvFbPrep p) {
  pv_fb_prep(p, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256, 4, (int)(threadIdx.x >> 6));
}

// WT: the WEIGHTED form (pv_sdec_fused_bf16_wt_kernel below; the plain-bf16 and bf16 three-product builds, whose pieces have fp32's
// exponent range): row (sample b, position n) carries a weight of its observation — pwt[n] (shared by all samples) or, with pw_img,
// pwt[row] (the index x is read at) — fetched with the observation one tile ahead; ll and dL/dlogit are multiplied by it in fp32, the
// latter before dL/dpre2 is formed and rounded (so d(bo) and the d(wo) column sums carry it too); a zero weight gives exactly zero
// for both; loc is not weighted.  The two kernels share one body (pv_sdec_fused_bf16_body.inc): the unweighted one's code is what it was.

// LIK: the likelihood is a compile-time choice (the rarely used ones must not cost the Bernoulli kernel registers)
// PREC: FB_P_* (above)
template <bool GRADS, int LIK, int PREC>
__global__ __launch_bounds__(FB_THREADS, 1) void pv_sdec_fused_bf16_kernel(PvFused f, PvEncFold e_arg) {
  (void)e_arg;                                   // (read in the epilogue only, through the kernarg pointer: see there)
  constexpr bool WT = false;
  const float* const pwt = nullptr;
  constexpr int pw_img = 0;
#include "pv_sdec_fused_bf16_body.inc"
}
// the weighted form (pv_ivae_weighted_* with PV_PLAN_FAST_WEIGHTS): a kernel name of its own, so that the unweighted instances keep
// theirs.  The weights travel in PvFused::park (a slot no 4-wave launch reads); pw_img: one weight per observation of every sample
template <bool GRADS, int LIK, int PREC>
__global__ __launch_bounds__(FB_THREADS, 1) void pv_sdec_fused_bf16_wt_kernel(PvFused f, PvEncFold e_arg, int pw_img) {
  (void)e_arg;
  static_assert(PREC == FB_P_X3 || PREC == FB_P_BF16, "weights of any magnitude need the bf16 pieces' exponent range");
  constexpr bool WT = true;
  const float* __restrict__ const pwt = static_cast<const float*>(f.park);
#include "pv_sdec_fused_bf16_body.inc"
}

extern "C" int pv_debug_read_trace(long long* out, int n) {
  if (n > 256) n = 256;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(fb_trace), n * sizeof(long long));
}

// Kernel choice.  Plain bf16 (fused = 3): the 8-wave kernel (pv_sdec_fused_w8.hip) when a workgroup gets at least ~6 of the
// 8 units a tile takes (batch >= ~32 at 28x28; below that most of a 128-row tile would idle and the 4-wave / 64-row kernel
// here is faster: 26 vs 30 us at batch 16).  Split precision (fused = 2): training launches run this file's 4-wave kernel;
// forward-only launches of enough units (decode, evaluate) the 8-wave build of pv_sdec_fused_w8x3.hip (round 3: 6.3 vs 5.0 M
// decoded images/s).  That source's training builds — 8 waves: 245 us, 4 waves: 188 us at batch 256, against 190 us here —
// stay selectable for A/B runs and are parity-tested (tests/test_gpu_parity.py: force_w8x3).
// Round 4: training launches of the fp32-class path run this file's fp16 builds — weights as two exact scaled pieces,
// activations one piece — once the rows a gradient sums are enough for the one-piece operands' independent rounding errors to
// average out (error table: profiles/r04a_fb_prec_table.txt, bars: every gradient tensor 1e-4 vs the oracle):
//   >= FB_H231_MIN_UNITS units (16 384 rows):   H231 (kind 28: dL/dpre split in both dgrads; worst tensor 1.6e-5 at C2)
//   >= FB_H221_MIN_UNITS units (524 288 rows):  H221 (kind 21: one piece everywhere; 6e-5 at C2's 2e5 rows, ~1 / sqrt(rows):
//                                               round 5 moved the gate from 2 M rows to where the model predicts <= 4e-5 and three
//                                               draws of the 64x64 config measure 4.3e-5 ... 5.1e-5 on the worst tensor —
//                                               profiles/r05u_grad_margin_h221_*.txt — C4's decoder launch 357 -> 327 us)
// smaller problems keep the bf16 three-product kernel (kind 0).
// Which build runs is a function of (fused mode, units, launch kind) and of pv_ivae_plan.dec_kernel (`sel`, 0 = by size: ABI v15,
// a PLAN field — no process-wide state).  sel, plain (fused 3): 1 the 4-wave kernel, 2 the 8-wave kernel.  sel, split precision
// (fused 2): 1 the bf16 three-product kernel (kind 0), 21 / 28 the fp16 builds; the experiments build (-DPV_EXPERIMENTS) also
// knows 4 / 8 (pv_sdec_fused_w8x3.hip's training forms), 23 / 31 / 33 / 26 / 27 / 29 (the error table's other corners), 41 / 48
// (pv_sdec_fused_w8h.hip) and, with sel == 0, the environment: PV_W8=0 / 1, PV_X3_KERNEL=old | 4 | 8 | h221 | h223 | ... | w221 | w231.
#ifndef FB_H231_MIN_UNITS
#define FB_H231_MIN_UNITS 1024         // 16 384 rows
#endif
#ifndef FB_H221_MIN_UNITS
#define FB_H221_MIN_UNITS 32768        // 524 288 rows (round 5; rounds 4: 131072 = 2 097 152 rows)
#endif
#ifndef FB_EXPERIMENTS
#ifdef PV_EXPERIMENTS
#define FB_EXPERIMENTS 1               // the error table's other corners (H223 / H321 / H333; Bernoulli training launches only)
#else
#define FB_EXPERIMENTS 0
#endif
#endif
static const int64_t fb_row_cap = (int64_t)1 << 30;          // (the pv_sdec_fused_w8*.hip kernels address rows by 32-bit BYTE offsets)
#ifdef PV_EXPERIMENTS
static int fb_env_plain() {
  static const int v = [] { const char* e = pv_exp_str("PV_W8"); return e ? (atoi(e) == 0 ? 0 : 1) : 2; }();
  return v;
}
static int fb_env_x3() {
  static const int v = [] {
    const char* e = pv_exp_str("PV_X3_KERNEL");
    return !e ? 2 : (e[0] == 'w' ? (atoi(e + 1) == 231 ? 48 : 41) : e[0] == 'o' ? 0 : (e[0] == 'h' ? (atoi(e + 1) == 221 ? 21 : atoi(e + 1) == 223 ? 23 : atoi(e + 1) == 321 ? 31 : atoi(e + 1) == 333 ? 33 : atoi(e + 1) == 231 ? 28 : 2)
                                                    : (atoi(e) == 8 ? 8 : (atoi(e) == 4 ? 4 : 2))));
  }();
  return v;
}
#else
static constexpr int fb_env_plain() { return 2; }
static constexpr int fb_env_x3() { return 2; }
#endif
// The builds `sel` can name, per fused mode; 0 names none (by problem size).  One table for pv_sdec_fused_sel_valid and for the
// resolver: a selection is valid exactly when it has a row that this build of the library contains.
// kind: the split-precision selection as fb_x3_kind returns it — sel itself, but sel 1 is kind 0; kind 8 is also what the size rule
// gives forward-only launches in both builds (exp_only is about naming it for training launches)
struct FbBuild { int fused, sel, kind, family, prec, x3_waves, ds; bool exp_only; };
static const FbBuild fb_builds[] = {
  {3, 1, 0, PV_DEC_W4, FB_P_BF16, 0, 0, false},
  {3, 2, 0, PV_DEC_W8, -1, 0, 0, false},
  {2, 1, 0, PV_DEC_W4, FB_P_X3, 0, 0, false},
  {2, 21, 21, PV_DEC_W4, FB_P_H221, 0, 0, false},
  {2, 28, 28, PV_DEC_W4, FB_P_H231, 0, 0, false},
  {2, 4, 4, PV_DEC_W8X3, -1, 4, 0, true},
  {2, 8, 8, PV_DEC_W8X3, -1, 8, 0, true},
  {2, 23, 23, PV_DEC_W4, FB_P_H223, 0, 0, true},
  {2, 31, 31, PV_DEC_W4, FB_P_H321, 0, 0, true},
  {2, 33, 33, PV_DEC_W4, FB_P_H333, 0, 0, true},
  {2, 26, 26, PV_DEC_W4, FB_P_H2A1, 0, 0, true},
  {2, 27, 27, PV_DEC_W4, FB_P_H2B1, 0, 0, true},
  {2, 29, 29, PV_DEC_W4, FB_P_H131, 0, 0, true},
  {2, 41, 41, PV_DEC_W8H, -1, 0, 0, true},
  {2, 48, 48, PV_DEC_W8H, -1, 0, 1, true},
};
// the row `sel` names for the fused mode; null: 0 (by size) or a selection without a row
static const FbBuild* fb_named(int fused, int sel) {
  for (const FbBuild& b : fb_builds)
    if (b.fused == fused && b.sel == sel) return &b;
  return nullptr;
}
bool pv_sdec_fused_sel_valid(int fused, int sel) {
  if (sel == 0) return true;
  const FbBuild* b = fb_named(fused, sel);
#ifdef PV_EXPERIMENTS
  return b != nullptr;
#else
  return b && !b->exp_only;
#endif
}
static bool fb_use_w8(int64_t units, int sel) {
  const FbBuild* b = fb_named(3, sel);
  const int v = b ? (b->family == PV_DEC_W8 ? 1 : 0) : fb_env_plain();   // 0 / 1 forced by a named row, 2 by problem size
  if (v != 2) return v != 0 && units * FD_UNIT < fb_row_cap;
  return units >= 6 * (int64_t)pv_sdec_fused_grid(units) && units * FD_UNIT < fb_row_cap;
}
// split precision: 0 = this file's 4-wave bf16 kernel, 21 (23 / 31 / 33) = its fp16 builds, 4 / 8 = pv_sdec_fused_w8x3.hip with
// that many waves
static int fb_x3_kind(int64_t units, bool grads, int sel) {
  const FbBuild* named = fb_named(2, sel);
  const int v = sel == 0 ? fb_env_x3() : (named ? named->kind : sel);     // (a selection without a row: fb_x3_build)
  if (v > 8) return grads ? v : (units * FD_UNIT < fb_row_cap && units >= 6 * (int64_t)pv_sdec_fused_grid(units) ? 8 : 0);
  if (units * FD_UNIT >= fb_row_cap) return 0;
  if (v != 2) return v;
  if (grads && units >= FB_H221_MIN_UNITS) return 21;
  if (grads && units >= FB_H231_MIN_UNITS) return 28;
  // training: this file's kernel.  The new source's 4-wave build measures the same (187.9 vs 189.7 us at batch 256 with every
  // offload and the epilogues folded into the consuming k-loops: profiles/r03_decoder_schedule_experiments.txt) — not worth a
  // switch of the two-rounds-tested default; its 8-wave build is slower (245 us).  Forward-only: the 8-wave build by size.
  if (grads) return 0;
  return units >= 6 * (int64_t)pv_sdec_fused_grid(units) ? 8 : 0;
}
// the table's row of a split-precision kind.  A kind without a row — a dec_kernel that pv_sdec_fused_sel_valid refuses, handed
// straight to the resolver — resolves to the split-precision source with a wave count that has no instance: its images (pre-scaled;
// fp16 pieces from kind 9 up), row-major records, four slot waves, and a launch that the launcher refuses.  (Before the table, a
// kind in 9 .. 39 without a build got the 4-wave three-product kernel on unscaled fp16 images instead: DESIGN 4.22.)
static FbBuild fb_x3_build(int kind) {
  for (const FbBuild& b : fb_builds)
    if (b.fused == 2 && b.kind == kind) return b;
  return FbBuild{2, kind, kind, PV_DEC_W8X3, -1, 0, 0, true};
}
static int fb_qswap_on();

// The resolver: the kernel the launch of (fused, units, grads, sel) runs — fb_use_w8 / fb_x3_kind, whose only caller this is — and
// what every consumer reads of it (pv_sdec_fused.h: PvDecChoice)
PvDecChoice pv_sdec_fused_choice(int fused, int64_t units, bool grads, int sel) {
  PvDecChoice c{};
  c.prec = -1; c.waves = 1; c.rec_fmt = PV_REC_ROWMAJOR;
  if (fused < 2) return c;                                             // PV_DEC_F32: no weight images, one slot per workgroup
  const bool x3 = fused == 2;
  int train_kind = 0;                                                  // (split precision: the training launch's kind)
  if (x3) {
    train_kind = fb_x3_kind(units, true, sel);
    const int fwd_kind = fb_x3_kind(units, false, sel);
    const int kind = grads ? train_kind : fwd_kind;
    const FbBuild b = fb_x3_build(kind), t = fb_x3_build(train_kind);
    c.family = b.family; c.prec = b.prec; c.x3_waves = b.x3_waves; c.ds = b.ds;
    c.img_mode = b.family == PV_DEC_W8H ? 2 : (kind > 8 ? 1 : 0);      // (fp16 pieces: every kind above the split-precision source's two)
    c.img_scale = b.family == PV_DEC_W4 ? 0.0f : 2.8853900817779268f;  // (the 8-wave sources want 2 log2(e) W and 2 log2(e) hz)
    c.waves = (train_kind == 8 || t.family == PV_DEC_W8H) ? 8 : FB_WAVES;
    c.rec_fmt = t.family == PV_DEC_W4 ? PV_REC_LANE_F32 : PV_REC_ROWMAJOR;   // (pv_sdec_fused_w8x3 / w8h.hip: row-major)
    c.weighted = train_kind == 0 && fwd_kind == 0;                     // (the bf16 three-product build for both launch kinds)
  } else {
    const bool w8 = fb_use_w8(units, sel);
    c.family = w8 ? PV_DEC_W8 : PV_DEC_W4;
    if (!w8) c.prec = FB_P_BF16;
    c.img_scale = w8 ? 2.8853900817779268f : 0.0f;
    c.waves = w8 ? 8 : FB_WAVES;
    c.rec_fmt = w8 ? PV_REC_LANE_BF16 : PV_REC_LANE_F32;
    c.weighted = !w8;
    c.hosts_guide = w8;
  }
  c.img_qswap = c.img_scale == 0.0f ? fb_qswap_on() : (!x3 && pv_sdec_fused_w8_qswap());
  static const int ablate = pv_exp_int("PV_FD_ABLATE", 0);          // (experiments build, bit 1024: the row-major fp32 form from both kernels)
  if (ablate & 1024) c.rec_fmt = PV_REC_ROWMAJOR;
#ifdef PV_EXPERIMENTS
  c.parks = x3 && train_kind == 8;                    // (parking slots: the 8-wave split-precision TRAINING form only)
#endif
  return c;
}
int64_t PvDecChoice::park_bytes(int grid) const { return parks ? pv_sdec_fused_w8x3_park_bytes(grid) : 0; }

// test hook (not in include/): the resolved choice of (fused, units, grads, sel) as integers — out[0] pv_sdec_fused_sel_valid, then
// family, prec, x3_waves, ds, waves, rec_fmt, parks, park_bytes at pv_sdec_fused_grid(units), img_mode, the bits of img_scale,
// img_qswap, weighted, hosts_guide (14 values).  tests/test_decoder_choice_cpu.py replays a recorded table through it
extern "C" int pv_debug_decoder_choice(int fused, int64_t units, int grads, int sel, int64_t* out) {
  if (!out) return PV_EINVAL;
  const PvDecChoice c = pv_sdec_fused_choice(fused, units, grads != 0, sel);
  unsigned scale_bits;
  memcpy(&scale_bits, &c.img_scale, sizeof scale_bits);
  const int64_t v[14] = {pv_sdec_fused_sel_valid(fused, sel), c.family, c.prec, c.x3_waves, c.ds, c.waves, c.rec_fmt, c.parks,
                         c.park_bytes(pv_sdec_fused_grid(units)), c.img_mode, scale_bits, c.img_qswap, c.weighted, c.hosts_guide};
  for (int i = 0; i < 14; ++i) out[i] = v[i];
  return 0;
}

// measurement hook (not in include/): the kernel a decoder launch of (fused mode, units, grads, likelihood) dispatches, spelled
// the way rocprofv3 prints it — bench.py puts it in `roofline.kernel` so that the line can be matched against
// profiles/*_kernel_stats.csv by name
extern "C" const char* pv_debug_decoder_kernel_name_fold(int grads, int lik) {      // (the launch that hosts the guide: pv_ivae_guide_folds)
  static thread_local char buf[128];
  // (training launches of the plain iVAE step also host the latent backward: build 2, pv_plan.hip's own_chain)
  snprintf(buf, sizeof buf, "void pv_sdec_w8_kernel<%s, %d, %d>(PvFused, PvEncFold)", grads ? "true" : "false", lik, grads ? 2 : 1);
  return buf;
}
extern "C" const char* pv_debug_decoder_kernel_name(int fused, int64_t units, int grads, int lik) {
  static thread_local char buf[128];
  const char* g = grads ? "true" : "false";
  const PvDecChoice c = pv_sdec_fused_choice(fused, units, grads != 0, 0);
  if (fused == 1) snprintf(buf, sizeof buf, "void pv_sdec_fused_kernel<%s>(PvFused)", g);
  else if (fused < 2) snprintf(buf, sizeof buf, "pv_gemm_kernel (layer-by-layer path)");
  else if (c.family == PV_DEC_W8H) snprintf(buf, sizeof buf, "void pv_sdec_w8h_kernel<%d, %s>(PvFused)", lik, c.ds ? "true" : "false");
  else if (c.family == PV_DEC_W8X3) snprintf(buf, sizeof buf, "void pv_sdec_w8x3_kernel<%s, %d, %d>(PvFused)", g, lik, c.x3_waves);
  else if (c.family == PV_DEC_W8) snprintf(buf, sizeof buf, "void pv_sdec_w8_kernel<%s, %d, 0>(PvFused, PvEncFold)", g, lik);
  else snprintf(buf, sizeof buf, "void pv_sdec_fused_bf16_kernel<%s, %d, %d>(PvFused, PvEncFold)", g, lik, c.prec);
  return buf;
}

// ... and the kernel a WEIGHTED decoder launch of the plan's route dispatches (pv_plan.hip: pv_debug_weighted_decoder_kernel_name):
// the 4-wave source in the bf16 build of the mode, which the routed plan's dec_kernel = 1 selects at every size
const char* pv_sdec_fused_bf16_wt_kernel_name(bool x3, int grads, int lik) {
  static thread_local char buf[128];
  const PvDecChoice c = pv_sdec_fused_choice(x3 ? 2 : 3, 0, grads != 0, 1);
  snprintf(buf, sizeof buf, "void pv_sdec_fused_bf16_wt_kernel<%s, %d, %d>(PvFused, PvEncFold, int)", grads ? "true" : "false", lik,
           c.prec);
  return buf;
}

// which column order a launch's weight images are in (pv_fb_layout.h): the 8-wave plain-bf16 kernel reads the q-swapped one
// (-0.6 % of its step); this file's 4-wave kernel the plain one — its transposing reads lose 80 % of their bank conflicts too
// (SQ_LDS_BANK_CONFLICT 8.0 M -> 1.6 M per launch, LDS-array cycles -19 %) and the launch does not move (144.3 vs 144.8 us:
// profiles/r06i_qswap_ab.txt), so it keeps the form without the operand selects.  PV_QSWAP=1 (experiments build) turns it on.
static int fb_qswap_on() {
  static const int v = pv_exp_int("PV_QSWAP", 0);
  return v != 0;
}
PvFbPrep pv_sdec_fused_bf16_prep_args(const PvFused& f, bool grads, const PvDecChoice& c) {
  static_assert(FB_WIMG_BYTES >= FB_SCALE_OFF + 16, "pv_sdec_fused.h and the LDS image layout disagree");
  PvFbPrep p{};
  p.W1 = f.W1; p.W2 = f.W2; p.img = f.wimg; p.zero = f.part_hz; p.wo = f.wo;
  p.nzero4 = grads ? (int64_t)f.B * f.kmax * (FD_H + (f.part_rs ? PV_RS_W : 0)) / 4 : 0;      // (dL/d(hz) slots + the row-sum slots behind them)
  p.mode = c.img_mode; p.scale = c.img_scale; p.qswap = c.img_qswap;
  return p;
}

int pv_sdec_fused_bf16_prep(const PvFused& f, bool grads, const PvDecChoice& c, hipStream_t s) {
  if (!f.wimg) return PV_EINVAL;
  const PvFbPrep p = pv_sdec_fused_bf16_prep_args(f, grads, c);
  const int64_t work = p.nzero4 > FD_H * (FD_H / 4) ? p.nzero4 : FD_H * (FD_H / 4);
  int blocks = (int)((work + 255) / 256);
  if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(pv_fb_prep_kernel, dim3(blocks), dim3(256), 0, s, p);
  PV_LAUNCH_CHECK();
  return 0;
}

int pv_sdec_fused_bf16_launch(const PvFused& f_in, int grid, bool grads, const PvDecChoice& c, hipStream_t s, const PvEncFold* fold,
                              const PvEncFold* chain, int weighted) {
  if (fold && !c.hosts_guide) return PV_EINVAL;       // (the folded guide lives in the 8-wave plain-bf16 kernel)
  // (weighted launches: the weights sit in f.park; no sample weights or repeated observations — pv_ivae_weighted_*'s scope)
  if (weighted && (fold || !f_in.park || f_in.sw || f_in.x_units != 0 || !c.weighted)) return PV_EINVAL;
  if (c.family == PV_DEC_W8) return pv_sdec_fused_w8_launch(f_in, grid, grads, s, fold);
#ifdef PV_EXPERIMENTS
  if (c.family == PV_DEC_W8H) return grads ? pv_sdec_fused_w8h_launch(f_in, grid, s, c) : PV_EINVAL;
#else
  if (c.family == PV_DEC_W8H || (grads && c.family == PV_DEC_W8X3)) return PV_EINVAL;   // (dropped variants: the experiments build)
#endif
  if (c.family == PV_DEC_W8X3) return pv_sdec_fused_w8x3_launch(f_in, grid, grads, s, c);
  if (c.family != PV_DEC_W4) return PV_EINVAL;
  const int prec = c.prec;
  PvFused f = f_in;
  static const int ablate = pv_exp_int("PV_FD_ABLATE", 0);
  f.ablate = ablate;
  f.qswap = fb_qswap_on();
  const size_t lds = FB_LDS_BYTES;
  const void* fn = nullptr;
#define FB_PICK_P(G, L, P) fn = reinterpret_cast<const void*>(&pv_sdec_fused_bf16_kernel<G, L, P>)
#define FB_PICK_WT(G, L)                                                                                    \
  do {                                                                                                      \
    if (prec == FB_P_BF16) fn = reinterpret_cast<const void*>(&pv_sdec_fused_bf16_wt_kernel<G, L, FB_P_BF16>); \
    else fn = reinterpret_cast<const void*>(&pv_sdec_fused_bf16_wt_kernel<G, L, FB_P_X3>);                   \
  } while (0)
#define FB_PICK(G, L)                                                                          \
  do {                                                                                         \
    if (prec == FB_P_BF16) FB_PICK_P(G, L, FB_P_BF16);                                         \
    else FB_PICK_P(G, L, FB_P_X3);                                                             \
  } while (0)
#define FB_PICK_G(L)                                                                           \
  do {                                                                                         \
    if (prec == FB_P_H231) FB_PICK_P(true, L, FB_P_H231);                                      \
    else if (prec == FB_P_H221) FB_PICK_P(true, L, FB_P_H221);                                 \
    else FB_PICK(true, L);                                                                     \
  } while (0)
  if (prec > FB_P_H221 && prec != FB_P_H231 && !(FB_EXPERIMENTS && grads && f.lik == PV_LIK_BERNOULLI)) return PV_EINVAL;
  if (prec >= FB_P_H221 && !grads) return PV_EINVAL;          // (forward-only launches never select the fp16 builds)
  if (weighted) {
    if (prec != FB_P_BF16 && prec != FB_P_X3) return PV_EINVAL;
    if (grads) {
      if (f.lik == PV_LIK_BERNOULLI) FB_PICK_WT(true, PV_LIK_BERNOULLI);
      else if (f.lik == PV_LIK_GAUSSIAN) FB_PICK_WT(true, PV_LIK_GAUSSIAN);
      else if (f.lik == PV_LIK_POISSON_LOG) FB_PICK_WT(true, PV_LIK_POISSON_LOG);
      else FB_PICK_WT(true, PV_LIK_CBERNOULLI);
    } else {
      if (f.lik == PV_LIK_BERNOULLI) FB_PICK_WT(false, PV_LIK_BERNOULLI);
      else if (f.lik == PV_LIK_GAUSSIAN) FB_PICK_WT(false, PV_LIK_GAUSSIAN);
      else if (f.lik == PV_LIK_POISSON_LOG) FB_PICK_WT(false, PV_LIK_POISSON_LOG);
      else FB_PICK_WT(false, PV_LIK_CBERNOULLI);
    }
  } else if (grads) {
    if (f.lik == PV_LIK_BERNOULLI) {
      FB_PICK_G(PV_LIK_BERNOULLI);
#if FB_EXPERIMENTS
      if (prec == FB_P_H223) FB_PICK_P(true, PV_LIK_BERNOULLI, FB_P_H223);
      else if (prec == FB_P_H321) FB_PICK_P(true, PV_LIK_BERNOULLI, FB_P_H321);
      else if (prec == FB_P_H333) FB_PICK_P(true, PV_LIK_BERNOULLI, FB_P_H333);
      else if (prec == FB_P_H2A1) FB_PICK_P(true, PV_LIK_BERNOULLI, FB_P_H2A1);
      else if (prec == FB_P_H2B1) FB_PICK_P(true, PV_LIK_BERNOULLI, FB_P_H2B1);
      else if (prec == FB_P_H131) FB_PICK_P(true, PV_LIK_BERNOULLI, FB_P_H131);
#endif
    }
    else if (f.lik == PV_LIK_GAUSSIAN) FB_PICK_G(PV_LIK_GAUSSIAN);
    else if (f.lik == PV_LIK_POISSON_LOG) {
      // (no fp16 build: their staged per-row exponent holds |dL/dlogit| < 2^15 only — pv_plan.hip: plan_sel keeps Poisson plans off them)
      if (prec >= FB_P_H221) return PV_EINVAL;
      FB_PICK(true, PV_LIK_POISSON_LOG);
    }
    else FB_PICK_G(PV_LIK_CBERNOULLI);
  } else {
    if (f.lik == PV_LIK_BERNOULLI) FB_PICK(false, PV_LIK_BERNOULLI);
    else if (f.lik == PV_LIK_GAUSSIAN) FB_PICK(false, PV_LIK_GAUSSIAN);
    else if (f.lik == PV_LIK_POISSON_LOG) FB_PICK(false, PV_LIK_POISSON_LOG);
    else FB_PICK(false, PV_LIK_CBERNOULLI);
  }
#undef FB_PICK_G
#undef FB_PICK
#undef FB_PICK_WT
#undef FB_PICK_P
  // (per device: a process may drive several; idempotent: a race between host threads only repeats the call)
  PV_TRY(pv_set_dynamic_lds(fn, (int)lds));          // (per device and kernel)
  PvEncFold ec{};                                   // (chain: the own-sample epilogue's latent backward, PvEncFold::chain)
  if (chain && grads) ec = *chain;
  int pw_img = weighted == PV_FDM_W_IMAGES ? 1 : 0;
  void* args[] = {&f, &ec, &pw_img};                 // (the unweighted kernels take the first two)
  hipError_t e2 = hipLaunchKernel(fn, dim3(grid), dim3(FB_THREADS), args, lds, s);
  if (e2 != hipSuccess) return (int)e2;
  PV_LAUNCH_CHECK();
  return 0;
}
