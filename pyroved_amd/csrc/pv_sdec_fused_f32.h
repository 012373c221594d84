// pv_sdec_fused_f32.h — what the f32-MFMA fused decoder kernels share: the LDS layout, the transposed layer / dgrad / wgrad
// streams and the lane sums of pv_sdec_fused.hip (one output channel) and pv_sdec_fused_mc.hip (2 .. 8 output channels).
// Device code only; every function is force-inlined, so a kernel compiles to what it did with these in its own source file.
#pragma once
#include "pv_sdec_fused.h"
#include "pv_sdec_prims.h"     // sd_exp / sd_log / sd_rcp (the rest of it is for the bf16-family kernels)

#define LDW 132        // LDS row stride of the weight images (floats): conflict-free ds_read_b128 over 16 rows
#define LDST 144       // LDS row stride of the staging buffers: stride % 32 == 16 -> conflict-free operand reads
#define OFF_W1 0
#define OFF_W2 (FD_H * LDW)
#define OFF_STA (2 * FD_H * LDW)
#define OFF_STB (OFF_STA + FD_UNIT * LDST)
#define OFF_WC0 (OFF_STB + FD_UNIT * LDST)
#define OFF_WC1 (OFF_WC0 + FD_H)
#define OFF_BC (OFF_WC1 + FD_H)
#define OFF_WO (OFF_BC + FD_H)
#define OFF_B1 (OFF_WO + FD_H)
#define OFF_B2 (OFF_B1 + FD_H)
#define OFF_DWO (OFF_B2 + FD_H)
#define OFF_INFO (OFF_DWO + FD_WAVES * FD_H)
#define OFF_RED (OFF_INFO + 64)
#define FD_LDS_FLOATS (OFF_RED + 64)
#define FD_THREADS (64 * FD_WAVES)


// keeps the machine scheduler from hoisting a whole layer's LDS operand loads ahead of its MFMAs
// (which would need hundreds of VGPRs); the partner wave on the SIMD hides the ds_read latency instead
#define FD_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#ifdef FD_EXP_NO_LDS_OPERANDS   // experiment build only: MFMA weight operands come from one LDS word (no traffic)
#define FD_WADDR(x) 0
#else
#define FD_WADDR(x) (x)
#endif

// tanh(x) = 1 - 2 / (e^{2x} + 1) on the raw v_exp_f32 / v_rcp_f32 (1 ulp each): 5 VALU issues.
// On gfx950 the f32-input MFMA shares the FP32 ALUs with VALU work (measured: every VALU instruction placed
// between two v_mfma_f32_16x16x4_f32 adds ~3.5 cycles to the stream, scripts/ubench/mfma_f32.hip), so the
// activation's instruction count is paid in full.  Absolute error <= ~2e-7 (cancellation near 0 is absolute,
// not relative: harmless for the sums it feeds); FD_TANH_POLY adds an odd polynomial for |x| < 0.125 (+7 issues).
__device__ __forceinline__ float fd_tanh(float x) {
#ifdef FD_EXP_NO_TANH      // experiment build only: prices the VALU cost of the activations
  return x * 0.5f;
#endif
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);       // e^{2x}
  const float t = 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
#ifdef FD_TANH_POLY
  const float x2 = x * x;
  const float p = x * (1.0f + x2 * (-0.33333334f + x2 * 0.13333334f));
  return fabsf(x) < 0.125f ? p : t;
#else
  return t;
#endif
}

// D[j][r] = b[j] + sum_k W[j][k] in[r][k]   (transposed layer, see pv_sdec_fused.hip); `out` is left PRE-activation
// except that, when ACT_HALF0, tanh is applied to out[0..3] while out[4..7] is still accumulating.
// The stream is 16 groups of (4 x ds_read_b128 -> 16 MFMAs); the next group's operands are fetched before the
// current group's MFMAs issue (explicit double buffer) and the scheduling fence keeps the compiler from hoisting
// more.  VALU work is placed INSIDE the groups so it issues in the shadow of this wave's own MFMAs (the two waves
// of a SIMD run in lock-step, so the partner cannot be relied on to cover it):
//   prep(jb) produces the input block in[jb] one group before its first use (the previous layer's activation),
//   and the finished half of the outputs is activated during the second half's groups.
template <bool ACT_HALF0, class Prep>
__device__ __forceinline__ void fd_layer_fwd(const float* __restrict__ Ws, const float* __restrict__ bs,
                                             f32x4 (&in)[8], f32x4 (&out)[8], int r, int q, Prep prep) {
  prep(0);
#pragma unroll
  for (int ob = 0; ob < 8; ++ob) out[ob] = *reinterpret_cast<const f32x4*>(bs + 16 * ob + 4 * q);
  const float* wb = Ws + r * LDW + 4 * q;
  f32x4 a[2][4];
#pragma unroll
  for (int o = 0; o < 4; ++o) a[0][o] = *reinterpret_cast<const f32x4*>(wb + FD_WADDR(16 * o * LDW));
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int half = g >> 3, jb = g & 7, oh = 4 * half;
    if (g + 1 < 16) {
      const int hn = (g + 1) >> 3, jn = (g + 1) & 7;
#pragma unroll
      for (int o = 0; o < 4; ++o)
        a[(g + 1) & 1][o] = *reinterpret_cast<const f32x4*>(wb + FD_WADDR(16 * (4 * hn + o) * LDW + 16 * jn));
    }
    FD_SCHED_FENCE();        // the prefetch must ISSUE before this group's MFMAs (else it is sunk behind them)
    if (half == 0 && jb + 1 < 8) prep(jb + 1);
    if (ACT_HALF0 && half == 1) {
      out[(2 * jb) >> 2][(2 * jb) & 3] = fd_tanh(out[(2 * jb) >> 2][(2 * jb) & 3]);
      out[(2 * jb + 1) >> 2][(2 * jb + 1) & 3] = fd_tanh(out[(2 * jb + 1) >> 2][(2 * jb + 1) & 3]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int o = 0; o < 4; ++o) out[oh + o] = MFMA(a[g & 1][o][i], in[jb][i], out[oh + o]);
    FD_SCHED_FENCE();
  }
}

// D[k][r] = sum_j W[j][k] dp[r][j]   (dgrad); 32 groups of (8 x ds_read_b32 -> 8 MFMAs), operands double-buffered.
// side(g) is independent VALU work issued in the shadow of group g's MFMAs.  No epilogue here.
template <class Side>
__device__ __forceinline__ void fd_layer_dgrad(const float* __restrict__ Ws, const f32x4 (&dp)[8],
                                               f32x4 (&out)[8], int r, int q, Side side) {
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) out[kb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* wb = Ws + 4 * q * LDW + r;
  float a[2][8];
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) a[0][kb] = wb[16 * kb];
#pragma unroll
  for (int g = 0; g < 32; ++g) {
    const int jb = g >> 2, i = g & 3;
    if (g + 1 < 32) {
      const int jn = (g + 1) >> 2, in_ = (g + 1) & 3;
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) a[(g + 1) & 1][kb] = wb[(16 * jn + in_) * LDW + 16 * kb];
    }
    FD_SCHED_FENCE();
    side(g);
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) out[kb] = MFMA(a[g & 1][kb], dp[jb][i], out[kb]);
    FD_SCHED_FENCE();
  }
}

// out *= 1 - h^2   (through the tanh that produced h)
__device__ __forceinline__ void fd_mul_dtanh(f32x4 (&out)[8], const f32x4 (&h)[8]) {
#pragma unroll
  for (int kb = 0; kb < 8; ++kb)
#pragma unroll
    for (int i = 0; i < 4; ++i) out[kb][i] *= 1.0f - h[kb][i] * h[kb][i];
}

__device__ __forceinline__ void fd_stage_write(float* __restrict__ st, const f32x4 (&v)[8], int r, int q) {
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) *reinterpret_cast<f32x4*>(st + r * LDST + 16 * jb + 4 * q) = v[jb];
}

// dW[16*wave + ..][k] += sum over the 16 staged rows of dpre[row][16*wave + j'] * h[row][k]
__device__ __forceinline__ void fd_wgrad_consume(const float* __restrict__ stA, const float* __restrict__ stB,
                                                 f32x4 (&accW)[8], float& db, int wave, int r, int q) {
  const float* ab = stA + q * LDST + 16 * wave + r;
  const float* bb = stB + q * LDST + r;
  float a[2], bv[2][8];
  a[0] = ab[0];
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) bv[0][kb] = bb[16 * kb];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s + 1 < 4) {
      a[(s + 1) & 1] = ab[4 * (s + 1) * LDST];
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) bv[(s + 1) & 1][kb] = bb[4 * (s + 1) * LDST + 16 * kb];
    }
    FD_SCHED_FENCE();
    db += a[s & 1];
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) accW[kb] = MFMA(a[s & 1], bv[s & 1][kb], accW[kb]);
    FD_SCHED_FENCE();
  }
}

__device__ __forceinline__ float fd_sum_q(float v) {      // over the 4 lanes l, l^16, l^32, l^48
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

__device__ __forceinline__ float fd_sum_r(float v) {      // over the 16 lanes of a row group
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}
