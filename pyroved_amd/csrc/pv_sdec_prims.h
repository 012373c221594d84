// pv_sdec_prims.h — the device primitives that the fused spatial-decoder kernels share (pv_sdec_fused.hip, pv_sdec_fused_bf16.hip,
// pv_sdec_fused_w8.hip, pv_sdec_fused_w8x3.hip, pv_sdec_fused_w8h.hip): one copy under the neutral prefix sd_.
// What is here is the SAME text in every kernel that uses it.  Helpers that share a name across those files but differ on purpose
// (*_sum_q, *_wgrad_consume, *_colsum_mfma, h8_tanh8 / fb_tanh8, h8_stage_store / fb_stage_store, h8_mma16, the fp32 kernel's
// likelihood) stay in their files, each with a line saying how it differs.  LDS maps, fences, A/B switches and layer loops are
// per kernel too.
#pragma once
#include "pv_common.h"         // f32x4, pv_cbern, LOG_SQRT_2PI, BERN_EPS
#include "pv_fb_layout.h"      // bf16x4 / bf16x8, fb_sl, LDB

typedef short short4_ __attribute__((ext_vector_type(4)));
typedef short short8_ __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) short4_ lds_short4;
typedef _Float16 half4_ __attribute__((ext_vector_type(4)));
typedef _Float16 half8_ __attribute__((ext_vector_type(8)));

#define LDS2 144                           // staging rows: 72 dwords -> the 4x16 transposing reads are conflict-free
#define SD_C 2.8853900817779268f           // 2 log2(e): tanh(x) = 1 - 2 / (exp2(C x) + 1)
#define SD_RC (1.0f / SD_C)
#define SD_RC2 (SD_RC * SD_RC)
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ f32x4 sd_mfma16(const bf16x4& a, const bf16x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(short4_, a), __builtin_bit_cast(short4_, b), c, 0, 0, 0);
}
__device__ __forceinline__ float sd_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ float sd_log(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }
__device__ __forceinline__ float sd_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

__device__ __forceinline__ bf16x8 sd_cat(const bf16x4& a, const bf16x4& b) {
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}
// the forward's activation operand under the q-swapped image layout (pv_fb_layout.h): lanes of groups q >= 2 hold their weight
// chunk's halves in the other order (sw: per lane, loop-invariant)
__device__ __forceinline__ bf16x8 sd_catq(bf16x4 a, bf16x4 b, bool sw) {
  typedef unsigned int u32x2_ __attribute__((ext_vector_type(2)));
  const u32x2_ ua = __builtin_bit_cast(u32x2_, a), ub = __builtin_bit_cast(u32x2_, b);
  const u32x2_ lo = {sw ? ub[0] : ua[0], sw ? ub[1] : ua[1]}, hi = {sw ? ua[0] : ub[0], sw ? ua[1] : ub[1]};
  return sd_cat(__builtin_bit_cast(bf16x4, lo), __builtin_bit_cast(bf16x4, hi));
}

// a zero the compiler cannot see through: lane-address arithmetic that depends on it is redone where it is used
// instead of being hoisted out of the tile loop and held in (or spilled from) registers for the whole kernel
__device__ __forceinline__ int sd_opaque0() { int z = 0; asm volatile("" : "+v"(z)); return z; }

// transposing LDS read (ds_read_b64_tr_b16) at a pointer / at an LDS byte address
__device__ __forceinline__ bf16x4 sd_tr(const __bf16* p) {
  const short4_ v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)p);
  return __builtin_bit_cast(bf16x4, v);
}
__device__ __forceinline__ bf16x4 sd_tr_at(unsigned lds_byte_addr) {
  const short4_ v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)(size_t)lds_byte_addr);
  return __builtin_bit_cast(bf16x4, v);
}
__device__ __forceinline__ bf16x4 sd_zero4() { const short4_ z = {0, 0, 0, 0}; return __builtin_bit_cast(bf16x4, z); }

// ---- LDS-DMA: 16 B per lane from global straight into LDS at (wave-uniform byte address) + 16 * lane.  hipcc
// does not count these in its s_waitcnt bookkeeping: sd_wait_vm0() before the landed data is read, and no
// compiler-visible global load may be pending when one is issued (the callers drain first).
__device__ __forceinline__ void sd_glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void sd_glds4(const void* gsrc, unsigned lds_dst) {     // 4 B per lane, 256 B per wave
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void sd_wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void sd_wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xc07f); }
// BYTES of weight images from their global copy, by the NW waves of the workgroup: BYTES / (NW KB) one-KB pieces per wave
template <int BYTES, int NW>
__device__ __forceinline__ void sd_reload(const char* __restrict__ gimg, unsigned lds_dst, int wave, int lane) {
  constexpr int PIECES = BYTES / (NW * 1024);
#pragma unroll
  for (int c = 0; c < PIECES; ++c) {
    const int off = (wave * PIECES + c) * 1024;
    sd_glds16(gimg + off + lane * 16, lds_dst + off);
  }
}

// lane offsets (elements) of the weight reads (pv_fb_layout.h):
//   forward: row 16*ob + r, logical chunk 4m + q -> physical chunk 4*(m ^ (r&3)) + (q ^ SL[r>>2])
//   dgrad  : lane i of 16-lane group q points at W[32m + 4q (+16) + r/4][...], swizzle 4*(r>>2) + SL[q]
struct SdAddr { int fb, fx[4], db, dx[4]; };
__device__ __forceinline__ SdAddr sd_addr(int r, int q) {
  SdAddr a;
  a.fb = r * LDB + 8 * (q ^ fb_sl(r >> 2));
  a.db = (4 * q + (r >> 2)) * LDB + 8 * ((r & 3) ^ fb_sl(q));
#pragma unroll
  for (int m = 0; m < 4; ++m) { a.fx[m] = 32 * (m ^ (r & 3)); a.dx[m] = 32 * (m ^ (r >> 2)); }
  return a;
}

// Elementwise phases are written as STAGES over all 32 values of a lane with scheduling fences in between: left alone,
// the compiler walks the values two at a time through the whole dependent chain (exp -> add -> rcp -> fma), and an in-order
// wave then pays every instruction's latency (~10 cycles each).
// tanh of x given C*x, in place: 1 - 2 rcp(exp2(.) + 1).  FENCE_MASK: the caller's stage-fence mask (0 = nothing crosses)
template <int FENCE_MASK = 0>
__device__ __forceinline__ void sd_tanh8(f32x4 (&v)[8]) {
#pragma unroll
  for (int jb = 0; jb < 8; ++jb)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[jb][i] = __builtin_amdgcn_exp2f(v[jb][i]);
  __builtin_amdgcn_sched_barrier(FENCE_MASK);
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) v[jb] = v[jb] + 1.0f;
  __builtin_amdgcn_sched_barrier(FENCE_MASK);
#pragma unroll
  for (int jb = 0; jb < 8; ++jb)
#pragma unroll
    for (int i = 0; i < 4; ++i) v[jb][i] = __builtin_amdgcn_rcpf(v[jb][i]);
  __builtin_amdgcn_sched_barrier(FENCE_MASK);
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) v[jb] = 1.0f - 2.0f * v[jb];
  __builtin_amdgcn_sched_barrier(FENCE_MASK);
}
// the four bf16 of a C/D block as fp32 (a shift / a mask each)
__device__ __forceinline__ f32x4 sd_f32_of(const bf16x4& h) {
  typedef unsigned uint2_ __attribute__((ext_vector_type(2)));
  const uint2_ u = __builtin_bit_cast(uint2_, h);
  f32x4 f;
  f[0] = __builtin_bit_cast(float, u[0] << 16);
  f[1] = __builtin_bit_cast(float, u[0] & 0xffff0000u);
  f[2] = __builtin_bit_cast(float, u[1] << 16);
  f[3] = __builtin_bit_cast(float, u[1] & 0xffff0000u);
  return f;
}

// 16 rows (lane (r, q): row `row`) of a staged tensor, row-major [rows][LDS2].  Inside every 16-column block the four 8-byte
// pieces are XOR-swizzled by (row>>2)&3: ds_write_b64 is banked mod 32 and serviced 16 lanes (16 rows, one q) at a time, and
// 72-dword rows alone would put rows r and r+4 on the same banks (4-way); the transposing reads (sd_stage_toff) undo the
// swizzle and stay conflict-free.
__device__ __forceinline__ void sd_stage_store(__bf16* __restrict__ sh, const bf16x4 (&h)[8], int row, int q) {
  row |= sd_opaque0();
  const int e = row * LDS2 + 4 * (q ^ ((row >> 2) & 3));
#pragma unroll
  for (int jb = 0; jb < 8; ++jb) *reinterpret_cast<bf16x4*>(sh + e + 16 * jb) = h[jb];
}
// lane offset of the transposing read of staged rows R0 + 4q .. 4q+3 (R0 a multiple of 16), columns 16*blk ..
__device__ __forceinline__ int sd_stage_toff(int r, int q) { return (4 * q + (r >> 2)) * LDS2 + 4 * ((r & 3) ^ q); }

// One pixel's log-likelihood ll, dL/dlogit dlda (before the row's weight) and mean locv, from the logit a and the datum xv.
// Bernoulli: -BCEWithLogits(lg, x) with lg = logit(pc) (torch: probs_to_logits, then binary_cross_entropy_with_logits), written with
// the identities 1 + exp(-|lg|) = 1 / max(pc, 1 - pc) and sigmoid(lg) = pc: the two logarithms lg is made of serve the
// softplus term too, and the row's dependent chain is exp -> rcp -> 2 log instead of seven transcendentals.
template <int LIK>
__device__ __forceinline__ void sd_pixel_lik(float a, float xv, float sig, int sigmoid_out, float& ll, float& dlda, float& locv) {
  if (LIK == PV_LIK_BERNOULLI) {
    const float pr = sd_rcp(1.0f + sd_exp(-a));
    const float pc = fminf(fmaxf(pr, BERN_EPS), 1.0f - BERN_EPS);
    const float lpc = sd_log(pc), l1pc = sd_log(1.0f - pc);
    const float lg = lpc - l1pc;
    ll = -(fmaxf(lg, 0.0f) - lg * xv - fmaxf(lpc, l1pc));
    const float mask = (pr >= BERN_EPS && pr <= 1.0f - BERN_EPS) ? 1.0f : 0.0f;
    dlda = (pc - xv) * mask;
    locv = pr;
  } else if (LIK == PV_LIK_CBERNOULLI) {
    pv_cbern(a, xv, ll, dlda, locv);
  } else if (LIK == PV_LIK_POISSON_LOG) {
    // Poisson with a log link, a = the log-rate clamped at 30: one transcendental.  The data-only term lgamma(x + 1) is not
    // computed here (pv_poisson_lognorm adds its sum to the step's scalars)
    const float ac = fminf(a, 30.0f);
    const float rate = sd_exp(ac);
    ll = xv * ac - rate;
    dlda = a <= 30.0f ? rate - xv : 0.0f;
    locv = rate;
  } else {
    const float pr = sigmoid_out ? sd_rcp(1.0f + sd_exp(-a)) : a;
    const float d = xv - pr;
    ll = -(d * d) / (2.0f * sig * sig) - sd_log(sig) - LOG_SQRT_2PI;
    dlda = -d / (sig * sig) * (sigmoid_out ? pr * (1.0f - pr) : 1.0f);
    locv = pr;
  }
}
