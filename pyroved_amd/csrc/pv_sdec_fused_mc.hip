// pv_sdec_fused_mc.hip — the fused persistent forward+backward kernel of the spatial decoder (pv_sdec_fused.hip) for a decoder
// with C = 2 .. 8 output channels per grid position (iVAE(..., channels=C); decoder.out = Linear(128, C)): a sibling of
// pv_sdec_fused_kernel on the same f32 matrix instructions.  The plan asks for it with PV_PLAN_FUSED_CHANNELS and fused == 1.
// Its WEIGHTED instances (C = 1 .. 8, PvFused::pw: per-observation weights of the likelihood) run the steps of pv_ivae_weighted_*:
// WEIGHTED == 1 with weights shared by all images, WEIGHTED == 2 with one weight per observation of every image (pv_ivae_weighted_images_*).
//
// Unchanged from the one-channel kernel (pv_sdec_fused_f32.h holds the shared streams): the tile loop, the transposed layers, the
// three register tiles, the two weight-gradient exchanges, the coordinate layer's backward and flush_hz.  A ROW is still one grid
// position of one sample; it now carries C observations x[row*C + c] and C outputs.  What differs sits between "layer 2 finished"
// and "tC = dL/dpre2", and in the epilogue:
//   forward     a[c] = h2 . Wo[c] + bo[c]: C partial dot products over the lane's 32 elements, each closed by fd_sum_q;
//   likelihood  per value, the one-channel kernel's four branches term for term; llrow[row] = sum_c ll, c ascending;
//   backward    dL/dh2[j] = sum_c dL/da_c Wo[c][j], c ascending, times 1 - h2^2;
//   d(wo)       a FOURTH staged exchange per tile, formed like the coordinate layer's dWc: the owning wave stages h2 through stA
//               and its unit's 16 x C values of dL/da through a side area; wave w then accumulates columns 16w .. 16w+15 of every
//               channel in C registers per lane (a lane covers four staged rows; fd_sum_q once in the epilogue).  Fixed summation
//               order, no LDS read-modify-write, no atomics: C VGPRs, one stage write and two barriers per unit;
//   d(bo)       from the same staged values: lane r < C of wave 0 adds its channel's four staged rows (one register).
// LDS: the one-channel layout with two regions re-used, so the total stays 157.5 KiB: Wo[C][128] (<= 4 KiB) takes the region of the
// eight per-wave d(wo) slots (OFF_DWO, 4 KiB: this kernel has no such slots), and the one-channel Wo row (OFF_WO, 128 floats) is the
// side area of the staged dL/da (16 x C <= 128 floats); bo[C] sits in the unused tail of OFF_INFO.
// Record (PV_REC_ROWMAJOR, FD_REC unchanged): channel 0 where the one-channel kernel writes (d(wo) slot 4, d(bo) slot 5 [0]), so the
// shared reductions finish W1, W2, b1, b2, Wc, Wo[0], bo[0] untouched; channel c >= 1: d(wo)[c] in spare slot 5 + c, d(bo)[c] at
// slot 5 [c], summed by pv_sdec_fused_mc_reduce_out.
// PvFused::ablate (profiling switches of the one-channel kernel) is ignored here.
#include "pv_sdec_fused_f32.h"

#define OFF_WOC OFF_DWO            // Wo[C][FD_H]
#define OFF_DA OFF_WO              // staged dL/da of one unit: [16 rows][C]
#define OFF_BO (OFF_INFO + 40)     // bo[C]  (OFF_INFO: [0,16) x0, [16,32) x1, [32] sample index)

// the likelihood of one value with pre-activation a and observation xv: pv_sdec_fused_kernel's four branches, term for term
__device__ __forceinline__ void fdm_pixel_lik(const PvFused& f, float a, float xv, float& ll, float& dlda, float& locv) {
  if (f.lik == PV_LIK_BERNOULLI) {
    // torch Bernoulli(probs=sigmoid(a)).log_prob(x): clamp_probs -> logits -> -BCEWithLogits
    const float pr = sd_rcp(1.0f + sd_exp(-a));
    const float pc = fminf(fmaxf(pr, BERN_EPS), 1.0f - BERN_EPS);
    const float lg = sd_log(pc) - sd_log(1.0f - pc);
    ll = -(fmaxf(lg, 0.0f) - lg * xv + sd_log(1.0f + sd_exp(-fabsf(lg))));
    const float mask = (pr >= BERN_EPS && pr <= 1.0f - BERN_EPS) ? 1.0f : 0.0f;
    dlda = (sd_rcp(1.0f + sd_exp(-lg)) - xv) * mask;
    locv = pr;
  } else if (f.lik == PV_LIK_CBERNOULLI) {
    pv_cbern(a, xv, ll, dlda, locv);
  } else if (f.lik == PV_LIK_POISSON_LOG) {
    const float ac = fminf(a, 30.0f);
    const float rate = sd_exp(ac);
    ll = xv * ac - rate;
    dlda = a <= 30.0f ? rate - xv : 0.0f;
    locv = rate;
  } else {
    const float pr = f.sigmoid_out ? sd_rcp(1.0f + sd_exp(-a)) : a;
    const float d = xv - pr;
    ll = -(d * d) / (2.0f * f.sig * f.sig) - sd_log(f.sig) - LOG_SQRT_2PI;
    dlda = -d / (f.sig * f.sig) * (f.sigmoid_out ? pr * (1.0f - pr) : 1.0f);
    locv = pr;
  }
}

// WEIGHTED (pv_ivae_weighted_*): observation (n, c) of every sample carries the weight f.pw[n * C + c] — ll and dL/da are multiplied
// by it where they are formed, loc is not; everything downstream is the same code.  C = 1 exists in this form only (the unweighted
// one-channel kernel is pv_sdec_fused_kernel): channel 0's d(wo) / d(bo) sit where the shared reduction expects them.
// WEIGHTED: 0 none, 1 (PV_FDM_W_SHARED) shared by all samples, 2 (PV_FDM_W_IMAGES, pv_ivae_weighted_images_*) f.pw is (M * C), one
// weight per observation of every sample, read at the index x is read at: f.pw[row * C + c]
template <bool GRADS, int C, int WEIGHTED>
__global__ __launch_bounds__(FD_THREADS, 2) void pv_sdec_fused_mc_kernel(PvFused f) {
  static_assert(WEIGHTED >= 0 && WEIGHTED <= 2 && C >= (WEIGHTED ? 1 : 2) && C <= 8 && C * FD_H <= FD_WAVES * FD_H && FD_UNIT * C <= FD_H && 40 + C <= 64, "LDS regions");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform: unit, sample and every 16 * wave offset stay scalar
  const int g = blockIdx.x, G = gridDim.x;

  // ---- stage the weights in LDS (once per kernel) ----
  for (int idx = tid; idx < FD_H * (FD_H / 4); idx += FD_THREADS) {
    const int row = idx >> 5, c4 = idx & 31;
    *reinterpret_cast<f32x4*>(sm + OFF_W1 + row * LDW + 4 * c4) = reinterpret_cast<const f32x4*>(f.W1)[idx];
    *reinterpret_cast<f32x4*>(sm + OFF_W2 + row * LDW + 4 * c4) = reinterpret_cast<const f32x4*>(f.W2)[idx];
  }
  for (int j = tid; j < FD_H; j += FD_THREADS) {
    sm[OFF_WC0 + j] = f.Wc[j * f.cd];
    sm[OFF_WC1 + j] = f.cd == 2 ? f.Wc[j * 2 + 1] : 0.0f;
    sm[OFF_BC + j] = f.bc[j];
    sm[OFF_B1 + j] = f.b1[j];
    sm[OFF_B2 + j] = f.b2[j];
  }
  for (int j = tid; j < C * FD_H; j += FD_THREADS) sm[OFF_WOC + j] = f.wo[j];
  if (tid < C) sm[OFF_BO + tid] = f.bo[tid];
  __syncthreads();

  const float* W1s = sm + OFF_W1;
  const float* W2s = sm + OFF_W2;
  float* stA = sm + OFF_STA;
  float* stB = sm + OFF_STB;

  // persistent accumulators: this wave's 16x128 slices of dW1 / dW2, bias / coordinate-layer sums, its 16 columns of every d(wo)[c]
  f32x4 accW1[8], accW2[8];
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) { accW1[kb] = f32x4{0, 0, 0, 0}; accW2[kb] = f32x4{0, 0, 0, 0}; }
  float db1 = 0.0f, db2 = 0.0f, aWc0 = 0.0f, aWc1 = 0.0f, ahz = 0.0f, abo = 0.0f;
  float adwo[C];
#pragma unroll
  for (int c = 0; c < C; ++c) adwo[c] = 0.0f;
  int cur_b = -1;
  const int upb = f.N / FD_UNIT;                       // units per sample (N = positions, N % 16 == 0)

  auto flush_hz = [&](int b) {
    // sample b's rows end (or the workgroup's do): publish this workgroup's partial dL/d(hz[b])
    const float t = fd_sum_q(ahz);
    const int64_t ub = (int64_t)b * upb;
    const int gfirst = (int)(((ub + 1) * G + f.units - 1) / f.units) - 1;   // first workgroup touching sample b
    if (q == 0) f.part_hz[((int64_t)b * f.kmax + (g - gfirst)) * FD_H + 16 * wave + r] = t;
  };

  const int64_t u_lo = (int64_t)g * f.units / G, u_hi = (int64_t)(g + 1) * f.units / G;
  for (int64_t u0 = u_lo; u0 < u_hi; u0 += FD_WAVES) {
    const int nact = (int)((u_hi - u0) < FD_WAVES ? (u_hi - u0) : FD_WAVES);
    const bool active = wave < nact;
    // The lane's row / quarter as values the compiler cannot trace to the lane index: every LDS address of the tile is then
    // formed inside the tile.  Left loop-invariant, some sixty of them — the small vectors sit above the 64 KiB a ds instruction's
    // immediate reaches, so every 16-column block is an address of its own — are computed once and kept in VGPRs for the whole
    // kernel, on top of the one-channel kernel's 256 + 26 spilled
    int r = lane & 15, q = lane >> 4;
    asm volatile("" : "+v"(r), "+v"(q));
    const int unit = (int)u0 + (active ? wave : 0);          // 32-bit index math: units < 2^31 / 16
    const int b = unit / upb, n = (unit - b * upb) * FD_UNIT + r;
    const int64_t row = (int64_t)unit * FD_UNIT + r;
    // three register tiles (16 rows x 128 cols each, 32 VGPRs) are rotated through the roles
    // h0 -> h1 -> h2/dpre2 -> dpre1 -> h0 (recomputed) -> dpre0 so that at most three are live
    f32x4 tA[8], tB[8], tC[8];
    float x0 = 0.0f, x1 = 0.0f;
    float dlda[C];                                            // dL/da_c of this lane's row (the same in its four q lanes)
#pragma unroll
    for (int c = 0; c < C; ++c) dlda[c] = 0.0f;
    const float* hzb = f.hz + (int64_t)b * FD_H;

    // coordinate layer, one 16-column block: h0[jb] = tanh(Wc x' + bc + hz[b])   (fc.py:226-237)
    auto coord_block = [&](f32x4 (&h0)[8], int jb) {
      const int j = 16 * jb + 4 * q;
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(sm + OFF_WC0 + j);
      const f32x4 w1 = *reinterpret_cast<const f32x4*>(sm + OFF_WC1 + j);
      const f32x4 bc = *reinterpret_cast<const f32x4*>(sm + OFF_BC + j);
      const f32x4 hz = *reinterpret_cast<const f32x4*>(hzb + j);
#pragma unroll
      for (int i = 0; i < 4; ++i) h0[jb][i] = fd_tanh(w0[i] * x0 + w1[i] * x1 + bc[i] + hz[i]);
    };

    if (active) {
      // ---- x' = rotate/scale/translate(grid[n])   (coord.py:47-88) ----
      const float* t = f.tp + (int64_t)b * 8;
      if (f.cd == 2) {
        const float gx = f.grid[2 * n], gy = f.grid[2 * n + 1];
        const float u0c = gx * t[0] - gy * t[1];
        const float u1c = gx * t[1] + gy * t[0];
        const float sc = t[2];
        x0 = u0c * sc + t[3];
        x1 = u1c * sc + t[4];
      } else {
        x0 = f.grid[n] + t[3];
      }
      // layer 1: its input h0 (tA) is produced block by block inside the MFMA stream; tB = pre-activation 1
      fd_layer_fwd<false>(W1s, sm + OFF_B1, tA, tB, r, q, [&](int jb) { coord_block(tA, jb); });
      // layer 2: activates its own input in place (tB -> h1) one block ahead; tC[0..3] = h2, tC[4..7] raw
      fd_layer_fwd<true>(W2s, sm + OFF_B2, tB, tC, r, q, [&](int jb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) tB[jb][i] = fd_tanh(tB[jb][i]);
      });
#pragma unroll
      for (int ob = 4; ob < 8; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) tC[ob][i] = fd_tanh(tC[ob][i]);
      // ---- output layer + likelihood, channel by channel ----
      float llsum = 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float part = 0.0f;
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(sm + OFF_WOC + c * FD_H + 16 * jb + 4 * q);
#pragma unroll
          for (int i = 0; i < 4; ++i) part += tC[jb][i] * wv[i];
        }
        const float a = fd_sum_q(part) + sm[OFF_BO + c];
        const float xv = f.x ? f.x[row * C + c] : 0.0f;
        const float pwv = WEIGHTED == 2 ? f.pw[row * C + c] : WEIGHTED == 1 ? f.pw[n * C + c] : 1.0f;
        float ll, locv;
        fdm_pixel_lik(f, a, xv, ll, dlda[c], locv);
        if (WEIGHTED) { ll *= pwv; dlda[c] *= pwv; }
        llsum += ll;
        if (q == 0 && f.loc) f.loc[row * C + c] = locv;
        FD_SCHED_FENCE();        // one channel at a time: hoisted, the C channels' Wo reads alone would take 32 C VGPRs
      }
      if (q == 0 && f.llrow) f.llrow[row] = llsum;
    }
    if (!GRADS) continue;

    // ---- d(wo), d(bo): exchange (dL/da = dlda, h2 = tC) one unit at a time, before tC is overwritten ----
    for (int c = 0; c < nact; ++c) {
      if (wave == c) {
        fd_stage_write(stA, tC, r, q);
        if (q == 0) {
#pragma unroll
          for (int ch = 0; ch < C; ++ch) sm[OFF_DA + r * C + ch] = dlda[ch];
        }
      }
      __syncthreads();
      const int rb = r < C ? r : C - 1;                      // (lanes r >= C read a valid value and drop it)
      const bool bo_lane = wave == 0 && r < C;
      constexpr int kRowsAhead = C <= 5 ? 2 : 1;
      // (two staged rows in flight up to five channels, one from six: with more, the 4 C + 4 values read ahead spill)
#pragma unroll kRowsAhead
      for (int s = 0; s < 4; ++s) {
        const float hv = stA[(4 * s + q) * LDST + 16 * wave + r];
        const float* da = sm + OFF_DA + (4 * s + q) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) adwo[ch] += da[ch] * hv;
        abo += bo_lane ? da[rb] : 0.0f;
      }
      __syncthreads();
    }
    if (active) {
      // tC = dL/d(pre-activation of layer 2) = (sum_c dL/da_c Wo[c]) * (1 - h2^2), one 16-column block at a time: the quarter
      // offset passes through an empty asm that also takes the previous block's result, so the C Wo reads of a block cannot
      // issue before that block is finished (left free, all 8 C reads are issued up front: 32 C VGPRs, every one of them spilled;
      // the scheduling fence alone does not hold them)
      int wq = q;
#pragma unroll
      for (int jb = 0; jb < 8; ++jb) {
        if (jb == 0) asm volatile("" : "+v"(wq));
        else asm volatile("" : "+v"(wq) : "v"(tC[jb - 1]));
        f32x4 gsum = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(sm + OFF_WOC + c * FD_H + 16 * jb + 4 * wq);
#pragma unroll
          for (int i = 0; i < 4; ++i) gsum[i] += dlda[c] * wv[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) tC[jb][i] = gsum[i] * (1.0f - tC[jb][i] * tC[jb][i]);
      }
    }

    // ---- wgrad of layer 2: exchange (dpre2 = tC, h1 = tB) one unit at a time ----
    for (int c = 0; c < nact; ++c) {
      if (wave == c) { fd_stage_write(stA, tC, r, q); fd_stage_write(stB, tB, r, q); }
      __syncthreads();
      fd_wgrad_consume(stA, stB, accW2, db2, wave, r, q);
      __syncthreads();
    }
    if (active) {
      fd_layer_dgrad(W2s, tC, tA, r, q, [](int) {});
      fd_mul_dtanh(tA, tB);                              // tA = dpre1 = (dpre2 W2) * (1 - h1^2)
      // tB = h0, recomputed (cheaper than keeping it live) in the shadow of the next dgrad's MFMAs
      fd_layer_dgrad(W1s, tA, tC, r, q, [&](int g) { if ((g & 3) == 0) coord_block(tB, g >> 2); });
      fd_mul_dtanh(tC, tB);                              // tC = dpre0 = (dpre1 W1) * (1 - h0^2)
    }
    // ---- wgrad of layer 1: exchange (dpre1 = tA, h0 = tB) ----
    for (int c = 0; c < nact; ++c) {
      if (wave == c) { fd_stage_write(stA, tA, r, q); fd_stage_write(stB, tB, r, q); }
      __syncthreads();
      fd_wgrad_consume(stA, stB, accW1, db1, wave, r, q);
      __syncthreads();
    }
    // ---- coordinate layer backward, row-local part: d(x') -> d(phi, scale, shift) per row ----
    if (active) {
      float d0 = 0.0f, d1 = 0.0f;
#pragma unroll
      for (int jb = 0; jb < 8; ++jb) {
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(sm + OFF_WC0 + 16 * jb + 4 * q);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(sm + OFF_WC1 + 16 * jb + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) { d0 += tC[jb][i] * w0[i]; d1 += tC[jb][i] * w1[i]; }
      }
      d0 = fd_sum_q(d0);
      d1 = fd_sum_q(d1);
      if (q == 0) {
        // (u0c, u1c, sc: read and formed again as at the top of the tile — the same bits — so that they are not carried
        //  through the tile's dgrad streams, where the registers run out)
        float u0c, u1c = 0.0f, sc = 1.0f;
        const float* t = f.tp + (int64_t)b * 8;
        if (f.cd == 2) {
          const float gx = f.grid[2 * n], gy = f.grid[2 * n + 1];
          u0c = gx * t[0] - gy * t[1];
          u1c = gx * t[1] + gy * t[0];
          sc = t[2];
        } else {
          u0c = f.grid[n];
        }
        f.rowtp[row] = sc * (d1 * u0c - d0 * u1c);
        f.rowtp[f.M + row] = d0 * u0c + d1 * u1c;
        f.rowtp[2 * f.M + row] = d0;
        f.rowtp[3 * f.M + row] = d1;
      }
    }
    // ---- coordinate layer backward, cross-row part: dWc, dbc/dhz via staged dpre0 ----
    for (int c = 0; c < nact; ++c) {
      if (wave == c) {
        fd_stage_write(stA, tC, r, q);
        if (q == 0) { sm[OFF_INFO + r] = x0; sm[OFF_INFO + 16 + r] = x1; }
        if (lane == 0) reinterpret_cast<int*>(sm + OFF_INFO)[32] = b;
      }
      __syncthreads();
      const int bc = reinterpret_cast<const int*>(sm + OFF_INFO)[32];     // workgroup-uniform
      if (bc != cur_b) {
        if (cur_b >= 0) flush_hz(cur_b);
        cur_b = bc;
        ahz = 0.0f;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float v = stA[(4 * s + q) * LDST + 16 * wave + r];
        ahz += v;
        aWc0 += v * sm[OFF_INFO + 4 * s + q];
        aWc1 += v * sm[OFF_INFO + 16 + 4 * s + q];
      }
      __syncthreads();
    }
  }
  if (!GRADS) return;

  // ---- publish this workgroup's partial gradients ----
  if (cur_b >= 0) flush_hz(cur_b);
  float* rec = f.part + (int64_t)g * FD_REC;
#pragma unroll
  for (int kb = 0; kb < 8; ++kb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // C/D layout: lane (col k' = r, q), reg i -> dW[16*wave + 4*q + i][16*kb + r]
      rec[(16 * wave + 4 * q + i) * FD_H + 16 * kb + r] = accW1[kb][i];
      rec[FD_H * FD_H + (16 * wave + 4 * q + i) * FD_H + 16 * kb + r] = accW2[kb][i];
    }
  const float t1 = fd_sum_q(db1), t2 = fd_sum_q(db2), tc0 = fd_sum_q(aWc0), tc1 = fd_sum_q(aWc1), tbo = fd_sum_q(abo);
  float* vec = rec + 2 * FD_H * FD_H;
  if (q == 0) {
    vec[16 * wave + r] = t1;
    vec[FD_H + 16 * wave + r] = t2;
    vec[2 * FD_H + 16 * wave + r] = tc0;
    vec[3 * FD_H + 16 * wave + r] = tc1;
    if (wave == 0 && r < C) vec[5 * FD_H + r] = tbo;              // d(bo)[r]
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float t = fd_sum_q(adwo[c]);
    if (q == 0) vec[(c == 0 ? 4 : 5 + c) * FD_H + 16 * wave + r] = t;   // d(wo)[c], columns 16 wave .. 16 wave + 15
  }
}

// ---- channels 1 .. C-1 of d(wo), d(bo): per-workgroup records -> flat gradient buffer -----------------------
// 64 outputs x 4 slices of the workgroup range per 256-thread block, slices combined in fixed order: the shared reduction's order
// (pv_sdec_fused_reduce_block), which sums channel 0
__global__ __launch_bounds__(256) void pv_sdec_fused_mc_reduce_out_kernel(const float* __restrict__ part, int G_, float* __restrict__ Gr,
                                                                          int64_t wo_off, int64_t bo_off, int C) {
  __shared__ float sm[4][64];
  const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int o = blockIdx.x * 64 + c, nw = (C - 1) * FD_H, total = nw + (C - 1);
  const int per = (G_ + 3) / 4;
  const int w0 = sl * per, w1 = min(G_, w0 + per);
  int src = 0;
  int64_t dst = 0;
  if (o < nw) {
    const int ch = 1 + o / FD_H, j = o % FD_H;
    src = 2 * FD_H * FD_H + (5 + ch) * FD_H + j;
    dst = wo_off + (int64_t)ch * FD_H + j;
  } else if (o < total) {
    const int ch = 1 + (o - nw);
    src = 2 * FD_H * FD_H + 5 * FD_H + ch;
    dst = bo_off + ch;
  }
  float v = 0.0f;
  if (o < total) {
#pragma unroll 8
    for (int w = w0; w < w1; ++w) v += part[(int64_t)w * FD_REC + src];
  }
  sm[sl][c] = v;
  __syncthreads();
  if (sl != 0 || o >= total) return;
  Gr[dst] = (sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c]);
}

int pv_sdec_fused_mc_reduce_out(const float* part, int grid, float* G, int64_t wo_off, int64_t bo_off, int C, hipStream_t s) {
  if (!part || !G || grid < 1 || C < 2 || C > PV_MAX_CHANNELS) return PV_EINVAL;
  const int total = (C - 1) * (FD_H + 1);
  hipLaunchKernelGGL(pv_sdec_fused_mc_reduce_out_kernel, dim3((total + 63) / 64), dim3(256), 0, s, part, grid, G, wo_off, bo_off, C);
  PV_LAUNCH_CHECK();
  return 0;
}

// ---- host side -----------------------------------------------------------------------------------------
// every C of 2 .. PV_MAX_CHANNELS has an instance (no spills under __launch_bounds__(512, 2): profiles/multichannel_fused_resource_usage.txt)
// weighted: C = 1 .. PV_MAX_CHANNELS (profiles/pixel_weights_resource_usage.txt: none of them spills, so none is refused here —
// a C whose weighted instance spilled would be taken out of this list and run the layered kernels); per image (weighted == 2,
// PV_FDM_W_IMAGES): the same list, profiles/image_weights_resource_usage.txt
static bool fdm_has_instance(int C, int weighted = 0) { return weighted >= 0 && weighted <= 2 && C >= (weighted ? 1 : 2) && C <= 8; }

bool pv_sdec_fused_mc_supported(const pv_ivae_plan* p) {
  if (!p || !(p->flags & PV_PLAN_FUSED_CHANNELS) || p->fused != 1) return false;
  if (!pv_sdec_fused_trunk_supported(p)) return false;
  const int C = p->out.out_dim;
  if (C < 2 || C > PV_MAX_CHANNELS || !fdm_has_instance(C) || p->n_pix % C != 0) return false;
  return (p->n_pix / C) % FD_UNIT == 0;
}

bool pv_sdec_fused_mc_weighted_supported(const pv_ivae_plan* p, bool per_image) {
  if (!p || p->fused != 1 || !pv_sdec_fused_trunk_supported(p)) return false;
  const int C = p->out.out_dim;
  if (C < 1 || C > PV_MAX_CHANNELS || !fdm_has_instance(C, per_image ? PV_FDM_W_IMAGES : PV_FDM_W_SHARED) || p->n_pix % C != 0) return false;
  if (C > 1 && !(p->flags & PV_PLAN_FUSED_CHANNELS)) return false;
  return (p->n_pix / C) % FD_UNIT == 0;
}

template <int C, int W>
static int fdm_launch(const PvFused& f, int grid, bool grads, hipStream_t s) {
  const size_t lds = FD_LDS_FLOATS * sizeof(float);
  if (grads) {
    PV_TRY(pv_set_dynamic_lds(reinterpret_cast<const void*>(&pv_sdec_fused_mc_kernel<true, C, W>), (int)lds));
    hipLaunchKernelGGL((pv_sdec_fused_mc_kernel<true, C, W>), dim3(grid), dim3(FD_THREADS), lds, s, f);
  } else {
    PV_TRY(pv_set_dynamic_lds(reinterpret_cast<const void*>(&pv_sdec_fused_mc_kernel<false, C, W>), (int)lds));
    hipLaunchKernelGGL((pv_sdec_fused_mc_kernel<false, C, W>), dim3(grid), dim3(FD_THREADS), lds, s, f);
  }
  PV_LAUNCH_CHECK();
  return 0;
}

template <int W>
static int fdm_launch_weighted(const PvFused& f, int C, int grid, bool grads, hipStream_t s) {
  switch (C) {
    case 1: return fdm_launch<1, W>(f, grid, grads, s);
    case 2: return fdm_launch<2, W>(f, grid, grads, s);
    case 3: return fdm_launch<3, W>(f, grid, grads, s);
    case 4: return fdm_launch<4, W>(f, grid, grads, s);
    case 5: return fdm_launch<5, W>(f, grid, grads, s);
    case 6: return fdm_launch<6, W>(f, grid, grads, s);
    case 7: return fdm_launch<7, W>(f, grid, grads, s);
    case 8: return fdm_launch<8, W>(f, grid, grads, s);
  }
  return PV_EINVAL;
}

int pv_sdec_fused_mc_launch(const PvFused& f_in, int C, int grid, bool grads, hipStream_t s, int w) {
  if (f_in.sw || f_in.x_units != 0 || f_in.part_rs || f_in.dhz_out || f_in.dzc_out) return PV_EINVAL;
  if (w ? !f_in.pw : f_in.wimg != nullptr) return PV_EINVAL;         // (one slot: the weights of a weighted launch, else nothing)
  if (!fdm_has_instance(C, w) || grid < 1 || f_in.N % FD_UNIT != 0 || f_in.units * FD_UNIT != f_in.M) return PV_EINVAL;
  PvFused f = f_in;
  f.ablate = 0;
  if (w == PV_FDM_W_IMAGES) return fdm_launch_weighted<PV_FDM_W_IMAGES>(f, C, grid, grads, s);
  if (w == PV_FDM_W_SHARED) return fdm_launch_weighted<PV_FDM_W_SHARED>(f, C, grid, grads, s);
  switch (C) {
    case 2: return fdm_launch<2, 0>(f, grid, grads, s);
    case 3: return fdm_launch<3, 0>(f, grid, grads, s);
    case 4: return fdm_launch<4, 0>(f, grid, grads, s);
    case 5: return fdm_launch<5, 0>(f, grid, grads, s);
    case 6: return fdm_launch<6, 0>(f, grid, grads, s);
    case 7: return fdm_launch<7, 0>(f, grid, grads, s);
    case 8: return fdm_launch<8, 0>(f, grid, grads, s);
  }
  return PV_EINVAL;
}
