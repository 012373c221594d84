// pv_sdec_fused.hip — fused persistent forward+backward kernel of the spatial decoder
// (pyroved/nets/fc.py:155-237 sDecoderNet + coord_latent, with utils/coord.py:47-88's transform and
// utils/prob.py:25-29's likelihood fused in) for the default architecture hidden_dim_d = [128, 128], tanh.
//
// Why one kernel: the loss is a plain sum over pixels, so dL/d(logit) of a pixel is known as soon as its
// forward finishes; forward, loss, dgrad and wgrad of a row tile can run back to back with every
// activation resident on chip.  HBM traffic per step drops from ~1.2 GB (layer-by-layer) to the
// observations (4 B/pixel) + 20 B/pixel of per-row outputs; the kernel is bound by the fp32 matrix
// pipe (v_mfma_f32_16x16x4_f32, 157 TF peak), not by HBM.
//
// Mapping (one persistent 512-thread workgroup per CU, 8 waves = 2 per SIMD so one wave's tanh / loss
// VALU work overlaps its partner's MFMAs):
//   * rows (b, n) are flattened; a wave owns 16 consecutive rows ("unit") at a time, a workgroup 8 units.
//   * Every layer is computed TRANSPOSED, D[j][r] = sum_k W[j][k] h[r][k]: the weight is the MFMA A
//     operand (read from LDS: row-major, stride 132 floats, one ds_read_b128 feeds 4 MFMAs) and the
//     activation is the B operand.  The 16x16x4 C/D layout (lane = column r, 4 regs = rows 4q..4q+3)
//     is then exactly the B-operand layout of the next layer with k = 16*jb + 4*q + i, so activations
//     stay in registers from the coordinate layer to the logit and back down the dgrad chain —
//     no transposes, no LDS round trips, no workgroup barriers in forward/dgrad.
//   * wgrad contracts over rows, which live on different waves: each wave owns a 16x128 slice of dW1
//     and dW2 in accumulator registers for the whole kernel (64 VGPRs) and the workgroup exchanges
//     (dpre, h) through a 16-row LDS staging buffer, one unit at a time.
//   * Per-workgroup partial gradients are written once at the end and summed in a fixed order by
//     pv_sdec_fused_reduce (no float atomics: bit-reproducible).
// LDS: W1, W2 (2 x 66 KiB), staging (18 KiB), small vectors: 157.5 KiB of the CU's 160 KiB.
#include "pv_sdec_fused_f32.h"  // the LDS layout, the layer / dgrad / wgrad streams and the lane sums (shared with pv_sdec_fused_mc.hip)
#include <stdlib.h>

template <bool GRADS>
__global__ __launch_bounds__(FD_THREADS, 2) void pv_sdec_fused_kernel(PvFused f) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
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
    sm[OFF_WO + j] = f.wo[j];
    sm[OFF_B1 + j] = f.b1[j];
    sm[OFF_B2 + j] = f.b2[j];
  }
  for (int j = tid; j < FD_WAVES * FD_H; j += FD_THREADS) sm[OFF_DWO + j] = 0.0f;
  __syncthreads();

  const float* W1s = sm + OFF_W1;
  const float* W2s = sm + OFF_W2;
  float* stA = sm + OFF_STA;
  float* stB = sm + OFF_STB;
  const float bo = f.bo[0];

  // persistent accumulators: this wave's 16x128 slices of dW1 / dW2, bias / coordinate-layer sums
  f32x4 accW1[8], accW2[8];
#pragma unroll
  for (int kb = 0; kb < 8; ++kb) { accW1[kb] = f32x4{0, 0, 0, 0}; accW2[kb] = f32x4{0, 0, 0, 0}; }
  float db1 = 0.0f, db2 = 0.0f, aWc0 = 0.0f, aWc1 = 0.0f, ahz = 0.0f, dbo = 0.0f;
  int cur_b = -1;
  const int upb = sd_units_per_sample(f.N);            // (the partition, its slots: pv_sdec_partition.h)

  auto flush_hz = [&](int b) {
    // sample b's rows end (or the workgroup's do): publish this workgroup's partial dL/d(hz[b])
    const float t = fd_sum_q(ahz);
    if (q == 0) f.part_hz[sd_slot<1>(b, g, 0, f.kmax, upb, G, f.units) * FD_H + 16 * wave + r] = t;
  };

  const int64_t u_lo = sd_unit_bound(g, f.units, G), u_hi = sd_unit_bound(g + 1, f.units, G);
  for (int64_t u0 = u_lo; u0 < u_hi; u0 += FD_WAVES) {
    const int nact = (int)((u_hi - u0) < FD_WAVES ? (u_hi - u0) : FD_WAVES);
    const bool active = wave < nact;
    const int unit = (int)u0 + (active ? wave : 0);          // 32-bit index math: units < 2^31 / 16
    const int b = unit / upb, n = (unit - b * upb) * FD_UNIT + r;
    const int64_t row = (int64_t)unit * FD_UNIT + r;
    // three register tiles (16 rows x 128 cols each, 32 VGPRs) are rotated through the roles
    // h0 -> h1 -> h2/dpre2 -> dpre1 -> h0 (recomputed) -> dpre0 so that at most three are live
    f32x4 tA[8], tB[8], tC[8];
    float x0 = 0.0f, x1 = 0.0f, u0c = 0.0f, u1c = 0.0f, sc = 1.0f;
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
        u0c = gx * t[0] - gy * t[1];
        u1c = gx * t[1] + gy * t[0];
        sc = t[2];
        x0 = u0c * sc + t[3];
        x1 = u1c * sc + t[4];
      } else {
        u0c = f.grid[n];
        x0 = u0c + t[3];
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
      // ---- output layer + likelihood ----
      float part = 0.0f;
#pragma unroll
      for (int jb = 0; jb < 8; ++jb) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(sm + OFF_WO + 16 * jb + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) part += tC[jb][i] * wv[i];
      }
      const float a = fd_sum_q(part) + bo;
      const float xv = f.x[f.x_units > 0 ? row % (f.x_units * FD_UNIT) : row];
      float ll, dlda, locv;
      if (f.lik == PV_LIK_BERNOULLI) {
        // torch Bernoulli(probs=sigmoid(a)).log_prob(x): clamp_probs -> logits -> -BCEWithLogits
        // (not sd_pixel_lik: this kernel keeps the literal softplus and sigmoid(lg) — seven transcendentals — and a run-time f.lik)
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
      if (f.sw) dlda *= f.sw[row / f.N];          // (jiVAE) weight of the row's sample
      if (q == 0) {
        if (f.llrow) f.llrow[row] = ll;
        if (f.loc) f.loc[row] = locv;
      }
      if (GRADS) {
        if (q == 0) dbo += dlda;
        // d(wo) partial: sum over this unit's rows, accumulated in the wave's private LDS slot
        float* dwo = sm + OFF_DWO + wave * FD_H;
        if (!(f.ablate & 8))
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
          f32x4 tv;
#pragma unroll
          for (int i = 0; i < 4; ++i) tv[i] = fd_sum_r(dlda * tC[jb][i]);
          if (r == 0) {
            f32x4* p = reinterpret_cast<f32x4*>(dwo + 16 * jb + 4 * q);
            *p = *p + tv;
          }
        }
        // tC = dL/d(pre-activation of layer 2)
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(sm + OFF_WO + 16 * jb + 4 * q);
#pragma unroll
          for (int i = 0; i < 4; ++i) tC[jb][i] = dlda * wv[i] * (1.0f - tC[jb][i] * tC[jb][i]);
        }
      }
    }
    if (!GRADS) continue;

    // ---- wgrad of layer 2: exchange (dpre2 = tC, h1 = tB) one unit at a time ----
    const int nex = (f.ablate & 1) ? 0 : nact;
    for (int c = 0; c < nex; ++c) {
      if (wave == c) { fd_stage_write(stA, tC, r, q); fd_stage_write(stB, tB, r, q); }
      __syncthreads();
      fd_wgrad_consume(stA, stB, accW2, db2, wave, r, q);
      __syncthreads();
    }
    if (active && !(f.ablate & 4)) {
      fd_layer_dgrad(W2s, tC, tA, r, q, [](int) {});
      fd_mul_dtanh(tA, tB);                              // tA = dpre1 = (dpre2 W2) * (1 - h1^2)
      // tB = h0, recomputed (cheaper than keeping it live) in the shadow of the next dgrad's MFMAs
      fd_layer_dgrad(W1s, tA, tC, r, q, [&](int g) { if ((g & 3) == 0) coord_block(tB, g >> 2); });
      fd_mul_dtanh(tC, tB);                              // tC = dpre0 = (dpre1 W1) * (1 - h0^2)
    }
    // ---- wgrad of layer 1: exchange (dpre1 = tA, h0 = tB) ----
    for (int c = 0; c < nex; ++c) {
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
        f.rowtp[row] = sc * (d1 * u0c - d0 * u1c);
        f.rowtp[f.M + row] = d0 * u0c + d1 * u1c;
        f.rowtp[2 * f.M + row] = d0;
        f.rowtp[3 * f.M + row] = d1;
      }
    }
    // ---- coordinate layer backward, cross-row part: dWc, dbc/dhz via staged dpre0 ----
    for (int c = 0; c < ((f.ablate & 2) ? 0 : nact); ++c) {
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
  const float t1 = fd_sum_q(db1), t2 = fd_sum_q(db2), tc0 = fd_sum_q(aWc0), tc1 = fd_sum_q(aWc1);
  if (q == 0) {
    rec[2 * FD_H * FD_H + 16 * wave + r] = t1;
    rec[2 * FD_H * FD_H + FD_H + 16 * wave + r] = t2;
    rec[2 * FD_H * FD_H + 2 * FD_H + 16 * wave + r] = tc0;
    rec[2 * FD_H * FD_H + 3 * FD_H + 16 * wave + r] = tc1;
  }
  const float tb = pv_wave_sum(dbo);
  if (lane == 0) sm[OFF_RED + wave] = tb;
  __syncthreads();
  if (tid < FD_H) {
    float v = 0.0f;
#pragma unroll
    for (int w = 0; w < FD_WAVES; ++w) v += sm[OFF_DWO + w * FD_H + tid];
    rec[2 * FD_H * FD_H + 4 * FD_H + tid] = v;
  }
  if (tid == 0) {
    float v = 0.0f;
    for (int w = 0; w < FD_WAVES; ++w) v += sm[OFF_RED + w];
    rec[2 * FD_H * FD_H + 5 * FD_H] = v;
  }
}

// ---- per-workgroup records -> flat gradient buffer (fixed summation order) ---------------------------
__global__ __launch_bounds__(256) void pv_sdec_fused_reduce_kernel(const float* __restrict__ part, int G_,
                                                                   float* __restrict__ Gr, PvFusedOffsets o, int cd,
                                                                   int dwo_slots) {
  __shared__ PvRedLds sm;
  pv_sdec_fused_reduce_block(part, G_, Gr, o, cd, dwo_slots, blockIdx.x, sm);
}

int pv_sdec_fused_reduce(const float* part, int grid, float* G, const PvFusedOffsets& o, int cd, int dwo_slots,
                         hipStream_t s) {
  hipLaunchKernelGGL(pv_sdec_fused_reduce_kernel, dim3(PV_FUSED_REDUCE_BLOCKS), dim3(256), 0, s, part, grid, G, o, cd,
                     dwo_slots);
  PV_LAUNCH_CHECK();
  return 0;
}

// ---- host side -----------------------------------------------------------------------------------------
bool pv_sdec_fused_supported(const pv_ivae_plan* p) {
  return pv_sdec_fused_trunk_supported(p) && p->n_pix % FD_UNIT == 0 && p->out.out_dim == 1;
}

// everything of pv_sdec_fused_supported but the output layer's width and the rows per sample (the multi-channel kernel's
// predicate, pv_sdec_fused_mc_supported, adds its own)
bool pv_sdec_fused_trunk_supported(const pv_ivae_plan* p) {
  if (!p || p->coord_dim < 1 || p->coord_dim > 2) return false;
  if (p->n_dec != 2) return false;
  const pv_layer& c = p->fc_coord;
  const pv_layer& l = p->fc_latent;
  if (c.out_dim != FD_H || c.b_off < 0 || l.out_dim != FD_H) return false;
  for (int i = 0; i < 2; ++i) {
    const pv_layer& d = p->dec[i];
    if (d.in_dim != FD_H || d.out_dim != FD_H || d.act != PV_ACT_TANH || d.b_off < 0) return false;
    if (d.w_off % 4 != 0) return false;          // 16-byte aligned rows for the LDS staging loads
  }
  if (p->out.in_dim != FD_H || p->out.b_off < 0) return false;
  return true;
}

static int fd_num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      cus = n;
    else
      cus = 256;          // MI355X; also the answer on a build box without a GPU
  }
  return cus;
}

int pv_sdec_fused_grid(int64_t units) { return sd_grid(units, fd_num_cus()); }

int pv_sdec_fused_kmax(int rows, int64_t units, int grid, int waves) { return sd_kmax(rows, units, grid, waves); }

// ---- test hooks (outside include/pyroved_amd.h): pv_sdec_partition.h evaluated on the host, in bulk.  Nothing touches the GPU ----
// bounds (G + 1): the workgroups' ranges; gfirst (samples); tail (2 G): [2 g] whether range g ends in a tail at 4-unit tiles, [2 g + 1] at
// 8-unit tiles; *grid = G for `cus` compute units (the caller sizes bounds and tail for G <= cus); *kmax for `waves` publishing waves
extern "C" int pv_debug_partition_table(int upb, int samples, int cus, int waves, int64_t* bounds, int32_t* gfirst, int32_t* tail,
                                        int32_t* grid, int32_t* kmax) {
  if (upb < 1 || samples < 1 || cus < 1 || waves < 1 || upb > INT32_MAX / FD_UNIT) return PV_EINVAL;
  const int rows = upb * FD_UNIT;
  const int64_t units = (int64_t)samples * sd_units_per_sample(rows);
  const int G = sd_grid(units, cus);
  for (int g = 0; g <= G; ++g) bounds[g] = sd_unit_bound(g, units, G);
  for (int g = 0; g < G; ++g) {
    tail[2 * g] = sd_ends_in_tail(bounds[g], bounds[g + 1], 4);
    tail[2 * g + 1] = sd_ends_in_tail(bounds[g], bounds[g + 1], 8);
  }
  for (int b = 0; b < samples; ++b) gfirst[b] = sd_gfirst(b, upb, G, units);
  *grid = G;
  *kmax = sd_kmax(rows, units, G, waves);
  return 0;
}

// the kernels' walk over every unit with U as the unit type: wave w of a workgroup starts at sd_pos_of(u_lo + w) and reaches its later
// units by sd_pos_advance(..., waves).  check: compare with the arrays instead of filling them.  Returns the units that differ
template <class U>
static int64_t fd_partition_walk(int upb, int64_t units, int G, int waves, int64_t x_units, int32_t* b, int32_t* loc, int64_t* xu,
                                 bool check) {
  int64_t bad = 0;
  for (int g = 0; g < G; ++g) {
    const U lo = (U)sd_unit_bound(g, units, G), hi = (U)sd_unit_bound(g + 1, units, G);
    for (int w = 0; w < waves && lo + w < hi; ++w) {
      SdPos<U> p = sd_pos_of<U>(lo + w, upb, (U)x_units);
      for (;; sd_pos_advance(p, waves, upb, (U)x_units)) {
        if (p.unit < lo || p.unit >= hi) return -1;
        if (check) bad += b[p.unit] != p.b || loc[p.unit] != p.loc || xu[p.unit] != (int64_t)p.xu;
        else { b[p.unit] = p.b; loc[p.unit] = p.loc; xu[p.unit] = (int64_t)p.xu; }
        if (p.unit + waves >= hi) break;
      }
    }
  }
  return bad;
}

// b, loc, xu (samples upb each): every unit's walked position on `grid` workgroups of `waves` waves; the 64-bit walk fills them and
// the 32-bit walk must agree.  x_units: 0, or the period of the observations in units
extern "C" int pv_debug_partition_walk(int upb, int samples, int grid, int waves, int64_t x_units, int32_t* b, int32_t* loc,
                                       int64_t* xu) {
  const int64_t units = (int64_t)samples * upb;
  if (upb < 1 || samples < 1 || waves < 1 || x_units < 0 || units > INT32_MAX / FD_UNIT || grid < 1 || grid > units) return PV_EINVAL;
  if (fd_partition_walk<int64_t>(upb, units, grid, waves, x_units, b, loc, xu, false) != 0) return PV_EINVAL;
  return fd_partition_walk<int>(upb, units, grid, waves, x_units, b, loc, xu, true) == 0 ? 0 : PV_EINVAL;
}

int pv_sdec_fused_launch(const PvFused& f_in, int grid, bool grads, hipStream_t s) {
  PvFused f = f_in;
  static const int ablate = pv_exp_int("PV_FD_ABLATE", 0);
  f.ablate = ablate;
  const size_t lds = FD_LDS_FLOATS * sizeof(float);
  PV_TRY(pv_set_dynamic_lds(reinterpret_cast<const void*>(&pv_sdec_fused_kernel<true>), (int)lds));
  PV_TRY(pv_set_dynamic_lds(reinterpret_cast<const void*>(&pv_sdec_fused_kernel<false>), (int)lds));
  if (grads)
    hipLaunchKernelGGL(pv_sdec_fused_kernel<true>, dim3(grid), dim3(FD_THREADS), lds, s, f);
  else
    hipLaunchKernelGGL(pv_sdec_fused_kernel<false>, dim3(grid), dim3(FD_THREADS), lds, s, f);
  PV_LAUNCH_CHECK();
  return 0;
}
