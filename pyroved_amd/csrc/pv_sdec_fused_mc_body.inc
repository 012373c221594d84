// pv_sdec_fused_mc_body.inc — the kernel of pv_sdec_fused_mc.hip, included once per likelihood family with
//   FDM_KERNEL  the __global__'s name        FDM_CAT  0: the per-value likelihoods (fdm_pixel_lik), 1: PV_LIK_CATEGORICAL
//   FDM_TAIL    0: every sample's positions fill its units (f.N % 16 == 0); 1: the tail form (PV_PLAN_FUSED_TAIL) — a sample
//               occupies f.N = 16 ceil(f.n_obs / 16) rows of the partition and observes the first f.n_obs of them
// so that each family is a kernel template of its own, written once: the per-value instances compile from this text with the
// categorical pass a constant-false block (their registers and code are what they were before the categorical family existed:
// profiles/categorical_resource_usage.txt), and the categorical instances carry no run-time likelihood switch.
template <bool GRADS, int C, int WEIGHTED>
__global__ __launch_bounds__(FD_THREADS, 2) void FDM_KERNEL(PvFused f) {
  constexpr bool CAT = FDM_CAT != 0;
  constexpr bool TAIL = FDM_TAIL != 0;
  static_assert(!CAT || C >= 2, "classes per row");
  static_assert(!CAT || !TAIL, "the tail form exists for the per-value likelihoods");
  static_assert(WEIGHTED >= 0 && WEIGHTED <= 2 && C >= ((WEIGHTED || TAIL) ? 1 : 2) && C <= 8, "instances");
  static_assert(C * FD_H <= FD_WAVES * FD_H && FD_UNIT * C <= FD_H && 40 + C <= 64, "LDS regions");
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
  const int upb = sd_units_per_sample(f.N);            // (N = rows per sample; the partition, its slots: pv_sdec_partition.h)

  auto flush_hz = [&](int b) {
    // sample b's rows end (or the workgroup's do): publish this workgroup's partial dL/d(hz[b])
    const float t = fd_sum_q(ahz);
    if (q == 0) f.part_hz[sd_slot<1>(b, g, 0, f.kmax, upb, G, f.units) * FD_H + 16 * wave + r] = t;
  };

  const int64_t u_lo = sd_unit_bound(g, f.units, G), u_hi = sd_unit_bound(g + 1, f.units, G);
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
    // TAIL: rows n >= f.n_obs of a sample are padding — no grid position, no observation, no weight: they read none of the three,
    // take the coordinates (0, 0) and dL/da = 0, and write zeros where the per-sample sums read all f.N rows (llrow, rowtp).
    // x, loc and the per-image weights keep the caller's layout: observation (b, n, c) at (b * n_obs + n) * C + c
    const bool valid = !TAIL || n < f.n_obs;
    const int64_t orow = TAIL ? (int64_t)b * f.n_obs + n : row;
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
      if (!valid) {
        // (x0 = x1 = 0)
      } else if (f.cd == 2) {
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
        if (CAT) {                 // the logit waits in dlda[c] for the pass below
          dlda[c] = a;
          FD_SCHED_FENCE();
          continue;
        }
        const float xv = (f.x && valid) ? f.x[orow * C + c] : 0.0f;
        const float pwv = !valid ? 0.0f : WEIGHTED == 2 ? f.pw[orow * C + c] : WEIGHTED == 1 ? f.pw[n * C + c] : 1.0f;
        float ll, locv;
        fdm_pixel_lik(f, a, xv, ll, dlda[c], locv);
        if (WEIGHTED) { ll *= pwv; dlda[c] *= pwv; }
        if (TAIL && !valid) { ll = 0.0f; dlda[c] = 0.0f; }
        llsum += ll;
        if (q == 0 && valid && f.loc) f.loc[orow * C + c] = locv;
        FD_SCHED_FENCE();        // one channel at a time: hoisted, the C channels' Wo reads alone would take 32 C VGPRs
      }
      if (CAT) {
        auto xw_of = [&](int c) {                            // the weighted observation w x of class c (x null: zeros)
          const float xv = f.x ? f.x[row * C + c] : 0.0f;
          return WEIGHTED == 2 ? xv * f.pw[row * C + c] : WEIGHTED == 1 ? xv * f.pw[n * C + c] : xv;
        };
        float mx = dlda[0];
#pragma unroll
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, dlda[c]);
        float se = 0.0f, sx = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          dlda[c] -= mx;                                     // <= 0: no exp overflows at any logit
          se += sd_exp(dlda[c]);
          sx += xw_of(c);
        }
        const float lnse = sd_log(se), rse = sd_rcp(se);     // lse = mx + lnse
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float xw = xw_of(c);
          const float pc = sd_exp(dlda[c]) * rse;
          llsum += xw * (dlda[c] - lnse);                    // xw = 0 gives exactly 0 however small p_c is
          dlda[c] = pc * sx - xw;
          if (q == 0 && f.loc) f.loc[row * C + c] = pc;
        }
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
        if (!valid) {
          u0c = 0.0f;                                  // (d0 = d1 = 0 exactly: the row's four entries are zeros)
        } else if (f.cd == 2) {
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

