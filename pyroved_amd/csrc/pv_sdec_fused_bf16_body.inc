// pv_sdec_fused_bf16_body.inc — the body of pv_sdec_fused_bf16.hip's 4-wave kernel, included ONCE PER __global__ that runs it:
// pv_sdec_fused_bf16_kernel (WT = false) and pv_sdec_fused_bf16_wt_kernel (WT = true).  Textual inclusion, not a shared
// __device__ function: inlined through a call the unweighted instances came out with other register allocation and instruction
// order than they had as a kernel of their own, and those instances are held to their code symbol by symbol
// (scripts/compare_kernel_asm.py).  In scope at the point of inclusion: the template parameters GRADS, LIK, PREC; the kernel
// argument `f` (PvFused, by value); constexpr bool WT; const float* pwt and int pw_img (WT: the weights and which index reads them).
  using PP = FbP<PREC>;
  using LL = FbLds<PREC>;
  constexpr bool F16 = PP::F16, OV = LL::OV;
  extern __shared__ __attribute__((aligned(16))) char smb[];
  FB_KSTAMP(0);                                                          // kernel entry
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.x, G = gridDim.x;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smb);
  const __bf16* W1h = reinterpret_cast<const __bf16*>(smb + LL::W1H);
  const __bf16* W1l = reinterpret_cast<const __bf16*>(smb + LL::W1L);
  const __bf16* W2h = reinterpret_cast<const __bf16*>(smb + LL::W2H);
  const __bf16* W2l = reinterpret_cast<const __bf16*>(smb + LL::W2L);
  __bf16* st2 = reinterpret_cast<__bf16*>(smb + LL::ST2);          // wgrad-2 staging (two-piece weights: over W1's images)
  __bf16* st1 = reinterpret_cast<__bf16*>(smb + LL::ST1);          // wgrad-1 staging (two-piece weights: over W2's images)
  constexpr int SB = LL::NAD_D * ST_ARR;                           // the second operand's arrays follow the first's
  float* vec = reinterpret_cast<float*>(smb + BO_VEC);
  float* info = reinterpret_cast<float*>(smb + BO_INFO);
  float* red = reinterpret_cast<float*>(smb + BO_RED);
  const char* gimg = reinterpret_cast<const char*>(f.wimg);

  // ---- weight images by LDS-DMA, fp32 vectors by hand ----
  // (round 6) Training launches of the two-piece builds wait for W2's images in every tile anyway (the barrier in front of the
  // forward of layer 2: they are reloaded per tile), so the prologue only waits for W1's: W2's 64 KB are requested LAST — behind
  // the vectors, the first unit's observations and its prefetch slots — and land under the first tile's coordinate layer and
  // forward of layer 1.
  constexpr bool LATE_W2 = OV && GRADS;
  sd_reload<IMG_BYTES, FB_WAVES>(gimg, lds0 + LL::W1H, wave, lane);
  if (!LATE_W2) sd_reload<IMG_BYTES, FB_WAVES>(gimg + 2 * IMG_BYTES, lds0 + LL::W2H, wave, lane);
  if (PP::WP == 2) {
    sd_reload<IMG_BYTES, FB_WAVES>(gimg + IMG_BYTES, lds0 + LL::W1L, wave, lane);
    if (!LATE_W2) sd_reload<IMG_BYTES, FB_WAVES>(gimg + 3 * IMG_BYTES, lds0 + LL::W2L, wave, lane);
  }
  // fp16 modes: the images' power-of-two scales (written by the preparation, pv_fb_layout.h); everything derived from them
  // is wave-uniform.  The forward un-scales in tanh's multiply (c1, c2); the backward carries kso * m down the dgrad chain
  // and removes uw2 / uw1 / u0 where a gradient leaves the kernel.
  float s1 = 1.0f, s2 = 1.0f, kso = 1.0f, c1 = SD_C, c2 = SD_C, uw2 = 1.0f, uw1 = 1.0f, u0 = 1.0f;
  if (F16) {
    const float* sc = reinterpret_cast<const float*>(gimg + FB_SCALE_OFF);
    s1 = __builtin_amdgcn_readfirstlane(sc[0]); s2 = __builtin_amdgcn_readfirstlane(sc[1]);
    kso = FB_KAPPA * __builtin_amdgcn_readfirstlane(sc[2]);
    c1 = SD_C / s1; c2 = SD_C / s2;
    uw2 = __builtin_amdgcn_ldexpf(1.0f / kso, -f.dl_exp);
    uw1 = uw2 / s2;
    u0 = 1.0f / (kso * s1 * s2);
  }
  for (int j = tid; j < FD_H; j += FB_THREADS) {
    vec[j] = f.Wc[j * f.cd];
    vec[FD_H + j] = f.cd == 2 ? f.Wc[j * 2 + 1] : 0.0f;
    vec[2 * FD_H + j] = f.bc[j];
    vec[3 * FD_H + j] = f.wo[j];
    vec[4 * FD_H + j] = f.b1[j] * s1;
    vec[5 * FD_H + j] = f.b2[j] * s2;
  }
  if (!LATE_W2) {
    sd_wait_vm0();
    __syncthreads();
  }
  const float bo = f.bo[0];

  // persistent accumulators: dW1 / dW2 rows 16*(2*wave + s) .. +15, s = 0, 1 ; bias sums likewise
  f32x4 accW1[2][8], accW2[2][8], accB1[2], accB2[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    accB1[s] = f32x4{0, 0, 0, 0};
    accB2[s] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) { accW1[s][kb] = f32x4{0, 0, 0, 0}; accW2[s][kb] = f32x4{0, 0, 0, 0}; }
  }
  float dbo = 0.0f;
  // plain bf16 has the registers to keep d(wo) per lane (row r's share of columns 16*jb + 4q + i) for the whole kernel:
  // one cross-row reduction at the end instead of one per tile
  f32x4 accWo[PP::KEEP_WO ? 8 : 1];
#pragma unroll
  for (int jb = 0; jb < (PP::KEEP_WO ? 8 : 1); ++jb) accWo[jb] = f32x4{0, 0, 0, 0};
  int cur_b = -1;                                    // the sample whose dL/d(hz) this WAVE is accumulating
  const int upb = sd_units_per_sample(f.N);          // (the partition, its slots and the walk: pv_sdec_partition.h)
  float* rec = f.part + (int64_t)g * FD_REC;
  // this wave's column-sum accumulators (lane l owns columns 2l, 2l+1 of each): d(wo), dL/d(hz[cur_b]) (flushed when the wave's
  // sample changes), dWc0, dWc1
  float2 cs_wo = float2{0.0f, 0.0f}, cs_hz = float2{0.0f, 0.0f}, cs_c0 = float2{0.0f, 0.0f}, cs_c1 = float2{0.0f, 0.0f};
  float2 cs_none = float2{0.0f, 0.0f};

  // (round 6) f.part_rs: the wave's running sums over its rows of sample cur_b of {ll, d(phi), d(scale), d(tx), d(ty)} — every lane
  // (r, q) carries row r's share (the four q copies are equal), published with dL/d(hz) instead of five stores per row and tile
  float rs0 = 0.0f, rs1 = 0.0f, rs2 = 0.0f, rs3 = 0.0f, rs4 = 0.0f;
  auto flush_hz = [&](int b) {
    // the wave's rows of sample b end (or the workgroup's do): publish its partial dL/d(hz[b]) in its own slot
    // (kmax counts FB_WAVES slots per workgroup that can touch a sample; unused slots stay zero)
    const int gfirst = sd_gfirst(b, upb, G, f.units);
    const int64_t slot = (int64_t)b * f.kmax + (g - gfirst) * FB_WAVES + wave;       // (sd_slot<FB_WAVES>, written out)
    *reinterpret_cast<float2*>(f.part_hz + slot * FD_H + 2 * lane) = cs_hz;
    cs_hz = float2{0.0f, 0.0f};
    if (GRADS && f.part_rs) {
      const float v0 = fb_row16_sum(rs0), v1 = fb_row16_sum(rs1), v2 = fb_row16_sum(rs2), v3 = fb_row16_sum(rs3), v4 = fb_row16_sum(rs4);
      if (lane == 0) {
        float* d = f.part_rs + slot * PV_RS_W;
        *reinterpret_cast<f32x4*>(d) = f32x4{v0, v1, v2, v3};
        d[4] = v4;
      }
      rs0 = rs1 = rs2 = rs3 = rs4 = 0.0f;
    }
  };

  // A unit's position is carried from tile to tile (round 2).  Units stay 64-bit here (this kernel also serves problems beyond 2^31 rows).
  const int64_t u_lo = sd_unit_bound(g, f.units, G), u_hi = sd_unit_bound(g + 1, f.units, G);
  using Pos = SdPos<int64_t>;
  auto pos_of = [&](int64_t unit_) { return sd_pos_of<int64_t>(unit_, upb, f.x_units); };
  auto advance = [&](Pos& p_, int by) { sd_pos_advance<int64_t>(p_, by, upb, f.x_units); };
  // (H231 build) a range of 4 n + 1 units ends with a column-parallel tail (below): the row-parallel tiles cover [u_lo, u_end), and
  // what a wave without a further unit prefetches is the TAIL unit's inputs (every wave takes part in the tail)
  constexpr bool TAIL = FB_TAIL && GRADS && PREC == FB_P_H231;
#ifdef PV_EXPERIMENTS
  const int qsw = f.qswap;                  // the images' column order (pv_fb_layout.h): plain in the shipped build
#else
  constexpr int qsw = 0;
#endif
  const bool has_tail = TAIL && sd_ends_in_tail(u_lo, u_hi, TILE_UNITS) && !(f.ablate & 512);   // (ablate: experiments build only)
  const int64_t u_end = has_tail ? u_hi - 1 : u_hi;
  const Pos pos_lo = pos_of(has_tail ? u_end : u_lo);   // what an out-of-range wave fetches instead (valid; unused without a tail)
  Pos pos_cur = pos_of(u_lo + wave < u_end ? u_lo + wave : (has_tail ? u_end : u_lo));
  Pos pos_nx = pos_cur;
  // the wave's observations are fetched one tile ahead (an HBM miss, and loads retire in order: fetched in the
  // tile itself it would hold up the coordinate layer's own small loads)
  float sw_next = 1.0f;                  // (jiVAE) weight of the unit's sample, fetched with its observations
  float pw_next = 1.0f;                  // (WT) weight of the row's observation, likewise
  auto x_of = [&](const Pos& p_) -> float {
    if (f.sw) sw_next = f.sw[p_.b];
    if constexpr (WT) pw_next = pwt[(pw_img ? p_.xu : (int64_t)p_.loc) * FD_UNIT + r];      // (wave-uniform choice)
    return f.x[p_.xu * FD_UNIT + r];
  };
  float xv_next = x_of(pos_cur);
  // ... and so are its other per-unit inputs (hz[b], tp[b], the unit's grid rows), by LDS-DMA into the wave's own
  // slots: the coordinate layer then starts from LDS instead of waiting ~1.5k cycles on dependent global loads
  float* chz = reinterpret_cast<float*>(smb + BO_CHZ) + wave * FD_H;
  float* ctp = reinterpret_cast<float*>(smb + BO_CTP) + wave * 64;
  float* cgr = reinterpret_cast<float*>(smb + BO_CGR) + wave * 64;
  auto fetch_unit_inputs = [&](const Pos& p_) {
    const int b_ = p_.b;
    const int n0 = p_.loc * FD_UNIT;
    sd_glds4(f.hz + (int64_t)b_ * FD_H + lane, lds0 + BO_CHZ + wave * (FD_H * 4));
    sd_glds4(f.hz + (int64_t)b_ * FD_H + 64 + lane, lds0 + BO_CHZ + wave * (FD_H * 4) + 256);
    sd_glds4(f.tp + (int64_t)b_ * 8 + (lane & 7), lds0 + BO_CTP + wave * 256);
    sd_glds4(f.grid + (int64_t)n0 * f.cd + (lane & (16 * f.cd - 1)), lds0 + BO_CGR + wave * 256);
  };
  fetch_unit_inputs(pos_cur);
  if (LATE_W2) {
    // everything requested so far lands (W1's images, the first unit's observations and slots) — the observation registers are
    // touched here so that the compiler's own wait for them stands HERE and not at their first use inside the tile, where it
    // would drain W2's requests as well — then W2's images are requested and the tile loop starts without waiting for them
    sd_wait_vm0();
    asm volatile("" : "+v"(xv_next), "+v"(sw_next));
    if constexpr (WT) asm volatile("" : "+v"(pw_next));
    sd_reload<IMG_BYTES, FB_WAVES>(gimg + 2 * IMG_BYTES, lds0 + LL::W2H, wave, lane);
    sd_reload<IMG_BYTES, FB_WAVES>(gimg + 3 * IMG_BYTES, lds0 + LL::W2L, wave, lane);
    __syncthreads();
  }
  int tile_no = -1;
  FB_KSTAMP(1);                                                          // prologue done
  for (int64_t ut = u_lo; ut < u_end; ut += TILE_UNITS) {
    ++tile_no;
    FB_STAMP(0);
    const int nact = (int)((u_end - ut) < TILE_UNITS ? (u_end - ut) : TILE_UNITS);
    if (ut + TILE_UNITS + wave < u_hi) advance(pos_nx, TILE_UNITS);     // the unit this wave fetches for the NEXT tile
    else pos_nx = pos_lo;
    int opq = 0;
    asm volatile("" : "+v"(opq));       // loop-variant zero: keeps LICM from hoisting the LDS-resident vectors
    const float* Wc0 = vec + opq;
    const float* Wc1 = vec + FD_H + opq;
    const float* bcs = vec + 2 * FD_H + opq;
    const float* wos = vec + 3 * FD_H + opq;
    const float* b1s = vec + 4 * FD_H + opq;
    const float* b2s = vec + 5 * FD_H + opq;

    // the wave's unit; an inactive wave (partial last tile) computes nothing and stages zeros
    const bool act = wave < nact;
    const int unit = (int)ut + (act ? wave : 0);
    const int bu = pos_cur.b;
    // the wave's sample changes with this tile: publish the old one's sums first (round 6: at the TOP of the tile — nothing between
    // here and the coordinate layer's column sums touches them — so that this tile's row sums can be added where they arise)
    if (GRADS && act && bu != cur_b) {
      if (cur_b >= 0) flush_hz(cur_b);
      cur_b = bu;
    }
    const int64_t row = (int64_t)unit * FD_UNIT + r;
    float x0, x1, u0c, u1c, sc;
    // this wave's LDS-DMA of the tile's inputs (issued a tile ago; first tile: in front of W2's images, which stay in flight)
    if (!(LATE_W2 && tile_no == 0)) sd_wait_vm0();
    {
      const float* t = ctp + opq;
      const float* gr = cgr + opq;
      if (f.cd == 2) {
        const float gx = gr[2 * r], gy = gr[2 * r + 1];
        u0c = gx * t[0] - gy * t[1];
        u1c = gx * t[1] + gy * t[0];
        sc = t[2];
        x0 = u0c * sc + t[3];
        x1 = u1c * sc + t[4];
      } else {
        u0c = gr[r]; u1c = 0.0f; sc = 1.0f;
        x0 = u0c + t[3]; x1 = 0.0f;
      }
    }
    const float* hzb = chz + opq;
    const float xv = xv_next, swv = sw_next;
    const float pwv = pw_next;

    f32x4 h0[8], tA[8], tB[8], tC[8];
    bf16x4 pAh[8], pAl[8], pBh[8], pBl[8];
    // (round 2) A wave without a unit of its own (partial last tile) runs the same straight-line code on a valid unit of
    // the workgroup's range (what its prefetch slots hold) with its dL/dlogit forced to zero — every gradient it stages or
    // accumulates is then zero, its per-row outputs are not stored — instead of skipping the phases under wave-uniform
    // branches: the merges those branches create cost register copies in every tile (pv_sdec_fused_w8.hip).
    {
      // ---- coordinate layer (fp32): h0 = tanh(Wc x' + bc + hz[b]) ----
#pragma unroll
      for (int jb = 0; jb < 8; ++jb) {
        const int j = 16 * jb + 4 * q;
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(Wc0 + j);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(Wc1 + j);
        const f32x4 bc = *reinterpret_cast<const f32x4*>(bcs + j);
        const f32x4 hz = *reinterpret_cast<const f32x4*>(hzb + j);
#pragma unroll
        for (int i = 0; i < 4; ++i) h0[jb][i] = w0[i] * x0 + w1[i] * x1 + bc[i] + hz[i];
      }
      fb_tanh8(h0);
      fb_presplit<F16, PP::FWD_LO>(h0, pBh, pBl);
    }
    FB_STAMP(1);
    fetch_unit_inputs(pos_nx);                   // the slots were consumed by the coordinate layer above
    if (OV && GRADS && tile_no > 0) {
      // W2's images were the previous tile's staging area: bring them back under the forward of layer 1.
      // (every compiler-visible load above has been consumed; none is issued before the barrier below)
      sd_wait_vm0();
      sd_reload<LL::RL_BYTES, FB_WAVES>(gimg + LL::RL2_SRC, lds0 + LL::RL2_LDS, wave, lane);
    }
    {
      fb_layer_fwd<PREC>(W1h, W1l, b1s, pBh, pBl, tB, r, q, qsw);
      fb_tanh8(tB, c1);                                          // tB = h1
      fb_presplit<F16, PP::HL>(tB, pBh, pBl);                    // feeds layer 2 and its wgrad
    }
    FB_STAMP(2);
    if (OV && GRADS) {
      sd_wait_vm0();
      __syncthreads();      // W2 landed everywhere; every wave is past its reads of W1 (staging may overwrite it)
    }
    FB_STAMP(3);
    float dlda = 0.0f;
    float frow = 0.0f;                                  // fp16 modes: what turns the row's normalised dL/dpre0 into the true one
    half4_ ph4 = half4_{};                              //             the row's 2^(e + dl_exp) as fp16 (staged activations)
    {
      fb_layer_fwd<PREC>(W2h, W2l, b2s, pBh, pBl, tC, r, q, qsw);
      FB_STAMP(16);
      fb_tanh8(tC, c2);                                          // tC = h2
      FB_STAMP(17);
      // ---- output layer + likelihood (fp32) ----
      // (four independent accumulation chains: one chain of 32 dependent multiply-adds is ~250 cycles of pure latency for the
      //  single wave of a SIMD)
      f32x4 part4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int jb = 0; jb < 8; ++jb) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wos + 16 * jb + 4 * q);
        part4 = part4 + tC[jb] * wv;
      }
      const float a = fb_sum_q((part4[0] + part4[1]) + (part4[2] + part4[3])) + bo;
      float ll, locv;
      // (sd_pixel_lik<LIK> written out: called as the function, this site compiles to other code — same math, see its comment)
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
      FB_STAMP(18);
      if constexpr (WT) {
        // (selects, not bare products: a zero weight gives zero whatever the row's unweighted values are)
        ll = pwv == 0.0f ? 0.0f : ll * pwv;
        dlda = pwv == 0.0f ? 0.0f : dlda * pwv;
      }
      dlda *= act ? swv : 0.0f;
      if (GRADS && f.part_rs) {
        rs0 += act ? ll : 0.0f;
        if (q == 0 && act && f.loc) f.loc[row] = locv;
      } else if (q == 0 && act) {
        if (f.llrow) f.llrow[row] = ll;
        if (f.loc) f.loc[row] = locv;
      }
      xv_next = x_of(pos_nx);                   // lands long before the next LDS-DMA issue point drains loads
      if (GRADS) {
        if (q == 0) dbo += dlda;
        if (PP::KEEP_WO) {
#pragma unroll
          for (int jb = 0; jb < 8; ++jb) accWo[jb] += dlda * tC[jb];
        } else {
          // d(wo)[j] += sum_rows dlda * h2[row][j]: W1's images are dead since the barrier above (the wgrad-2 staging
          // goes there next), so the wave's own staging rows serve as the transpose buffer
          f32x4 pv_[8];
#pragma unroll
          for (int jb = 0; jb < 8; ++jb) pv_[jb] = dlda * tC[jb];
          fb_colsum<0>(pv_, reinterpret_cast<float*>(st2) + (16 * wave) * (LDS2 / 2), cs_wo, cs_none, cs_none, nullptr,
                       nullptr, lane, r, q);
        }
        FB_STAMP(19);
        float dn = dlda;                       // the row factor of dpre2
        if (F16) {
          // dL/dlogit = m 2^e: the mantissa (times kappa s_o) goes down the dgrad chain, the exponent into the staged rows
          const int e = __builtin_amdgcn_frexp_expf(dlda);
          dn = __builtin_amdgcn_frexp_mantf(dlda) * kso;
          const _Float16 ph = (_Float16)__builtin_amdgcn_ldexpf(1.0f, e + f.dl_exp);
          ph4 = half4_{ph, ph, ph, ph};
          frow = __builtin_amdgcn_ldexpf(u0, e);
        }
#pragma unroll
        for (int jb = 0; jb < 8; ++jb) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wos + 16 * jb + 4 * q);
#pragma unroll
          for (int i = 0; i < 4; ++i) tC[jb][i] = dn * wv[i] * (1.0f - tC[jb][i] * tC[jb][i]);  // dpre2
        }
        FB_STAMP(20);
        fb_presplit<F16, PP::DL2>(tC, pAh, pAl);                     // feeds the wgrad and the dgrad of layer 2
      }
    }
    FB_STAMP(4);
    pos_cur = pos_nx;                     // (unit, bu, row of THIS tile were taken above)
    if (!GRADS) continue;
    const int ksteps = nact > 2 ? 2 : 1;          // rows 32.. are only staged (as zeros or not) when a unit owns them

    // ---- wgrad of layer 2: stage (dpre2, h1) of all 64 rows over W1's images, one pass ----
    fb_stage_store<LL::NAD_D == 2, false>(st2, st2 + ST_ARR, pAh, pAl, 16 * wave + r, q);
    fb_stage_store<PP::WG3, F16>(st2 + SB, st2 + SB + ST_ARR, pBh, pBl, 16 * wave + r, q, ph4);
    __syncthreads();
    FB_STAMP(5);
    fb_wgrad_consume<PREC>(st2, accW2, accB2, wave, r, q, ksteps);
    if (OV) {
      __syncthreads();
      FB_STAMP(6);
      sd_wait_vm0();                                   // (stores only: nothing the compiler still waits for)
      sd_reload<LL::RL_BYTES, FB_WAVES>(gimg + LL::RL1_SRC, lds0 + LL::RL1_LDS, wave, lane);   // W1 comes back under the dgrad of layer 2
    }
    {
      fb_layer_dgrad<PREC, PP::DGR2_LO>(W2h, W2l, pAh, pAl, tA, r, q, qsw);
      fb_mul_dtanh(tA, tB);                                      // tA = dpre1 (fp16 modes: times s2 kso / m 2^e ... carried)
      fb_presplit<F16, PP::DL1>(tA, pAh, pAl);                   // feeds the dgrad and the wgrad of layer 1
    }
    FB_STAMP(7);
    if (OV) {
      sd_wait_vm0();
      __syncthreads();      // W1 landed everywhere; every wave is past its reads of W2
    }
    FB_STAMP(8);
    {
      fb_layer_dgrad<PREC, PP::DGR1_LO>(W1h, W1l, pAh, pAl, tC, r, q, qsw);
      fb_mul_dtanh(tC, h0);                                      // tC = dpre0 (fp16 modes: normalised; frow restores the row)
      // ---- coordinate layer, cross-row part: dhz[b] = sum_rows dpre0, dWc_k = sum_rows dpre0 * x'_k.  Wave-local
      // (the unit's rows all belong to this wave and to one sample): W2's images are dead since the barrier above, so
      // the wave's own rows of the wgrad-1 staging area serve as the transpose buffer.  No workgroup barrier.
      if (F16) {
        if (q == 0) {
          info[16 * wave + r] = frow * x0; info[TILE_ROWS + 16 * wave + r] = frow * x1; info[2 * TILE_ROWS + 16 * wave + r] = frow;
        }
        fb_colsum<3>(tC, reinterpret_cast<float*>(st1) + (16 * wave) * (LDS2 / 2), cs_hz, cs_c0, cs_c1,
                     info + 16 * wave, info + TILE_ROWS + 16 * wave, lane, r, q, info + 2 * TILE_ROWS + 16 * wave);
      } else {
        if (q == 0) { info[16 * wave + r] = x0; info[TILE_ROWS + 16 * wave + r] = x1; }
        fb_colsum<2>(tC, reinterpret_cast<float*>(st1) + (16 * wave) * (LDS2 / 2), cs_hz, cs_c0, cs_c1,
                     info + 16 * wave, info + TILE_ROWS + 16 * wave, lane, r, q);
      }
      fb_presplit<F16, PP::WG3>(h0, pBh, pBl);
    }
    FB_STAMP(9);
    // ---- wgrad of layer 1: stage (dpre1, h0) over W2's images ----
    fb_stage_store<LL::NAD_D == 2, false>(st1, st1 + ST_ARR, pAh, pAl, 16 * wave + r, q);
    fb_stage_store<PP::WG3, F16>(st1 + SB, st1 + SB + ST_ARR, pBh, pBl, 16 * wave + r, q, ph4);
    __syncthreads();
    FB_STAMP(10);
    fb_wgrad_consume<PREC>(st1, accW1, accB1, wave, r, q, ksteps);
    FB_STAMP(21);
    // ---- coordinate layer backward (fp32): row-local part ----
    {
      f32x4 d04 = {0.0f, 0.0f, 0.0f, 0.0f}, d14 = {0.0f, 0.0f, 0.0f, 0.0f};      // (independent chains, as the logit's)
#pragma unroll
      for (int jb = 0; jb < 8; ++jb) {
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(Wc0 + 16 * jb + 4 * q);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(Wc1 + 16 * jb + 4 * q);
        d04 = d04 + tC[jb] * w0;
        d14 = d14 + tC[jb] * w1;
      }
      float d0 = fb_sum_q((d04[0] + d04[1]) + (d04[2] + d04[3]));
      float d1 = fb_sum_q((d14[0] + d14[1]) + (d14[2] + d14[3]));
      if (F16) { d0 *= frow; d1 *= frow; }
      if (f.part_rs) {
        if (act) {
          rs1 += sc * (d1 * u0c - d0 * u1c);
          rs2 += d0 * u0c + d1 * u1c;
          rs3 += d0;
          rs4 += d1;
        }
      } else if (q == 0 && act) {
        f.rowtp[row] = sc * (d1 * u0c - d0 * u1c);
        f.rowtp[f.M + row] = d0 * u0c + d1 * u1c;
        f.rowtp[2 * f.M + row] = d0;
        f.rowtp[3 * f.M + row] = d1;
      }
    }
    FB_STAMP(22);
    if (OV) __syncthreads();   // the staging area is free again (the next tile's W2 reload lands here)
    FB_STAMP(13);
  }
  if constexpr (TAIL) {
    if (has_tail) {
      // ================= column-parallel tail: ONE unit, four waves (helpers above the kernel) =================
      using TL = FbTailLds<PREC>;
      ++tile_no;
      const float* Wc0 = vec;
      const float* Wc1 = vec + FD_H;
      const float* bcs = vec + 2 * FD_H;
      const float* wos = vec + 3 * FD_H;
      const float* b1s = vec + 4 * FD_H;
      const float* b2s = vec + 5 * FD_H;
      const int bu = pos_cur.b;                          // (every wave's prefetch slots hold the tail unit's inputs)
      const int64_t row = (int64_t)u_end * FD_UNIT + r;
      float x0, x1, u0c, u1c, sc;
      sd_wait_vm0();
      if (f.cd == 2) {
        const float gx = cgr[2 * r], gy = cgr[2 * r + 1];
        u0c = gx * ctp[0] - gy * ctp[1];
        u1c = gx * ctp[1] + gy * ctp[0];
        sc = ctp[2];
        x0 = u0c * sc + ctp[3];
        x1 = u1c * sc + ctp[4];
      } else {
        u0c = cgr[r]; u1c = 0.0f; sc = 1.0f;
        x0 = u0c + ctp[3]; x1 = 0.0f;
      }
      FB_TSTAMP(0);
      const float xv = xv_next, swv = sw_next;
      f32x4 h0o[2], h1o[2], h2o[2], t2[2];
      bf16x4 oh[2], ol[2], pH0[8], pH1[8], pAh[8], pAl[8];
      // ---- coordinate layer, own blocks ----
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const int j = 16 * (2 * wave + o) + 4 * q;
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(Wc0 + j);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(Wc1 + j);
        const f32x4 bc = *reinterpret_cast<const f32x4*>(bcs + j);
        const f32x4 hz = *reinterpret_cast<const f32x4*>(chz + j);
#pragma unroll
        for (int i = 0; i < 4; ++i) h0o[o][i] = w0[i] * x0 + w1[i] * x1 + bc[i] + hz[i];
      }
      fb_tanh2(h0o, SD_C);
      fb_presplit2<false>(h0o, oh, ol);
      fb_xchg_put(smb, TL::E, oh, wave, lane);
      if (tile_no > 0) {                                  // W2's lo image was the previous tile's staging area
        sd_wait_vm0();
        sd_reload<LL::RL_BYTES, FB_WAVES>(gimg + LL::RL2_SRC, lds0 + LL::RL2_LDS, wave, lane);
      }
      FB_TSTAMP(1);
      __syncthreads();                                                   // exchange 0: h0
      FB_TSTAMP(2);
      fb_xchg_get(smb, TL::E, pH0, lane);
      fb_tail_fwd<PREC>(W1h, W1l, b1s, pH0, h1o, wave, r, q, qsw);
      fb_tanh2(h1o, c1);
      fb_presplit2<false>(h1o, oh, ol);
      fb_xchg_put(smb, TL::E + 4096, oh, wave, lane);
      FB_TSTAMP(3);
      sd_wait_vm0();
      FB_TSTAMP(4);
      __syncthreads();                                                   // exchange 1: h1; W2 landed
      FB_TSTAMP(5);
      fb_xchg_get(smb, TL::E + 4096, pH1, lane);
      fb_tail_fwd<PREC>(W2h, W2l, b2s, pH1, h2o, wave, r, q, qsw);
      fb_tanh2(h2o, c2);
      float* rp = reinterpret_cast<float*>(smb + TL::RP);
      {
        f32x4 p4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int o = 0; o < 2; ++o) p4 = p4 + h2o[o] * *reinterpret_cast<const f32x4*>(wos + 16 * (2 * wave + o) + 4 * q);
        const float part = fb_sum_q((p4[0] + p4[1]) + (p4[2] + p4[3]));
        if (q == 0) rp[16 * wave + r] = part;
      }
      FB_TSTAMP(6);
      __syncthreads();                                                   // exchange 2: the logit's per-wave partial sums
      FB_TSTAMP(7);
      const float a = ((rp[r] + rp[16 + r]) + (rp[32 + r] + rp[48 + r])) + bo;
      float ll, locv, dlda;
      sd_pixel_lik<LIK>(a, xv, f.sig, f.sigmoid_out, ll, dlda, locv);
      dlda *= swv;
      if (wave == 0) {
        // (the tail's row sums ride in wave 0's slot: its sample check first — the tile loop's, at the top of the tile)
        if (bu != cur_b) {
          if (cur_b >= 0) flush_hz(cur_b);
          cur_b = bu;
        }
        if (f.part_rs) rs0 += ll;
        if (q == 0) {
          if (f.llrow && !f.part_rs) f.llrow[row] = ll;
          if (f.loc) f.loc[row] = locv;
          dbo += dlda;
        }
      }
      // d(wo)[j] += sum_rows dlda h2[row][j], own blocks (transpose buffer: this wave's quarter of the not yet staged dpre arrays)
      {
        float* wov = reinterpret_cast<float*>(smb + TL::WOV);
        f32x4 pv_[2];
#pragma unroll
        for (int o = 0; o < 2; ++o) pv_[o] = dlda * h2o[o];
        float cs[3];
        fb_tail_colsum<1>(pv_, reinterpret_cast<float*>(smb + TL::SD) + wave * (16 * 36), nullptr, nullptr, nullptr, lane, r, q, cs);
        if (lane < 32) wov[32 * wave + lane] = cs[0];
      }
      // dL/dlogit = m 2^e: the mantissa (times kappa s_o) goes down the dgrad chain, the exponent into the staged rows
      const int ex = __builtin_amdgcn_frexp_expf(dlda);
      const float dn = __builtin_amdgcn_frexp_mantf(dlda) * kso;
      const _Float16 ph = (_Float16)__builtin_amdgcn_ldexpf(1.0f, ex + f.dl_exp);
      const half4_ ph4 = half4_{ph, ph, ph, ph};
      const float frow = __builtin_amdgcn_ldexpf(u0, ex);
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wos + 16 * (2 * wave + o) + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) t2[o][i] = dn * wv[i] * (1.0f - h2o[o][i] * h2o[o][i]);     // dpre2
      }
      fb_presplit2<true>(t2, oh, ol);
      fb_xchg_put(smb, TL::E, oh, wave, lane);
      fb_xchg_put(smb, TL::E + 4096, ol, wave, lane);
      FB_TSTAMP(8);
      __syncthreads();                                                   // exchange 3: dpre2 (hi, lo)
      FB_TSTAMP(9);
      fb_xchg_get(smb, TL::E, pAh, lane);
      fb_xchg_get(smb, TL::E + 4096, pAl, lane);
      // ---- weight gradients: the unit's 16 rows, staged by wave 0 in compact arrays, contracted with the 16-row instruction ----
      __bf16* tsd = reinterpret_cast<__bf16*>(smb + TL::SD);
      __bf16* tsa = reinterpret_cast<__bf16*>(smb + TL::SA);
      auto stage = [&](const bf16x4 (&dh)[8], const bf16x4 (&dl)[8], const bf16x4 (&hh)[8]) {
        if (wave == 0) {
          fb_stage_store<true, false>(tsd, tsd + 16 * LDS2, dh, dl, r, q);
          fb_stage_store<false, true>(tsa, tsa, hh, dl, r, q, ph4);
        }
      };
      stage(pAh, pAl, pH1);
      FB_TSTAMP(10);
      __syncthreads();
      FB_TSTAMP(11);
      fb_wgrad_consume16<PREC>(tsd, tsa, accW2, accB2, wave, r, q);
      FB_TSTAMP(12);
      // ---- dgrad of layer 2, own blocks ----
      fb_tail_dgrad<PREC, PP::DGR2_LO>(W2h, W2l, pAh, pAl, t2, wave, r, q, qsw);
#pragma unroll
      for (int o = 0; o < 2; ++o) t2[o] = t2[o] * (1.0f - h1o[o] * h1o[o]);          // dpre1 (carried scales as in the tile loop)
      fb_presplit2<true>(t2, oh, ol);
      fb_xchg_put(smb, TL::E, oh, wave, lane);                          // (every wave read exchange 3 before the staging barrier)
      fb_xchg_put(smb, TL::E + 4096, ol, wave, lane);
      FB_TSTAMP(13);
      __syncthreads();                                                   // exchange 4: dpre1; the staged rows are consumed
      FB_TSTAMP(14);
      fb_xchg_get(smb, TL::E, pAh, lane);
      fb_xchg_get(smb, TL::E + 4096, pAl, lane);
      // ---- dgrad of layer 1, own blocks ----
      fb_tail_dgrad<PREC, PP::DGR1_LO>(W1h, W1l, pAh, pAl, t2, wave, r, q, qsw);
#pragma unroll
      for (int o = 0; o < 2; ++o) t2[o] = t2[o] * (1.0f - h0o[o] * h0o[o]);          // dpre0, normalised (frow restores the row)
      FB_TSTAMP(15);
      stage(pAh, pAl, pH0);
      {
        // coordinate layer: the column sums dL/d(hz), dWc0, dWc1 of the own blocks and the row-local partial sums
        // (transpose buffer: W2's lo image — the tail is the last tile and every wave is past the dgrad of layer 2; the rows'
        //  weights 2^e, 2^e x0, 2^e x1 in the wave's own slots of the tile loop's `info` rows)
        float* vv = reinterpret_cast<float*>(smb + TL::V);
        if (q == 0) {
          info[16 * wave + r] = frow * x0; info[TILE_ROWS + 16 * wave + r] = frow * x1; info[2 * TILE_ROWS + 16 * wave + r] = frow;
        }
        float cs[3];
        fb_tail_colsum<3>(t2, reinterpret_cast<float*>(smb + LL::W2L) + wave * (16 * 36), info + 2 * TILE_ROWS + 16 * wave,
                          info + 16 * wave, info + TILE_ROWS + 16 * wave, lane, r, q, cs);
        if (lane < 32) {
          vv[32 * wave + lane] = cs[0];
          vv[FD_H + 32 * wave + lane] = cs[1];
          vv[2 * FD_H + 32 * wave + lane] = cs[2];
        }
        f32x4 d04 = {0.0f, 0.0f, 0.0f, 0.0f}, d14 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int o = 0; o < 2; ++o) {
          const int j = 16 * (2 * wave + o) + 4 * q;
          d04 = d04 + t2[o] * *reinterpret_cast<const f32x4*>(Wc0 + j);
          d14 = d14 + t2[o] * *reinterpret_cast<const f32x4*>(Wc1 + j);
        }
        const float d0 = fb_sum_q((d04[0] + d04[1]) + (d04[2] + d04[3]));
        const float d1 = fb_sum_q((d14[0] + d14[1]) + (d14[2] + d14[3]));
        if (q == 0) { rp[16 * wave + r] = d0; rp[64 + 16 * wave + r] = d1; }      // (the logit's partials were read before barrier 3)
      }
      FB_TSTAMP(16);
      __syncthreads();
      FB_TSTAMP(17);
      fb_wgrad_consume16<PREC>(tsd, tsa, accW1, accB1, wave, r, q);
      FB_TSTAMP(18);
      if (wave == 0) {
        const float* vv = reinterpret_cast<const float*>(smb + TL::V);
        const float* wov = reinterpret_cast<const float*>(smb + TL::WOV);
        const float2 a0 = *reinterpret_cast<const float2*>(vv + 2 * lane);
        const float2 a1 = *reinterpret_cast<const float2*>(vv + FD_H + 2 * lane);
        const float2 a2 = *reinterpret_cast<const float2*>(vv + 2 * FD_H + 2 * lane);
        const float2 aw = *reinterpret_cast<const float2*>(wov + 2 * lane);
        cs_hz.x += a0.x; cs_hz.y += a0.y;
        cs_c0.x += a1.x; cs_c0.y += a1.y;
        cs_c1.x += a2.x; cs_c1.y += a2.y;
        cs_wo.x += aw.x; cs_wo.y += aw.y;
        {
          const float* dp = rp;
          const float d0 = ((dp[r] + dp[16 + r]) + (dp[32 + r] + dp[48 + r])) * frow;
          const float d1 = ((dp[64 + r] + dp[80 + r]) + (dp[96 + r] + dp[112 + r])) * frow;
          if (f.part_rs) {
            rs1 += sc * (d1 * u0c - d0 * u1c);
            rs2 += d0 * u0c + d1 * u1c;
            rs3 += d0;
            rs4 += d1;
          } else if (q == 0) {
            f.rowtp[row] = sc * (d1 * u0c - d0 * u1c);
            f.rowtp[f.M + row] = d0 * u0c + d1 * u1c;
            f.rowtp[2 * f.M + row] = d0;
            f.rowtp[3 * f.M + row] = d1;
          }
        }
      }
    }
  }
  FB_KSTAMP(2);                                                          // last tile done
  if (!GRADS) return;

  // (round 6) this workgroup's units are exactly ONE sample (batch == grid): it hands the latent backward the sample's dL/d(hz),
  // dL/dz and row sums itself — its four waves' partials summed next to the other column sums — instead of four slots each
  const bool own = f.dhz_out != nullptr && u_lo == (int64_t)g * upb && u_hi - u_lo == upb;
  if (cur_b >= 0 && !own) flush_hz(cur_b);
  if (PP::KEEP_WO) {
    // (every wave is past the last tile's barriers: the wgrad-2 staging rows are free)
    f32x4 t[8];
#pragma unroll
    for (int jb = 0; jb < 8; ++jb) t[jb] = accWo[PP::KEEP_WO ? jb : 0];
    fb_colsum<0>(t, reinterpret_cast<float*>(st2) + (16 * wave) * (LDS2 / 2), cs_wo, cs_none, cs_none, nullptr, nullptr,
                 lane, r, q);
  }
  // (round 6, third cut: PvEncFold::chain) a workgroup that owns its sample also runs the sample's latent backward and encoder
  // chain below (pv_sdec_fused_w8.hip has the story); the operands are requested here, ahead of the 138 KB of record stores
  // (`e` is read through an opaque pointer into the kernarg segment HERE: named directly, the compiler fetches its fields at kernel
  //  entry and carries them — spilled, 51 -> 92 SGPRs — through the tile loop: +3 us on the launch even with the chain switched off)
  const PvEncFoldArg ep_ = pv_kernarg_fold();
  const bool own_chain = own && ep_->chain && f.part_rs && f.dzc_out;
  float ch_whd[16], ch_a1 = 0.0f, ch_a0 = 0.0f, ch_z = 0.0f, ch_sig = 1.0f, ch_ep = 0.0f, ch_sp = 0.0f;
  f32x4 ch_w1[16];
  if (own_chain) {
    const int ho = ep_->head.out_dim;
    if (tid < FD_H) {
      const float* Wh = ep_->params + ep_->head.w_off + tid;
#pragma unroll
      for (int o = 0; o < 16; ++o) ch_whd[o] = Wh[(o < ho ? o : ho - 1) * FD_H];          // (clamped: multiplied by a zero below)
      ch_a1 = ep_->eact1[(int64_t)g * FD_H + tid];
      ch_a0 = ep_->eact0[(int64_t)g * FD_H + tid];
    }
    // (second hidden layer: thread (c = tid & 31, jg = tid >> 5) holds W1[16 jg .. 16 jg + 15][4c .. 4c + 3])
    const float* W1c = ep_->params + ep_->enc1.w_off + 4 * (tid & 31) + (16 * (tid >> 5)) * FD_H;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) ch_w1[jj] = *reinterpret_cast<const f32x4*>(W1c + jj * FD_H);
    if (lane < ep_->z_dim && wave < 2) {
      ch_z = ep_->z[(int64_t)g * ep_->z_dim + lane];
      ch_sig = ep_->z_scale[(int64_t)g * ep_->z_dim + lane];
      ch_ep = ep_->eps[(int64_t)g * ep_->z_dim + lane];
      ch_sp = ep_->head_out[(int64_t)g * ep_->ldh + ep_->z_dim + lane];
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int j0 = 16 * (2 * wave + s);
    if (f.ablate & 1024) {                   // (experiments build: the row-major form of rounds 1-5, 128 scattered 4-byte stores per wave)
#pragma unroll
      for (int kb = 0; kb < 8; ++kb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // C/D layout: lane (col k' = r, q), reg i -> dW[j0 + 4*q + i][16*kb + r]
          rec[(j0 + 4 * q + i) * FD_H + 16 * kb + r] = accW1[s][kb][i] * uw1;
          rec[FD_H * FD_H + (j0 + 4 * q + i) * FD_H + 16 * kb + r] = accW2[s][kb][i] * uw2;
        }
    } else {
      // LANE-NATIVE (pv_sdec_fused.h PV_REC_LANE_F32): every accumulator block as it sits in registers, one 1 KB-contiguous
      // 16-byte-per-lane store each — 32 store instructions per wave instead of 128
      f32x4* rec4 = reinterpret_cast<f32x4*>(rec);
#pragma unroll
      for (int kb = 0; kb < 8; ++kb) {
        rec4[(((0 * FB_WAVES + wave) * 2 + s) * 8 + kb) * 64 + lane] = accW1[s][kb] * uw1;
        rec4[(((1 * FB_WAVES + wave) * 2 + s) * 8 + kb) * 64 + lane] = accW2[s][kb] * uw2;
      }
    }
    // bias gradients: every column of accB holds the same sums; lane (col 0, q), reg i -> row j0 + 4q + i
    if (r == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        rec[2 * FD_H * FD_H + j0 + 4 * q + i] = accB1[s][i] * uw1;
        rec[2 * FD_H * FD_H + FD_H + j0 + 4 * q + i] = accB2[s][i] * uw2;
      }
    }
  }
  const float tb = pv_wave_sum(dbo);
  if (lane == 0) red[wave] = tb;
  __syncthreads();          // every wave is done with every staging area
  {
    // per-wave column sums -> the record (waves in ascending order): dWc0 | dWc1 | dwo, through the (free) first staging area
    float* d = reinterpret_cast<float*>(st2);
    *reinterpret_cast<float2*>(d + (3 * wave + 0) * FD_H + 2 * lane) = cs_wo;
    *reinterpret_cast<float2*>(d + (3 * wave + 1) * FD_H + 2 * lane) = cs_c0;
    *reinterpret_cast<float2*>(d + (3 * wave + 2) * FD_H + 2 * lane) = cs_c1;
    float* dh = d + 3 * FB_WAVES * FD_H;                  // own: [wave][128] dL/d(hz) partials, then [wave][8] row sums, then [2][16] dz partials
    float wzv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (own) {
      *reinterpret_cast<float2*>(dh + wave * FD_H + 2 * lane) = cs_hz;
      if (f.part_rs) {
        const float v0 = fb_row16_sum(rs0), v1 = fb_row16_sum(rs1), v2 = fb_row16_sum(rs2), v3 = fb_row16_sum(rs3), v4 = fb_row16_sum(rs4);
        if (lane == 0) {
          float* rr = dh + FB_WAVES * FD_H + 8 * wave;
          rr[0] = v0; rr[1] = v1; rr[2] = v2; rr[3] = v3; rr[4] = v4;
        }
      }
      if (f.dzc_out && tid < FD_H) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wzv[i] = i < f.lat_in ? f.Wz[(int64_t)tid * f.lat_in + i] : 0.0f;
      }
    }
    __syncthreads();
    float dhz_j = 0.0f;
    if (tid < FD_H) {
      float vo = 0.0f, v0 = 0.0f, v1 = 0.0f;
#pragma unroll
      for (int w = 0; w < FB_WAVES; ++w) {
        vo += d[(3 * w + 0) * FD_H + tid];
        v0 += d[(3 * w + 1) * FD_H + tid];
        v1 += d[(3 * w + 2) * FD_H + tid];
        if (own) dhz_j += dh[w * FD_H + tid];
      }
      rec[2 * FD_H * FD_H + 2 * FD_H + tid] = v0;
      rec[2 * FD_H * FD_H + 3 * FD_H + tid] = v1;
      rec[2 * FD_H * FD_H + 4 * FD_H + tid] = vo;
      if (own) f.dhz_out[(int64_t)g * FD_H + tid] = dhz_j;
    }
    if (own) {
      if (f.part_rs && tid < 5) {
        const float* rr = dh + FB_WAVES * FD_H + tid;
        f.part_rs[((int64_t)g * f.kmax) * PV_RS_W + tid] = (rr[0] + rr[8]) + (rr[16] + rr[24]);      // (slot 0 of the sample; the others stay zero)
      }
      if (f.dzc_out) {
        // dL/dz[i] = sum_j dL/d(hz[j]) Wz[j][i]: threads 0 .. 127 hold dL/d(hz[j]) (waves 0, 1)
        float* dzp = dh + FB_WAVES * FD_H + 8 * FB_WAVES;
        if (wave < 2) {
          for (int i = 0; i < f.lat_in; ++i) {
            const float pz = pv_wave_sum(dhz_j * (i < 4 ? wzv[i] : f.Wz[(int64_t)tid * f.lat_in + i]));
            if (lane == 0) dzp[16 * wave + i] = pz;
          }
        }
        __syncthreads();
        if (tid < f.lat_in) f.dzc_out[(int64_t)g * f.lat_in + tid] = dzp[tid] + dzp[16 + tid];
      }
      if (own_chain) {
        // ---- the sample's latent backward + encoder chain (pv_sdec_fused_w8.hip's epilogue, for this kernel's four waves):
        //   dhead from the row sums and dL/dz;  edp1 = (dhead Whead) * act'(eact1);  edp0 = (edp1 W1) * act'(eact0)
        // waves 0 and 1 run the head backward each for itself (wave-private LDS words, no barrier) and take 64 entries of edp1;
        // every thread contracts its 16 x 4 block of W1; threads 0 .. 127 add the 8 partial sums of their column.
        const float* rr = dh + FB_WAVES * FD_H;
        const float* dzp = dh + FB_WAVES * FD_H + 8 * FB_WAVES;
        float* cs = dh + FB_WAVES * FD_H + 8 * FB_WAVES + 64;        // [0..127] two waves' words, [128..255] edp1, [256 + 128 jg ..] partials
        if (wave < 2) {
          float* csw = cs + 64 * wave;
          if (lane < 5) {
            const float v = (rr[lane] + rr[8 + lane]) + (rr[16 + lane] + rr[24 + lane]);
            csw[lane] = v;
            if (tid == 0) ep_->llb[g] = v;
          }
          if (lane >= 8 && lane < 8 + f.lat_in) csw[lane] = dzp[lane - 8] + dzp[16 + lane - 8];
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          PvHeadBwd hb{};
          hb.coord_dim = ep_->coord_dim; hb.has_r = ep_->has_r; hb.has_t = ep_->has_t; hb.has_s = ep_->has_s;
          hb.tp0 = ep_->tp0; hb.tp1 = ep_->tp1; hb.sc_prior = ep_->sc_prior;
          if (lane < 16) {
            if (lane < ep_->z_dim) {
              float g_, ds_;
              const float dz = pv_head_dz(hb, lane, [&](int c) { return csw[1 + c]; }, [&](int k) { return csw[8 + k]; });
              pv_head_bwd_math(dz, ch_z, ch_sig, ch_ep, ch_sp, ep_->beta, 0, g_, ds_);
              if (wave == 0) {
                ep_->dhead[(int64_t)g * ep_->ldh + lane] = g_;
                ep_->dhead[(int64_t)g * ep_->ldh + ep_->z_dim + lane] = ds_;
              }
              csw[16 + lane] = g_;
              csw[16 + ep_->z_dim + lane] = ds_;
            } else if (lane + ep_->z_dim < 16) {
              csw[16 + ep_->z_dim + lane] = 0.0f;                      // (entries 2 z_dim .. 15)
            }
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          float v = 0.0f;
#pragma unroll
          for (int o = 0; o < 16; ++o) v += csw[16 + o] * ch_whd[o];
          v *= pv_act_grad2(ch_a1, 0.0f, ep_->enc1.act);
          ep_->edp1[(int64_t)g * FD_H + tid] = v;
          cs[128 + tid] = v;
        }
        __syncthreads();
        {
          const int c = tid & 31, jg = tid >> 5;
          f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const f32x4 ev = *reinterpret_cast<const f32x4*>(cs + 128 + 16 * jg + 4 * u);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc += ch_w1[4 * u + i] * ev[i];
          }
          *reinterpret_cast<f32x4*>(cs + 256 + 128 * jg + 4 * c) = acc;
        }
        __syncthreads();
        if (tid < FD_H) {
          float y = 0.0f;
#pragma unroll
          for (int jg = 0; jg < 8; ++jg) y += cs[256 + 128 * jg + tid];
          y *= pv_act_grad2(ch_a0, 0.0f, ep_->enc0.act);
          ep_->edp0[(int64_t)g * FD_H + tid] = y;
        }
      }
    }
  }
  if (tid == 0) {
    float v = 0.0f;
    for (int w = 0; w < FB_WAVES; ++w) v += red[w];
    rec[2 * FD_H * FD_H + 5 * FD_H] = v;
  }
#ifdef FB_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  FB_KSTAMP(3);                                                          // record written
