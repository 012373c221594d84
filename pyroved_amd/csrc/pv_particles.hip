// pv_particles.hip — the kernels of the multi-particle ELBO step (pv_particles.h): the guide's expansion into P decoder samples per
// image, the latent backward that reduces them, and the importance-weighted bound's weights.  Every sum runs in a fixed order (particles ascending, no float atomics): a step
// is bit-reproducible run to run.
#include "pv_particles.h"
#include <cmath>

#define PX_THREADS 128
#define PX_MAX_Z 256
#define PX_MAX_LAT 256

// latent coordinates in front of the content columns (base.py:97-119: _split_latent)
template <class D> __device__ __forceinline__ int px_coord_cols(const D& d) {
  if (d.coord_dim == 1) return d.has_t ? 1 : 0;
  if (d.coord_dim == 2) return (d.has_r ? 1 : 0) + (d.has_t ? 2 : 0) + (d.has_s ? 1 : 0);
  return 0;
}

// ---- expansion: one workgroup per image ----
__global__ __launch_bounds__(PX_THREADS) void pv_particle_expand_kernel(PvParticleExpand e) {
  __shared__ float sm[16];
  __shared__ float sh_z[PX_MAX_Z];
  __shared__ float sh_in[PX_MAX_LAT];
  const int b = blockIdx.x, t = threadIdx.x, zd = e.z_dim;
  const int idx = px_coord_cols(e), L = zd - idx, lat_in = L + e.c_dim;
  const float inv_p = 1.0f / (float)e.P;
  float lp = 0.0f, lq = 0.0f;
  for (int p = 0; p < e.P; ++p) {
    const int64_t s = (int64_t)p * e.B + b;
    for (int i = t; i < zd; i += PX_THREADS) {
      const float mu = e.head[(int64_t)b * e.ldh + i];
      const float sig = pv_softplus(e.head[(int64_t)b * e.ldh + zd + i]);
      const float z = mu + sig * e.eps[s * zd + i];
      e.z[s * zd + i] = z;
      sh_z[i] = z;
      if (p == 0) {
        e.z_scale[(int64_t)b * zd + i] = sig;
        if (e.z_loc_out) e.z_loc_out[(int64_t)b * zd + i] = mu;
        if (e.z_scale_out) e.z_scale_out[(int64_t)b * zd + i] = sig;
      }
      if (e.kl_mode == PV_KL_SAMPLED) {
        const float d = z - mu;
        lq += -(d * d) / (2.0f * (sig * sig)) - logf(sig) - LOG_SQRT_2PI;      // torch.distributions.Normal.log_prob
        lp += -(z * z) / 2.0f - LOG_SQRT_2PI;
      } else if (p == 0) {                             // (the closed form does not depend on the draw)
        float aq, ap;
        pv_kl_analytic_terms(mu, sig, aq, ap);
        lq += aq;
        lp += ap;
      }
    }
    __syncthreads();
    if (t == 0) {
      e.sw[s] = inv_p;
      if (e.tp) {
        float c = 1.0f, sn = 0.0f, sc = 1.0f, tx = 0.0f, ty = 0.0f;
        int k = 0;
        if (e.coord_dim == 1) {
          if (e.has_t) tx = sh_z[0] * e.tp0;
        } else if (e.coord_dim == 2) {
          if (e.has_r) { const float phi = sh_z[k++]; c = cosf(phi); sn = sinf(phi); }
          if (e.has_t) { tx = sh_z[k] * e.tp0; ty = sh_z[k + 1] * e.tp1; k += 2; }
          if (e.has_s) sc = 1.0f + e.sc_prior * sh_z[k++];
        }
        float* o = e.tp + s * 8;
        o[0] = c; o[1] = sn; o[2] = sc; o[3] = tx; o[4] = ty;
      }
    }
    for (int i = t; i < lat_in; i += PX_THREADS) {     // cat([z content, y]) (ivae.py:194-195)
      const float v = i < L ? sh_z[idx + i] : e.y[(int64_t)b * e.c_dim + (i - L)];
      sh_in[i] = v;
      if (e.zy) e.zy[s * lat_in + i] = v;
    }
    __syncthreads();
    if (e.hz) {
      for (int j = t; j < e.H0; j += PX_THREADS) {
        const float* w = e.Wz + (int64_t)j * lat_in;
        float v = 0.0f;
        for (int k = 0; k < lat_in; ++k) v += sh_in[k] * w[k];
        e.hz[s * e.H0 + j] = e.hz_scale != 0.0f ? e.hz_scale * v : v;
      }
    }
    __syncthreads();                                   // (sh_z / sh_in are rewritten by the next particle)
  }
  lp = pv_block_sum(lp, sm);
  lq = pv_block_sum(lq, sm);
  if (t == 0) {
    const float w = e.kl_mode == PV_KL_SAMPLED ? e.beta * inv_p : e.beta;
    e.kl_part[2 * b] = w * lp;
    e.kl_part[2 * b + 1] = w * lq;
  }
}

int pv_particle_expand(const PvParticleExpand& e, hipStream_t s) {
  if (e.B < 1 || e.P < 1 || e.z_dim < 1 || e.z_dim > PX_MAX_Z || e.z_dim + e.c_dim > PX_MAX_LAT) return PV_EINVAL;
  if (!e.head || !e.eps || !e.z || !e.z_scale || !e.sw || !e.kl_part || (e.c_dim > 0 && !e.y) || (e.hz && !e.Wz)) return PV_EINVAL;
  hipLaunchKernelGGL(pv_particle_expand_kernel, dim3(e.B), dim3(PX_THREADS), 0, s, e);
  PV_LAUNCH_CHECK();
  return 0;
}

// ---- particle-reducing latent backward: one workgroup (256 threads) per image ----
__device__ __forceinline__ void pv_particle_bwd_block(const PvParticleBwd& p, int b) {
  __shared__ float sm[16];
  __shared__ float sh_a[5];
  __shared__ float sh_dhz[512];
  __shared__ float sh_dzc[PX_MAX_LAT];
  __shared__ float sh_dh[2 * PX_MAX_Z];
  __shared__ float sh_e[2][256];
  const int t = threadIdx.x, B = p.hb.B, zd = p.hb.z_dim;
  const int ldh = p.hb.ldh > 0 ? p.hb.ldh : 2 * zd;
  const int n_content = zd - px_coord_cols(p.hb);
  float acc_g = 0.0f, acc_ds = 0.0f, ll_acc = 0.0f;
  for (int q = 0; q < p.P; ++q) {
    const int64_t s = (int64_t)q * B + b;              // decoder sample (q, b)
    if (p.llkb) {
      if (t == 0) sh_a[0] = p.llkb[s];
      if (!p.fwd_only) {
        if (t >= 1 && t < 5) sh_a[t] = p.dtp ? p.dtp[s * 4 + (t - 1)] : 0.0f;
        for (int k = t; k < n_content; k += 256) sh_dzc[k] = p.dzc[s * p.ldzc + k];
      }
    } else {
      if (p.part_rs) {
        // the decoder launch summed its rows per (sample, slot): the sample's kmax slots in ascending order
        if (t < 5) {
          const float* pr = p.part_rs + (s * p.kmax) * PV_RS_W + t;
          float v = 0.0f;
          for (int kk = 0; kk < p.kmax; ++kk) v += pr[(int64_t)kk * PV_RS_W];
          sh_a[t] = v;
        }
      } else {
        const int64_t r0 = s * p.N;
        float a[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int n = t; n < p.N; n += 256) {
          a[0] += p.llrow[r0 + n];
          if (!p.fwd_only)
            for (int c = 0; c < 4; ++c) a[1 + c] += p.rowtp[(int64_t)c * p.M + r0 + n];
        }
        for (int c = 0; c < 5; ++c) {
          const float v = pv_block_sum(a[c], sm);
          if (t == 0) sh_a[c] = v;
        }
      }
      if (!p.fwd_only) {
        for (int j = t; j < p.H; j += 256) {           // dL/d(hz_s): the sample's slots in ascending order
          const float* ph = p.part_hz + (s * p.kmax) * p.H + j;
          float v = 0.0f;
          for (int kk = 0; kk < p.kmax; ++kk) v += ph[(int64_t)kk * p.H];
          p.dhz[s * p.H + j] = v;
          sh_dhz[j] = v;
        }
        __syncthreads();
        if (t < n_content) {                           // dL/d(z content) = dhz Wz, ascending j
          float v = 0.0f;
          for (int j = 0; j < p.H; ++j) v += sh_dhz[j] * p.Wz[(int64_t)j * p.lat_in + t];
          sh_dzc[t] = v;
        }
      }
    }
    __syncthreads();
    const float w = p.sw[s];
    if (t == 0) ll_acc += w * (p.ll_s ? p.ll_s[s] : sh_a[0]);
    if (!p.fwd_only && t < zd) {
      const float dz = pv_head_dz(p.hb, t, [&](int c) { return sh_a[1 + c]; }, [&](int k) { return sh_dzc[k]; });
      const int64_t e = s * zd + t;
      float g, ds;
      pv_head_bwd_math_kl(p.hb.kl_mode, dz, p.hb.z[e], p.hb.head[(int64_t)b * ldh + t], p.hb.z_scale[(int64_t)b * zd + t], p.hb.eps[e],
                          p.hb.head[(int64_t)b * ldh + zd + t], p.hb.beta * w, p.hb.scale_direct, g, ds);
      acc_g += g;
      acc_ds += ds;
    }
    __syncthreads();                                   // (sh_a / sh_dhz / sh_dzc are rewritten by the next particle)
  }
  if (t == 0) p.llb[b] = p.llb_add ? ll_acc + p.llb_add[b] : ll_acc;
  if (p.fwd_only) return;
  if (t < zd) {
    p.hb.dhead[(int64_t)b * ldh + t] = acc_g;
    p.hb.dhead[(int64_t)b * ldh + zd + t] = acc_ds;
    sh_dh[t] = acc_g;
    sh_dh[zd + t] = acc_ds;
  }
  if (p.enc_n <= 0) return;
  // ---- the image's encoder dgrad chain (fixed summation order: ascending j) ----
  __syncthreads();
  const int ne = p.enc_n;
  int cur = 0;
  {
    const pv_layer hd = p.enc_head, l = p.enc_l[ne - 1];
    const float* Wh = p.enc_params + hd.w_off;
    for (int k = t; k < l.out_dim; k += 256) {
      float v = 0.0f;
      for (int o = 0; o < hd.out_dim; ++o) v += sh_dh[o] * Wh[(int64_t)o * hd.in_dim + k];
      v *= pv_act_grad2(p.enc_act[ne - 1][(int64_t)b * l.out_dim + k], 0.0f, l.act);
      p.enc_dp[ne - 1][(int64_t)b * l.out_dim + k] = v;
      sh_e[cur][k] = v;
    }
    __syncthreads();
  }
  for (int li = ne - 1; li > 0; --li) {
    const pv_layer l = p.enc_l[li], lp = p.enc_l[li - 1];
    const float* W = p.enc_params + l.w_off;
    for (int k = t; k < l.in_dim; k += 256) {
      float v = 0.0f;
      for (int j = 0; j < l.out_dim; ++j) v += sh_e[cur][j] * W[(int64_t)j * l.in_dim + k];
      v *= pv_act_grad2(p.enc_act[li - 1][(int64_t)b * lp.out_dim + k], 0.0f, lp.act);
      p.enc_dp[li - 1][(int64_t)b * lp.out_dim + k] = v;
      sh_e[cur ^ 1][k] = v;
    }
    __syncthreads();
    cur ^= 1;
  }
}

__global__ __launch_bounds__(256) void pv_particle_bwd_kernel(PvParticleBwd p) { pv_particle_bwd_block(p, blockIdx.x); }

// workgroups [0, nred) sum the fused decoder's per-workgroup gradient records, the rest run the particle backward
__global__ __launch_bounds__(256) void pv_particle_bwd_reduce_kernel(PvParticleBwd p, const float* __restrict__ part, int G_,
                                                                     float* __restrict__ Gr, PvFusedOffsets o, int cd, int fmt) {
  __shared__ PvRedLds smr;
  const int nred = pv_fused_reduce_blocks(fmt);
  if ((int)blockIdx.x < nred) pv_sdec_fused_reduce_block(part, G_, Gr, o, cd, 0, blockIdx.x, smr, fmt);
  else pv_particle_bwd_block(p, blockIdx.x - nred);
}

static int particle_bwd_check(const PvParticleBwd& p) {
  if (p.P < 1 || p.hb.B < 1 || p.hb.z_dim < 1 || p.hb.z_dim > PX_MAX_Z || !p.sw || !p.llb) return PV_EINVAL;
  if (p.llkb) {
    if (!p.fwd_only && (!p.dzc || (p.hb.coord_dim > 0 && !p.dtp))) return PV_EINVAL;
  } else {
    if (p.H > 512 || p.lat_in > PX_MAX_LAT || p.kmax < 1) return PV_EINVAL;
    if (!p.part_rs && !p.llrow) return PV_EINVAL;
    if (!p.fwd_only && (!p.part_hz || !p.dhz || !p.Wz || (!p.part_rs && !p.rowtp))) return PV_EINVAL;
  }
  if (p.enc_n > 0) {                                   // the chain's LDS rows
    if (p.enc_head.out_dim != 2 * p.hb.z_dim) return PV_EINVAL;
    for (int i = 0; i < p.enc_n; ++i)
      if (p.enc_l[i].out_dim > 256) return PV_EINVAL;
  }
  return 0;
}

int pv_particle_bwd(const PvParticleBwd& p, hipStream_t s) {
  PV_TRY(particle_bwd_check(p));
  hipLaunchKernelGGL(pv_particle_bwd_kernel, dim3(p.hb.B), dim3(256), 0, s, p);
  PV_LAUNCH_CHECK();
  return 0;
}

int pv_particle_bwd_reduce(const PvParticleBwd& p, const float* part, int grid, float* G, const PvFusedOffsets& o, int cd,
                           hipStream_t s, int rec_fmt) {
  PV_TRY(particle_bwd_check(p));
  hipLaunchKernelGGL(pv_particle_bwd_reduce_kernel, dim3(pv_fused_reduce_blocks(rec_fmt) + p.hb.B), dim3(256), 0, s, p, part, grid, G, o,
                     cd, rec_fmt);
  PV_LAUNCH_CHECK();
  return 0;
}

// ---- importance-weighted (Renyi) bound: the P samples' weights, one wave per image ----
__global__ __launch_bounds__(64) void pv_renyi_weights_kernel(PvRenyiWeights r) {
  __shared__ float sh_a[PV_RENYI_MAX_P], sh_lp[PV_RENYI_MAX_P], sh_lq[PV_RENYI_MAX_P];
  const int b = blockIdx.x, t = threadIdx.x, zd = r.z_dim;
  const float oma = 1.0f - r.alpha;
  for (int p = 0; p < r.P; ++p) {
    const int64_t s = (int64_t)p * r.B + b;
    float lp = 0.0f, lq = 0.0f;
    for (int i = t; i < zd; i += 64) {
      const float z = r.z[s * zd + i], e = r.eps[s * zd + i], sig = r.z_scale[(int64_t)b * zd + i];
      lq += pv_lw_logq(e, sig);
      lp += pv_lw_logp(z);
    }
    lp = r.beta * pv_wave_sum(lp);
    lq = r.beta * pv_wave_sum(lq);
    if (t == 0) {
      sh_lp[p] = lp;
      sh_lq[p] = lq;
      sh_a[p] = oma * pv_log_weight(r.llkb[s], lp, lq);
    }
  }
  if (t != 0) return;                                  // (thread 0 reads back what it wrote: no barrier)
  float m = sh_a[0];
  for (int p = 1; p < r.P; ++p) m = fmaxf(m, sh_a[p]);
  float sum = 0.0f;
  for (int p = 0; p < r.P; ++p) sum += expf(sh_a[p] - m);
  const float inv = 1.0f / sum, lsum = logf(sum);
  float klp = 0.0f, klq = 0.0f, ent = 0.0f;
  for (int p = 0; p < r.P; ++p) {
    const int64_t s = (int64_t)p * r.B + b;
    const float d = sh_a[p] - m, w = expf(d) * inv;
    r.sw[s] = w;
    if (r.weights_out) r.weights_out[s] = w;
    klp += w * sh_lp[p];
    klq += w * sh_lq[p];
    ent -= w * (d - lsum);                             // H(w_b) = - sum_p w log w, log w = d - log(sum)
  }
  r.kl_part[2 * b] = klp;
  r.kl_part[2 * b + 1] = klq;
  r.c[b] = (ent - logf((float)r.P)) / oma;
}

int pv_renyi_weights(const PvRenyiWeights& r, hipStream_t s) {
  if (r.B < 1 || r.P < 1 || r.P > PV_RENYI_MAX_P || r.z_dim < 1 || !std::isfinite(r.alpha) || r.alpha == 1.0f) return PV_EINVAL;
  if (!r.llkb || !r.z || !r.eps || !r.z_scale || !r.sw || !r.kl_part || !r.c) return PV_EINVAL;
  hipLaunchKernelGGL(pv_renyi_weights_kernel, dim3(r.B), dim3(64), 0, s, r);
  PV_LAUNCH_CHECK();
  return 0;
}

// ---- held-out log-evidence (pv_particles.h; include/pyroved_amd.h: pv_ivae_evidence_accumulate) ----
__global__ __launch_bounds__(64) void pv_evidence_lw_kernel(PvEvidenceLw e) {
  const int b = blockIdx.x, t = threadIdx.x, zd = e.z_dim;
  for (int p = 0; p < e.P; ++p) {
    const int64_t s = (int64_t)p * e.B + b;
    float lp = 0.0f, lq = 0.0f;
    for (int i = t; i < zd; i += 64) {
      const float z = e.z[s * zd + i], ep = e.eps[s * zd + i], sig = e.z_scale[(int64_t)b * zd + i];
      lq += pv_lw_logq(ep, sig);
      lp += pv_lw_logp(z);
    }
    lp = e.beta * pv_wave_sum(lp);
    lq = e.beta * pv_wave_sum(lq);
    if (t == 0) e.lw[s] = pv_log_weight(e.llkb[s], lp, lq);
  }
}
int pv_evidence_lw(const PvEvidenceLw& e, hipStream_t s) {
  if (e.B < 1 || e.P < 1 || e.P > PV_RENYI_MAX_P || e.z_dim < 1) return PV_EINVAL;
  if (!e.llkb || !e.z || !e.eps || !e.z_scale || !e.lw) return PV_EINVAL;
  hipLaunchKernelGGL(pv_evidence_lw_kernel, dim3(e.B), dim3(64), 0, s, e);
  PV_LAUNCH_CHECK();
  return 0;
}

__global__ __launch_bounds__(256) void pv_poisson_lognorm_particles_kernel(const float* __restrict__ x, int64_t N, float* __restrict__ llkb,
                                                                           int64_t B, int P) {
  __shared__ double sm[4];
  const float* xb = x + (int64_t)blockIdx.x * N;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) acc += (double)lgammaf(xb[i] + 1.0f);
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  const double c = (sm[0] + sm[1]) + (sm[2] + sm[3]);
  for (int p = threadIdx.x; p < P; p += 256) {
    float* d = llkb + (int64_t)p * B + blockIdx.x;
    *d = (float)((double)*d - c);
  }
}
int pv_poisson_lognorm_particles(const float* x, int64_t B, int64_t N, float* llkb, int P, hipStream_t s) {
  if (!x || !llkb || B <= 0 || N <= 0 || P < 1) return PV_EINVAL;
  hipLaunchKernelGGL(pv_poisson_lognorm_particles_kernel, dim3((unsigned)B), dim3(256), 0, s, x, N, llkb, B, P);
  PV_LAUNCH_CHECK();
  return 0;
}

// the running state per image, {m, s, q, unused}: one thread per image walks the chunk's P log-weights in ascending p — the chunk's
// maximum first, then the sums against max(m_old, chunk maximum).  first != 0: the state is written, never read
#define PV_LME_THREADS 256
__global__ __launch_bounds__(PV_LME_THREADS) void pv_logmeanexp_update_kernel(const float* __restrict__ lw, int P, int B,
                                                                              float* __restrict__ state, int first) {
  const int b = blockIdx.x * PV_LME_THREADS + threadIdx.x;
  if (b >= B) return;
  float m = lw[b];
  for (int p = 1; p < P; ++p) m = fmaxf(m, lw[(int64_t)p * B + b]);
  float sum = 0.0f, sq = 0.0f;
  float4* st = reinterpret_cast<float4*>(state) + b;
  if (!first) {
    const float4 o = *st;
    m = fmaxf(m, o.x);
    const float r = expf(o.x - m);                     // (1 when the maximum stays; an underflow leaves exactly 0)
    sum = o.y * r;
    sq = o.z * (r * r);
  }
  for (int p = 0; p < P; ++p) {
    const float e = expf(lw[(int64_t)p * B + b] - m);
    sum += e;
    sq += e * e;
  }
  *st = float4{m, sum, sq, 0.0f};
}
__global__ __launch_bounds__(PV_LME_THREADS) void pv_logmeanexp_finish_kernel(const float* __restrict__ state, int B, float log_k,
                                                                              float* __restrict__ log_mean, float* __restrict__ ess) {
  const int b = blockIdx.x * PV_LME_THREADS + threadIdx.x;
  if (b >= B) return;
  const float4 o = reinterpret_cast<const float4*>(state)[b];
  log_mean[b] = o.x + (logf(o.y) - log_k);
  if (ess) ess[b] = (o.y * o.y) / o.z;
}

extern "C" int pv_logmeanexp_update(const float* lw, int32_t P, int32_t B, float* state, int first, void* stream) {
  if (!lw || !state || P < 1 || B < 1 || ((uintptr_t)state & 15) != 0) return PV_EINVAL;
  hipLaunchKernelGGL(pv_logmeanexp_update_kernel, dim3((B + PV_LME_THREADS - 1) / PV_LME_THREADS), dim3(PV_LME_THREADS), 0,
                     (hipStream_t)stream, lw, P, B, state, first);
  PV_LAUNCH_CHECK();
  return 0;
}
extern "C" int pv_logmeanexp_finish(const float* state, int32_t B, int64_t K_total, float* log_mean, float* ess, void* stream) {
  if (!state || !log_mean || B < 1 || K_total < 1 || ((uintptr_t)state & 15) != 0) return PV_EINVAL;
  hipLaunchKernelGGL(pv_logmeanexp_finish_kernel, dim3((B + PV_LME_THREADS - 1) / PV_LME_THREADS), dim3(PV_LME_THREADS), 0,
                     (hipStream_t)stream, state, B, (float)log((double)K_total), log_mean, ess);
  PV_LAUNCH_CHECK();
  return 0;
}
