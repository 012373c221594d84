// pv_particles.h — the multi-particle ELBO (Trace_ELBO / TraceMeanField_ELBO with num_particles = P > 1; pv_particles.hip).
// One encoder pass over the B images, P decoder samples per image ordered [p][b] (sample s = p * B + b — the order jiVAE's
// enumerated decoder samples already have), each weighted sw[s] = 1 / P; their dL/dz is reduced over p, in ascending p, into the
// image's head gradient.
// The importance-weighted (Renyi) bound is the same step with another fill of sw: pv_renyi_weights, below.
#pragma once
#include "pv_common.h"
#include "pv_kernels.h"
#include "pv_sdec_fused.h"

// guide side, after the head: per decoder sample (p, b) the reparameterised z, the transform parameters, the decoder's latent
// input and (spatial decoder on the fused path) fc_latent; per image the KL partial sums
struct PvParticleExpand {
  const float* head; int ldh;       // (B, ldh): [mu | softplus input]
  const float* eps;                 // (P*B, z_dim), rows [p][b]
  const float* y;                   // (B, c_dim) or null
  float* z;                         // (P*B, z_dim)
  float* z_scale;                   // (B, z_dim)
  float* z_loc_out; float* z_scale_out;   // optional (B, z_dim) copies for the caller
  float* tp;                        // (P*B, 8): cos, sin, scale, tx, ty (null when coord_dim == 0)
  float* zy;                        // (P*B, lat_in) = [z content | y_b] when c_dim > 0, else null
  float* hz; const float* Wz; int H0;     // (P*B, H0) = fc_latent(decoder latent input), or null: not wanted here
  float hz_scale;                   // hz is stored multiplied by this (0: unscaled); see PvFused::hz_scale
  float* sw;                        // (P*B) <- 1 / P
  float* kl_part;                   // (B, 2): beta * {log p, log q} — sampled form: the mean over p; analytic form: once per image
  int B, P, z_dim, c_dim, coord_dim, has_r, has_t, has_s;
  float tp0, tp1, sc_prior, beta;
  int kl_mode;
};
int pv_particle_expand(const PvParticleExpand& e, hipStream_t s);

// the particle-reducing latent backward: one workgroup per image b, its P samples in ascending p
//   llb[b]   = sum_p sw[s] ll_s (+ llb_add[b])
//   dhead[b] = sum_p pv_head_bwd_math_kl(dz_s, ..., beta * sw[s])        (the decoder's dz_s arrives weighted by sw[s])
// fused form (llkb == null): gathers ll_s, d(phi, scale, tx, ty) and dL/d(hz_s) from the fused decoder launch's outputs as
// pv_latent_bwd does per sample (dhz[s] is written for fc_latent's weight gradient), dL/dz_s = dhz_s Wz;
// layered form: reads ll_s, dL/d(decoder latent input) and d(phi, scale, tx, ty) the layer-by-layer backward left.
// enc_n > 0: the image's encoder dgrad chain follows in the same workgroup (PvLatentBwd::enc_*).
struct PvParticleBwd {
  const float* llrow; const float* rowtp; const float* part_hz; const float* part_rs; const float* Wz; float* dhz;
  int64_t M; int N, kmax, H, lat_in;
  const float* llkb; const float* dzc; int64_t ldzc; const float* dtp;     // (P*B), (P*B, ldzc), (P*B, 4)
  const float* sw;                  // (P*B)
  float* llb;                       // (B)
  const float* llb_add;             // (B) or null: added to llb[b] (the Renyi bound's c_b, pv_renyi_weights)
  const float* ll_s;                // (P*B) or null, fused form: ll_s is read here, not gathered from the decoder launch's outputs (the
                                    //   Renyi step's loss is that of the forward launch its weights came from)
  int P, fwd_only;
  PvHeadBwd hb;                     // z, eps: (P*B, z_dim); z_scale, head, dhead: per image; dzc / dtp fields unused
  int enc_n;
  const float* enc_params;
  pv_layer enc_l[PV_MAX_LAYERS];
  pv_layer enc_head;
  const float* enc_act[PV_MAX_LAYERS];
  float* enc_dp[PV_MAX_LAYERS];
};
int pv_particle_bwd(const PvParticleBwd& p, hipStream_t s);
// ... in one launch with the sums of the fused decoder's gradient records (as pv_latent_bwd_reduce)
int pv_particle_bwd_reduce(const PvParticleBwd& p, const float* part, int grid, float* G, const PvFusedOffsets& o, int cd,
                           hipStream_t s, int rec_fmt);

// the importance-weighted (Renyi, alpha != 1; alpha = 0: IWAE) bound's per-sample weights: one workgroup per image b,
//   lw_pb = ll_pb + beta (log p(z_pb) - log q(z_pb | x_b)),   a_pb = (1 - alpha) lw_pb,   w_pb = softmax_p a_pb   (max subtracted)
//   sw[p B + b] = w_pb (and weights_out)
//   kl_part[b]  = {sum_p w_pb beta log p(z_pb), sum_p w_pb beta log q(z_pb | x_b)}   (replaces the mean the expansion wrote)
//   c[b]        = L_b - sum_p w_pb lw_pb = (H(w_b) - log P) / (1 - alpha),   L_b = (logsumexp_p a_pb - log P) / (1 - alpha)
// so that llb[b] = sum_p w_pb ll_pb + c[b] (PvParticleBwd::llb_add) and the two kl_part columns finish to the bound's four scalars.
// The sums over p run in ascending order in one thread (P is small: 2 .. 16 in practice, at most PV_RENYI_MAX_P): no atomics.
#define PV_RENYI_MAX_P 1024
struct PvRenyiWeights {
  const float* llkb;                // (P*B) log p(x_b | z_pb)
  const float* z; const float* eps; // (P*B, z_dim)
  const float* z_scale;             // (B, z_dim)
  float* sw;                        // (P*B)
  float* weights_out;               // (P*B) or null
  float* kl_part;                   // (B, 2)
  float* c;                         // (B)
  int B, P, z_dim;
  float beta, alpha;
};
int pv_renyi_weights(const PvRenyiWeights& r, hipStream_t s);

// one sample's log-weight lw_pb = ll_pb + beta (log p(z_pb) - log q(z_pb | x_b)), the arithmetic shared by pv_renyi_weights and the
// evidence estimate (pv_evidence_lw) so that both form the same bits: one latent coordinate's two terms (a lane walks
// i = t, t + 64, ..; the wave's sums follow, pv_wave_sum, scaled by beta), and the sum.  Pure functions of values: the callers keep
// their own loops and index arithmetic, so that pv_renyi_weights_kernel compiles to the instructions it had before the functions
// existed (scripts/compare_kernel_asm.py --source pv_particles.hip)
__device__ __forceinline__ float pv_lw_logq(float e, float sig) { return -(e * e) / 2.0f - logf(sig) - LOG_SQRT_2PI; }   // Normal(mu, sig).log_prob(mu + sig eps)
__device__ __forceinline__ float pv_lw_logp(float z) { return -(z * z) / 2.0f - LOG_SQRT_2PI; }                          // Normal(0, 1).log_prob(z)
__device__ __forceinline__ float pv_log_weight(float ll, float lp, float lq) { return ll + (lp - lq); }

// ---- held-out log-evidence: log p^(x_b) = logsumexp_k lw_kb - log K, streamed over chunks of P <= PV_RENYI_MAX_P particles ----
// lw[p B + b] = pv_log_weight(llkb[p B + b], ...) for the chunk's P samples of every image: one wave per image
struct PvEvidenceLw {
  const float* llkb;                // (P*B) log p(x_b | z_pb), every normaliser included
  const float* z; const float* eps; // (P*B, z_dim)
  const float* z_scale;             // (B, z_dim)
  float* lw;                        // (P*B)
  int B, P, z_dim;
  float beta;
};
int pv_evidence_lw(const PvEvidenceLw& e, hipStream_t s);
// the Poisson likelihood's per-image normaliser on P samples: llkb[p B + b] -= sum_i lgamma(x[b N + i] + 1), p < P (the sibling of
// pv_poisson_lognorm_rows without its K <= 256; the same float64 sum)
int pv_poisson_lognorm_particles(const float* x, int64_t B, int64_t N, float* llkb, int P, hipStream_t s);
// (pv_logmeanexp_update / pv_logmeanexp_finish, the running state per image: include/pyroved_amd.h)
