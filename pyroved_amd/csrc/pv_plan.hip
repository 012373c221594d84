// pv_plan.hip — host-side orchestration of one iVAE SVI step behind the C ABI (include/pyroved_amd.h).
// Enqueues, on the caller's stream, the kernel sequence that replaces
//   SVItrainer.train's `self.svi.step(x)` (trainers/svi.py:104-113)
//     -> Trace_ELBO.loss_and_grads(iVAE.model, iVAE.guide) (models/ivae.py:165-221)
//     -> pyro.optim.Adam -> zero_grads.
// No allocation, no synchronisation, no retained state: everything lives in the caller's plan.
#include "pv_common.h"
#include <algorithm>
#include <cmath>
#include <stdlib.h>
#include "pv_kernels.h"
#include "pv_sdec_fused.h"
#include "pv_linear.h"
#include "pv_convstack.h"
#include "pv_side.h"
#include "pv_conv.h"
#include "pv_particles.h"

namespace {

struct Carver {
  char* base;
  int64_t off;
  float* take(int64_t nfloats) {
    float* p = base ? (float*)(base + off) : nullptr;
    off += pv_align_up(nfloats * (int64_t)sizeof(float), 256);
    return p;
  }
};

struct Layout {
  // encoder
  float* xin; float* eact[PV_MAX_LAYERS]; float* epre[PV_MAX_LAYERS];
  float* head; float* dhead; float* z; float* z_scale; float* tp; float* zy;
  float* edp[PV_MAX_LAYERS];               // dL/d(pre-activation) of every encoder hidden layer
  bool enc_compact; float* kl_part; int kl_blocks;   // compact encoder kernels (pv_encoder.hip)
  unsigned* enc_flags;                               // ... their merged launch's tile flags (8 per row block; any content)
  // decoder
  float* hz; float* h0; float* dact[PV_MAX_LAYERS]; float* dpre_[PV_MAX_LAYERS];
  float* logits; float* llrow; float* llb; float* dbuf[2];
  float* part_dwo; float* part_dbo; float* part_hz; float* part_wc; float* part_tp;
  float* dhz; float* dtp; float* dzc;
  float* row_ll;                           // (B) unweighted ll_b (plan->row_elbo)
  float* alpha; float* sw; float* llkb;    // jiVAE: class probabilities (B, K), decoder row weights (K*B), ll per (k, b)
  float* jfix;                              // jiVAE without enumeration: correction of the guide's discrete log-prob sum
  // convolutional encoder (plan->n_enc_ops > 0): activation shapes / buffers, flattened features, gradient ping-pong
  bool enc_ext;                            // external encoder: (z_loc, z_scale) given, gradients handed back
  bool enc_conv; pvcs::Shape ces[PV_MAX_OPS + 1]; float* cea[PV_MAX_OPS + 1]; float* cfeat; float* cg[2];
  float* ceg[PV_MAX_OPS + 1];                              // per-op gradients dL/d(cea[i]) (the weight gradients run on the side stream)
  float* ccol; int64_t cF; float* cbn; int cbn_maxC;
  pvcs::WtPlan cwtp; char* cwt;                            // the step's tiled conv-encoder weights
  unsigned char* ccode;                                    // max-pool winners of the fused first block
  unsigned char* ccode2;                                   // ... of the convolution + max-pool pairs further up
  float* chead_wt;                                         // the head's weight re-indexed channels-last (null: GEMM path)
  char* cfin_ws; int64_t cfin_bytes;                       // the conv encoder's weight-gradient partials until the one finish launch
  void* scratch; int64_t scratch_bytes;    // split-K partials / colsum partials (used by one call at a time)
  int64_t rows;                            // decoder rows: B*N (spatial) or B (vanilla)
  int nchunk, rows_per_chunk;
  // fused persistent decoder path
  bool fused; int f_grid, f_kmax;
  PvDecChoice dec;                                          // the decoder kernel the layout's TRAINING launch runs (layout_choice, below)
  float* f_part; float* f_part_hz; float* f_rowtp; float* f_wimg; float* f_park;
  // multi-particle ELBO (pv_ivae_particles_*): P decoder samples per image ordered [p][b]; z, tp, zy, hz, sw, llkb hold P*B rows.
  // The count travels here, not in the ABI struct; 1 everywhere else
  int P;
  // importance-weighted (Renyi) bound with P > 1 (pv_particles.h: pv_renyi_weights): sw is filled with the softmax weights, and
  // c_b (B) gets room behind everything else
  bool renyi; float* r_c;
  double* pl_part;                                          // Poisson plans: pv_poisson_lognorm's partial sums (PV_POISSON_PARTS doubles)
  // held-out log-evidence (pv_ivae_evidence_accumulate): the multi-particle layout at EVERY P (P == 1 too: sw, llkb and the expansion),
  // without the buffers only a backward pass touches, and the chunk's (P, B) log-weights behind everything else
  bool ev; float* ev_lw;
  int64_t total;
};

// What the launches read of the step's objective (include/pyroved_amd.h: pv_ivae_objective) that does NOT decide the layout — the
// call arguments next to the Layout (L.P and L.renyi do decide it and live there).  Filled by resolve(), below
struct ObjArgs {
  float alpha = 0.0f; float* wout = nullptr;   // Renyi bound (L.renyi): its order; the caller's optional (P*B) copy of the weights
  const float* pw = nullptr;                   // per-observation weights of the likelihood: (n_pix) floats shared by all images, or null
  bool pw_img = false;                         // ... (batch * n_pix) instead: one weight per observation of every image (the layout of x)
  int fdm() const { return !pw ? 0 : pw_img ? PV_FDM_W_IMAGES : PV_FDM_W_SHARED; }   // the fused decoder kernels' weighted instance
};

// jiVAE (discrete_dim = K > 0): K decoder samples per input, ordered [k][b]; head = [mu | softplus input | class logits]
static inline int64_t plan_K(const pv_ivae_plan* p) { return p->discrete_dim > 0 ? p->discrete_dim : 0; }
// conv mode of the convolutional encoder (pv_convstack.h: 0 fp32-class fp16 pieces, 1 mixed, 2 fp32-class three bf16 pieces,
// 3 one fp16 piece).  fused == 3 is the throughput precision; conv_wide (a weight left fp16's range) selects the range-free
// bf16 forms of either precision
static inline int plan_conv_mode(const pv_ivae_plan* p) {
  if (p->fused == 3) return p->conv_wide ? 1 : 3;
  if (p->conv_wide) return 2;
  if (p->flags & PV_PLAN_CONV_X3) return 0;
  // round 5: the cheaper backward (pv_convstack.h mode 4) where the stack's gradient sums are long enough
  return pvcs::conv_mode_for(4, p->enc_ops, p->n_enc_ops, p->enc_ndim, p->batch, 1, p->enc_in_dim);
}
// Channels per grid position of a spatial decoder (iVAE(..., channels = C)): its output layer's width.  n_pix counts OBSERVATIONS
// per sample, positions * C: the encoder's input, x / loc and the Poisson normaliser run over n_pix; the decoder's rows per sample,
// the grid, the row chunks and the per-sample segment sums run over the positions.  Vanilla decoders: C = 1, positions = n_pix
static inline int64_t plan_C(const pv_ivae_plan* p) { return p->coord_dim > 0 ? p->out.out_dim : 1; }
static inline int64_t plan_pos(const pv_ivae_plan* p) { return p->n_pix / plan_C(p); }
// Rows per sample of the plan's DECODER layout: the positions — rounded up to a multiple of 16 where PV_PLAN_FUSED_TAIL takes effect
// (pv_sdec_fused.h: pv_sdec_fused_tail; the padding rows observe nothing and contribute exact zeros).  The layout's rows, the fused
// launch's partition, the latent backward and the per-sample segment sums run over plan_rows; the grid, x / loc, the encoder, the
// Poisson normaliser and the weights keep plan_pos / n_pix.  Everywhere the flag does not take effect the two are the same number
static inline int64_t plan_rows(const pv_ivae_plan* p) { return pv_sdec_fused_rows_per_sample(p); }
// PV_LIK_CATEGORICAL: the classes per position — the spatial decoder's channels, or the group width a vanilla plan names in out._pad
// (its decoder's n_pix outputs are channel-last, C consecutive logits per position); 1 for every per-value likelihood
static inline int plan_group(const pv_ivae_plan* p) {
  return p->lik != PV_LIK_CATEGORICAL ? 1 : (p->coord_dim > 0 ? p->out.out_dim : p->out._pad);
}
// The fused persistent decoder kernel a plan runs on, if any: the one-channel kernels (every `fused` mode) or the f32 kernel's
// multi-channel sibling (pv_sdec_fused_mc.hip: PV_PLAN_FUSED_CHANNELS with fused == 1 and 2 .. PV_MAX_CHANNELS channels).  The two
// predicates exclude each other (out.out_dim == 1 / >= 2)
static inline bool plan_fused_mc(const pv_ivae_plan* p) { return pv_sdec_fused_mc_supported(p); }
static inline bool plan_fused_ok(const pv_ivae_plan* p) { return pv_sdec_fused_supported(p) || plan_fused_mc(p); }
static inline int64_t plan_S(const pv_ivae_plan* p) { return (plan_K(p) > 0 ? plan_K(p) : 1) * (int64_t)p->batch; }
// decoder samples of a training step: jiVAE's K per input or the multi-particle ELBO's P (never both)
static inline int64_t step_S(const pv_ivae_plan* p, const Layout& L) { return plan_S(p) * L.P; }
static inline int64_t plan_head_w(const pv_ivae_plan* p) { return 2 * (int64_t)p->z_dim + plan_K(p); }
static inline int64_t plan_lat_in(const pv_ivae_plan* p) {
  return (p->coord_dim > 0 ? p->latent_dim : p->z_dim) + p->c_dim + plan_K(p);
}

// The decoder-kernel selection a plan runs with.  Poisson plans on the split-precision path (fused = 2) take the bf16 three-product
// kernel at every size: the fp16 builds the size rule picks from 16 384 rows up stage a row's 2^e of dL/dlogit = m 2^e as fp16, which
// holds |rate - x| < 2^15 only — counts (and rates up to exp(30)) go far beyond that, and an overflow there turns the weight gradients
// into inf silently.  bf16 pieces have fp32's exponent range.  Asking for the fp16 builds by name is refused (valid_plan).
// Every launch of a TRAINING layout takes this selection, the forward-only one of a call without gradients included (so evaluate runs
// the 4-wave kind 0 whatever the size: its layout — waves, records — is the training step's); pv_ivae_decode has a layout of its own
// and no fp16 build to avoid, so it keeps the plan's dec_kernel and with it the 8-wave forward-only build at large sizes.
static inline int plan_sel(const pv_ivae_plan* p) {
  return (p->lik == PV_LIK_POISSON_LOG && p->fused == 2 && p->dec_kernel == 0) ? 1 : p->dec_kernel;
}
// ... resolved (pv_sdec_fused.h: PvDecChoice) for the launch of `rows` decoder rows in a layout of the training step: plan_sel, because
// the fp16 builds must stay away from Poisson plans.  (The other resolution is decode_fused_run's.)
static inline PvDecChoice layout_choice(const pv_ivae_plan* p, int64_t rows, bool grads) {
  PvDecChoice c = pv_sdec_fused_choice(p->fused, rows / FD_UNIT, grads, plan_sel(p));
  if (plan_fused_mc(p)) c.family = PV_DEC_F32_MC;
  return c;
}

bool valid_plan(const pv_ivae_plan* p) {
  if (!p || p->batch <= 0 || p->n_pix <= 0 || p->z_dim <= 0) return false;
  if (p->coord_dim < 0 || p->coord_dim > 2) return false;
  if (p->n_enc_ops < 0 || p->n_enc_ops > PV_MAX_OPS) return false;
  if (p->n_enc_ops > 0 && (p->c_dim != 0 || p->discrete_dim != 0 || (p->enc_ndim != 1 && p->enc_ndim != 2))) return false;
  if (p->ext_encoder && (p->c_dim != 0 || p->discrete_dim != 0)) return false;
  if (!p->ext_encoder && p->n_enc_ops == 0 && (p->n_enc < 1 || p->n_enc > PV_MAX_LAYERS)) return false;
  if (p->n_dec < 1 || p->n_dec > PV_MAX_LAYERS) return false;
  if (p->discrete_dim < 0 || (!p->ext_encoder && p->head.out_dim != plan_head_w(p))) return false;
  if (p->discrete_dim > 0 && p->c_dim != 0) return false;                            // jiVAE: no conditioning vector
  if ((p->row_w || p->row_elbo || p->dy) && (p->discrete_dim > 0 || p->n_enc_ops > 0 || p->ext_encoder)) return false;
  if (p->dy && p->c_dim == 0) return false;
  if (p->lik != PV_LIK_BERNOULLI && p->lik != PV_LIK_GAUSSIAN && p->lik != PV_LIK_CBERNOULLI && p->lik != PV_LIK_POISSON_LOG &&
      p->lik != PV_LIK_CATEGORICAL)
    return false;
  if (p->lik == PV_LIK_CATEGORICAL) {
    // the C logits of a position are one observation: 2 .. PV_MAX_CHANNELS classes, no output sigmoid, the fc-encoder iVAE alone
    const int C = plan_group(p);
    if (C < 2 || C > PV_MAX_CHANNELS || p->n_pix % C != 0 || p->sigmoid_out) return false;
    if (p->discrete_dim > 0 || p->n_enc_ops > 0 || p->ext_encoder || p->ext_decoder || p->row_w || p->row_elbo || p->dy) return false;
  } else if (p->lik == PV_LIK_POISSON_LOG) {
    if (p->sigmoid_out) return false;                               // the decoder's output is the log-rate
    if (p->row_w || p->row_elbo || p->dy) return false;             // (per-image outputs would need the per-image normaliser)
    if (p->fused == 2 && p->dec_kernel > 1) return false;           // (the fp16 builds: plan_sel)
  } else if (p->lik != PV_LIK_GAUSSIAN && !p->sigmoid_out) return false;   // probs outside (0,1): unsupported
  if (p->coord_dim > 0 && (p->out.out_dim < 1 || p->out.out_dim > PV_MAX_CHANNELS || p->n_pix % p->out.out_dim != 0)) return false;
  // several channels per position: the fc-encoder iVAE on the layer-by-layer kernels
  if (p->coord_dim > 0 && p->out.out_dim > 1 &&
      (p->discrete_dim > 0 || p->row_w || p->row_elbo || p->dy || p->n_enc_ops > 0 || p->ext_encoder || p->ext_decoder))
    return false;
  if (p->coord_dim == 0 && p->out.out_dim != p->n_pix) return false;
  if (p->dec_kernel != 0 && !pv_sdec_fused_sel_valid(p->fused, p->dec_kernel)) return false;
  if (p->kl_mode != PV_KL_SAMPLED && p->kl_mode != PV_KL_ANALYTIC) return false;
  if (p->kl_mode == PV_KL_ANALYTIC && p->discrete_dim > 0) return false;            // (TraceEnum_ELBO has no mean-field form)
  return true;
}

// inference_only: encode / decode process B samples (jiVAE's K-fold enumeration exists only in the training step)
// encode_only (with inference_only): none of the decoder's per-row buffers is touched, so they get no room
// P > 1 (training step only): the multi-particle ELBO's layout; P == 1 is byte for byte the one-particle layout
// renyi (with P > 1): room for c_b at the very end, behind the multi-particle layout, which is unchanged
// evidence (training-step form only, never with renyi): Layout::ev — a forward-only layout of its own, no other query's size moves
void carve(const pv_ivae_plan* p, char* base, Layout& L, bool inference_only = false, bool encode_only = false, int P = 1,
           bool renyi = false, bool evidence = false) {
  Carver c{base, 0};
  L.P = inference_only ? 1 : P;
  L.renyi = renyi && L.P > 1;
  L.ev = evidence && !inference_only;
  const bool bwd = !L.ev;                            // room for what only a backward pass reads or writes
  // N: the decoder's rows per sample (spatial: grid positions) or its output width (vanilla)
  const int64_t B = p->batch, N = encode_only ? 0 : plan_rows(p), z = p->z_dim, Cn = plan_C(p);
  const int64_t lat_in = plan_lat_in(p), K = plan_K(p), S = inference_only ? p->batch : plan_S(p) * L.P, hw = plan_head_w(p);
  const bool multi = K > 0 || L.P > 1 || L.ev;      // several decoder samples per input
  L.rows = p->coord_dim > 0 ? S * N : S;
  const int64_t R = L.rows;
  L.xin = p->c_dim > 0 ? c.take(B * (p->n_pix + p->c_dim)) : nullptr;
  int64_t maxe = 0;
  L.enc_ext = p->ext_encoder != 0;
  L.enc_conv = !L.enc_ext && p->n_enc_ops > 0;
  const int n_enc = (L.enc_conv || L.enc_ext) ? 0 : p->n_enc;
  pvcs::Needs cnd;
  for (auto& e : L.ceg) e = nullptr;
  L.cfeat = L.cg[0] = L.cg[1] = L.ccol = L.cbn = nullptr; L.cF = 0; L.cbn_maxC = 0; L.cwt = nullptr; L.ccode = nullptr; L.ccode2 = nullptr; L.chead_wt = nullptr; L.cfin_ws = nullptr; L.cfin_bytes = 0;
  if (L.enc_conv) {
    L.ces[0] = pvcs::Shape{p->enc_in_dim[0], p->enc_ndim == 2 ? p->enc_in_dim[1] : 1, 1};
    if ((int64_t)L.ces[0].H * L.ces[0].W == p->n_pix && pvcs::stack_shapes(p->enc_ops, p->n_enc_ops, p->enc_ndim, B, L.ces, cnd)) {
      L.cea[0] = nullptr;
      for (int i = 0; i < p->n_enc_ops; ++i) L.cea[i + 1] = c.take(L.ces[i + 1].elems(B));
      const pvcs::Shape& fe = L.ces[p->n_enc_ops];
      L.cF = (int64_t)fe.H * fe.W * fe.C;
      L.cfeat = c.take(B * L.cF);
      if (pv_convhead_supported(L.cF, p->head.out_dim)) {
        L.chead_wt = c.take((int64_t)p->head.out_dim * L.cF);
        pvcs::upd(cnd.scratch, pv_convhead_ws((int)B, L.cF, p->head.out_dim));
      }
      L.cg[0] = c.take(cnd.maxact); L.cg[1] = c.take(cnd.maxact);
      if (!inference_only) {
        const bool c1 = pvcs::c1pool_fusable(p->enc_ops, p->n_enc_ops, p->enc_ndim, L.ces[0]);   // (its backward never writes dL/d(cea[1]))
        for (int i = 1; i < p->n_enc_ops; ++i) L.ceg[i] = (i == 1 && c1) ? nullptr : c.take(L.ces[i].elems(B));
      }
      L.ccol = c.take(cnd.maxcol);
      pvcs::wt_layout(p->enc_ops, p->n_enc_ops, p->enc_ndim, 0, plan_conv_mode(p), false, L.cwtp);
      L.cwt = reinterpret_cast<char*>(c.take((L.cwtp.bytes + 3) / 4));
      L.ccode = cnd.code_bytes ? reinterpret_cast<unsigned char*>(c.take((cnd.code_bytes + 3) / 4)) : nullptr;
      L.ccode2 = cnd.code2_bytes ? reinterpret_cast<unsigned char*>(c.take((cnd.code2_bytes + 3) / 4)) : nullptr;
      L.cbn = c.take(pvcs::bn_floats(cnd)); L.cbn_maxC = cnd.bn_maxC;
    } else {
      L.cF = -1;                                   // inconsistent op sequence: rejected by the entry points
    }
  }
  for (int i = 0; i < n_enc; ++i) {
    L.eact[i] = c.take(B * p->enc[i].out_dim);
    L.epre[i] = p->enc[i].act == PV_ACT_GELU ? c.take(B * p->enc[i].out_dim) : nullptr;
    if (p->enc[i].out_dim > maxe) maxe = p->enc[i].out_dim;
  }
  L.head = c.take(B * hw);
  L.dhead = c.take(B * hw);
  L.z = c.take((L.P > 1 ? S : B) * z);
  L.z_scale = c.take(B * z);
  L.tp = c.take(S * 8);
  L.zy = (p->c_dim > 0 || K > 0) ? c.take(S * lat_in) : nullptr;
  L.alpha = K > 0 ? c.take(B * K) : nullptr;
  L.sw = multi ? c.take(S) : nullptr;
  for (int i = 0; i < n_enc; ++i) L.edp[i] = c.take(B * p->enc[i].out_dim);
  L.enc_compact = !L.enc_conv && !L.enc_ext && pv_enc_compact_supported(p);
  L.kl_blocks = (int)((B + 15) / 16);
  L.kl_part = c.take(2 * (B > L.kl_blocks ? B : L.kl_blocks));   // (per 16-row block — or per sample when the guide rides in the decoder launch)
  L.enc_flags = reinterpret_cast<unsigned*>(c.take(8 * L.kl_blocks));     // (the merged encoder launch's tile flags)
  c.take(1024 + 16);                                 // (PvEncFold::coop_flags of the experiments-only shared first layer: the workspace size stays)
  int64_t maxd = 0;
  L.fused = p->fused && plan_fused_ok(p) && !(K > 0 && !L.enc_compact);   // (jiVAE + generic encoder: layered)
  L.f_grid = L.f_kmax = 0;
  L.f_part = L.f_part_hz = L.f_rowtp = L.f_wimg = L.f_park = nullptr;
  L.dec = PvDecChoice{};
  for (int i = 0; i < p->n_dec; ++i) {
    L.dact[i] = L.fused ? nullptr : c.take(R * p->dec[i].out_dim);
    L.dpre_[i] = (!L.fused && p->dec[i].act == PV_ACT_GELU) ? c.take(R * p->dec[i].out_dim) : nullptr;
    if (p->dec[i].out_dim > maxd) maxd = p->dec[i].out_dim;
  }
  int64_t scratch = 0;
  auto upd = [&](int64_t v) { if (v > scratch) scratch = v; };
  if (p->coord_dim > 0) {
    const int64_t H0 = p->fc_coord.out_dim;
    if (H0 > maxd) maxd = H0;
    L.hz = c.take(S * H0);
    L.h0 = L.fused ? nullptr : c.take(R * H0);
    if (L.fused) {
      const int64_t units = R / FD_UNIT;
      L.f_grid = pv_sdec_fused_grid(units);
      L.dec = layout_choice(p, R, true);
      L.f_kmax = pv_sdec_fused_kmax((int)N, units, L.f_grid, L.dec.waves);   // (the bf16 kernels publish dL/d(hz) per wave)
      L.f_part = c.take((int64_t)L.f_grid * FD_REC);
      L.f_part_hz = c.take(S * L.f_kmax * (H0 + PV_RS_W));        // (+ the row-sum slots behind it: PvFused::part_rs, one zero fill)
      L.f_rowtp = c.take(4 * R);
      L.f_wimg = c.take(FB_WIMG_BYTES / (int64_t)sizeof(float));
      const int64_t park = inference_only ? 0 : L.dec.park_bytes(L.f_grid);
      L.f_park = park ? c.take(park / (int64_t)sizeof(float)) : nullptr;
      upd(pv_colsum_ws(B, (int)H0));
    }
    L.logits = nullptr;
    L.llrow = c.take(R);
    const int64_t ob = pv_out_lik_blocks(R);
    L.part_dwo = c.take(ob * p->out.in_dim * Cn);
    L.part_dbo = c.take(ob * Cn);
    // row chunks per sample for the coord_latent backward: >= ~1024 workgroups overall
    int nchunk = (int)((1024 + B - 1) / B);
    if (nchunk > (N + 31) / 32) nchunk = (int)((N + 31) / 32);
    if (nchunk < 1) nchunk = 1;
    L.rows_per_chunk = (int)((N + nchunk - 1) / nchunk);
    if (L.rows_per_chunk < 1) L.rows_per_chunk = 1;
    L.nchunk = (int)((N + L.rows_per_chunk - 1) / L.rows_per_chunk);
    L.part_hz = bwd ? c.take(S * L.nchunk * H0) : nullptr;
    L.part_wc = bwd ? c.take(S * L.nchunk * H0 * p->coord_dim) : nullptr;
    L.part_tp = bwd ? c.take(S * L.nchunk * 4) : nullptr;
    L.dhz = bwd ? c.take(S * H0) : nullptr;
    L.dtp = bwd ? c.take(S * 4) : nullptr;
    L.dzc = bwd ? c.take(S * lat_in) : nullptr;
    upd(gemm_ws_need(S, H0, lat_in));          // hz
    upd(gemm_ws_need(H0, lat_in, S));          // dWz
    upd(gemm_ws_need(S, lat_in, H0));          // dzc
  } else {
    L.hz = L.h0 = nullptr;
    L.logits = c.take(S * N);
    L.llrow = c.take(S * N);
    L.part_dwo = L.part_dbo = L.part_hz = L.part_wc = L.part_tp = L.dhz = L.dtp = nullptr;
    L.nchunk = L.rows_per_chunk = 0;
    L.dzc = bwd ? c.take(S * lat_in) : nullptr;
    if (N > maxd) maxd = N;
    upd(gemm_ws_need(S, N, p->out.in_dim));
    upd(gemm_ws_need(N, p->out.in_dim, S));
    upd(gemm_ws_need(S, p->out.in_dim, N));
    upd(pv_colsum_ws(S, (int)N));
  }
  L.llb = c.take(B);
  L.row_ll = c.take(B);
  L.llkb = multi ? c.take(S) : nullptr;
  L.jfix = K > 0 ? c.take(4) : nullptr;
  L.dbuf[0] = (L.fused || !bwd) ? nullptr : c.take(R * maxd);
  L.dbuf[1] = (L.fused || !bwd) ? nullptr : c.take(R * maxd);
  // scratch: the largest split-K / colsum requirement of any single call
  upd(cnd.scratch);
  for (int i = 0; i < n_enc; ++i) {
    upd(gemm_ws_need(B, p->enc[i].out_dim, p->enc[i].in_dim));
    upd(gemm_ws_need(p->enc[i].out_dim, p->enc[i].in_dim, B));
    upd(gemm_ws_need(B, p->enc[i].in_dim, p->enc[i].out_dim));
    upd(pv_colsum_ws(B, p->enc[i].out_dim));
  }
  if (!L.enc_ext) {
    upd(gemm_ws_need(B, hw, p->head.in_dim));
    upd(gemm_ws_need(hw, p->head.in_dim, B));
    upd(gemm_ws_need(B, p->head.in_dim, hw));
    upd(pv_colsum_ws(B, (int)hw));
  }
  for (int i = 0; i < p->n_dec && !L.fused; ++i) {
    upd(gemm_ws_need(R, p->dec[i].out_dim, p->dec[i].in_dim));
    upd(gemm_ws_need(p->dec[i].out_dim, p->dec[i].in_dim, R));
    upd(gemm_ws_need(R, p->dec[i].in_dim, p->dec[i].out_dim));
    upd(pv_colsum_ws(R, p->dec[i].out_dim));
  }
  L.scratch_bytes = pv_align_up(scratch, 256);
  L.scratch = base ? (void*)(base + c.off) : nullptr;
  c.off += L.scratch_bytes;
  if (L.enc_conv && L.cF >= 0) {
    L.cfin_bytes = pv_align_up(cnd.wg_sum, 256);
    L.cfin_ws = base ? base + c.off : nullptr;
    c.off += L.cfin_bytes;
  }
  L.r_c = L.renyi ? c.take(B) : nullptr;           // (behind everything else: the multi-particle layout's offsets stay)
  // (at the very end, training layouts of Poisson plans only: every other offset is what it was)
  L.pl_part = (p->lik == PV_LIK_POISSON_LOG && !inference_only && bwd) ? reinterpret_cast<double*>(c.take(2 * PV_POISSON_PARTS)) : nullptr;
  L.ev_lw = L.ev ? c.take(S) : nullptr;
  L.total = c.off;
}

// the conv encoder as pv_convstack.h takes it: the activations (a[0] = x: one input channel, (B, 1, H, W) is already channels-last),
// the scratch with the step's tiled weights (both orientations: the backward reuses what the forward's launch tiled) and the head
struct ConvEnc {
  float* a[PV_MAX_OPS + 1];
  pvcs::Scratch sc;
  bool hfused;                                      // the head on the kernels of pv_convhead.hip (its weight re-indexed channels-last)
  ConvEnc(const pv_ivae_plan* p, const Layout& L)
      : sc{L.ccol, L.scratch, L.scratch_bytes, L.cbn, L.cbn_maxC, p->bn_eval, plan_conv_mode(p)},
        hfused(pv_convhead_supported(L.cF, p->head.out_dim) && L.chead_wt) {
    a[0] = const_cast<float*>(p->x);
    for (int i = 1; i <= p->n_enc_ops; ++i) a[i] = L.cea[i];
    sc.wt = L.cwt; sc.wtp = &L.cwtp;
    sc.code = L.ccode; sc.code2 = L.ccode2;
  }
  pvcs::ConvHead head(const pv_ivae_plan* p, const Layout& L) const {
    return {p->head, p->params, p->grads, L.cea[p->n_enc_ops], L.ces[p->n_enc_ops], (int)p->batch, hfused ? L.chead_wt : nullptr,
            L.cfeat, L.head, L.dhead, L.scratch, L.scratch_bytes};
  }
};

// convolutional encoder: x viewed as (B, 1, *enc_in_dim) -> op sequence -> flatten (C, spatial) -> L.head
// prep != null: the spatial decoder's weight images are written by the same tiling launch (pv_conv_wprep_table)
// hp != null: the caller's next launch (pv_head_fwd_blocks) sums the conv head's partial sums itself — *hp is filled when that form ran
struct PvHeadPart { const float* part = nullptr; const float* bias = nullptr; int nseg = 0, out = 0; };
int conv_encoder_fwd(const pv_ivae_plan* p, const Layout& L, hipStream_t s, const PvFbPrep* prep = nullptr, PvHeadPart* hp = nullptr) {
  if (L.cF < 0 || p->head.in_dim != L.cF) return PV_EINVAL;
  ConvEnc ce(p, L);
  pvcs::time_heaviest_conv(ce.sc, p->enc_ops, p->n_enc_ops, p->enc_ndim, (int)p->batch, L.ces, p->conv_ev_start, p->conv_ev_stop,
                           p->conv_ev_flops);
  const pvcs::Shape& fe = L.ces[p->n_enc_ops];
  const PvWprepEntry he = pvcs::head_entry(p->params + p->head.w_off, L.chead_wt, p->head.out_dim, fe.C, (int64_t)fe.H * fe.W);
  PV_TRY(pvcs::wt_prep(p->params, p->enc_ops, p->n_enc_ops, p->enc_ndim, 0, plan_conv_mode(p), L.cwtp, L.cwt, true, s, &he,
                       ce.hfused ? 1 : 0, prep));
  PV_TRY(pvcs::stack_fwd(p->params, p->enc_ops, p->n_enc_ops, p->enc_ndim, (int)p->batch, ce.a, L.ces, ce.sc, s));
  PV_TRY(pvcs::conv_head_fwd(ce.head(p, L), s, hp ? &hp->part : nullptr, hp ? &hp->nseg : nullptr));
  if (hp && hp->part) { hp->bias = bias_of(p->params, p->head); hp->out = p->head.out_dim; }
  return 0;
}

int encoder_fwd(const pv_ivae_plan* p, const Layout& L, hipStream_t s, const PvFbPrep* prep = nullptr, PvHeadPart* hp = nullptr) {
  if (L.enc_conv) return conv_encoder_fwd(p, L, s, prep, hp);
  const int64_t B = p->batch;
  const float* in = p->x;
  int64_t ldin = p->n_pix;
  if (p->c_dim > 0) {
    if (!p->y) return PV_EINVAL;
    PV_TRY(pv_concat(p->x, p->n_pix, p->n_pix, p->y, p->c_dim, p->c_dim, L.xin, B, s));
    in = L.xin; ldin = p->n_pix + p->c_dim;
  }
  for (int i = 0; i < p->n_enc; ++i) {
    const pv_layer& l = p->enc[i];
    if (l.in_dim != ldin) return PV_EINVAL;
    PV_TRY(linear_fwd(in, ldin, p->params + l.w_off, bias_of(p->params, l), L.eact[i], L.epre[i], l.out_dim, B, l.in_dim, l.out_dim, l.act,
                      L.scratch, L.scratch_bytes, s));
    in = L.eact[i]; ldin = l.out_dim;
  }
  const pv_layer& h = p->head;
  if (h.in_dim != ldin) return PV_EINVAL;
  return linear_fwd(in, ldin, p->params + h.w_off, bias_of(p->params, h), L.head, nullptr, h.out_dim, B, h.in_dim, h.out_dim, PV_ACT_NONE,
                    L.scratch, L.scratch_bytes, s);
}

// decoder forward from the decoder's latent input zin (B, lat_in); tp must be filled for coord_dim > 0.
// leaves the last hidden activation in L.dact[n_dec-1]; for coord_dim == 0 also the logits in L.logits
int decoder_hidden_fwd(const pv_ivae_plan* p, const Layout& L, const float* zin, int64_t ldz, int64_t lat_in,
                       hipStream_t s) {
  const int64_t R = L.rows;
  const int64_t B = p->coord_dim > 0 ? R / plan_pos(p) : R;    // decoder samples (jiVAE: K per input)
  const float* in;
  int64_t ldin;
  if (p->coord_dim > 0) {
    const int64_t H0 = p->fc_coord.out_dim;
    if (p->fc_latent.in_dim != lat_in || p->fc_latent.out_dim != H0 || p->fc_coord.in_dim != p->coord_dim)
      return PV_EINVAL;
    PV_TRY(linear_fwd(zin, ldz, p->params + p->fc_latent.w_off, nullptr, L.hz, nullptr, H0, B, lat_in, H0,
                      PV_ACT_NONE, L.scratch, L.scratch_bytes, s));
    PvCoordLat c{};
    c.grid = p->grid; c.tp = L.tp; c.Wc = p->params + p->fc_coord.w_off; c.bc = p->params + p->fc_coord.b_off;
    c.hz = L.hz; c.h0 = L.h0; c.M = R; c.N = (int)plan_pos(p); c.cd = p->coord_dim; c.H0 = (int)H0;
    PV_TRY(pv_coordlat_fwd(c, s));
    in = L.h0; ldin = H0;
  } else {
    in = zin; ldin = ldz;
    if (p->dec[0].in_dim != lat_in) return PV_EINVAL;
  }
  for (int i = 0; i < p->n_dec; ++i) {
    const pv_layer& l = p->dec[i];
    if (i > 0 || p->coord_dim > 0) { if (l.in_dim != ldin) return PV_EINVAL; }
    // instrumentation: the last hidden layer's forward GEMM is the layered path's representative kernel
    const bool timed = (i == p->n_dec - 1) && p->ev_start && p->ev_stop;
    if (timed) (void)hipEventRecord((hipEvent_t)p->ev_start, s);
    PV_TRY(linear_fwd(in, ldin, p->params + l.w_off, bias_of(p->params, l), L.dact[i],
                      L.dpre_[i], l.out_dim, R, l.in_dim, l.out_dim, l.act, L.scratch, L.scratch_bytes, s));
    if (timed) (void)hipEventRecord((hipEvent_t)p->ev_stop, s);
    in = L.dact[i]; ldin = l.out_dim;
  }
  if (p->out.in_dim != ldin) return PV_EINVAL;
  if (p->coord_dim == 0) {
    PV_TRY(linear_fwd(in, ldin, p->params + p->out.w_off, bias_of(p->params, p->out),
                      L.logits, nullptr, p->n_pix, R, p->out.in_dim, p->n_pix, PV_ACT_NONE, L.scratch,
                      L.scratch_bytes, s));
  }
  return 0;
}

// wgrad problem of one Linear: dw[N,K] = dpre[M,N]^T x[M,K], db[N] = colsum(dpre)
PvGemm wgrad_problem(const float* dpre, int64_t lddp, const float* x, int64_t ldx, float* dw, float* db, int64_t M,
                     int64_t K, int64_t N) {
  PvGemm g{};
  g.A = dpre; g.a_rs = 1; g.a_cs = lddp;
  g.B = x; g.b_rs = ldx; g.b_cs = 1;
  g.C = dw; g.ldc = K; g.M = (int)N; g.N = (int)K; g.K = (int)M;
  g.act = PV_ACT_NONE;
  g.rowsumA = db;
  return g;
}

typedef PvFinishArgs PvFinish;
inline int finish_scalars(const PvFinish& f, hipStream_t s) {
  return pv_finish_scalars(f.llb, f.B, f.scalars, f.kl_part, f.n_part, f.beta, s);
}

// one-tile-per-workgroup weight gradients, four problems a launch: the loss scalars (fin) ride in the first launch, the optimizer
// update (adam; *adam_done set) in the last, which must be the one that finalises the step's last gradient
int wgrad_small_chunks(const PvGemm* g, int n, hipStream_t s, const PvFinish* fin = nullptr, const PvAdamFuse* adam = nullptr,
                       bool* adam_done = nullptr) {
  for (int i = 0; i < n; i += 4) {
    const bool last = i + 4 >= n;
    PV_TRY(pv_wgrad_small(g + i, n - i < 4 ? n - i : 4, s, last ? adam : nullptr, i == 0 ? fin : nullptr));
    if (last && adam) *adam_done = true;
  }
  return 0;
}

// a long contraction over a few output tiles (jiVAE's fc_latent: K*B decoder samples onto 128 x lat_in) would sit on a handful of
// workgroups in the one-tile-per-workgroup launch: such a problem wants the split-K GEMM
bool wants_split_k(const PvGemm& e) {
  const int64_t tiles = (int64_t)((e.M + 15) / 16) * ((e.N + 15) / 16);
  return e.K > 1024 && tiles < 128 && pv_gemm_pick_splits(e.M, e.N, e.K) > 1;
}

// the fc encoder's weight-gradient problems: the head's, then the hidden layers' from the last to the first (1 + n_enc of them)
int encoder_wgrad_problems(const pv_ivae_plan* p, const Layout& L, PvGemm* probs) {
  const int64_t B = p->batch;
  const int ne = p->n_enc;
  float* G = p->grads;
  const pv_layer& hd = p->head;
  int np = 0;
  probs[np++] = wgrad_problem(L.dhead, hd.out_dim, L.eact[ne - 1], hd.in_dim, G + hd.w_off, bias_of(G, hd), B, hd.in_dim, hd.out_dim);
  const float* xin = p->c_dim > 0 ? L.xin : p->x;
  const int64_t ldx = p->n_pix + p->c_dim;
  for (int i = ne - 1; i >= 0; --i) {
    const pv_layer& l = p->enc[i];
    probs[np++] = wgrad_problem(L.edp[i], l.out_dim, i > 0 ? L.eact[i - 1] : xin, i > 0 ? p->enc[i - 1].out_dim : ldx, G + l.w_off,
                                bias_of(G, l), B, l.in_dim, l.out_dim);
  }
  return np;
}

// `extra` and the compact (fc) encoder's problems as ONE one-tile-per-workgroup launch (the launch that closes an own-sample step);
// -1 when one of them wants the split-K GEMM or they are more than that launch takes
int one_launch_wgrad_problems(const pv_ivae_plan* p, const Layout& L, const PvGemm* extra, int n_extra, PvGemm (&probs)[4]) {
  if (p->batch > 4096 || n_extra + 1 + p->n_enc > 4) return -1;
  for (int i = 0; i < n_extra; ++i) {
    if (wants_split_k(extra[i])) return -1;
    probs[i] = extra[i];
  }
  return n_extra + encoder_wgrad_problems(p, L, probs + n_extra);
}

// conv encoder backward from L.dhead: the head (features2latent), then the op sequence in reverse — input gradients on s, kernel-3
// weight gradients on the side stream, joined before their one finish launch; the caller's small weight gradients (`extra`) ride along
int conv_encoder_bwd(const pv_ivae_plan* p, const Layout& L, const PvGemm* extra, int n_extra, hipStream_t s, const PvFinish* fin,
                     const PvAdamFuse* adam, bool* adam_done, bool head_side) {
  const int64_t B = p->batch;
  ConvEnc ce(p, L);
  hipStream_t side = pv_side_stream_for(s, p->flags);
  PvSideJoin sj;                                    // joins the side stream on an early return
  // the head's weight gradient needs dhead only: on the side stream (forked off the launch that wrote dhead) next to the input gradient
  hipStream_t hs = s;
  if (ce.hfused) {
    if (head_side && side) { PV_TRY(pv_fork_to(side, s)); sj.fork(s, side); hs = side; }
    else pv_fork_disarm();
  }
  // ... and so do the small weight gradients the caller hands over (fc_latent's: they need the latent-backward launch's results
  // only) with the loss scalars riding: behind the head's on the side stream instead of at the very end of the step.
  // The optimizer update is then a launch of its own after the last reduction (round 5: the closing launch 13.6 -> ~6 us).
  auto extra_early = [&]() -> int {
    if (hs != side || !side || n_extra < 1 || n_extra > 4) return 0;
    PV_TRY(pv_wgrad_small(extra, n_extra, side, nullptr, fin));
    n_extra = 0; fin = nullptr;
    return 0;
  };
  float* g = nullptr;
  bool g_is_pre = false;
  int pp = ce.hfused ? 1 : 0;                       // (dL/d(features) lands in cg[1] in either form; first free ping-pong buffer: cg[0])
  PV_TRY(pvcs::conv_head_bwd(ce.head(p, L), p->enc_ops[p->n_enc_ops - 1], hs, side != nullptr, L.cg, pp, &g, &g_is_pre, s, extra_early));
  PvFinishList wfin{};                              // the weight gradients' reductions: one launch after the stack
  wfin.base = L.cfin_ws; wfin.cap = L.cfin_bytes;
  ce.sc.fin = &wfin;
  // kernel-3 weight gradients on the side stream, the input-gradient chain on s (every op's gradient in its own buffer);
  // joined before the finish
  bool joined = false;
  sj.fork(s, side);
  ce.sc.side = side; ce.sc.side_joined = &joined;
  PV_TRY(pvcs::stack_bwd(p->params, p->grads, p->enc_ops, p->n_enc_ops, p->enc_ndim, (int)B, ce.a, L.ces, g, L.cg, pp, false,
                         nullptr, ce.sc, s, 0, g_is_pre, side ? L.ceg : nullptr));
  if (side && !joined) PV_TRY(pv_stream_after(s, side));
  sj.joined();
  PV_TRY(pv_wgrad_finish_all(&wfin, s));
  if (fin && n_extra < 1) PV_TRY(finish_scalars(*fin, s));
  // (the loss scalars ride in the first of these launches; every other gradient is final by now, so pv_ivae_step's Adam update
  //  rides in the last one: its own outputs in its epilogue, the rest of the flat buffer by guest workgroups)
  return wgrad_small_chunks(extra, n_extra, s, fin, (adam_done && B <= 4096) ? adam : nullptr, adam_done);
}

// encoder backward from dL/d(head pre-activations) (L.dhead): the dgrad chain through the hidden layers, then
// every weight gradient of the encoder (plus `extra`, e.g. fc_latent's) in one multi-GEMM launch per 4 problems
// adam / adam_done: pv_ivae_step's optimizer update, applied inside the weight-gradient launch when that single launch
// finalises every encoder gradient (compact encoder, <= 4 problems); *adam_done tells the caller whether it was
// dgrad_done: the compact encoder's dgrad chain already ran (inside pv_latent_bwd_reduce); the loss scalars then ride
// in the weight-gradient launch
int encoder_bwd(const pv_ivae_plan* p, const Layout& L, const PvGemm* extra, int n_extra, hipStream_t s,
                const PvFinish* fin = nullptr, const PvAdamFuse* adam = nullptr, bool* adam_done = nullptr,
                bool dgrad_done = false, bool head_side = false) {
  const int64_t B = p->batch;
  void* ws = L.scratch;
  const int64_t wsb = L.scratch_bytes;
  const int ne = p->n_enc;
  const pv_layer& hd = p->head;
  if (L.enc_ext) {                                   // dhead already sits in the caller's ext_dhead
    if (fin) PV_TRY(finish_scalars(*fin, s));
    return wgrad_small_chunks(extra, n_extra, s);
  }
  if (L.enc_conv) return conv_encoder_bwd(p, L, extra, n_extra, s, fin, adam, adam_done, head_side);
  if (L.enc_compact && dgrad_done) {
    // nothing to launch here
  } else if (L.enc_compact) {
    PvEncDgrad d{};
    d.params = p->params; d.n_enc = ne; d.B = (int)B; d.head = hd; d.dhead = L.dhead;
    for (int i = 0; i < ne; ++i) { d.enc[i] = p->enc[i]; d.eact[i] = L.eact[i]; d.edp[i] = L.edp[i]; }
    if (fin) {
      d.fin_llb = fin->llb; d.fin_scalars = fin->scalars; d.fin_kl_part = fin->kl_part; d.fin_n_part = fin->n_part; d.fin_beta = fin->beta;
    }
    PV_TRY(pv_enc_dgrad(d, s));
  } else {
    PV_TRY(linear_dgrad(L.dhead, hd.out_dim, p->params + hd.w_off, L.edp[ne - 1], hd.in_dim, L.eact[ne - 1], L.epre[ne - 1],
                        hd.in_dim, p->enc[ne - 1].act, B, hd.in_dim, hd.out_dim, ws, wsb, s));
    for (int i = ne - 1; i > 0; --i) {
      const pv_layer& l = p->enc[i];
      PV_TRY(linear_dgrad(L.edp[i], l.out_dim, p->params + l.w_off, L.edp[i - 1], l.in_dim, L.eact[i - 1],
                          L.epre[i - 1], p->enc[i - 1].out_dim, p->enc[i - 1].act, B, l.in_dim, l.out_dim, ws, wsb, s));
    }
  }
  PvGemm probs[PV_MAX_LAYERS + 4];
  int np = 0;
  for (int i = 0; i < n_extra; ++i) {
    // split-K GEMM where the workspace has the room, finished before the one-tile-per-workgroup launch so that its fused Adam
    // guests see the final gradient
    const PvGemm& e = extra[i];
    if (wants_split_k(e) && gemm_ws_need(e.M, e.N, e.K) <= wsb) PV_TRY(pv_gemm(e, pv_gemm_pick_splits(e.M, e.N, e.K), ws, wsb, s));
    else probs[np++] = e;
  }
  np += encoder_wgrad_problems(p, L, probs + np);
  const PvFinish* fin_w = (L.enc_compact && dgrad_done) ? fin : nullptr;     // (otherwise pv_enc_dgrad hosted it)
  if (B <= 4096) {
    const bool ride = np <= 4 && adam_done && L.enc_compact;
    return wgrad_small_chunks(probs, np, s, fin_w, ride ? adam : nullptr, adam_done);
  }
  // long contractions: split-K GEMMs, one launch pair each
  if (fin_w) PV_TRY(finish_scalars(*fin_w, s));
  for (int i = 0; i < np; ++i)
    PV_TRY(pv_gemm(probs[i], pv_gemm_pick_splits(probs[i].M, probs[i].N, probs[i].K), ws, wsb, s));
  return 0;
}

// ---- the plan's latent description, written once for every argument block that carries it ----
// the latent geometry (which of z's leading columns are rotation / translation / scale, their priors, the KL weight and form) on
// PvHead, PvHeadBwd, PvEncFwd or PvEncFold — kl_mode where the block has it (PvEncFold's launches take it as an argument)
template <class D> auto set_kl_mode(D& d, int m, int) -> decltype((void)(d.kl_mode = m)) { d.kl_mode = m; }
template <class D> void set_kl_mode(D&, int, long) {}
template <class D> void latent_geometry(D& d, const pv_ivae_plan* p) {
  d.z_dim = p->z_dim; d.coord_dim = p->coord_dim;
  d.has_r = p->has_r; d.has_t = p->has_t; d.has_s = p->has_s;
  d.tp0 = p->t_prior[0]; d.tp1 = p->t_prior[1]; d.sc_prior = p->sc_prior; d.beta = p->beta;
  set_kl_mode(d, p->kl_mode, 0);
}
// where the head lives: the encoder's merged [mu | softplus input (| class logits)] rows in the workspace, or the caller's
// (z_loc, z_scale) of an external encoder
template <class D> void head_source(D& d, const pv_ivae_plan* p, const Layout& L) {
  d.head = L.enc_ext ? p->ext_head : L.head; d.scale_direct = L.enc_ext ? 1 : 0;
  d.ldh = L.enc_ext ? 0 : (int)plan_head_w(p);
  d.w = p->row_w;
}
// the head's backward (reparameterised sample + KL terms -> L.dhead) without its inputs from the decoder (dzc, dtp)
PvHeadBwd head_bwd_desc(const pv_ivae_plan* p, const Layout& L) {
  PvHeadBwd hb{};
  latent_geometry(hb, p);
  head_source(hb, p, L);
  hb.z = L.z; hb.z_scale = L.z_scale; hb.eps = p->eps; hb.B = p->batch;
  hb.dhead = L.enc_ext ? p->ext_dhead : L.dhead;
  return hb;
}
// the fused spatial decoder's weights (pv_sdec_fused.h: coord_latent, two hidden layers of 128, the output layer)
void fused_weights(PvFused& f, const pv_ivae_plan* p) {
  f.Wc = p->params + p->fc_coord.w_off; f.bc = p->params + p->fc_coord.b_off;
  f.W1 = p->params + p->dec[0].w_off; f.b1 = p->params + p->dec[0].b_off;
  f.W2 = p->params + p->dec[1].w_off; f.b2 = p->params + p->dec[1].b_off;
  f.wo = p->params + p->out.w_off; f.bo = p->params + p->out.b_off;
}

// plan->row_w / row_elbo on the paths that form ll_b with pv_segsum: keep the unweighted ll_b, weight what the loss sums
int weigh_llb(const pv_ivae_plan* p, const Layout& L, hipStream_t s) {
  if (p->row_elbo) {
    hipError_t e = hipMemcpyAsync(L.row_ll, L.llb, (size_t)p->batch * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return (int)e;
  }
  if (p->row_w) PV_TRY(pv_scale_rows(L.llb, p->row_w, p->batch, 1, s));
  return 0;
}

// plan->row_elbo (per-sample ELBO terms) and plan->dy (dloss/dy = the y columns of dL/d(encoder input) and of
// dL/d(decoder latent input) `dzc`), after the step's other work
int extra_outputs(const pv_ivae_plan* p, const Layout& L, const float* dzc, int64_t lat_in, hipStream_t s) {
  const int64_t B = p->batch;
  if (p->row_elbo)
    PV_TRY(pv_row_elbo(L.row_ll, L.z, L.head, L.z_scale, (int)B, p->z_dim, (int)plan_head_w(p), p->beta, p->row_elbo, s,
                       p->kl_mode));
  if (p->dy && dzc) {
    const pv_layer& l0 = p->enc[0];
    const int64_t N = p->n_pix, c = p->c_dim;
    if (l0.in_dim != N + c) return PV_EINVAL;
    PvGemm g{};
    g.A = L.edp[0]; g.a_rs = l0.out_dim; g.a_cs = 1;                         // (B, H)
    g.B = p->params + l0.w_off + N; g.b_rs = l0.in_dim; g.b_cs = 1;          // B(j, i) = W0[j][N + i]
    g.C = p->dy; g.ldc = c; g.M = (int)B; g.N = (int)c; g.K = l0.out_dim;
    g.act = PV_ACT_NONE;
    PV_TRY(pv_gemm(g, 1, L.scratch, L.scratch_bytes, s));
    PV_TRY(pv_add_cols(p->dy, c, dzc + (lat_in - c), lat_in, B, (int)c, s));
  }
  return 0;
}

// dL/dz from the decoder (dzc: content/y columns; dtp: phi, scale, tx, ty) -> head -> encoder
int latent_encoder_bwd(const pv_ivae_plan* p, const Layout& L, int64_t lat_in, int dtp_sb, int dtp_sc,
                       hipStream_t s) {
  PvHeadBwd hb = head_bwd_desc(p, L);
  hb.dzc = L.dzc; hb.ldzc = lat_in; hb.dtp = L.dtp; hb.dtp_sb = dtp_sb; hb.dtp_sc = dtp_sc;
  PV_TRY(pv_head_bwd(hb, s));
  PV_TRY(encoder_bwd(p, L, nullptr, 0, s));
  return extra_outputs(p, L, L.dzc, lat_in, s);
}

// guide: encoder -> (z_loc, z_scale) -> z = z_loc + z_scale*eps, sampled-KL terms, transform parameters
// hzr != null (not the compact encoder): fc_latent of the spatial decoder may ride in the head launch — hzr->done says whether it did
// (kl: the KL sums of scalars[2], [3] left as partials in L.kl_part: pass them to pv_finish_scalars)
struct PvHzReq { const float* zin; int64_t ldz; int lat_in, H; const float* Wz; float* hz; bool done, kl; };
int guide_fwd(const pv_ivae_plan* p, const Layout& L, hipStream_t s, const PvFbPrep* prep = nullptr,
              float hz_scale = 0.0f, PvHzReq* hzr = nullptr) {
  if (L.enc_compact) {
    PvEncFwd e{};
    if (prep) e.prep = *prep;
    e.params = p->params; e.n_enc = p->n_enc; e.head = p->head;
    for (int i = 0; i < p->n_enc; ++i) { e.enc[i] = p->enc[i]; e.eact[i] = L.eact[i]; }
    e.x = p->x; e.ldx = p->n_pix;
    if (p->c_dim > 0) {
      if (!p->y) return PV_EINVAL;
      PV_TRY(pv_concat(p->x, p->n_pix, p->n_pix, p->y, p->c_dim, p->c_dim, L.xin, p->batch, s));
      e.x = L.xin; e.ldx = p->n_pix + p->c_dim;
    }
    e.eps = p->eps; e.y = p->y; e.head_out = L.head; e.z = L.z; e.z_scale = L.z_scale;
    e.z_loc_out = p->z_loc; e.z_scale_out = p->z_scale;
    e.tp = p->coord_dim > 0 ? L.tp : nullptr; e.zy = L.zy; e.kl_part = L.kl_part;
    e.beta_disc = p->beta_disc; e.K = (int)plan_K(p); e.alpha = L.alpha; e.sw = L.sw;
    e.w = p->row_w;
    if (p->coord_dim > 0) { e.hz = L.hz; e.Wz = p->params + p->fc_latent.w_off; e.H0 = p->fc_coord.out_dim; }
    e.hz_scale = hz_scale;
    e.flags = (p->flags & PV_PLAN_ENC_TWO_LAUNCH) ? nullptr : L.enc_flags;
    e.spin_limit = (p->flags & PV_PLAN_ENC_NO_WAIT) ? 0 : 256;
    e.B = p->batch; e.c_dim = p->c_dim;
    latent_geometry(e, p);
    return pv_enc_fwd(e, s);
  }
  if (prep && !L.enc_conv) return PV_EINVAL;      // (stand-alone preparation on this path)
  // a conv encoder in front of the spatial decoder (hzr): the conv head's partial sums, this head and fc_latent in ONE launch of
  // ceil(B / 16) workgroups (PV_HEAD_MERGE=0: the four launches)
  static const int ab_merge = pv_exp_int("PV_HEAD_MERGE", 1);
  const bool blocks = ab_merge && hzr && L.enc_conv && !L.enc_ext && plan_K(p) == 0 && p->head.out_dim == (int)plan_head_w(p);
  PvHeadPart hp;
  if (!L.enc_ext) PV_TRY(encoder_fwd(p, L, s, prep, blocks ? &hp : nullptr));
  PvHead h{};
  if (hp.part) { h.ch_part = hp.part; h.ch_bias = hp.bias; h.ch_nseg = hp.nseg; h.ch_out = hp.out; h.head_w = L.head; }
  if (blocks) {
    h.kl_part = L.kl_part; hzr->kl = true;
    if (hzr->lat_in <= 16) {
      h.zin = hzr->zin; h.ldz = hzr->ldz; h.lat_in = hzr->lat_in; h.H = hzr->H; h.Wz = hzr->Wz; h.hz = hzr->hz;
      hzr->done = true;
    }
  }
  latent_geometry(h, p);
  head_source(h, p, L);
  h.eps = p->eps; h.y = p->y; h.z = L.z; h.z_scale = L.z_scale;
  h.z_loc_out = p->z_loc; h.z_scale_out = p->z_scale;
  h.tp = p->coord_dim > 0 ? L.tp : nullptr; h.zy = L.zy; h.scalars = p->scalars;
  h.B = p->batch; h.c_dim = p->c_dim;
  const int64_t K = plan_K(p);
  if (K > 0) h.zy = nullptr;                      // (written per decoder sample below)
  if (blocks) PV_TRY(pv_head_fwd_blocks(h, s));
  else PV_TRY(pv_head_fwd(h, s));
  if (K > 0) {
    const int n_content = p->coord_dim > 0 ? p->latent_dim : p->z_dim;
    PV_TRY(pv_jiv_expand(L.head, (int)plan_head_w(p), L.z, p->z_dim, n_content, p->coord_dim > 0 ? L.tp : nullptr, L.zy,
                         L.alpha, L.sw, p->scalars, p->beta_disc, p->batch, (int)K, s));
  }
  return 0;
}

// ---- multi-particle ELBO (L.P > 1; pv_particles.h) ----
// The guide: the encoder ONCE over the B images, then one launch that expands the head into the P*B decoder samples [p][b].
// The compact encoder's launch also samples with the first B rows of eps — particle 0's — into the rows the expansion then writes
// for every particle (and hosts `prep`, the bf16 decoder's weight images); a generic fc encoder stops at the head.
// hz != null: fc_latent per sample rides in the expansion (the fused decoder's input), stored multiplied by hz_scale
// img != null: the encoder as one workgroup per image (pv_guide_img.hip) where the one-particle step would run it so
int particle_guide(const pv_ivae_plan* p, const Layout& L, hipStream_t s, const PvFbPrep* prep, float hz_scale, float* hz,
                   const PvEncFold* img = nullptr) {
  // (the expansion and the particle backward derive the content columns from the invariance flags: they must be the plan's)
  const int ncoord = p->coord_dim == 1 ? (p->has_t ? 1 : 0)
                                       : p->coord_dim == 2 ? (p->has_r ? 1 : 0) + (p->has_t ? 2 : 0) + (p->has_s ? 1 : 0) : 0;
  if (p->coord_dim > 0 && p->z_dim - ncoord != p->latent_dim) return PV_EINVAL;
  if (img) PV_TRY(pv_guide_img_launch(*img, prep, hz_scale, (int)p->batch, s, p->kl_mode));
  else if (L.enc_compact) PV_TRY(guide_fwd(p, L, s, prep, hz_scale));
  else if (prep) return PV_EINVAL;
  else PV_TRY(encoder_fwd(p, L, s));
  PvParticleExpand e{};
  latent_geometry(e, p);
  e.head = L.head; e.ldh = (int)plan_head_w(p); e.eps = p->eps; e.y = p->y;
  e.z = L.z; e.z_scale = L.z_scale; e.z_loc_out = p->z_loc; e.z_scale_out = p->z_scale;
  e.tp = p->coord_dim > 0 ? L.tp : nullptr; e.zy = p->c_dim > 0 ? L.zy : nullptr;
  if (hz) { e.hz = hz; e.Wz = p->params + p->fc_latent.w_off; e.H0 = p->fc_coord.out_dim; e.hz_scale = hz_scale; }
  e.sw = L.sw; e.kl_part = L.kl_part;
  e.B = (int)p->batch; e.P = L.P; e.c_dim = p->c_dim;
  return pv_particle_expand(e, s);
}
// the particle-reducing latent backward without its inputs from the decoder
PvParticleBwd particle_bwd_desc(const pv_ivae_plan* p, const Layout& L) {
  PvParticleBwd pb{};
  pb.hb = head_bwd_desc(p, L);
  pb.sw = L.sw; pb.llb = L.llb; pb.P = L.P;
  pb.llb_add = L.renyi ? L.r_c : nullptr;
  return pb;
}
// the Renyi bound's weights from the P samples' log-likelihoods in L.llkb: sw, the image's KL row, c_b
int renyi_weights(const pv_ivae_plan* p, const Layout& L, const ObjArgs& o, hipStream_t s) {
  PvRenyiWeights r{};
  r.llkb = L.llkb; r.z = L.z; r.eps = p->eps; r.z_scale = L.z_scale;
  r.sw = L.sw; r.weights_out = o.wout; r.kl_part = L.kl_part; r.c = L.r_c;
  r.B = (int)p->batch; r.P = L.P; r.z_dim = p->z_dim; r.beta = p->beta; r.alpha = o.alpha;
  return pv_renyi_weights(r, s);
}
// the scopes of pv_ivae_particles_*: the fc-encoder iVAE (spatial or vanilla decoder, with or without c_dim), layered or on the
// bf16-class fused decoder kernels
static bool particles_supported(const pv_ivae_plan* p) {
  return p->discrete_dim == 0 && p->n_enc_ops == 0 && !p->ext_encoder && !p->ext_decoder && !p->row_w && !p->row_elbo && !p->dy &&
         !p->class_onehot && p->fused != 1;
}

// the plan-side conditions of the folded guide (PvEncFold): plain-bf16 fused decoder, the plain two-hidden-layer fc encoder, no
// conditioning vector / discrete latent / per-sample weights; the launch-side ones are PvDecChoice::hosts_guide and pv_sdec_fused_w8_fold_ok's
// (plan_guide_one_image: the architecture one workgroup can run a whole image's guide for — the fold in the decoder launch and the
//  per-image guide launch, pv_guide_img.hip)
static bool plan_guide_one_image(const pv_ivae_plan* p, const Layout& L);
static bool plan_guide_may_fold(const pv_ivae_plan* p, const Layout& L) {
  // (the hosting launch computes the sampled KL form only: it sits at the register ceiling — the analytic form runs the guide as its own launch)
  // (multi-particle: one image's guide feeds P samples that sit in P different workgroups' unit ranges — decided on (B, P), never
  //  on the sample count alone: B = 128, P = 2 has the 256 samples of a foldable batch)
  return p->fused == 3 && L.P == 1 && !(p->flags & PV_PLAN_NO_ENC_FOLD) && p->kl_mode == PV_KL_SAMPLED && plan_guide_one_image(p, L);
}
static bool plan_guide_one_image(const pv_ivae_plan* p, const Layout& L) {
  const int64_t z = p->z_dim;
  return p->fused >= 2 && L.fused && L.enc_compact && !L.enc_ext && plan_K(p) == 0 &&
         p->c_dim == 0 && !p->row_w && !p->row_elbo && !p->dy && p->n_enc == 2 && p->enc[0].in_dim == p->n_pix &&
         p->enc[0].out_dim <= FD_H && p->enc[1].out_dim <= FD_H && p->head.out_dim == 2 * z && z <= 16 && plan_lat_in(p) <= 16 &&
         p->enc[0].w_off % 4 == 0 && p->enc[1].w_off % 4 == 0 && p->head.w_off % 4 == 0 && p->enc[1].in_dim % 4 == 0 &&
         p->head.in_dim % 4 == 0 && p->coord_dim > 0 &&
         // the folded prologue also reads the decoder's hidden matrices, the observations and the parameter base as float4
         // (the Python engine aligns every offset; a raw C-ABI caller need not) — otherwise the guide keeps its launch
         p->dec[0].w_off % 4 == 0 && p->dec[1].w_off % 4 == 0 && p->n_pix % 4 == 0 &&
         ((uintptr_t)p->params & 15) == 0 && ((uintptr_t)p->x & 15) == 0;
}

// ---- loss_and_grads with the fused persistent spatial-decoder kernel (pv_sdec_fused.hip), step by step ----
// what the steps hand to one another
struct FusedStep {
  const pv_ivae_plan* p; const Layout& L; const ObjArgs& o; bool grads; hipStream_t s;
  const float* zin; int64_t ldz;                     // the decoder's latent input: z's content columns, or the materialised concatenation
  PvDecChoice dec;                                   // the kernel the decoder launch runs: record format, hz scale, weight images, fold
  PvFused f{};                                       // the decoder launch's arguments
  PvEncFold ef{};                                    // one image's guide per workgroup: hosted by the decoder launch (fold), the per-image guide
                                                     // launch, and the latent backward + encoder chain in a decoder launch's epilogue (own chain)
  bool fold = false;                                 // the guide rides in the decoder launch
  bool kl_part = false;                              // the guide left the KL sums of scalars[2], [3] as partials in L.kl_part ...
  int kl_n = 0;                                      // ... that many: per sample when a workgroup runs an image's guide, else per 16-row block
  // the closing form
  PvLatentBwd lb{};                                  // latent backward + record sums, followed by the encoder backward
  PvParticleBwd pb{};                                // ... its particle-reducing form (L.P > 1)
  bool chain = false;                                // compact encoder: every sample's dgrad chain runs in its latent-backward workgroup
  PvGemm wz;                                         // fc_latent: dWz = dhz^T zin; its row sums are fc_coord's bias gradient (dbc = sum_b dhz[b])
                                                     // (jiVAE: over the K*B decoder samples, zin = [z content | onehot(k)])
  PvGemm tail[4]; int tail_np = -1;                  // own chain: the ONE closing launch's weight-gradient problems
  bool own_chain() const { return tail_np > 0; }
};

void fused_decoder_args(FusedStep& st) {
  const pv_ivae_plan* p = st.p; const Layout& L = st.L;
  const int64_t B = p->batch, N = plan_rows(p), R = L.rows, K = plan_K(p), S = step_S(p, L);   // jiVAE: S = K*B decoder samples, rows R = S*N (N: rows per sample)
  const bool multi = K > 0 || L.P > 1;               // (multi-particle: S = P*B, each weighted 1/P against the same B observations)
  PvFused& f = st.f;
  fused_weights(f, p);
  f.x = p->x; f.grid = p->grid; f.tp = L.tp; f.hz = L.hz;
  f.llrow = L.llrow; f.loc = p->loc; f.rowtp = L.f_rowtp; f.part_hz = L.f_part_hz; f.part = L.f_part;
  // (round 6) training launches of the 4-wave kernels (pv_sdec_fused_bf16.hip: the ones that write PV_REC_LANE_F32 records) hand
  // over per-slot row sums instead of rows.  NOT the 8-wave throughput kernel: it has no registers for five running sums, and
  // keeping them in LDS cost its in-order waves what the next launch saved (read-modify-write: +-0 on the step; ds_add_f32: +1.4 us
  // on the kernel — profiles/r06h_row_sums_ab.txt)
  f.part_rs = (st.grads && st.dec.rec_fmt == PV_REC_LANE_F32) ? L.f_part_hz + S * L.f_kmax * FD_H : nullptr;
  f.wimg = L.f_wimg; f.park = L.f_park;                // (a weighted launch puts the weights in wimg's slot: fused_decoder_launch)
  f.M = R; f.units = R / FD_UNIT; f.N = (int)N; f.cd = p->coord_dim; f.B = (int)S; f.lik = p->lik;
  f.n_obs = pv_sdec_fused_tail(p) ? (int)plan_pos(p) : 0;          // (the tail form: a sample observes fewer rows than it occupies)
  f.sw = multi ? L.sw : p->row_w; f.x_units = multi ? B * N / FD_UNIT : 0;
  f.sigmoid_out = p->sigmoid_out; f.kmax = L.f_kmax; f.sig = p->decoder_sig; f.sel = plan_sel(p);
  // fp16 builds of the fp32-class kernel: where the per-row exponent of dL/dlogit is centred (|dL/dlogit| <= 1 for the Bernoulli
  // likelihoods; ~ residual / sig^2 for the Gaussian): exact powers of two either way, only the representable RANGE moves
  f.dl_exp = 4;
  if (p->lik == PV_LIK_GAUSSIAN && p->decoder_sig > 0.0f) {
    int e2 = 0;
    (void)frexpf(p->decoder_sig * p->decoder_sig, &e2);      // sig^2 = m 2^e2, m in [0.5, 1)
    f.dl_exp = e2 < -40 ? -40 : (e2 > 40 ? 40 : e2);
  }
}

void fold_args(PvEncFold& ef, const pv_ivae_plan* p, const Layout& L) {
  ef.params = p->params; ef.enc0 = p->enc[0]; ef.enc1 = p->enc[1]; ef.head = p->head;
  ef.x = p->x; ef.ldx = p->n_pix; ef.eps = p->eps;
  ef.eact0 = L.eact[0]; ef.eact1 = L.eact[1]; ef.head_out = L.head;
  ef.z = L.z; ef.z_scale = L.z_scale; ef.z_loc_out = p->z_loc; ef.z_scale_out = p->z_scale;
  ef.tp = L.tp; ef.kl_part = L.kl_part; ef.hz = L.hz; ef.Wz = p->params + p->fc_latent.w_off;
  ef.lat_in = (int)plan_lat_in(p);
  latent_geometry(ef, p);
}

// the guide, in the cheapest form the plan allows: folded into the decoder launch (nothing to launch here), one workgroup per
// image, the compact encoder's tiled launch, or the generic / conv encoder followed by the head — each with the preparation of the
// bf16 decoder's weight images where fused >= 2
int fused_guide(FusedStep& st) {
  const pv_ivae_plan* p = st.p; const Layout& L = st.L; hipStream_t s = st.s;
  PvFused& f = st.f;
  const int64_t B = p->batch, lat_in = plan_lat_in(p);
  const float* Wz = p->params + p->fc_latent.w_off;
  st.kl_n = L.kl_blocks;
  st.kl_part = L.enc_compact;
  if (L.P > 1 || L.ev) {
    // multi-particle: the guide never rides in the decoder launch; the encoder once, the expansion writes hz for the P*B samples
    if (p->fused < 2) return PV_EINVAL;
    if (L.enc_compact) {
      const PvFbPrep prep = pv_sdec_fused_bf16_prep_args(f, st.grads, st.dec);
      f.hz_scale = prep.scale;
      fold_args(st.ef, p, L);
      const bool img = plan_guide_one_image(p, L) && pv_guide_img_ok(st.ef, (int)B) &&
                       !(p->flags & (PV_PLAN_ENC_TILED | PV_PLAN_ENC_TWO_LAUNCH | PV_PLAN_ENC_NO_WAIT));
      PV_TRY(particle_guide(p, L, s, &prep, f.hz_scale, L.hz, img ? &st.ef : nullptr));
    } else {
      PV_TRY(particle_guide(p, L, s, nullptr, 0.0f, L.hz));
      PV_TRY(pv_sdec_fused_bf16_prep(f, st.grads, st.dec, s));
    }
    st.kl_n = (int)B;
    st.kl_part = true;
    return 0;
  }
  // ---- the guide folded into the decoder launch (pv_sdec_fused.h PvEncFold): the plain-bf16 8-wave kernel, a workgroup's units a
  // whole number of images, the plain fc encoder of two hidden layers — BASELINE's headline config is exactly this.  No encoder
  // launch, no weight-image copy, no hand-off: the step is decoder launch -> latent backward + record sums -> small weight gradients.
  if (plan_guide_may_fold(p, L)) {       // (no cross-workgroup hand-off in it: fine under stream capture too)
    f.hz_scale = st.dec.img_scale;
    st.fold = st.dec.hosts_guide && pv_sdec_fused_w8_fold_ok(f, L.f_grid);
    if (!st.fold) f.hz_scale = 0.0f;
  }
  if (st.fold) {
    fold_args(st.ef, p, L);
    st.kl_n = (int)B;
    if (st.grads) {
      // the hosting launch owns whole images: it sums their per-row outputs itself in its epilogue (PvFused::part_rs, first slot),
      // and its dL/d(hz): the eight waves' partials summed next to the other column sums (PvFused::dhz_out)
      f.part_rs = L.f_part_hz + plan_S(p) * L.f_kmax * FD_H;
      f.dhz_out = L.dhz; f.dzc_out = L.dzc;
    }
    return 0;
  }
  if (p->fused >= 2 && L.enc_compact) {
    const PvFbPrep prep = pv_sdec_fused_bf16_prep_args(f, st.grads, st.dec);
    f.hz_scale = prep.scale;                          // the compact encoder's last launch writes scale * hz directly
    // (round 6) the guide as one workgroup per image (pv_guide_img.hip: no tile hand-offs, 11-13 us where the tiled one-launch
    // encoder takes 18-19) for the minibatch sizes where every image streaming the first-layer matrix from L2 is still cheaper
    // than that latency; the flags that are about the tiled encoder's launch form keep the tiled encoder
    fold_args(st.ef, p, L);
    if (plan_guide_one_image(p, L) && pv_guide_img_ok(st.ef, (int)B) &&
        !(p->flags & (PV_PLAN_ENC_TILED | PV_PLAN_ENC_TWO_LAUNCH | PV_PLAN_ENC_NO_WAIT))) {
      st.kl_n = (int)B;
      return pv_guide_img_launch(st.ef, &prep, f.hz_scale, (int)B, s, p->kl_mode);
    }
    return guide_fwd(p, L, s, &prep, f.hz_scale);
  }
  // conv encoder: the decoder's weight images ride in its weight-tiling launch; generic encoders: a launch of their own
  PvHzReq hzr{st.zin, st.ldz, (int)lat_in, FD_H, Wz, L.hz, false, false};
  const bool prep_in_enc = p->fused >= 2 && L.enc_conv;
  const PvFbPrep prep = p->fused >= 2 ? pv_sdec_fused_bf16_prep_args(f, st.grads, st.dec) : PvFbPrep{};
  PV_TRY(guide_fwd(p, L, s, prep_in_enc ? &prep : nullptr, 0.0f, &hzr));
  if (p->fused >= 2 && !prep_in_enc) {
    PV_TRY(pv_sdec_fused_bf16_prep(f, st.grads, st.dec, s));
  } else if (p->fused < 2 && st.grads) {
    hipError_t e = hipMemsetAsync(L.f_part_hz, 0, (size_t)(plan_S(p) * L.f_kmax * FD_H) * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
  }
  st.kl_part = L.enc_compact || hzr.kl;
  if (!L.enc_compact && !hzr.done) {                 // fc_latent did not ride in the head launch
    if (lat_in <= 16) PV_TRY(pv_smallk_linear(st.zin, st.ldz, Wz, L.hz, B, (int)lat_in, FD_H, s));
    else PV_TRY(linear_fwd(st.zin, st.ldz, Wz, nullptr, L.hz, nullptr, FD_H, B, lat_in, FD_H, PV_ACT_NONE, L.scratch, L.scratch_bytes, s));
  }
  return 0;
}

// how the step closes after the decoder launch: (a) pv_latent_bwd_reduce (per sample: ll_b, d(phi, scale, tx, ty), dL/d(hz),
// dL/d(z content), head backward -> L.dhead; in the same launch the per-workgroup gradient records summed into the flat gradient)
// followed by the encoder backward, or (b) the own chain: every workgroup of the decoder launch owns one image and runs its latent
// backward and encoder chain in its epilogue, and ONE launch of workgroups that need nothing from each other closes the step
void fused_closing_form(FusedStep& st, const PvAdamFuse* adam, bool* adam_done) {
  const pv_ivae_plan* p = st.p; const Layout& L = st.L;
  PvFused& f = st.f;
  const int64_t N = plan_rows(p), R = L.rows, z = p->z_dim, K = plan_K(p), S = step_S(p, L), lat_in = plan_lat_in(p);
  const int H = FD_H;
  const float* Wz = p->params + p->fc_latent.w_off;
  // (round 6) the 4-wave kernels too hand over dL/d(hz) and dL/dz, wherever every workgroup's units are exactly one sample
  // (batch == grid, e.g. C2's 256 on 256 CUs)
  if (!f.dhz_out && f.part_rs && K == 0 && L.P == 1 && lat_in <= 16 && S == L.f_grid && f.units == S * (N / FD_UNIT) && !p->dy &&
      st.dec.rec_fmt == PV_REC_LANE_F32) {
    f.dhz_out = L.dhz; f.dzc_out = L.dzc; f.Wz = Wz; f.lat_in = (int)lat_in;
  }
  PvLatentBwd& lb = st.lb;
  lb.llrow = L.llrow; lb.rowtp = L.f_rowtp; lb.part_hz = L.f_part_hz; lb.Wz = Wz;
  lb.part_rs = f.part_rs;
  lb.dhz_ready = f.dhz_out ? 1 : 0;
  lb.dzc_in = f.dzc_out;
  lb.llb = L.llb; lb.dhz = L.dhz; lb.M = R; lb.N = (int)N; lb.kmax = L.f_kmax; lb.H = H; lb.lat_in = (int)lat_in;
  lb.hb = head_bwd_desc(p, L);
  lb.K = (int)K; lb.alpha = L.alpha; lb.beta_disc = p->beta_disc;
  lb.row_ll = p->row_elbo ? L.row_ll : nullptr; lb.dzc_out = p->dy ? L.dzc : nullptr;
  // compact encoder: every sample's dgrad chain runs in its latent_bwd workgroup (one dependent launch less)
  st.chain = L.enc_compact && !L.enc_ext && 2 * z + K <= 256;
  if (st.chain) {
    lb.enc_n = p->n_enc; lb.enc_params = p->params; lb.enc_head = p->head;
    for (int i = 0; i < p->n_enc; ++i) { lb.enc_l[i] = p->enc[i]; lb.enc_act[i] = L.eact[i]; lb.enc_dp[i] = L.edp[i]; }
  }
  if (L.P > 1) {
    PvParticleBwd& pb = st.pb;
    pb = particle_bwd_desc(p, L);
    pb.llrow = L.llrow; pb.rowtp = L.f_rowtp; pb.part_hz = L.f_part_hz; pb.part_rs = f.part_rs; pb.Wz = Wz; pb.dhz = L.dhz;
    pb.M = R; pb.N = (int)N; pb.kmax = L.f_kmax; pb.H = H; pb.lat_in = (int)lat_in;
    if (L.renyi) pb.ll_s = L.llkb;                   // (the loss of the forward launch the weights came from)
    if (st.chain) {
      pb.enc_n = p->n_enc; pb.enc_params = p->params; pb.enc_head = p->head;
      for (int i = 0; i < p->n_enc; ++i) { pb.enc_l[i] = p->enc[i]; pb.enc_act[i] = L.eact[i]; pb.enc_dp[i] = L.edp[i]; }
    }
  }
  st.wz = wgrad_problem(L.dhz, H, st.zin, st.ldz, p->grads + p->fc_latent.w_off, p->grads + p->fc_coord.b_off, S, lat_in, H);
  // (round 6, third cut) the own chain: where every workgroup of the decoder launch owns one image — the launch that hosts the
  // guide, or a 4-wave launch at batch == grid (f.dhz_out / dzc_out / part_rs together) — it also runs the image's latent backward
  // and encoder chain in its epilogue (PvEncFold::chain), and the step closes with record sums, small weight gradients and loss
  // scalars in one launch (pv_elementwise.hip: pv_rec_wgrad_kernel).
  // Needs what that epilogue is written for — the plain iVAE step: no per-sample weights / extra outputs, a head of <= 16 outputs,
  // two hidden layers of width 128, the sampled KL form (the analytic form takes the latent-backward launch) — and, with the
  // optimizer riding, records + tiles covering every parameter.
  // The hosting launch then writes NO per-row outputs (L.llrow / L.f_rowtp, the dL/d(hz) slots): their only readers after a training
  // step are the latent-backward launches (not run here), row_elbo, dy, per-sample weights and the K > 0 forms — all excluded below.
  if (st.chain && f.part_rs && f.dhz_out && f.dzc_out && K == 0 && !p->row_w && p->kl_mode == PV_KL_SAMPLED && !p->row_elbo &&
      !p->dy && p->head.out_dim <= 16 && p->n_enc == 2 && p->enc[0].out_dim == FD_H && p->enc[1].in_dim == FD_H &&
      p->enc[1].out_dim == FD_H && p->head.in_dim == FD_H) {
    st.tail_np = one_launch_wgrad_problems(p, L, &st.wz, 1, st.tail);
    if (st.tail_np > 0 && adam) {
      // every PARAMETER must be finalised by a record block or a tile (the launch has no Adam guests): the plan's layers, counted,
      // against what the records and the tiles cover.  What else the flat buffer holds — alignment padding, batch-norm statistics —
      // never has a gradient or a moment, and Adam leaves such an element where it is.
      auto lsz = [](const pv_layer& l) { return (int64_t)l.in_dim * l.out_dim + (l.b_off >= 0 ? l.out_dim : 0); };
      int64_t want = lsz(p->head) + lsz(p->fc_coord) + lsz(p->fc_latent) + lsz(p->out);
      for (int i = 0; i < p->n_enc; ++i) want += lsz(p->enc[i]);
      for (int i = 0; i < p->n_dec; ++i) want += lsz(p->dec[i]);
      int64_t cov = 2 * (int64_t)H * H + (int64_t)H * (3 + p->coord_dim) + 1;
      for (int i = 0; i < st.tail_np; ++i) cov += (int64_t)st.tail[i].M * st.tail[i].N + (st.tail[i].rowsumA ? st.tail[i].M : 0);
      if (cov != want || !adam_done || p->n_dec != 2) st.tail_np = -1;
    }
  }
  if (st.own_chain()) {
    PvEncFold& ef = st.ef;
    ef.chain = 1 | ((p->flags & PV_PLAN_GENERIC_TILE_LOOP) ? PV_CHAIN_GENERIC_LOOP : 0);
    ef.dhead = L.dhead; ef.ldh = (int)plan_head_w(p); ef.edp0 = L.edp[0]; ef.edp1 = L.edp[1]; ef.llb = L.llb;
  }
}

int fused_decoder_launch(FusedStep& st) {
  const pv_ivae_plan* p = st.p;
  const bool timed = p->ev_start && p->ev_stop;
  if (timed) (void)hipEventRecord((hipEvent_t)p->ev_start, st.s);
  if (p->fused >= 2) {
    // (weighted steps on the bf16-class kernels — weighted_route with PV_PLAN_FAST_WEIGHTS: the weights ride in the slot of `park`,
    //  which no 4-wave launch reads; the routed plan's dec_kernel = 1 keeps every launch on the 4-wave kernel)
    PvFused f = st.f;
    if (st.o.pw) f.park = const_cast<float*>(st.o.pw);
    PV_TRY(pv_sdec_fused_bf16_launch(f, st.L.f_grid, st.grads, st.dec, st.s, st.fold ? &st.ef : nullptr,
                                     (st.own_chain() && !st.fold) ? &st.ef : nullptr, st.o.fdm()));
  }
  else if (st.dec.family == PV_DEC_F32_MC || st.o.pw) {
    // several channels per row: the f32 kernel's sibling, then (training) the sums of channels 1 .. C-1 of d(wo), d(bo) into the
    // flat gradient — in front of every launch that reads it, the one that applies Adam included
    // (weighted steps, st.o.pw: its weighted instances at every channel count — the entry point routed the plan here,
    //  weighted_route; with one channel there is nothing for the second launch to sum)
    PvFused f = st.f;
    f.wimg = nullptr; f.park = nullptr;
    if (st.o.pw) f.pw = st.o.pw;
    PV_TRY(pv_sdec_fused_mc_launch(f, (int)plan_C(p), st.L.f_grid, st.grads, st.s, st.o.fdm()));
    if (st.grads && plan_C(p) > 1) PV_TRY(pv_sdec_fused_mc_reduce_out(st.L.f_part, st.L.f_grid, p->grads, p->out.w_off, p->out.b_off, (int)plan_C(p), st.s));
  }
  else PV_TRY(pv_sdec_fused_launch(st.f, st.L.f_grid, st.grads, st.s));
  if (timed) (void)hipEventRecord((hipEvent_t)p->ev_stop, st.s);
  return 0;
}

// no gradients: ll_b from the decoder's rows, the loss scalars, the extra outputs
int fused_close_forward(const FusedStep& st) {
  const pv_ivae_plan* p = st.p; const Layout& L = st.L; hipStream_t s = st.s;
  const int64_t B = p->batch, N = plan_rows(p), K = plan_K(p);
  if (K > 0) {                                       // llb[b] = sum_k alpha_bk ll_kb
    PvLatentBwd lf{};
    lf.llrow = L.llrow; lf.llb = L.llb; lf.M = L.rows; lf.N = (int)N; lf.H = 0; lf.K = (int)K; lf.alpha = L.alpha;
    lf.hb.B = (int)B; lf.fwd_only = 1;
    PV_TRY(pv_latent_bwd(lf, s));
    return pv_finish_scalars(L.llb, (int)B, p->scalars, L.kl_part, L.kl_blocks, 1.0f, s);
  }
  if (L.P > 1) {                                     // llb[b] = sum_p sw ll_pb
    PvParticleBwd pf = particle_bwd_desc(p, L);
    pf.llrow = L.llrow; pf.M = L.rows; pf.N = (int)N; pf.kmax = 1; pf.fwd_only = 1;
    if (L.renyi) {                                   // ... with the bound's weights: llb[b] = sum_p w_pb ll_pb + c_b
      PV_TRY(pv_segsum(L.llrow, step_S(p, L), N, L.llkb, s));
      PV_TRY(renyi_weights(p, L, st.o, s));
      pf.llkb = L.llkb;
    }
    PV_TRY(pv_particle_bwd(pf, s));
    return pv_finish_scalars(L.llb, (int)B, p->scalars, L.kl_part, st.kl_n, 1.0f, s);
  }
  PV_TRY(pv_segsum(L.llrow, B, N, L.llb, s));
  PV_TRY(weigh_llb(p, L, s));
  PV_TRY(pv_finish_scalars(L.llb, (int)B, p->scalars, st.kl_part ? L.kl_part : nullptr, st.kl_n, 1.0f /* partials come scaled */, s));
  return extra_outputs(p, L, nullptr, plan_lat_in(p), s);
}

// Renyi bound, gradient step: the weights need every sample's log-likelihood before the decoder launch that applies them to
// dL/dlogit, and that launch fuses forward and backward — so a forward-only decoder launch runs first (the one a call without
// gradients makes), then the per-sample sums and the weights.  The forward-only launch may be another kernel with other weight
// images than the training launch (pv_sdec_fused_bf16_prep_args): it then gets its own preparation, and the training launch's —
// the guide hosted it — is repeated.  hz keeps the training launch's scale either way (a kernel that wants it scaled scales an
// unscaled one itself).
int fused_renyi_forward(const FusedStep& st) {
  const pv_ivae_plan* p = st.p; const Layout& L = st.L; hipStream_t s = st.s;
  PvFused ff = st.f;
  ff.part_rs = nullptr; ff.dhz_out = ff.dzc_out = nullptr;            // rows of ll, as every forward-only launch writes them
  const PvDecChoice fwd = layout_choice(p, L.rows, false), &trn = st.dec;
  const bool same_images = fwd.img_mode == trn.img_mode && fwd.img_scale == trn.img_scale && fwd.img_qswap == trn.img_qswap;
  if (!same_images) PV_TRY(pv_sdec_fused_bf16_prep(ff, false, fwd, s));
  PV_TRY(pv_sdec_fused_bf16_launch(ff, L.f_grid, false, fwd, s));
  if (!same_images) PV_TRY(pv_sdec_fused_bf16_prep(st.f, true, trn, s));
  PV_TRY(pv_segsum(L.llrow, step_S(p, L), plan_rows(p), L.llkb, s));
  return renyi_weights(p, L, st.o, s);
}

int fused_close(FusedStep& st, const PvAdamFuse* adam, bool* adam_done) {
  const pv_ivae_plan* p = st.p; const Layout& L = st.L; hipStream_t s = st.s;
  const PvFusedOffsets o{p->dec[0].w_off, p->dec[0].b_off, p->dec[1].w_off, p->dec[1].b_off,
                         p->fc_coord.w_off, p->out.w_off, p->out.b_off};
  // conv encoder with a side stream: the head's weight gradient forks off the closing launch (conv_encoder_bwd)
  static const int ab_side = pv_exp_int("PV_HEAD_SIDE", 1);
  static const int ab_fin = pv_exp_int("PV_FIN_RIDE", 1);
  const bool head_side = ab_side && L.enc_conv && !L.enc_ext && pv_side_stream_for(s, p->flags) && !pv_convhead_wgrad_uses_ws() &&
                         pv_convhead_supported(L.cF, p->head.out_dim) && L.chead_wt;
  if (head_side) pv_fork_arm();
  PvFinish fin{L.llb, (int)p->batch, p->scalars, st.kl_part ? L.kl_part : nullptr, st.kl_n, 1.0f /* partials come scaled */};
  if (st.own_chain()) {
    PV_TRY(pv_rec_wgrad(L.f_part, L.f_grid, p->grads, o, p->coord_dim, st.dec.rec_fmt, st.tail, st.tail_np, adam, &fin, s));
    if (adam) *adam_done = true;
    return extra_outputs(p, L, L.dzc, plan_lat_in(p), s);
  }
  if (L.P > 1) PV_TRY(pv_particle_bwd_reduce(st.pb, L.f_part, L.f_grid, p->grads, o, p->coord_dim, s, st.dec.rec_fmt));
  else PV_TRY(pv_latent_bwd_reduce(st.lb, L.f_part, L.f_grid, p->grads, o, p->coord_dim, s, st.dec.rec_fmt));
  // the loss scalars ride in the encoder dgrad launch (compact encoder), in the last weight-gradient launch (conv encoder) or get their own
  const bool fin_rides = L.enc_compact || (ab_fin && L.enc_conv && !L.enc_ext);
  if (!fin_rides) PV_TRY(finish_scalars(fin, s));
  PV_TRY(encoder_bwd(p, L, &st.wz, 1, s, fin_rides ? &fin : nullptr, adam, adam_done, st.chain, head_side));
  return extra_outputs(p, L, L.dzc, plan_lat_in(p), s);
}

// the step's launch sequence
int loss_and_grads_fused(const pv_ivae_plan* p, const Layout& L, const ObjArgs& obj, int want_grads, hipStream_t s,
                         const PvAdamFuse* adam = nullptr, bool* adam_done = nullptr) {
  const int64_t K = plan_K(p), lat_in = plan_lat_in(p);
  if (p->fc_latent.in_dim != lat_in) return PV_EINVAL;
  if (K > 0 && !L.enc_compact) return PV_EINVAL;
  const bool cat_in = p->c_dim > 0 || K > 0;         // the decoder's latent input is a materialised concatenation
  FusedStep st{p, L, obj, want_grads != 0, s, cat_in ? L.zy : L.z + (p->z_dim - p->latent_dim), cat_in ? lat_in : (int64_t)p->z_dim,
               want_grads ? L.dec : layout_choice(p, L.rows, false)};
  fused_decoder_args(st);
  PV_TRY(fused_guide(st));
  if (L.renyi && want_grads) PV_TRY(fused_renyi_forward(st));
  if (want_grads) fused_closing_form(st, adam, adam_done);
  PV_TRY(fused_decoder_launch(st));
  return want_grads ? fused_close(st, adam, adam_done) : fused_close_forward(st);
}

int loss_and_grads_layered(const pv_ivae_plan* p, const Layout& L, const ObjArgs& obj, int want_grads, hipStream_t s) {
  const int64_t K = plan_K(p);
  // N: rows per sample of the spatial decoder (positions; Cn channels each) or the vanilla decoder's output width
  const int64_t B = p->batch, N = plan_pos(p), Cn = plan_C(p), R = L.rows, z = p->z_dim;
  const int64_t S = step_S(p, L);                    // decoder samples (jiVAE: K per input, ordered [k][b]; multi-particle: [p][b])
  const int P = L.P;
  const int64_t reps = K > 0 ? K : P;                // decoder passes against the same B observations
  const int64_t lat_in = plan_lat_in(p);
  float* G = p->grads;
  void* ws = L.scratch;
  const int64_t wsb = L.scratch_bytes;
  const int nd = p->n_dec;

  // ---------------- forward ----------------
  if (P > 1) PV_TRY(particle_guide(p, L, s, nullptr, 0.0f, nullptr));
  else PV_TRY(guide_fwd(p, L, s));
  const bool sampled = K > 0 && p->class_onehot != nullptr;       // jiVAE without enumeration (plan->class_onehot)
  if (sampled) {
    if (p->coord_dim > 0) return PV_EINVAL;
    PV_TRY(pv_jiv_sampled_prep(L.alpha, p->class_onehot, L.sw, L.jfix, p->beta_disc, (int)B, (int)K, s));
  }
  const int coord = (int)(z - p->latent_dim);
  const bool cat_in = p->c_dim > 0 || K > 0;
  const float* zin = cat_in ? L.zy : (p->coord_dim > 0 ? L.z + coord : L.z);
  const int64_t ldz = cat_in ? lat_in : z;
  PV_TRY(decoder_hidden_fwd(p, L, zin, ldz, lat_in, s));

  float* cur = L.dbuf[0];      // dL/d(pre-activation) of the layer being processed
  float* oth = L.dbuf[1];
  const float* hlast = L.dact[nd - 1];
  const int Hl = p->dec[nd - 1].out_dim;
  // Renyi bound: sw is known only once every sample's ll is — the likelihood pass that forms ll and the one that applies sw to
  // dL/dlogit run apart, with the weights kernel between them (below)
  const bool renyi = L.renyi;
  PvOutLik o{};
  if (p->coord_dim > 0) {
    o.h = hlast; o.hpre = L.dpre_[nd - 1]; o.ldh = Hl; o.wo = p->params + p->out.w_off;
    o.bo = bias_of(p->params, p->out); o.x = p->x; o.loc = p->loc; o.llrow = L.llrow;
    o.dpre = (want_grads && !renyi) ? cur : nullptr; o.part_dwo = L.part_dwo; o.part_dbo = L.part_dbo; o.M = R; o.H = Hl;
    o.lik = p->lik; o.sigmoid_out = p->sigmoid_out; o.act_last = p->dec[nd - 1].act; o.sig = p->decoder_sig;
    o.sw = reps > 1 ? L.sw : p->row_w; o.N = (int)N; o.xmod = reps > 1 ? B * N : 0;
    o.pw = obj.pw; o.pw_img = obj.pw_img ? 1 : 0;
    PV_TRY(Cn > 1 ? pv_out_lik_mc(o, (int)Cn, s) : pv_out_lik(o, s));
  } else {
    // oth <- dL/dlogits (R, N); jiVAE: one pass per enumerated class against the same observations, rows then
    // weighted by alpha (the decoder's gradients become the enumerated expectation)
    // (multi-particle: one pass per particle, rows weighted 1/P)
    for (int64_t k = 0; k < reps; ++k)
      PV_TRY(pv_lik_elem(L.logits + k * B * N, p->x, B * N, p->lik, p->sigmoid_out, p->decoder_sig,
                         p->loc ? p->loc + k * B * N : nullptr, L.llrow + k * B * N, want_grads ? oth + k * B * N : nullptr, s,
                         obj.pw, N, obj.pw_img, plan_group(p)));
    if (reps > 1 && want_grads && !renyi) PV_TRY(pv_scale_rows(oth, L.sw, R, N, s));
    if (K == 0 && p->row_w && want_grads) PV_TRY(pv_scale_rows(oth, p->row_w, R, N, s));
  }
  if (K > 0) {
    PV_TRY(pv_segsum(L.llrow, S, N, L.llkb, s));
    // (the drawn class's score-function term -log_r (onehot - alpha) carries ll_b itself: the per-image normaliser goes in here)
    if (sampled && p->lik == PV_LIK_POISSON_LOG) PV_TRY(pv_poisson_lognorm_rows(p->x, B, N, L.llkb, (int)K, s));
    if (!want_grads && sampled)
      PV_TRY(pv_jiv_combine_sampled(L.llkb, L.alpha, p->class_onehot, L.llb, nullptr, 0, 0, nullptr, 0, (int)z, (int)B,
                                    (int)K, p->beta, p->beta_disc, 0, nullptr, nullptr, nullptr, s));
    else if (!want_grads) PV_TRY(pv_jiv_combine(L.llkb, L.alpha, L.llb, nullptr, 0, 0, nullptr, 0, (int)z, (int)B, (int)K,
                                           p->beta_disc, 0, s));
  } else if (P > 1) {                                // llb[b] = sum_p sw ll_pb
    PV_TRY(pv_segsum(L.llrow, S, N, L.llkb, s));
    if (renyi) {
      PV_TRY(renyi_weights(p, L, obj, s));
      if (want_grads && p->coord_dim > 0) {            // the second likelihood pass: dL/dpre and the output layer's partials
        o.dpre = cur; o.llrow = nullptr; o.loc = nullptr;
        PV_TRY(Cn > 1 ? pv_out_lik_mc(o, (int)Cn, s) : pv_out_lik(o, s));
      } else if (want_grads) {
        PV_TRY(pv_scale_rows(oth, L.sw, R, N, s));
      }
    }
    PvParticleBwd pf = particle_bwd_desc(p, L);
    pf.llkb = L.llkb; pf.fwd_only = 1;
    PV_TRY(pv_particle_bwd(pf, s));
  } else {
    PV_TRY(pv_segsum(L.llrow, B, N, L.llb, s));
    PV_TRY(weigh_llb(p, L, s));
  }
  if (K > 0 && want_grads) {
    // (llb is formed by pv_jiv_combine at the end of the decoder backward; the scalars are finished there)
  } else
  PV_TRY(pv_finish_scalars(L.llb, (int)B, p->scalars, (L.enc_compact || P > 1) ? L.kl_part : nullptr, P > 1 ? (int)B : L.kl_blocks,
                           1.0f /* partials come scaled */, s));
  if (!want_grads && sampled) PV_TRY(pv_jiv_sampled_fix(p->scalars, L.jfix, s));
  if (!want_grads) return extra_outputs(p, L, nullptr, lat_in, s);

  // ---------------- backward: decoder ----------------
  if (p->coord_dim > 0) {
    const int64_t ob = pv_out_lik_blocks(R);
    PV_TRY(pv_reduce_partials(L.part_dwo, (int)ob, Cn * Hl, G + p->out.w_off, Cn * Hl, s));
    if (p->out.b_off >= 0) PV_TRY(pv_reduce_partials(L.part_dbo, (int)ob, Cn, G + p->out.b_off, Cn, s));
  } else {
    // out layer of the vanilla decoder: logits = hlast Wout^T + bout
    PV_TRY(linear_wgrad(oth, N, hlast, Hl, G + p->out.w_off, bias_of(G, p->out), R, Hl, N,
                        ws, wsb, s));
    PV_TRY(linear_dgrad(oth, N, p->params + p->out.w_off, cur, Hl, hlast, L.dpre_[nd - 1], Hl, p->dec[nd - 1].act, R,
                        Hl, N, ws, wsb, s));
  }
  for (int i = nd - 1; i >= 0; --i) {
    const pv_layer& l = p->dec[i];
    const float* in; const float* inpre; int64_t ldin; int act_in;
    if (i > 0) { in = L.dact[i - 1]; inpre = L.dpre_[i - 1]; ldin = p->dec[i - 1].out_dim; act_in = p->dec[i - 1].act; }
    else if (p->coord_dim > 0) { in = L.h0; inpre = nullptr; ldin = p->fc_coord.out_dim; act_in = PV_ACT_TANH; }
    else { in = zin; inpre = nullptr; ldin = ldz; act_in = PV_ACT_NONE; }
    PV_TRY(linear_wgrad(cur, l.out_dim, in, ldin, G + l.w_off, bias_of(G, l), R, l.in_dim,
                        l.out_dim, ws, wsb, s));
    if (i > 0 || p->coord_dim > 0) {
      PV_TRY(linear_dgrad(cur, l.out_dim, p->params + l.w_off, oth, l.in_dim, in, inpre, ldin, act_in, R, l.in_dim,
                          l.out_dim, ws, wsb, s));
      float* t = cur; cur = oth; oth = t;
    } else {
      // vanilla decoder: dL/d(decoder latent input) (B, lat_in)
      PV_TRY(linear_dgrad(cur, l.out_dim, p->params + l.w_off, L.dzc, lat_in, nullptr, nullptr, 0, PV_ACT_NONE, R,
                          l.in_dim, l.out_dim, ws, wsb, s));
    }
  }
  if (p->coord_dim > 0) {
    // cur = dL/d(pre-tanh of coord_latent) (R, H0)
    const int H0 = p->fc_coord.out_dim;
    PvCoordLatBwd cb{};
    cb.dpre0 = cur; cb.grid = p->grid; cb.tp = L.tp; cb.Wc = p->params + p->fc_coord.w_off;
    cb.part_hz = L.part_hz; cb.part_wc = L.part_wc; cb.part_tp = L.part_tp;
    cb.N = (int)N; cb.cd = p->coord_dim; cb.H0 = H0; cb.rows_per_chunk = L.rows_per_chunk;
    PV_TRY(pv_coordlat_bwd(cb, L.nchunk, (int)S, s));
    const int np = (int)(S * L.nchunk);
    PV_TRY(pv_reduce_mid(L.part_hz, (int)S, L.nchunk, H0, L.dhz, s));
    PV_TRY(pv_reduce_partials(L.part_hz, np, H0, G + p->fc_coord.b_off, H0, s));
    PV_TRY(pv_reduce_partials(L.part_wc, np, (int64_t)H0 * p->coord_dim, G + p->fc_coord.w_off,
                              (int64_t)H0 * p->coord_dim, s));
    PV_TRY(pv_reduce_mid(L.part_tp, (int)S, L.nchunk, 4, L.dtp, s));
    // fc_latent: hz = zin Wz^T
    PV_TRY(linear_wgrad(L.dhz, H0, zin, ldz, G + p->fc_latent.w_off, nullptr, S, lat_in, H0, ws, wsb, s));
    PV_TRY(linear_dgrad(L.dhz, H0, p->params + p->fc_latent.w_off, L.dzc, lat_in, nullptr, nullptr, 0, PV_ACT_NONE, S,
                        lat_in, H0, ws, wsb, s));
  }

  if (K > 0) {
    // sum the K replicas' dL/dz, form ll_b and the class-logit gradients; then the loss scalars
    if (sampled)
      PV_TRY(pv_jiv_combine_sampled(L.llkb, L.alpha, p->class_onehot, L.llb, L.dzc, (int)lat_in, (int)(lat_in - K), L.dhead,
                                    (int)plan_head_w(p), (int)z, (int)B, (int)K, p->beta, p->beta_disc, 1, L.z, L.head,
                                    L.z_scale, s));
    else
    PV_TRY(pv_jiv_combine(L.llkb, L.alpha, L.llb, L.dzc, (int)lat_in, (int)(lat_in - K), L.dhead, (int)plan_head_w(p), (int)z,
                          (int)B, (int)K, p->beta_disc, 1, s, p->coord_dim > 0 ? L.dtp : nullptr));
    PV_TRY(pv_finish_scalars(L.llb, (int)B, p->scalars, L.enc_compact ? L.kl_part : nullptr, L.kl_blocks, 1.0f, s));
    if (sampled) PV_TRY(pv_jiv_sampled_fix(p->scalars, L.jfix, s));
  }
  if (P > 1) {                                       // the P samples' dL/dz reduced into the image's head gradient, then the encoder
    PvParticleBwd pb = particle_bwd_desc(p, L);
    pb.llkb = L.llkb; pb.dzc = L.dzc; pb.ldzc = lat_in; pb.dtp = p->coord_dim > 0 ? L.dtp : nullptr;
    PV_TRY(pv_particle_bwd(pb, s));
    return encoder_bwd(p, L, nullptr, 0, s);
  }
  return latent_encoder_bwd(p, L, lat_in, 4, 1, s);
}

}  // namespace

extern "C" int pv_version(void) { return PV_ABI_VERSION; }
extern "C" int pv_experiments_build(void) {
#ifdef PV_EXPERIMENTS
  return 1;
#else
  return 0;
#endif
}

// the plan pv_ivae_decode works on; jiVAE.decode(z, y) (jivae.py:255-267) is one decoder row block
// per given (z, one-hot class) pair — the class vector is a conditioning input there, not an enumeration axis
static pv_ivae_plan decode_plan(const pv_ivae_plan* plan) {
  pv_ivae_plan lay = *plan;
  if (lay.discrete_dim > 0) {
    lay.c_dim += lay.discrete_dim;
    lay.head.out_dim -= lay.discrete_dim;
    lay.discrete_dim = 0;
    lay.flags &= ~PV_PLAN_FUSED_TAIL;                  // (the bit does nothing for a discrete latent: its decode keeps today's kernels)
  }
  return lay;
}

static pv_ivae_plan guide_plan(const pv_ivae_plan* plan);
// several channels per position with an external decoder: refused (the guide plan below no longer knows the decoder); the
// categorical likelihood, which exists for several channels only, likewise (the guide plan would replace it by a per-value one)
static bool ext_decoder_channels(const pv_ivae_plan* plan) {
  return plan->ext_decoder && ((plan->coord_dim > 0 && plan->out.out_dim > 1) || plan->lik == PV_LIK_CATEGORICAL);
}

// the likelihood branch a forward-only launch borrows to turn logits into `loc`: the Gaussian one (sigmoid(a) or a) for every
// likelihood whose mean is that; the Poisson's own for its rate exp(min(a, 30)); the categorical's own for the class
// probabilities softmax(a)
static int loc_lik(const pv_ivae_plan* lay) {
  return (lay->lik == PV_LIK_POISSON_LOG || lay->lik == PV_LIK_CATEGORICAL) ? lay->lik : PV_LIK_GAUSSIAN;
}

// ---- forward-only decode on the fused spatial-decoder kernel (models/base.py:145-171) ----
// decode(z, angle, shift, scale) of an invariant model whose decoder the fused kernel is specialised for: the per-sample
// transform is the uniform (angle, scale, shift), hz = fc_latent(z), and the persistent kernel runs its forward half only
// and writes `loc` — no (B N) x 128 activation is materialised (the layered path needs 3 of them: 63 GB at B = 32768).
// Always at fp32-class precision (fused = 1: f32 matrix instructions; otherwise bf16 split precision), whatever the
// training precision: reconstructions are what parity is judged on.
struct DecodeLayout { float* tp; float* hz; float* wimg; float* xdummy; void* scratch; int64_t scratch_bytes, total; };
static bool decode_fused(const pv_ivae_plan* lay) { return lay->fused && lay->coord_dim > 0 && plan_fused_ok(lay); }
static void carve_decode(const pv_ivae_plan* lay, char* base, DecodeLayout& D) {
  Carver c{base, 0};
  const int64_t B = lay->batch, H0 = lay->fc_coord.out_dim, lat_in = plan_lat_in(lay);
  D.tp = c.take(B * 8);
  D.hz = c.take(B * H0);
  D.wimg = c.take(FB_WIMG_BYTES / (int64_t)sizeof(float));
  D.xdummy = c.take(FD_UNIT);
  D.scratch_bytes = pv_align_up(lat_in > 16 ? gemm_ws_need(B, H0, lat_in) : 0, 256);
  D.scratch = base ? (void*)(base + c.off) : nullptr;
  c.off += D.scratch_bytes;
  D.total = c.off;
}
static int decode_fused_run(const pv_ivae_plan* lay, const float* z, float angle, float shift_x, float shift_y, float scale,
                            float* loc, hipStream_t s) {
  DecodeLayout D;
  carve_decode(lay, (char*)lay->ws, D);
  if (lay->ws_bytes < D.total) return PV_EWS;
  const int64_t B = lay->batch, N = plan_rows(lay), lat_in = plan_lat_in(lay);      // N: rows per sample
  const int H = FD_H;
  if (lay->fc_latent.in_dim != lat_in) return PV_EINVAL;
  PV_TRY(pv_fill_tp(D.tp, (int)B, angle, scale, shift_x, shift_y, s));
  if (lat_in <= 16) PV_TRY(pv_smallk_linear(z, lat_in, lay->params + lay->fc_latent.w_off, D.hz, B, (int)lat_in, H, s));
  else PV_TRY(linear_fwd(z, lat_in, lay->params + lay->fc_latent.w_off, nullptr, D.hz, nullptr, H, B, lat_in, H, PV_ACT_NONE,
                         D.scratch, D.scratch_bytes, s));
  hipError_t e = hipMemsetAsync(D.xdummy, 0, FD_UNIT * sizeof(float), s);
  if (e != hipSuccess) return (int)e;
  PvFused f{};
  f.x = D.xdummy; f.x_units = 1;                       // (no observations: every unit reads the same 16 zeros)
  f.grid = lay->grid; f.tp = D.tp; f.hz = D.hz;
  fused_weights(f, lay);
  f.llrow = nullptr; f.loc = loc; f.wimg = D.wimg;
  f.M = B * N; f.units = f.M / FD_UNIT; f.N = (int)N; f.cd = lay->coord_dim; f.B = (int)B;
  f.n_obs = pv_sdec_fused_tail(lay) ? (int)plan_pos(lay) : 0;      // (loc is (B, positions, C): the padding rows write nothing)
  f.lik = loc_lik(lay); f.sigmoid_out = lay->sigmoid_out; f.sig = 1.0f;         // loc = sigmoid(a) or a (Poisson: exp(a))
  f.sel = lay->dec_kernel;                             // (forward-only: no fp16 build, the parent's selection for every likelihood)
  const int grid = pv_sdec_fused_grid(f.units);
  if (plan_fused_mc(lay)) {                            // loc is (B, N, C); no observations at all (x null: zeros)
    f.x = nullptr; f.x_units = 0; f.wimg = nullptr;
    return pv_sdec_fused_mc_launch(f, (int)plan_C(lay), grid, false, s);
  }
  if (lay->fused == 1) return pv_sdec_fused_launch(f, grid, false, s);
  f.hz_scale = 0.0f;                                   // hz is written unscaled here; the 8-wave kernels scale it themselves
  // The other resolution: decode promises fp32-class output in every bf16-class mode, so fused == 3 too takes the split-precision
  // kernels (resolved as fused = 2), and — forward-only, no fp16 build to keep a Poisson plan away from — the plan's own dec_kernel, not plan_sel
  const PvDecChoice c = pv_sdec_fused_choice(2, f.units, false, lay->dec_kernel);
  PV_TRY(pv_sdec_fused_bf16_prep(f, false, c, s));     // weight images, pre-scaled or not as the launch below reads them
  return pv_sdec_fused_bf16_launch(f, grid, false, c, s);
}

// what: PV_WS_ALL = enough for every entry point at this batch; PV_WS_STEP / _ENCODE / _DECODE = for that call alone
// (the training step's fused layout is far smaller than the layered one pv_ivae_decode uses at the same batch)
extern "C" int64_t pv_ivae_workspace_bytes_for(const pv_ivae_plan* plan, int what) {
  if (what < PV_WS_ALL || what > PV_WS_DECODE) return PV_EINVAL;
  if (plan && plan->ext_decoder) {                       // only the guide half runs in the library
    const pv_ivae_plan q = guide_plan(plan);
    if (!valid_plan(&q) || ext_decoder_channels(plan)) return PV_EINVAL;
    Layout L;
    carve(&q, nullptr, L, what == PV_WS_ENCODE, what == PV_WS_ENCODE);
    return L.total;
  }
  if (!valid_plan(plan)) return PV_EINVAL;
  Layout L;
  int64_t total = 0;
  if (what == PV_WS_ALL || what == PV_WS_STEP) {
    carve(plan, nullptr, L);
    total = L.total;
  }
  if (what == PV_WS_ALL || what == PV_WS_ENCODE) {   // encode / decode always use the layered layout, B samples
    pv_ivae_plan q = *plan;
    q.fused = 0;
    carve(&q, nullptr, L, true, true);
    if (L.total > total) total = L.total;
  }
  if (what == PV_WS_ALL || what == PV_WS_DECODE) {
    pv_ivae_plan q = decode_plan(plan);
    if (decode_fused(&q)) {
      DecodeLayout D;
      carve_decode(&q, nullptr, D);
      if (D.total > total) total = D.total;
    } else {
      carve(&q, nullptr, L, true);
      if (L.total > total) total = L.total;
    }
  }
  return total;
}

extern "C" int64_t pv_ivae_workspace_bytes(const pv_ivae_plan* plan) { return pv_ivae_workspace_bytes_for(plan, PV_WS_ALL); }

extern "C" int pv_ivae_uses_fused(const pv_ivae_plan* plan) {
  return valid_plan(plan) && plan->fused && plan_fused_ok(plan) ? 1 : 0;
}

extern "C" int pv_ivae_guide_folds(const pv_ivae_plan* plan) {
  if (!valid_plan(plan) || !plan->fused || !pv_sdec_fused_supported(plan)) return 0;
  Layout L;
  carve(plan, nullptr, L);                             // (offsets only: nothing is dereferenced)
  if (!L.fused || !plan_guide_may_fold(plan, L)) return 0;
  PvFused f{};
  f.M = L.rows; f.units = L.rows / FD_UNIT; f.N = plan->n_pix; f.B = (int)plan_S(plan);
  return L.dec.hosts_guide && pv_sdec_fused_w8_fold_ok(f, L.f_grid) ? 1 : 0;
}

// test hook (not in include/; pv_convstack.h: conv_trace): offsets into plan->ws of the conv encoder's stored activations and
// max-pool winners after a pv_ivae_loss_and_grads call — tests/test_gpu_parity.py compares gradients with the float64 oracle
// under the HIP forward's own decisions and counts the decisions that differ
extern "C" int pv_debug_ivae_conv_trace(const pv_ivae_plan* plan, int64_t* out) {
  if (!valid_plan(plan) || !plan->ws || !out || plan->n_enc_ops <= 0) return PV_EINVAL;
  Layout L;
  carve(plan, (char*)plan->ws, L);
  if (!L.enc_conv || L.cF < 0 || plan->ws_bytes < L.total) return PV_EINVAL;
  pvcs::conv_trace(plan->enc_ops, plan->n_enc_ops, plan->enc_ndim, plan->batch, L.ces, L.cea, L.ccode, L.ccode2,
                   (const char*)plan->ws, out);
  return 0;
}

// Poisson plans: the data-only normaliser C = sum lgamma(x + 1) into the finished scalars ([1] -= C, [0] += C): two small trailing
// launches on the caller's stream (partial sums, then their fixed-order sum), after the step's own launches and before anything
// reads the scalars.  The same
// correction for every objective (C does not depend on the latent sample).  The sampled-class jiVAE objective is the exception:
// its score-function term needs the per-image value, which went into llkb in front of pv_jiv_combine_sampled (nothing to do here).
static int poisson_lognorm(const pv_ivae_plan* plan, const Layout& L, const ObjArgs& o, hipStream_t s) {
  if (plan->lik != PV_LIK_POISSON_LOG || (plan_K(plan) > 0 && plan->class_onehot)) return 0;
  return pv_poisson_lognorm(plan->x, (int64_t)plan->batch * plan->n_pix, L.pl_part, plan->scalars, s, o.pw, plan->n_pix, o.pw_img);
}

// ---- external decoder (plan->ext_decoder): the library's half of the step works on a copy of the plan whose decoder is
// a placeholder vanilla one (all of z is "content": no transform parameters, no fc_latent product)
static pv_ivae_plan guide_plan(const pv_ivae_plan* plan) {
  pv_ivae_plan q = *plan;
  q.fused = 0; q.coord_dim = 0; q.has_r = q.has_t = q.has_s = 0; q.latent_dim = q.z_dim;
  q.lik = PV_LIK_GAUSSIAN; q.sigmoid_out = 1;
  q.n_dec = 1;
  q.dec[0] = pv_layer{q.z_dim + q.c_dim, 16, PV_ACT_NONE, 0, 0, -1};
  q.out = pv_layer{16, q.n_pix, PV_ACT_NONE, 0, 0, -1};
  q.row_w = nullptr; q.row_elbo = nullptr; q.dy = nullptr;
  return q;
}

extern "C" int pv_ivae_guide(const pv_ivae_plan* plan, void* stream) {
  PV_RANGE("pv_ivae_guide");
  if (!plan || !plan->ext_decoder || plan->discrete_dim > 0 || plan->row_w || plan->row_elbo || plan->dy) return PV_EINVAL;
  if (ext_decoder_channels(plan)) return PV_EINVAL;
  const pv_ivae_plan q = guide_plan(plan);
  if (!valid_plan(&q) || !q.params || !q.x || !q.eps || !q.scalars || !q.ws || !q.ext_z) return PV_EINVAL;
  if (q.ext_encoder && !q.ext_head) return PV_EINVAL;
  Layout L;
  carve(&q, (char*)q.ws, L);
  if (q.ws_bytes < L.total) return PV_EWS;
  hipStream_t s = (hipStream_t)stream;
  PV_TRY(guide_fwd(&q, L, s));
  hipError_t e = hipMemcpyAsync(q.ext_z, L.z, (size_t)q.batch * q.z_dim * sizeof(float), hipMemcpyDeviceToDevice, s);
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int pv_ivae_guide_backward(const pv_ivae_plan* plan, int want_grads, void* stream) {
  PV_RANGE("pv_ivae_guide_backward");
  if (!plan || !plan->ext_decoder || plan->discrete_dim > 0 || ext_decoder_channels(plan)) return PV_EINVAL;
  const pv_ivae_plan q = guide_plan(plan);
  if (!valid_plan(&q) || !q.params || !q.eps || !q.scalars || !q.ws || !q.ext_ll) return PV_EINVAL;
  if (want_grads && (!q.ext_dz || (!q.ext_encoder && !q.grads) || (q.ext_encoder && !q.ext_dhead))) return PV_EINVAL;
  Layout L;
  carve(&q, (char*)q.ws, L);
  if (q.ws_bytes < L.total) return PV_EWS;
  hipStream_t s = (hipStream_t)stream;
  // scalars[1] = sum log p(x|z) from the caller; [2], [3] from the guide (kernel partials on the compact encoder path)
  PV_TRY(pv_finish_scalars(q.ext_ll, 1, q.scalars, L.enc_compact ? L.kl_part : nullptr, L.kl_blocks, 1.0f, s));
  if (!want_grads) return 0;
  L.dzc = const_cast<float*>(q.ext_dz);                // d(-ll)/dz for every column of z
  return latent_encoder_bwd(&q, L, q.z_dim, 4, 1, s);
}

// ---- per-observation weights of the likelihood (v17, added without a layout change; include/pyroved_amd.h) ----
// loss = -( sum_b sum_i w_i log p(x_bi | z_b) + beta sum_b [log p(z_b) - log q(z_b | x_b)] ), w (n_pix) shared by all images.
// Scope: the one-particle ELBO (either KL form) of the fc-encoder iVAE, spatial or vanilla decoder, every likelihood
// PV_PLAN_FAST_WEIGHTS takes effect: one channel, the fused kernels' architecture, a bf16-class `fused`, no build asked for by name
// but the 4-wave bf16 one (dec_kernel 1) — the weighted instances of pv_sdec_fused_bf16.hip's 4-wave kernel take the decoder
static bool weighted_fast(const pv_ivae_plan* p) {
  return (p->flags & PV_PLAN_FAST_WEIGHTS) && p->coord_dim > 0 && p->out.out_dim == 1 && pv_sdec_fused_supported(p) &&
         (p->fused == 2 || p->fused == 3) && (p->dec_kernel == 0 || p->dec_kernel == 1);
}
static bool weighted_scope(const pv_ivae_plan* p) {
  if (!(valid_plan(p) && p->discrete_dim == 0 && p->n_enc_ops == 0 && !p->ext_encoder && !p->ext_decoder && !p->row_w &&
        !p->row_elbo && !p->dy && !p->class_onehot))
    return false;
  if ((p->flags & PV_PLAN_FAST_WEIGHTS) && p->dec_kernel > 1) return false;      // (the fp16 builds, the 8-wave kernel: no weighted form)
  return p->fused != 3 || weighted_fast(p);
}
// The plan a weighted call runs: the caller's with `fused` rewritten to the kernel family that has a weighted form — 1 where the
// weighted instances of the fused f32 kernel take the decoder (one channel asked with fused 1 or 2: fused = 2 promises fp32-class
// results and the f32 kernel delivers them; several channels as the unweighted plan decides: PV_PLAN_FUSED_CHANNELS and fused == 1),
// 0 (the layer-by-layer kernels) everywhere else.  The fp16-piece decoder kernels and the 8-wave bf16 kernel have no weighted form;
// the 4-wave kernel's bf16 builds have one, taken on request (weighted_fast): `fused` stays, dec_kernel = 1 names that kernel for
// every launch of the step at every size, and the guide keeps a launch of its own (the kernel that could host it is the 8-wave one)
// (per_image: pv_ivae_weighted_images_* — the same routing over the per-image instances' list, which today is the same list)
static pv_ivae_plan weighted_route(const pv_ivae_plan* p, bool per_image = false) {
  pv_ivae_plan q = *p;
  // (PV_PLAN_FUSED_TAIL is the caller's fused == 1 alone: a fused == 2 plan that routes to the f32 kernel below answers as without the bit)
  if (p->fused != 1) q.flags &= ~PV_PLAN_FUSED_TAIL;
  if (weighted_fast(p)) {
    q.dec_kernel = 1;
    q.flags |= PV_PLAN_NO_ENC_FOLD;
    return q;
  }
  if (q.fused == 2 && q.coord_dim > 0 && q.out.out_dim == 1) q.fused = 1;
  if (!(q.fused == 1 && pv_sdec_fused_mc_weighted_supported(&q, per_image) && plan_fused_ok(&q))) q.fused = 0;
  return q;
}
extern "C" int pv_ivae_weighted_uses_fused(const pv_ivae_plan* plan) {
  if (!weighted_scope(plan)) return 0;
  const pv_ivae_plan q = weighted_route(plan);
  return (q.fused == 1 || weighted_fast(plan)) ? 1 : 0;
}
// test hook (not in include/), in the style of pv_debug_decoder_kernel_name: the decoder kernel a weighted call of the plan launches,
// spelled the way rocprofv3 prints it (per_image: pv_ivae_weighted_images_*; grads: the gradient call / the forward-only one)
extern "C" const char* pv_debug_weighted_decoder_kernel_name(const pv_ivae_plan* plan, int per_image, int grads) {
  if (!weighted_scope(plan)) return "";
  if (weighted_fast(plan)) return pv_sdec_fused_bf16_wt_kernel_name(plan->fused == 2, grads, plan->lik);
  const pv_ivae_plan q = weighted_route(plan, per_image != 0);
  if (q.fused != 1) return "pv_gemm_kernel (layer-by-layer path)";
  static thread_local char buf[96];
  snprintf(buf, sizeof buf, "void pv_sdec_fused_mc%s_kernel<%s, %d, %d>(PvFused)", pv_sdec_fused_tail(&q) ? "_tail" : "",
           grads ? "true" : "false", (int)plan_C(&q), per_image ? PV_FDM_W_IMAGES : PV_FDM_W_SHARED);
  return buf;
}

// test hook (not in include/), in the same style: the decoder kernel a call of a PV_LIK_CATEGORICAL plan launches — weighted: 0 the
// unweighted entry points, 1 pv_ivae_weighted_*, 2 pv_ivae_weighted_images_*; '' for a plan those calls refuse
extern "C" const char* pv_debug_categorical_decoder_kernel_name(const pv_ivae_plan* plan, int weighted, int grads) {
  if (!plan || weighted < 0 || weighted > 2 || plan->lik != PV_LIK_CATEGORICAL) return "";
  if (weighted ? !weighted_scope(plan) : !valid_plan(plan)) return "";
  const pv_ivae_plan q = weighted ? weighted_route(plan, weighted == 2) : *plan;
  static thread_local char buf[160];
  if (!(q.fused == 1 && plan_fused_mc(&q))) {            // the likelihood launch of the layer-by-layer path
    if (q.coord_dim > 0) snprintf(buf, sizeof buf, "void pv_out_lik_mc_cat_kernel<%d>(PvOutLik) (layer-by-layer path)", plan_group(&q));
    else snprintf(buf, sizeof buf, "void pv_lik_elem_cat_kernel<%d>(float const*, float const*, long, float*, float*, float*, float const*, long) "
                  "(layer-by-layer path)", plan_group(&q));
    return buf;
  }
  snprintf(buf, sizeof buf, "void pv_sdec_fused_mc_cat_kernel<%s, %d, %d>(PvFused)", grads ? "true" : "false", (int)plan_C(&q), weighted);
  return buf;
}

// ---- the importance-weighted (Renyi / IWAE) bound (v17, added without a layout change; include/pyroved_amd.h) ----
// everything the multi-particle objective refuses, at every P; the sampled KL form only (the analytic one has no per-sample weight)
static bool renyi_ok(const pv_ivae_plan* plan, int32_t P, float alpha) {
  return P >= 1 && P <= PV_RENYI_MAX_P && std::isfinite(alpha) && alpha != 1.0f && valid_plan(plan) && particles_supported(plan) &&
         plan->kl_mode == PV_KL_SAMPLED;
}

// ---- one resolution of (plan, objective) behind the workspace query and the two calls (include/pyroved_amd.h: pv_ivae_objective) ----
struct Resolved {
  const pv_ivae_plan* plan; pv_ivae_plan routed;   // the plan to run: the caller's, or the copy a route made (`routed`)
  Layout L; ObjArgs o;
  float* ones;                                      // Renyi bound with ONE particle: the caller's weights_out — the bound is the ELBO,
};                                                  // the one weight per image is 1, written behind the step's launches
// Validates the descriptor alone and against the plan, routes, carves; PV_EINVAL before any
// pointer is touched.  call == false: the workspace query (offsets only: r.L.total), call == true: a call that runs — the plan's
// buffers are checked as well (want_grads: the gradient buffers too), the workspace's size last (PV_EWS).
static int resolve(const pv_ivae_plan* plan, const pv_ivae_objective& d, bool call, int want_grads, Resolved& r) {
  const int P = d.num_particles;
  const bool renyi = d.bound == PV_BOUND_RENYI, per_image = d.obs_w_kind == PV_OBS_W_PER_IMAGE;
  const bool weighted = d.obs_w_kind == PV_OBS_W_SHARED || per_image;
  if ((!renyi && d.bound != PV_BOUND_ELBO) || (!weighted && d.obs_w_kind != PV_OBS_W_NONE) || P < 1) return PV_EINVAL;
  // combinations no kernel path exists for: weights with several particles or the Renyi bound; the bound's output without the bound
  if ((weighted && (P > 1 || renyi)) || (!renyi && d.weights_out) || (call && weighted && !d.obs_w)) return PV_EINVAL;
  if (renyi && !renyi_ok(plan, P, call ? d.alpha : 0.0f)) return PV_EINVAL;      // (the query does not see alpha)
  r.plan = plan;
  if (weighted) {
    if (!weighted_scope(plan)) return PV_EINVAL;
    r.routed = weighted_route(plan, per_image);
    r.plan = &r.routed;
  } else if (plan && plan->ext_decoder) {           // only the guide half runs in the library (pv_ivae_guide / pv_ivae_guide_backward):
    if (call || ext_decoder_channels(plan)) return PV_EINVAL;                     // no step, and PV_WS_STEP is that half's layout
    r.routed = guide_plan(plan);
    r.plan = &r.routed;
  }
  const pv_ivae_plan* p = r.plan;
  // (a weighted route's copy — the caller's plan passed weighted_scope — is validated by the calls only: a dec_kernel naming a
  //  bf16-class build is PV_EINVAL on the f32 kernel the route chose, while the query has always answered with that plan's size)
  if (((call || !weighted) && !valid_plan(p)) || (P > 1 && !particles_supported(p))) return PV_EINVAL;
  if (call) {
    if (!p->params || !p->x || !p->eps || !p->scalars || !p->ws || (want_grads && !p->grads)) return PV_EINVAL;
    if (p->ext_encoder && (!p->ext_head || (want_grads && !p->ext_dhead))) return PV_EINVAL;
    if (p->coord_dim > 0 && !p->grid) return PV_EINVAL;
  }
  carve(p, call ? (char*)p->ws : nullptr, r.L, false, false, P, renyi);
  if (call && p->ws_bytes < r.L.total) return PV_EWS;
  r.o = ObjArgs{};
  if (r.L.renyi) { r.o.alpha = d.alpha; r.o.wout = d.weights_out; }
  if (weighted) { r.o.pw = d.obs_w; r.o.pw_img = per_image; }
  r.ones = (renyi && P == 1) ? d.weights_out : nullptr;
  return 0;
}
static int one_particle_weights(const Resolved& r, void* stream) {
  if (!r.ones) return 0;
  const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)r.ones, 0x3f800000 /* 1.0f */, (size_t)r.plan->batch, (hipStream_t)stream);
  return e == hipSuccess ? 0 : (int)e;
}

static int64_t workspace_bytes_impl(const pv_ivae_plan* plan, const pv_ivae_objective& d) {
  Resolved r;
  const int e = resolve(plan, d, false, 0, r);
  return e ? e : r.L.total;
}

// the step's launches without the optimizer
static int launches(const Resolved& r, int want_grads, hipStream_t s) {
  const pv_ivae_plan* p = r.plan;
  // the sampled-class objective (Trace_ELBO on a drawn class) exists for the vanilla decoder only — the reference's own model
  // cannot run it with invariances (models/jivae.py:181-189) — and only the layer-by-layer path implements it
  if (p->class_onehot && (r.L.fused || p->coord_dim > 0)) return PV_EINVAL;
  if (r.L.fused) PV_TRY(loss_and_grads_fused(p, r.L, r.o, want_grads, s));
  else PV_TRY(loss_and_grads_layered(p, r.L, r.o, want_grads, s));
  return poisson_lognorm(p, r.L, r.o, s);
}
static int loss_and_grads_impl(const pv_ivae_plan* plan, const pv_ivae_objective& d, int want_grads, void* stream) {
  Resolved r;
  PV_TRY(resolve(plan, d, true, want_grads, r));
  PV_TRY(launches(r, want_grads, (hipStream_t)stream));
  return one_particle_weights(r, stream);
}

// SVI.step in one call.  On the fused-decoder path with the compact encoder or a conv encoder the Adam update rides in the last
// gradient launch (pv_wgrad.hip: every element is updated by whoever finalises its gradient; bit-identical to
// pv_ivae_loss_and_grads + pv_adam_step, one launch fewer); everywhere else it is exactly that pair of calls.
static int step_impl(const pv_ivae_plan* plan, const pv_ivae_objective& d, void* stream) {
  Resolved r;
  PV_TRY(resolve(plan, d, true, 1, r));
  const pv_ivae_plan* p = r.plan;
  hipStream_t s = (hipStream_t)stream;
  bool done = false;
  // extra outputs (dy, row_elbo) are computed AFTER the encoder backward from the first-layer weights: with Adam
  // riding in that launch they would see the updated weights — such plans take the two-call sequence
  if (p->adam_m && p->adam_v && p->adam_step >= 1 && p->n_params > 0 && !p->ext_encoder && !p->dy && !p->row_elbo &&
      r.L.fused && (r.L.enc_compact || r.L.enc_conv)) {  // (conv encoder: in the launch of fc_latent's weight gradient, the step's last)
    const double bc1 = 1.0 - pow((double)p->adam_beta1, (double)p->adam_step);
    const double bc2 = 1.0 - pow((double)p->adam_beta2, (double)p->adam_step);
    const PvAdamFuse ad{p->params, p->grads, p->adam_m, p->adam_v, p->n_params, p->adam_beta1,
                        p->adam_beta2, p->adam_eps, (float)((double)p->lr / bc1), (float)sqrt(bc2)};
    PV_TRY(loss_and_grads_fused(p, r.L, r.o, 1, s, &ad, &done));
    PV_TRY(poisson_lognorm(p, r.L, r.o, s));
  } else {
    PV_TRY(launches(r, 1, s));
  }
  if (!done)
    PV_TRY(pv_adam_step(p->params, p->grads, p->adam_m, p->adam_v, p->n_params, p->lr, p->adam_beta1, p->adam_beta2, p->adam_eps,
                        p->adam_step, stream));
  return one_particle_weights(r, stream);
}

// ---- the entry points: every public function opens its own range and hands its objective to the three functions above ----
// (a null descriptor is the plain one-particle ELBO)
static const pv_ivae_objective plain_obj = {1, PV_BOUND_ELBO, 0.0f, PV_OBS_W_NONE, nullptr, nullptr};
static pv_ivae_objective particles_obj(int32_t P) { return {P, PV_BOUND_ELBO, 0.0f, PV_OBS_W_NONE, nullptr, nullptr}; }
static pv_ivae_objective renyi_obj(int32_t P, float alpha, float* weights_out) {
  return {P, PV_BOUND_RENYI, alpha, PV_OBS_W_NONE, nullptr, weights_out};
}
// (a null weight pointer is the plain call)
static pv_ivae_objective weights_obj(int kind, const float* w) { return {1, PV_BOUND_ELBO, 0.0f, w ? kind : PV_OBS_W_NONE, w, nullptr}; }

extern "C" int64_t pv_ivae_objective_workspace_bytes(const pv_ivae_plan* plan, const pv_ivae_objective* objective) {
  return workspace_bytes_impl(plan, objective ? *objective : plain_obj);
}
extern "C" int pv_ivae_objective_loss_and_grads(const pv_ivae_plan* plan, const pv_ivae_objective* objective, int want_grads,
                                                void* stream) {
  PV_RANGE("pv_ivae_objective_loss_and_grads");
  return loss_and_grads_impl(plan, objective ? *objective : plain_obj, want_grads, stream);
}
extern "C" int pv_ivae_objective_step(const pv_ivae_plan* plan, const pv_ivae_objective* objective, void* stream) {
  PV_RANGE("pv_ivae_objective_step");
  return step_impl(plan, objective ? *objective : plain_obj, stream);
}

extern "C" int pv_ivae_loss_and_grads(const pv_ivae_plan* plan, int want_grads, void* stream) {
  PV_RANGE("pv_ivae_loss_and_grads");
  return loss_and_grads_impl(plan, plain_obj, want_grads, stream);
}
extern "C" int pv_ivae_step(const pv_ivae_plan* plan, void* stream) {
  PV_RANGE("pv_ivae_step");
  return step_impl(plan, plain_obj, stream);
}

extern "C" int64_t pv_ivae_particles_workspace_bytes(const pv_ivae_plan* plan, int32_t num_particles) {
  return workspace_bytes_impl(plan, particles_obj(num_particles));
}
extern "C" int pv_ivae_particles_loss_and_grads(const pv_ivae_plan* plan, int32_t num_particles, int want_grads, void* stream) {
  PV_RANGE("pv_ivae_particles_loss_and_grads");
  return loss_and_grads_impl(plan, particles_obj(num_particles), want_grads, stream);
}
extern "C" int pv_ivae_particles_step(const pv_ivae_plan* plan, int32_t num_particles, void* stream) {
  PV_RANGE("pv_ivae_particles_step");
  return step_impl(plan, particles_obj(num_particles), stream);
}

extern "C" int64_t pv_ivae_renyi_workspace_bytes(const pv_ivae_plan* plan, int32_t num_particles) {
  return workspace_bytes_impl(plan, renyi_obj(num_particles, 0.0f, nullptr));
}
extern "C" int pv_ivae_renyi_loss_and_grads(const pv_ivae_plan* plan, int32_t num_particles, float alpha, int want_grads,
                                            float* weights_out, void* stream) {
  PV_RANGE("pv_ivae_renyi_loss_and_grads");
  return loss_and_grads_impl(plan, renyi_obj(num_particles, alpha, weights_out), want_grads, stream);
}
extern "C" int pv_ivae_renyi_step(const pv_ivae_plan* plan, int32_t num_particles, float alpha, float* weights_out, void* stream) {
  PV_RANGE("pv_ivae_renyi_step");
  return step_impl(plan, renyi_obj(num_particles, alpha, weights_out), stream);
}

// ---- held-out log-evidence (v17, added without a layout change; include/pyroved_amd.h) ----
// One chunk of P particles of the plan's batch: the launches of the {P, PV_BOUND_RENYI} forward-only call up to the per-sample ll,
// then — instead of the bound's weights and scalars — the chunk's log-weights and the running state per image.
// Scope: what that objective accepts, at every P in 1 .. PV_RENYI_MAX_P; the plan's kl_mode is not consulted (a log-weight is a
// sampled quantity) and runs as PV_KL_SAMPLED; loc is ignored.
static bool evidence_ok(const pv_ivae_plan* plan, int32_t P) {
  return P >= 1 && P <= PV_RENYI_MAX_P && valid_plan(plan) && particles_supported(plan);
}
static pv_ivae_plan evidence_plan(const pv_ivae_plan* plan) {
  pv_ivae_plan q = *plan;
  q.kl_mode = PV_KL_SAMPLED; q.loc = nullptr;
  return q;
}
// the P*B samples' log p(x_b | z_pb) into L.llkb, layer by layer ...
static int evidence_ll_layered(const pv_ivae_plan* p, const Layout& L, hipStream_t s) {
  const int64_t B = p->batch, N = plan_pos(p), Cn = plan_C(p), z = p->z_dim, S = step_S(p, L), lat_in = plan_lat_in(p);
  const int nd = p->n_dec;
  PV_TRY(particle_guide(p, L, s, nullptr, 0.0f, nullptr));
  const bool cat_in = p->c_dim > 0;
  const float* zin = cat_in ? L.zy : (p->coord_dim > 0 ? L.z + (z - p->latent_dim) : L.z);
  PV_TRY(decoder_hidden_fwd(p, L, zin, cat_in ? lat_in : z, lat_in, s));
  if (p->coord_dim > 0) {
    PvOutLik o{};
    o.h = L.dact[nd - 1]; o.hpre = L.dpre_[nd - 1]; o.ldh = p->dec[nd - 1].out_dim; o.wo = p->params + p->out.w_off;
    o.bo = bias_of(p->params, p->out); o.x = p->x; o.llrow = L.llrow;
    o.part_dwo = L.part_dwo; o.part_dbo = L.part_dbo; o.M = L.rows; o.H = p->dec[nd - 1].out_dim;
    o.lik = p->lik; o.sigmoid_out = p->sigmoid_out; o.act_last = p->dec[nd - 1].act; o.sig = p->decoder_sig;
    o.sw = L.sw; o.N = (int)N; o.xmod = B * N;
    PV_TRY(Cn > 1 ? pv_out_lik_mc(o, (int)Cn, s) : pv_out_lik(o, s));
  } else {
    for (int64_t k = 0; k < L.P; ++k)                // one pass per particle against the same observations
      PV_TRY(pv_lik_elem(L.logits + k * B * N, p->x, B * N, p->lik, p->sigmoid_out, p->decoder_sig, nullptr, L.llrow + k * B * N,
                         nullptr, s, nullptr, N, false, plan_group(p)));
  }
  return pv_segsum(L.llrow, S, N, L.llkb, s);
}
// ... or with the forward-only launch of the bf16-class fused decoder kernels (fused 2 / 3), which leaves rows
static int evidence_ll_fused(const pv_ivae_plan* p, const Layout& L, hipStream_t s) {
  const int64_t lat_in = plan_lat_in(p);
  if (p->fc_latent.in_dim != lat_in) return PV_EINVAL;
  const bool cat_in = p->c_dim > 0;
  const ObjArgs obj{};
  FusedStep st{p, L, obj, false, s, cat_in ? L.zy : L.z + (p->z_dim - p->latent_dim), cat_in ? lat_in : (int64_t)p->z_dim,
               layout_choice(p, L.rows, false)};
  fused_decoder_args(st);
  PV_TRY(fused_guide(st));
  PV_TRY(fused_decoder_launch(st));
  return pv_segsum(L.llrow, step_S(p, L), plan_rows(p), L.llkb, s);
}

extern "C" int64_t pv_ivae_evidence_workspace_bytes(const pv_ivae_plan* plan, int32_t P) {
  if (!evidence_ok(plan, P)) return PV_EINVAL;
  const pv_ivae_plan q = evidence_plan(plan);
  Layout L;
  carve(&q, nullptr, L, false, false, P, false, true);
  return L.total;
}
extern "C" int pv_ivae_evidence_accumulate(const pv_ivae_plan* plan, int32_t P, float* state, int first, void* stream) {
  PV_RANGE("pv_ivae_evidence_accumulate");
  if (!evidence_ok(plan, P) || !state) return PV_EINVAL;
  const pv_ivae_plan q = evidence_plan(plan);
  const pv_ivae_plan* p = &q;
  if (!p->params || !p->x || !p->eps || !p->ws || (p->c_dim > 0 && !p->y) || (p->coord_dim > 0 && !p->grid)) return PV_EINVAL;
  Layout L;
  carve(p, (char*)p->ws, L, false, false, P, false, true);
  if (p->ws_bytes < L.total) return PV_EWS;
  hipStream_t s = (hipStream_t)stream;
  PV_TRY(L.fused ? evidence_ll_fused(p, L, s) : evidence_ll_layered(p, L, s));
  // every normaliser a log_prob has: the Poisson's data-only one is not in the rows the decoder launches leave
  if (p->lik == PV_LIK_POISSON_LOG) PV_TRY(pv_poisson_lognorm_particles(p->x, p->batch, p->n_pix, L.llkb, P, s));
  PvEvidenceLw e{};
  e.llkb = L.llkb; e.z = L.z; e.eps = p->eps; e.z_scale = L.z_scale; e.lw = L.ev_lw;
  e.B = (int)p->batch; e.P = P; e.z_dim = p->z_dim; e.beta = p->beta;
  PV_TRY(pv_evidence_lw(e, s));
  return pv_logmeanexp_update(L.ev_lw, P, (int32_t)p->batch, state, first, stream);
}

// (the query of both weighted families: it never sees the pointer, and the per-image instances' list is the shared ones')
extern "C" int64_t pv_ivae_weighted_workspace_bytes(const pv_ivae_plan* plan) {
  return workspace_bytes_impl(plan, pv_ivae_objective{1, PV_BOUND_ELBO, 0.0f, PV_OBS_W_SHARED, nullptr, nullptr});
}
extern "C" int pv_ivae_weighted_loss_and_grads(const pv_ivae_plan* plan, const float* pixel_w, int want_grads, void* stream) {
  PV_RANGE("pv_ivae_weighted_loss_and_grads");
  return loss_and_grads_impl(plan, weights_obj(PV_OBS_W_SHARED, pixel_w), want_grads, stream);
}
extern "C" int pv_ivae_weighted_step(const pv_ivae_plan* plan, const float* pixel_w, void* stream) {
  PV_RANGE("pv_ivae_weighted_step");
  return step_impl(plan, weights_obj(PV_OBS_W_SHARED, pixel_w), stream);
}
extern "C" int pv_ivae_weighted_images_loss_and_grads(const pv_ivae_plan* plan, const float* image_w, int want_grads, void* stream) {
  PV_RANGE("pv_ivae_weighted_images_loss_and_grads");
  return loss_and_grads_impl(plan, weights_obj(PV_OBS_W_PER_IMAGE, image_w), want_grads, stream);
}
extern "C" int pv_ivae_weighted_images_step(const pv_ivae_plan* plan, const float* image_w, void* stream) {
  PV_RANGE("pv_ivae_weighted_images_step");
  return step_impl(plan, weights_obj(PV_OBS_W_PER_IMAGE, image_w), stream);
}

extern "C" int pv_ivae_encode(const pv_ivae_plan* plan, float* z_loc, float* z_scale, void* stream) {
  PV_RANGE("pv_ivae_encode");
  if (!plan || ext_decoder_channels(plan)) return PV_EINVAL;
  pv_ivae_plan lay = plan->ext_decoder ? guide_plan(plan) : *plan;
  if (!valid_plan(&lay) || plan->ext_encoder || !plan->params || !plan->x || !plan->ws || !z_loc || !z_scale) return PV_EINVAL;
  lay.fused = 0;
  plan = &lay;
  Layout L;
  carve(plan, (char*)plan->ws, L, true, true);
  if (plan->ws_bytes < L.total) return PV_EWS;
  hipStream_t s = (hipStream_t)stream;
  PV_TRY(encoder_fwd(plan, L, s));
  // split the merged head: z_loc = head[:, :z], z_scale = softplus(head[:, z:])  (fc.py:59-60)
  PvHead h{};
  h.head = L.head; h.eps = L.z_scale /* unused values; any valid buffer */; h.z = L.z; h.z_scale = L.z_scale;
  h.z_loc_out = z_loc; h.z_scale_out = z_scale; h.tp = nullptr; h.zy = nullptr; h.scalars = (float*)L.dhead;
  h.B = plan->batch; h.z_dim = plan->z_dim; h.c_dim = 0; h.coord_dim = 0; h.beta = 0.0f;
  h.ldh = (int)plan_head_w(plan);
  PV_TRY(pv_head_fwd(h, s));
  if (plan->discrete_dim > 0 && plan->alpha)
    PV_TRY(pv_softmax_rows(L.head + 2 * plan->z_dim, plan_head_w(plan), plan->batch, plan->discrete_dim, plan->alpha, s));
  return 0;
}

extern "C" int pv_ivae_decode(const pv_ivae_plan* plan, const float* z, float angle, float shift_x, float shift_y,
                              float scale, float* loc, void* stream) {
  PV_RANGE("pv_ivae_decode");
  if (!valid_plan(plan) || !plan->params || !plan->ws || !z || !loc) return PV_EINVAL;
  if (plan->coord_dim > 0 && !plan->grid) return PV_EINVAL;
  pv_ivae_plan lay = decode_plan(plan);
  plan = &lay;
  if (decode_fused(plan)) return decode_fused_run(plan, z, angle, shift_x, shift_y, scale, loc, (hipStream_t)stream);
  lay.fused = 0;
  Layout L;
  carve(plan, (char*)plan->ws, L, true);
  if (plan->ws_bytes < L.total) return PV_EWS;
  hipStream_t s = (hipStream_t)stream;
  const int64_t B = plan->batch, N = plan->n_pix, R = L.rows;
  const int64_t lat_in = plan_lat_in(plan);
  if (plan->coord_dim > 0) PV_TRY(pv_fill_tp(L.tp, (int)B, angle, scale, shift_x, shift_y, s));
  PV_TRY(decoder_hidden_fwd(plan, L, z, lat_in, lat_in, s));
  const int nd = plan->n_dec;
  if (plan->coord_dim > 0) {
    PvOutLik o{};
    o.h = L.dact[nd - 1]; o.ldh = plan->dec[nd - 1].out_dim; o.wo = plan->params + plan->out.w_off;
    o.bo = bias_of(plan->params, plan->out);
    o.x = L.llrow /* unused for loc */; o.loc = loc; o.llrow = nullptr; o.dpre = nullptr; o.M = R;
    o.H = plan->dec[nd - 1].out_dim; o.lik = loc_lik(plan); o.sigmoid_out = plan->sigmoid_out; o.sig = 1.0f;
    o.act_last = plan->dec[nd - 1].act;
    if (plan_C(plan) > 1) { o.x = nullptr; return pv_out_lik_mc(o, (int)plan_C(plan), s); }
    return pv_out_lik(o, s);
  }
  return pv_lik_elem(L.logits, plan->lik == PV_LIK_CATEGORICAL ? nullptr : L.logits, B * N, loc_lik(plan), plan->sigmoid_out, 1.0f, loc,
                     nullptr, nullptr, s, nullptr, 0, false, plan_group(plan));
}
