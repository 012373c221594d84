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
// Its TAIL instances (pv_sdec_fused_mc_tail_kernel, C = 1 .. 6 and 8, all three weight forms; PV_PLAN_FUSED_TAIL) run plans whose
// positions are no multiple of 16: described where they are instantiated, below.
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
//
// CAT (PV_LIK_CATEGORICAL; pv_sdec_fused_mc_cat_kernel, instances of their own: pv_sdec_fused_mc_body.inc holds the kernel and is
// included once per family): the C outputs of a row are the logits of ONE observation on the simplex.  The channel
// loop leaves a_c in dlda[c]; a second pass forms, c ascending, max_c a_c, sum_c exp(a_c - max), sum_c xw_c (xw = w x, the weighted
// observation) and from them  ll = sum_c xw_c (a_c - lse),  dL/da_c = p_c sum_c xw_c - xw_c,  loc_c = p_c = exp(a_c - max) / sum.
// log p_c is a_c - lse, never log(p_c).  x and w are read twice (cache hits) instead of held in 2 C registers across the pass.
// Everything from the d(wo) exchange onward is the same code.
//
// TAIL (PV_PLAN_FUSED_TAIL; pv_sdec_fused_mc_tail_kernel, instances of their own from the same text): positions that are no multiple
// of 16.  A sample occupies f.N = 16 ceil(f.n_obs / 16) rows of the partition — units, workgroup ranges, flush_hz and kmax are the
// padded layout's, unchanged — and observes the first f.n_obs.  A padding row reads neither the grid nor x nor a weight, runs the
// layers at the coordinates (0, 0) (finite values), and has ll = 0 and dL/da_c = 0 set where they are formed: from there on it is the
// weighted instances' zero-weight row — tC = 0 (1 - h2^2) = 0, and every staged product, d(x') and dL/d(hz) term it contributes is
// an exact zero.  It writes no loc and DOES write llrow = 0 and rowtp = 0: the per-sample sums read all f.N rows of a workspace
// that arrives with any content.  x, loc and per-image weights are indexed by observation, (b n_obs + n) C + c.  C = 1 .. 6 and 8
// in all three weight forms (not 7: fdm_has_tail_instance), the unweighted C = 1 included (its record is the one-channel
// kernel's: nothing for the second launch to sum).
#define FDM_KERNEL pv_sdec_fused_mc_kernel
#define FDM_CAT 0
#define FDM_TAIL 0
#include "pv_sdec_fused_mc_body.inc"
#undef FDM_KERNEL
#undef FDM_TAIL
#define FDM_KERNEL pv_sdec_fused_mc_tail_kernel
#define FDM_TAIL 1
#include "pv_sdec_fused_mc_body.inc"
#undef FDM_KERNEL
#undef FDM_CAT
#undef FDM_TAIL
// the categorical instances: C = 2 .. 8 (one class is no distribution), unweighted and both weighted forms
#define FDM_KERNEL pv_sdec_fused_mc_cat_kernel
#define FDM_CAT 1
#define FDM_TAIL 0
#include "pv_sdec_fused_mc_body.inc"
#undef FDM_KERNEL
#undef FDM_CAT
#undef FDM_TAIL

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
// PV_LIK_CATEGORICAL: C = 2 .. PV_MAX_CHANNELS in all three forms (profiles/categorical_resource_usage.txt)
static bool fdm_has_cat_instance(int C, int weighted = 0) { return weighted >= 0 && weighted <= 2 && C >= 2 && C <= 8; }
static bool fdm_lik_instance(int lik, int C, int weighted) {
  return lik == PV_LIK_CATEGORICAL ? fdm_has_cat_instance(C, weighted) : fdm_has_instance(C, weighted);
}
// the tail form (pv_sdec_fused_mc_tail_kernel): per-value likelihoods, C = 1 .. 6 and 8 in all three weight forms.  C = 7 is taken
// out: its unweighted training instance spills (3 VGPRs, 16 bytes of scratch per lane; profiles/any_size_resource_usage.txt), and
// one list serves the three forms because a plan's unweighted and weighted calls share the layout — seven channels whose
// positions are no multiple of 16 stay on the layer-by-layer kernels, and no C = 7 tail instance is compiled
static bool fdm_has_tail_instance(int lik, int C, int weighted = 0) {
  return lik != PV_LIK_CATEGORICAL && weighted >= 0 && weighted <= 2 && C >= 1 && C <= 8 && C != 7;
}

bool pv_sdec_fused_tail(const pv_ivae_plan* p) {
  if (!p || !(p->flags & PV_PLAN_FUSED_TAIL) || p->fused != 1 || !pv_sdec_fused_trunk_supported(p)) return false;
  if (p->discrete_dim > 0 || p->n_enc_ops > 0 || p->ext_encoder || p->ext_decoder || p->row_w || p->row_elbo || p->dy) return false;
  const int C = p->out.out_dim;
  if (C < 1 || C > PV_MAX_CHANNELS || p->n_pix % C != 0 || (C > 1 && !(p->flags & PV_PLAN_FUSED_CHANNELS))) return false;
  // (one list for the three weight forms: a plan's unweighted and weighted calls share the decision, and with it the layout)
  for (int w = 0; w <= 2; ++w)
    if (!fdm_has_tail_instance(p->lik, C, w)) return false;
  return (p->n_pix / C) % FD_UNIT != 0;
}
int64_t pv_sdec_fused_rows_per_sample(const pv_ivae_plan* p) {
  const int64_t pos = p->n_pix / (p->coord_dim > 0 ? p->out.out_dim : 1);
  return pv_sdec_fused_tail(p) ? (pos + FD_UNIT - 1) / FD_UNIT * FD_UNIT : pos;
}

bool pv_sdec_fused_mc_supported(const pv_ivae_plan* p) {
  if (pv_sdec_fused_tail(p)) return true;              // (one channel too: the unweighted tail form exists at C = 1)
  if (!p || !(p->flags & PV_PLAN_FUSED_CHANNELS) || p->fused != 1) return false;
  if (!pv_sdec_fused_trunk_supported(p)) return false;
  const int C = p->out.out_dim;
  if (C < 2 || C > PV_MAX_CHANNELS || !fdm_lik_instance(p->lik, C, 0) || p->n_pix % C != 0) return false;
  return (p->n_pix / C) % FD_UNIT == 0;
}

bool pv_sdec_fused_mc_weighted_supported(const pv_ivae_plan* p, bool per_image) {
  if (pv_sdec_fused_tail(p)) return true;
  if (!p || p->fused != 1 || !pv_sdec_fused_trunk_supported(p)) return false;
  const int C = p->out.out_dim;
  if (C < 1 || C > PV_MAX_CHANNELS || !fdm_lik_instance(p->lik, C, per_image ? PV_FDM_W_IMAGES : PV_FDM_W_SHARED) || p->n_pix % C != 0) return false;
  if (C > 1 && !(p->flags & PV_PLAN_FUSED_CHANNELS)) return false;
  return (p->n_pix / C) % FD_UNIT == 0;
}

template <int C, int W>
static int fdm_cat_launch(const PvFused& f, int grid, bool grads, hipStream_t s) {
  const size_t lds = FD_LDS_FLOATS * sizeof(float);
  if (grads) {
    PV_TRY(pv_set_dynamic_lds(reinterpret_cast<const void*>(&pv_sdec_fused_mc_cat_kernel<true, C, W>), (int)lds));
    hipLaunchKernelGGL((pv_sdec_fused_mc_cat_kernel<true, C, W>), dim3(grid), dim3(FD_THREADS), lds, s, f);
  } else {
    PV_TRY(pv_set_dynamic_lds(reinterpret_cast<const void*>(&pv_sdec_fused_mc_cat_kernel<false, C, W>), (int)lds));
    hipLaunchKernelGGL((pv_sdec_fused_mc_cat_kernel<false, C, W>), dim3(grid), dim3(FD_THREADS), lds, s, f);
  }
  PV_LAUNCH_CHECK();
  return 0;
}

template <int W>
static int fdm_cat_launch_any(const PvFused& f, int C, int grid, bool grads, hipStream_t s) {
  switch (C) {
    case 2: return fdm_cat_launch<2, W>(f, grid, grads, s);
    case 3: return fdm_cat_launch<3, W>(f, grid, grads, s);
    case 4: return fdm_cat_launch<4, W>(f, grid, grads, s);
    case 5: return fdm_cat_launch<5, W>(f, grid, grads, s);
    case 6: return fdm_cat_launch<6, W>(f, grid, grads, s);
    case 7: return fdm_cat_launch<7, W>(f, grid, grads, s);
    case 8: return fdm_cat_launch<8, W>(f, grid, grads, s);
  }
  return PV_EINVAL;
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

template <int C, int W>
static int fdm_tail_launch(const PvFused& f, int grid, bool grads, hipStream_t s) {
  const size_t lds = FD_LDS_FLOATS * sizeof(float);
  if (grads) {
    PV_TRY(pv_set_dynamic_lds(reinterpret_cast<const void*>(&pv_sdec_fused_mc_tail_kernel<true, C, W>), (int)lds));
    hipLaunchKernelGGL((pv_sdec_fused_mc_tail_kernel<true, C, W>), dim3(grid), dim3(FD_THREADS), lds, s, f);
  } else {
    PV_TRY(pv_set_dynamic_lds(reinterpret_cast<const void*>(&pv_sdec_fused_mc_tail_kernel<false, C, W>), (int)lds));
    hipLaunchKernelGGL((pv_sdec_fused_mc_tail_kernel<false, C, W>), dim3(grid), dim3(FD_THREADS), lds, s, f);
  }
  PV_LAUNCH_CHECK();
  return 0;
}

template <int W>
static int fdm_tail_launch_any(const PvFused& f, int C, int grid, bool grads, hipStream_t s) {
  switch (C) {
    case 1: return fdm_tail_launch<1, W>(f, grid, grads, s);
    case 2: return fdm_tail_launch<2, W>(f, grid, grads, s);
    case 3: return fdm_tail_launch<3, W>(f, grid, grads, s);
    case 4: return fdm_tail_launch<4, W>(f, grid, grads, s);
    case 5: return fdm_tail_launch<5, W>(f, grid, grads, s);
    case 6: return fdm_tail_launch<6, W>(f, grid, grads, s);
    case 8: return fdm_tail_launch<8, W>(f, grid, grads, s);
  }
  return PV_EINVAL;
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
  if (grid < 1 || f_in.N % FD_UNIT != 0 || f_in.units * FD_UNIT != f_in.M || f_in.n_obs < 0) return PV_EINVAL;
  const bool tail = f_in.n_obs > 0;                                  // the rows a sample observes are fewer than the rows it occupies
  if (tail ? !fdm_has_tail_instance(f_in.lik, C, w) : !fdm_lik_instance(f_in.lik, C, w)) return PV_EINVAL;
  if (tail && (f_in.n_obs >= f_in.N || f_in.N - f_in.n_obs >= FD_UNIT || (int64_t)f_in.B * f_in.N != f_in.M)) return PV_EINVAL;
  PvFused f = f_in;
  f.ablate = 0;
  if (tail) {
    if (w == PV_FDM_W_IMAGES) return fdm_tail_launch_any<PV_FDM_W_IMAGES>(f, C, grid, grads, s);
    if (w == PV_FDM_W_SHARED) return fdm_tail_launch_any<PV_FDM_W_SHARED>(f, C, grid, grads, s);
    return fdm_tail_launch_any<0>(f, C, grid, grads, s);
  }
  if (f.lik == PV_LIK_CATEGORICAL) {                                 // the likelihood kind is a compile-time property of its instances
    if (w == PV_FDM_W_IMAGES) return fdm_cat_launch_any<PV_FDM_W_IMAGES>(f, C, grid, grads, s);
    if (w == PV_FDM_W_SHARED) return fdm_cat_launch_any<PV_FDM_W_SHARED>(f, C, grid, grads, s);
    return fdm_cat_launch_any<0>(f, C, grid, grads, s);
  }
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
