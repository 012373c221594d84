// pv_sdec_fused.h — the fused persistent spatial-decoder forward+backward kernel (pv_sdec_fused.hip).
#pragma once
#include "pv_common.h"
#include "pv_sdec_partition.h"  // FD_UNIT (rows per wave tile) and the row partition's arithmetic

#define FD_H 128               // hidden width the kernel is specialised for (hidden_dim_d = [128, 128])
#define FD_WAVES 8             // waves per workgroup (2 per SIMD)
#define FD_REC (2 * FD_H * FD_H + 14 * FD_H)  // floats of one per-workgroup partial-gradient record:
// [dW1 HxH | dW2 HxH | db1 H | db2 H | dWc0 H | dWc1 H | dwo H | dbo (1, padded to H) | 8 spare slots x H]
// (the spare slots are summed into dwo by the reduction when it is called with dwo_slots = 1; both kernels now
//  sum their d(wo) in LDS and leave the slots unused; the multi-channel kernel, pv_sdec_fused_mc.hip, puts channel c >= 1 there:
//  d(wo)[c] in spare slot c - 1, d(bo)[c] at [c] of the dbo slot — summed by pv_sdec_fused_mc_reduce_out, never with dwo_slots = 1)
#define PV_RS_W 8               // floats per slot of PvFused::part_rs (5 used)
#define FB_WIMG_BYTES (4 * FD_H * FD_H * 2 + 256)   // split-precision kernels: global copy of the four LDS weight images (+ the fp16 modes' scales)

struct PvFused {
  const float* x;        // (M) observations, M = B*N rows (b, n)
  const float* grid;     // (N, cd)
  const float* tp;       // (B, 8) cos, sin, scale, tx, ty
  const float* hz;       // (B, H) fc_latent(z), multiplied by hz_scale when that is non-zero
  float hz_scale;        // what the producer of hz already multiplied it by (pv_sdec_fused_w8.hip wants 2 log2(e) * hz)
  const float *Wc, *bc;  // coord_latent.fc_coord (H, cd), (H)
  const float *W1, *b1;  // decoder.fc_layers.0 (H, H), (H)
  const float *W2, *b2;  // decoder.fc_layers.2
  const float *wo, *bo;  // decoder.out (1, H), (1)
  float* llrow;          // (M) log-likelihood per row (null: not wanted — forward-only decode)
  float* loc;            // (M) decoder output or null
  float* rowtp;          // (4, M) per-row d(phi), d(scale), d(tx), d(ty)
  float* part_hz;        // (B * kmax, H) partial sums of dL/d(hz), zero-filled by the caller
  float* part_rs;        // (round 6) (B * kmax, PV_RS_W) or null.  Not null (training launches of the kernels that support it):
                         //   instead of writing llrow / rowtp per ROW the kernel publishes, in the slot of part_hz's scheme, the
                         //   sums over a wave's rows of a sample of {ll, d(phi), d(scale), d(tx), d(ty)} — pv_latent_bwd_reduce then
                         //   adds kmax slots per sample where it loaded and block-reduced 5 x N rows; zero-filled with part_hz
                         //   (it FOLLOWS part_hz's B * kmax * H floats in memory)
  float* part;           // (G, FD_REC) per-workgroup partial gradients
  float* dhz_out;        // (round 6) (B, H) or null.  Not null (the launch that hosts the guide: one image per workgroup): the workgroup
                         //   sums its waves' dL/d(hz) partials itself and writes the image's dL/d(hz) here — pv_latent_bwd_reduce then
                         //   reads it instead of adding kmax slots of part_hz (PvLatentBwd::dhz_ready)
  float* dzc_out;        // (round 6) (B, lat_in) or null, with dhz_out: ... and the image's dL/dz = dL/d(hz) Wz (PvLatentBwd::dzc_in)
  const float* Wz;       //   coord_latent.fc_latent.weight (H, lat_in) and lat_in, for dzc_out (the 4-wave kernels; the hosting 8-wave
  int lat_in;            //   launch has them in PvEncFold).  dhz_out / dzc_out are only set when every workgroup's unit range is exactly
                         //   ONE sample (grid == B, units == B * N / 16, x_units == 0): the caller's promise, re-checked by the kernel
  const float* sw;       // per-sample weight of dL/dlogit (jiVAE: alpha[b][k] of sample (k, b)); null: 1
  int64_t x_units;       // > 0: the observations repeat every x_units units (jiVAE: B*N/16; x is (B, N)); 0: x is (M)
  union {
  void* wimg;            // bf16x3 kernel only: FB_WIMG_BYTES of pre-split weight images (pv_sdec_fused_bf16_prep)
  const float* pw;       // weighted launches of pv_sdec_fused_mc.hip only (pv_sdec_fused_mc_launch(..., weighted = 1 or 2)): (N * C)
                         //   per-observation weights of the likelihood, shared by all samples (pv_ivae_weighted_*), or (M * C), one per
                         //   observation of every sample (weighted = 2, pv_ivae_weighted_images_*).  The f32 kernels
                         //   have no weight images, so the two share the slot: the struct keeps its size and every field its offset —
                         //   and with them every kernel that takes a PvFused its argument layout, hidden arguments included
  };
  void* park;            // 8-wave split-precision kernel only: pv_sdec_fused_w8x3_park_bytes(grid) of per-wave parking slots
                         //   — and, no 4-wave launch reading it, the slot the WEIGHTED 4-wave launches of pv_sdec_fused_bf16.hip
                         //   (pv_sdec_fused_bf16_launch(..., weighted)) take for their per-observation weights: (N) floats shared by
                         //   all samples or (M) in the layout of x.  They need wimg, so `pw` above is not theirs to use
  int64_t M;             // rows
  int64_t units;         // M / FD_UNIT
  int N, cd, B, lik, sigmoid_out, kmax;
  int ablate;            // profiling only (env PV_FD_ABLATE): 1 skip wgrad exchanges, 2 skip coord-layer exchange,
                         // 4 skip dgrad, 8 skip d(wo) reduction  -> wrong gradients, used to price the phases
  int qswap;             // the weight images are in the q-swapped column order (pv_fb_layout.h; set by the 4-wave kernel's launcher)
  float sig;
  int sel;               // pv_ivae_plan.dec_kernel: which build of the decoder kernel runs (0: by problem size; pv_sdec_fused_bf16.hip)
  int dl_exp;            // fp16 modes (pv_sdec_fused_bf16.hip): exponent bias of the per-row dL/dlogit factor folded into the
                         // staged activations: 2^dl_exp * |dL/dlogit| should sit around 1 .. 2^8 (Bernoulli 4; Gaussian: -log2(1 / sig^2))
  int n_obs;             // tail launches of pv_sdec_fused_mc.hip only (pv_sdec_fused_mc_launch with n_obs > 0; PV_PLAN_FUSED_TAIL):
                         // the positions a sample observes, n_obs < N = 16 ceil(n_obs / 16) — N stays "rows per sample" of the partition,
                         // M = B N, and rows n >= n_obs of a sample are padding.  x, loc and the per-image weights are (B, n_obs, C).
                         // 0 everywhere else.  (It takes the struct's four bytes of tail padding: size and every offset stay)
};
static_assert(sizeof(PvFused) == 280, "PvFused is a kernel argument: its size is part of every kernel's argument layout");

// ---- the guide folded into the decoder launch (round 5; pv_sdec_fused_w8.hip) -------------------------------------------------
// When a workgroup's unit range is a whole number of images (batch a multiple of the grid: BASELINE's batch 256 on 256 CUs is one
// image per workgroup) the workgroup can run its images' guide ITSELF in the launch's prologue — fcEncoderNet.forward (nets/fc.py:
// 51-61) as fp32 matrix-vector products straight from the L2-resident weights, the reparameterised sample and its sampled-KL terms
// (models/ivae.py:204-221), _split_latent (models/base.py:97-119) and fc_latent(z) — and convert the decoder's two hidden weight
// matrices into its own LDS images: the encoder launch (18.7 us of dependent latency for 51 MFLOP), its hand-off protocol and the
// global weight-image copy all disappear from the step.  Everything the backward launches read is written exactly where the
// encoder launch would have put it.
struct PvEncFold {
  const float* params;
  pv_layer enc0, enc1, head;       // two hidden layers (widths 128) + the merged [mu | softplus input] head
  const float* x; int64_t ldx;     // (B, ldx) observations (the encoder's input: x.view(B, N))
  const float* eps;                // (B, z_dim)
  float* eact0; float* eact1;      // hidden activations (B, 128)
  float* head_out;                 // (B, 2 z_dim)
  float* z; float* z_scale; float* z_loc_out; float* z_scale_out;
  float* tp;                       // (B, 8) cos, sin, scale, tx, ty
  float* kl_part;                  // (B, 2): beta * log p(z_b), beta * log q(z_b | x_b)
  float* hz; const float* Wz;      // (B, 128) fc_latent(z content) * C ; fc_latent.weight (128, lat_in)
  int lat_in, z_dim, coord_dim, has_r, has_t, has_s;
  float tp0, tp1, sc_prior, beta;
  int img_per_wg;                  // images per workgroup (B / grid): 1
  // (round 6, third cut) chain != 0: the workgroup also runs its image's latent backward (models/ivae.py's guide differentiated:
  // head backward from dL/dz and the sampled-KL terms) and the encoder's input-gradient chain in the launch's EPILOGUE — it holds
  // the image's row sums, dL/d(hz) and dL/dz there already (PvFused::part_rs / dhz_out / dzc_out) — so that the step's closing launch
  // has no per-sample work left (pv_elementwise.hip: pv_rec_wgrad_kernel).  Needs head.out_dim <= 16.  A training launch with chain
  // set writes NO per-row outputs (PvFused::llrow / rowtp stay untouched, part_hz and all but the image's first part_rs slot too):
  // the row sums are formed on chip and consumed here.  The plan asks for it only where nothing else reads rows (pv_plan.hip).
  // Bit 0 asks for the chain; bit 1 (PV_CHAIN_GENERIC_LOOP, from PV_PLAN_GENERIC_TILE_LOOP) is read by the 8-wave launcher alone: the
  // image-owning training launch keeps the generic tile loop where it would take the full-tile one (pv_sdec_fused_w8.hip, build 4 —
  // same results bit for bit; an A/B and test switch).  The kernels test chain != 0.
#define PV_CHAIN_GENERIC_LOOP 2
  int chain;
  float* dhead; int ldh;          // (B, ldh) dL/d[mu | softplus input]
  float* edp0; float* edp1;        // (B, 128) dL/dpre of the two hidden layers
  float* llb;                      // (B) the image's log-likelihood
  // (round 6, fourth cut) coop != 0 (with chain, grid == 256): the guide's first layer is shared among the 32 workgroups of a group
  // (pv_sdec_fused_w8.hip).  coop_flags: grid + 1 words of any content — [g] workgroup g's hand-off tag, [grid] a word that the
  // step's closing launch increments (PvWgradSmall::tick), so that no launch's tag repeats an earlier one's
  int coop;
  unsigned* coop_flags;
};
// A kernel (PvFused f, PvEncFold e) whose EPILOGUE alone needs `e` reads it there through this pointer into the kernarg segment, made
// opaque at the point of use: named directly, the compiler fetches the fields at kernel entry and carries them — spilled — through
// the tile loop (pv_sdec_fused_bf16.hip: 51 -> 92 spilled SGPRs and +3 us on the launch; with the pointer: 42).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) PvEncFold* PvEncFoldArg;
__device__ __forceinline__ PvEncFoldArg pv_kernarg_fold() {
  const __attribute__((address_space(4))) char* k = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  PvEncFoldArg p = (PvEncFoldArg)(k + ((sizeof(PvFused) + alignof(PvEncFold) - 1) / alignof(PvEncFold)) * alignof(PvEncFold));
  asm volatile("" : "+s"(p));
  return p;
}
#else
typedef const PvEncFold* PvEncFoldArg;
__device__ inline PvEncFoldArg pv_kernarg_fold() { return nullptr; }      // (host pass of the same source: never called)
#endif
// the same guide as a launch of its own, one workgroup per image (pv_guide_img.hip; round 6): for the plans the fold cannot take.
// prep != null: guest workgroups write the decoder's weight images / clear its dL/d(hz) slots; hz_mul: what hz leaves multiplied by
#define PV_GUIDE_IMG_MAX_BATCH 384     // (measured, scripts/ab_guide_img.py: -7..-10 % of the step at batch 64, -6..-9 % at 128, -2..-4 % at 256, +-0 at 512)
struct PvFbPrep;
bool pv_guide_img_ok(const PvEncFold& e, int B);
// kl_mode: PV_KL_SAMPLED / PV_KL_ANALYTIC — what kl_part holds (a launch argument: PvEncFold is also the hosting decoder launch's, which runs the sampled form only)
int pv_guide_img_launch(const PvEncFold& e, const PvFbPrep* prep, float hz_mul, int B, hipStream_t s, int kl_mode = PV_KL_SAMPLED);
// whether the launch of f on `grid` workgroups has the geometry that hosts the guide: one image per workgroup (the caller checks the
// encoder's architecture, and PvDecChoice::hosts_guide that the launch runs the kernel the guide lives in)
bool pv_sdec_fused_w8_fold_ok(const PvFused& f, int grid);

// true when the plan's architecture is the one the fused kernel is specialised for
bool pv_sdec_fused_supported(const pv_ivae_plan* p);
// workgroups the kernel runs with: sd_grid (pv_sdec_partition.h) at the device's number of CUs
int pv_sdec_fused_grid(int64_t units);
// dL/d(hz) slots per sample of `rows` rows (sd_kmax: the workgroups that can touch one sample's rows, times the waves that publish)
int pv_sdec_fused_kmax(int rows, int64_t units, int grid, int waves);
// launches the kernel (grads = false: forward + likelihood only)
int pv_sdec_fused_launch(const PvFused& f, int grid, bool grads, hipStream_t s);
// ---- several output channels per row (pv_sdec_fused_mc.hip; the plan asks with PV_PLAN_FUSED_CHANNELS, fused == 1) ----
// the architecture of pv_sdec_fused_supported without its conditions on the output layer's width and the rows per sample
bool pv_sdec_fused_trunk_supported(const pv_ivae_plan* p);
// true when the plan runs the multi-channel kernel: the flag, fused == 1, that architecture, 2 <= out.out_dim <= PV_MAX_CHANNELS
// with an instance of the kernel, and positions (n_pix / out.out_dim) a multiple of 16 — or pv_sdec_fused_tail(p), below, at
// every channel count it accepts, one included (the plan then runs the kernel's tail form)
bool pv_sdec_fused_mc_supported(const pv_ivae_plan* p);
// f as for pv_sdec_fused_launch with C values per row: x and loc are (M, C) channel-last (x null: zeros — forward-only decode),
// wo (C, H), bo (C); llrow (M) sums the row's C values, c ascending.  Record (PV_REC_ROWMAJOR): channel 0's d(wo) / d(bo) where
// the one-channel kernel puts them (slot 4, slot 5 [0]); channel c >= 1: d(wo)[c] in slot 5 + c, d(bo)[c] at slot 5 [c].
// PV_EINVAL for sw, x_units, part_rs, dhz_out, dzc_out or wimg set, or a C without an instance.  f.ablate is ignored.
// weighted: the weighted instances (C = 1 .. PV_MAX_CHANNELS; C = 1 exists in this form only): f.pw (the slot of wimg) must be set;
// ll and dL/da of observation (n, c) of every sample are multiplied by pw[n * C + c]; loc is not.  The record is the unweighted launch's
// weighted == PV_FDM_W_IMAGES (pv_ivae_weighted_images_*): f.pw is (M * C), one weight per observation of every sample in the
// layout of x — observation (row, c) is multiplied by pw[row * C + c]; the same instances list, everything else as PV_FDM_W_SHARED
// f.n_obs > 0: the tail form (PV_PLAN_FUSED_TAIL; per-value likelihoods, C = 1 .. 6 and 8 in all three weight forms): a sample
// occupies f.N = 16 ceil(n_obs / 16) rows, M = B N, of which it observes the first n_obs; x, loc and per-image weights are
// (B, n_obs, C), shared weights (n_obs, C), the grid (n_obs, cd); llrow (M) and rowtp (4, M) get zeros in the padding rows
#define PV_FDM_W_SHARED 1
#define PV_FDM_W_IMAGES 2
int pv_sdec_fused_mc_launch(const PvFused& f, int C, int grid, bool grads, hipStream_t s, int weighted = 0);
// ---- positions that are no multiple of 16 (PV_PLAN_FUSED_TAIL; the tail instances of pv_sdec_fused_mc.hip) ----
// true when the flag takes effect on the plan: fused == 1, the trunk's architecture, positions % 16 != 0, the fc-encoder iVAE (no
// discrete latent, no convolutional / external networks, no per-image outputs), a per-value likelihood, and one channel or
// 2 .. 6 or 8 with PV_PLAN_FUSED_CHANNELS (seven: the unweighted instance spills, so the count stays layered).  The unweighted
// and both weighted entry points then run the tail instances
bool pv_sdec_fused_tail(const pv_ivae_plan* p);
// rows per sample of the plan's DECODER layout: the positions (n_pix / channels), rounded up to a multiple of 16 where
// pv_sdec_fused_tail(p).  Layout, launch arguments and per-sample reductions take it; x, loc, the encoder, the weights keep n_pix
int64_t pv_sdec_fused_rows_per_sample(const pv_ivae_plan* p);
// true when a WEIGHTED step of the plan (pv_ivae_weighted_*) runs that kernel: fused == 1, the trunk's architecture, positions a
// multiple of 16, a weighted instance for the channel count — one channel, or 2 .. PV_MAX_CHANNELS with PV_PLAN_FUSED_CHANNELS
// (per_image: the instances of pv_ivae_weighted_images_*); or pv_sdec_fused_tail(p): the tail form's weighted instances
bool pv_sdec_fused_mc_weighted_supported(const pv_ivae_plan* p, bool per_image = false);
// sums the records' entries of channels 1 .. C-1 — (C - 1) (H + 1) outputs, each over the `grid` records in the shared reduction's
// fixed order (four slices of ascending workgroups) — into G + wo_off + c H and G + bo_off + c; channel 0 is the shared reduction's
int pv_sdec_fused_mc_reduce_out(const float* part, int grid, float* G, int64_t wo_off, int64_t bo_off, int C, hipStream_t s);
// ---- which fused decoder kernel a launch runs, and everything that follows from it (pv_sdec_fused_bf16.hip) ----
// ONE resolved decision per (fused mode, units, launch kind, pv_ivae_plan.dec_kernel): layouts, preparations, launches, reductions and
// the name hooks read its fields and never its inputs.  pv_sdec_fused_choice is the only reader of the size thresholds, the row cap
// and the experiments build's environment switches.
enum PvDecFamily {
  PV_DEC_F32 = 0,      // pv_sdec_fused.hip: the f32-MFMA kernel (fused == 1) ...
  PV_DEC_F32_MC,       // ... and its multi-channel sibling, pv_sdec_fused_mc.hip (the plan decides between the two: pv_plan.hip)
  PV_DEC_W4,           // pv_sdec_fused_bf16.hip: the 4-wave source, in the precision build `prec`
  PV_DEC_W8,           // pv_sdec_fused_w8.hip: the 8-wave plain-bf16 kernel — the one that can host the guide
  PV_DEC_W8X3,         // pv_sdec_fused_w8x3.hip: the split-precision source with `x3_waves` waves
  PV_DEC_W8H           // pv_sdec_fused_w8h.hip: the 8-wave fp16 kernel (experiments build; training launches)
};
struct PvDecChoice {
  // the launch of the (grads) the choice was resolved for
  int family;          // PvDecFamily
  int prec;            // PV_DEC_W4: the build (pv_sdec_fused_bf16.hip FB_P_*); -1 otherwise
  int x3_waves;        // PV_DEC_W8X3: 8 or 4 (0: a selection without an instance — the launcher refuses it); 0 otherwise
  int ds;              // PV_DEC_W8H: dL/dpre split in both dgrads (H231) or not (H221); 0 otherwise
  int img_mode;        // its weight images (PvFbPrep::mode) ...
  float img_scale;     // ... what they are pre-scaled by (0: unscaled) — and what hz must arrive multiplied by ...
  int img_qswap;       // ... and whether they are in the q-swapped column order (pv_fb_layout.h)
  // the TRAINING form of the same (fused, units, dec_kernel), whatever the launch kind: a step's layout is sized for it, and a
  // forward-only launch into a training layout leaves its slots and records alone
  int waves;           // waves per workgroup that publish a dL/d(hz) slot (sizes part_hz; 1: the f32 kernels, one slot per workgroup)
  int rec_fmt;         // the record format (PV_REC_*) the training launch writes
  bool parks;          // the training form needs PvFused::park ...
  int64_t park_bytes(int grid) const;      // ... that many bytes of it (0: none)
  // both launch kinds
  bool weighted;       // a weighted instance exists (PV_DEC_W4 in a bf16 build for training and forward-only launches alike)
  bool hosts_guide;    // the kernel is the one that can host the guide (pv_sdec_fused_w8_fold_ok: whether this launch's geometry can)
};
// fused: pv_ivae_plan.fused (<= 1: PV_DEC_F32); units: rows / FD_UNIT; sel: pv_ivae_plan.dec_kernel (0: by problem size)
PvDecChoice pv_sdec_fused_choice(int fused, int64_t units, bool grads, int sel);
// whether `sel` (pv_ivae_plan.dec_kernel) names a decoder-kernel build this library contains for the fused mode (the table the
// resolver reads)
bool pv_sdec_fused_sel_valid(int fused, int sel);

// the bf16-class kernels (c.family >= PV_DEC_W4), same interface as pv_sdec_fused_launch; _prep must run first on the same stream,
// once per parameter state: it writes f.wimg as `c` wants the images and, with grads, zero-fills f.part_hz
int pv_sdec_fused_bf16_prep(const PvFused& f, bool grads, const PvDecChoice& c, hipStream_t s);
// ... or, as arguments for a kernel that hosts the preparation (pv_fb_layout.h: pv_fb_prep)
struct PvFbPrep;
PvFbPrep pv_sdec_fused_bf16_prep_args(const PvFused& f, bool grads, const PvDecChoice& c);
bool pv_sdec_fused_w8_qswap();          // the 8-wave plain-bf16 kernel's images are in the q-swapped column order (pv_fb_layout.h)
// c: the choice resolved for (grads).  weighted (PV_FDM_W_SHARED / PV_FDM_W_IMAGES; pv_ivae_weighted_* with PV_PLAN_FAST_WEIGHTS):
// the weighted instances of the 4-wave kernel's bf16 builds; the weights — (N), or (M) in the layout of x — travel in f.park.
// PV_EINVAL where c.weighted is false, or with fold, f.sw or f.x_units set
int pv_sdec_fused_bf16_launch(const PvFused& f, int grid, bool grads, const PvDecChoice& c, hipStream_t s,
                              const PvEncFold* fold = nullptr,
                              const PvEncFold* chain = nullptr,      // chain: the 4-wave kernels' own-sample epilogue (PvEncFold::chain)
                              int weighted = 0);
const char* pv_sdec_fused_bf16_wt_kernel_name(bool x3, int grads, int lik);      // (as rocprofv3 prints it)
int pv_sdec_fused_w8_launch(const PvFused& f, int grid, bool grads, hipStream_t s, const PvEncFold* fold = nullptr);
// the 8-wave split-precision kernel (pv_sdec_fused_w8x3.hip; images pre-scaled by 2 log2(e) like the plain 8-wave kernel's)
int pv_sdec_fused_w8x3_launch(const PvFused& f, int grid, bool grads, hipStream_t s, const PvDecChoice& c);   // c.x3_waves: 8 or 4
int64_t pv_sdec_fused_w8x3_park_bytes(int grid);
// the 8-wave fp16 kernel of the fp32-class path (pv_sdec_fused_w8h.hip; training launches; prep mode 2); c.ds: dL/dpre split
int pv_sdec_fused_w8h_launch(const PvFused& f, int grid, hipStream_t s, const PvDecChoice& c);
// sums the per-workgroup records (ascending workgroup order) into the flat gradient buffer
struct PvFusedOffsets { int64_t W1, b1, W2, b2, Wc, wo, bo; };
int pv_sdec_fused_reduce(const float* part, int grid, float* G, const PvFusedOffsets& o, int cd, int dwo_slots,
                         hipStream_t s);

// ---- the reduction's workgroup body (256 threads), shared with the launch that also hosts pv_latent_bwd -------
// 64 float4 outputs x 4 slices of the workgroup range per 256-thread block (a wave reads 1 KB per record, eight
// records in flight); slices combined in fixed order
#define PV_FUSED_REDUCE_BLOCKS (((2 * FD_H * FD_H + 5 * FD_H + 1 + 3) / 4 + 63) / 64)
// (round 6) Record FORMATS of the two HxH weight-gradient partials — a private contract between a decoder kernel's epilogue and
// this reduction; everything from float 2*H*H on (bias / coordinate / output-layer vectors) is the same in all of them:
//   PV_REC_ROWMAJOR  [m][row][col] fp32 (rounds 1-5; the f32-MFMA kernel and the experiments builds): a lane of the C/D layout
//                    holds ONE column of four rows, so every store instruction wrote 4 x 64-byte segments — 128 (64) scattered
//                    4-byte store instructions per wave, 6-12 k cycles of store issue per workgroup at the end of the launch;
//   PV_REC_LANE_F32  LANE-NATIVE fp32 (the 4-wave kernels of pv_sdec_fused_bf16.hip): chunk (16 bytes)
//                    [m][wave][s][kb][lane] = the lane's accumulator block accW_m[s][kb] as it sits in registers — rows
//                    16 (2 wave + s) + 4 q + i (i = 0..3), column 16 kb + r: ONE 1 KB-contiguous store instruction per block;
//   PV_REC_LANE_BF16 lane-native PACKED (the 8-wave throughput kernel, pv_sdec_fused_w8.hip): chunk [wave][s][o][lane] =
//                    {W1 rows (i0, i1), W1 rows (i2, i3), W2 rows (i0, i1), W2 rows (i2, i3)} as bf16 pairs — rows
//                    32 jp + 16 (s ^ kh) + 4 q + i, column 64 kh + 16 o + r (jp = wave >> 1, kh = wave & 1) — in the record's first H*H
//                    floats: half the bytes (the weights they update were rounded to bf16 in the forward anyway; the reader sums in
//                    fp32) and 8 store instructions per wave.
// The reduction reads 16 bytes per thread and record either way and writes each output element once; per element the records are
// summed in the same fixed order as before (four slices of ascending workgroups): the fp32 formats give the same bits.
#define PV_REC_ROWMAJOR 0
#define PV_REC_LANE_F32 1
#define PV_REC_LANE_BF16 2
#define PV_FUSED_REDUCE_VEC_BLOCKS (((5 * FD_H + 1 + 3) / 4 + 63) / 64)
#define PV_FUSED_REDUCE_MAT_BLOCKS_F32 ((2 * FD_H * FD_H / 4) / 64)                     // 128
#define PV_FUSED_REDUCE_MAT_BLOCKS_BF16 ((2 * (FD_H / 2) * FD_H / 4) / 64)              // 64
__host__ __device__ inline int pv_fused_reduce_mat_blocks(int fmt) {
  return fmt == PV_REC_LANE_BF16 ? PV_FUSED_REDUCE_MAT_BLOCKS_BF16 : PV_FUSED_REDUCE_MAT_BLOCKS_F32;
}
__host__ __device__ inline int pv_fused_reduce_blocks(int fmt) {
  return fmt == PV_REC_ROWMAJOR ? PV_FUSED_REDUCE_BLOCKS : pv_fused_reduce_mat_blocks(fmt) + PV_FUSED_REDUCE_VEC_BLOCKS;
}
// one block = 64 chunks = ONE accumulator block of one wave (thread c = lane c of that wave), four slices of the workgroup range
// a finished gradient element: into the flat gradient, or (ad: pv_ivae_step's optimizer riding in the reducing launch) straight
// through torch.optim.Adam's update of its parameter — the element's gradient slot is then left zeroed (pv_common.h: pv_adam_update)
#ifndef PV_RED_UNROLL
#define PV_RED_UNROLL 8          // records in flight per thread of a reducing block
#endif
struct PvRecAdam { PvAdamFuse a; int on; };       // (by value: the address of a kernel argument would put it in scratch memory)
// How a reducing block ends.  Its four waves hand their slice partials over through LDS ONCE (PvRedLds: 8 KB, one pv_lds_barrier —
// nothing but LDS is handed over) and then EVERY thread finalises its share of the block's elements: (s0 + s1) + (s2 + s3) of the
// element's four slice partials, then pv_rec_fin.  Which elements a thread finalises depends on the block and the thread alone, so
// with Adam riding in the launch the thread requests their p / m / v (cold: no earlier launch of the step touched them) right behind
// the loads of its LAST batch of records — the loop's last PV_RED_UNROLL records are peeled for that: the requests queue behind the
// record loads, a counted wait on those does not wait for them, and their round trip runs under the last batch's arrival and the LDS
// exchange; the update then runs on registers.  (Requested at block entry they sit at the head of an in-order queue: measured
// slower.  Before, wave 0 alone ran eight load -> update -> store chains per lane one after the other, behind the last barrier.)
typedef f32x4 PvRedLds[2][4][64];
struct PvRecOps { float p, m, v; };                // one element's Adam operands, requested ahead of its update
// (ADAM: ad.on as a template argument — the reducing bodies exist once per value, chosen at their entry: behind a run-time `if`
//  around the requests alone, the counted waits on the record loads would have to assume that nothing was issued after them)
template <bool ADAM>
__device__ __forceinline__ PvRecOps pv_rec_request(const float* __restrict__ Gr, int idx, const PvRecAdam& ad) {
  PvRecOps q = {0.0f, 0.0f, 0.0f};
  if (ADAM) { const int64_t i = (Gr - ad.a.g) + idx; q.p = ad.a.p[i]; q.m = ad.a.m[i]; q.v = ad.a.v[i]; }
  return q;
}
// pv_adam_update (pv_common.h) on operands already in registers: the same expressions in the same order — and the same ROUNDINGS.
// Which of the expressions' multiply-adds the compiler contracts depends on the code around them: in pv_adam_kernel (the separate
// optimizer launch these bytes are held to, tests/test_gpu_record_finalise.py) and in pv_adam_update as the reducing blocks inlined
// it before, the moments' products and sums stay separate instructions and the parameter's update is one fused multiply-add; with
// one element per thread it fused the moments' too (parameters one ulp off after three steps).  So the form is written out here.
__device__ __forceinline__ void pv_adam_update_ops(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t i, float gi, float pi, float mi, float vi,
                                                   float b1, float b2, float eps, float step_size, float bc2_sqrt) {
#pragma clang fp contract(off)
  mi = mi + (gi - mi) * (1.0f - b1);
  vi = vi * b2 + (1.0f - b2) * gi * gi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = __builtin_fmaf(-step_size, mi / denom, pi);      // pi - step_size * (mi / denom), one rounding
  m[i] = mi; v[i] = vi;
  g[i] = 0.0f;
}
template <bool ADAM>
__device__ __forceinline__ void pv_rec_fin(float* __restrict__ Gr, int idx, float v, const PvRecOps& q, const PvRecAdam& ad) {
  if (ADAM) pv_adam_update_ops(ad.a.p, ad.a.g, ad.a.m, ad.a.v, (Gr - ad.a.g) + idx, v, q.p, q.m, q.v, ad.a.b1, ad.a.b2, ad.a.eps,
                                ad.a.step_size, ad.a.bc2_sqrt);
  else Gr[idx] = v;
}
// the records [w0, w1) of a slice, in ascending order: all but the last PV_RED_UNROLL in the loop, those as one peeled batch whose
// loads are followed by `request` (a slice shorter than a batch runs the loop alone).  add(v) sums one record's chunk of type V
template <typename V, typename Add, typename Req>
__device__ __forceinline__ void pv_rec_stream(const float* __restrict__ p, int w0, int w1, Add add, Req request) {
  const bool peel = w1 - w0 >= PV_RED_UNROLL;
  const int wl = peel ? w1 - PV_RED_UNROLL : w1;
#pragma unroll PV_RED_UNROLL
  for (int w = w0; w < wl; ++w) add(*reinterpret_cast<const V*>(p + (int64_t)w * FD_REC));
  V t[PV_RED_UNROLL];
  if (peel) {
#pragma unroll
    for (int k = 0; k < PV_RED_UNROLL; ++k) t[k] = *reinterpret_cast<const V*>(p + (int64_t)(wl + k) * FD_REC);
  }
  request();
  if (peel) {
#pragma unroll
    for (int k = 0; k < PV_RED_UNROLL; ++k) add(t[k]);
  }
}
// Lane-native matrix blocks: thread (chunk c, slice sl) sums its slice of chunk c and then finalises component sl of that chunk —
// row row0(c >> 4) + sl, column col(c & 15) — of W1 and W2 (packed format) or of the block's one matrix (fp32 format): the 16 lanes
// that share a row write 16 consecutive columns.  LDS as float [matrix][slice][component][chunk]: a thread stores and loads at
// consecutive chunks, no bank conflicts either way.
template <int FMT, bool ADAM>
__device__ __forceinline__ void pv_sdec_fused_reduce_block_lane(const float* __restrict__ part, int G_, float* __restrict__ Gr,
                                                                const PvFusedOffsets& o, int block, f32x4 (*sm)[4][64],
                                                                const PvRecAdam& ad) {
  const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int per = (G_ + 3) / 4;
  const int w0 = sl * per, w1 = min(G_, w0 + per);
  const float* pbase = part + 4 * (block * 64 + c);
  float* lds = reinterpret_cast<float*>(sm);
  const int r = c & 15, q = c >> 4;
  int ia, ib = 0;                                                      // the thread's elements in the flat gradient
  if (FMT == PV_REC_LANE_BF16) {
    const int oo = block & 3, s_ = (block >> 2) & 1, wave = block >> 3, jp = wave >> 1, kh = wave & 1;
    const int row0 = 32 * jp + 16 * (s_ ^ kh) + 4 * q, col = 64 * kh + 16 * oo + r;
    ia = o.W1 + (row0 + sl) * FD_H + col;
    ib = o.W2 + (row0 + sl) * FD_H + col;
  } else {
    const int kb = block & 7, s_ = (block >> 3) & 1, wave = (block >> 4) & 3, m = block >> 6;
    const int row0 = 16 * (2 * wave + s_) + 4 * q, col = 16 * kb + r;
    ia = (m == 0 ? o.W1 : o.W2) + (row0 + sl) * FD_H + col;
  }
  f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 0.0f, 0.0f};
  PvRecOps qa = {0.0f, 0.0f, 0.0f}, qb = {0.0f, 0.0f, 0.0f};
  if (FMT == PV_REC_LANE_BF16) {
    typedef unsigned int u32x4_ __attribute__((ext_vector_type(4)));
    pv_rec_stream<u32x4_>(pbase, w0, w1, [&](const u32x4_ v) {
      a[0] += __uint_as_float(v[0] << 16); a[1] += __uint_as_float(v[0] & 0xffff0000u);
      a[2] += __uint_as_float(v[1] << 16); a[3] += __uint_as_float(v[1] & 0xffff0000u);
      b[0] += __uint_as_float(v[2] << 16); b[1] += __uint_as_float(v[2] & 0xffff0000u);
      b[2] += __uint_as_float(v[3] << 16); b[3] += __uint_as_float(v[3] & 0xffff0000u);
    }, [&]() { qa = pv_rec_request<ADAM>(Gr, ia, ad); qb = pv_rec_request<ADAM>(Gr, ib, ad); });
  } else {
    pv_rec_stream<f32x4>(pbase, w0, w1, [&](const f32x4 v) { a += v; }, [&]() { qa = pv_rec_request<ADAM>(Gr, ia, ad); });
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lds[(sl * 4 + i) * 64 + c] = a[i];
    if (FMT == PV_REC_LANE_BF16) lds[((4 + sl) * 4 + i) * 64 + c] = b[i];
  }
  pv_lds_barrier();
  const float* la = lds + sl * 64 + c;                                 // [slice s][component sl][chunk c] at la[s * 256]
  pv_rec_fin<ADAM>(Gr, ia, (la[0] + la[256]) + (la[512] + la[768]), qa, ad);
  if (FMT == PV_REC_LANE_BF16) pv_rec_fin<ADAM>(Gr, ib, (la[1024] + la[1280]) + (la[1536] + la[1792]), qb, ad);
}
// the flat-gradient index of element ei (< total) of a record read as plain floats, or -1 where the slot has no parameter (the
// second coordinate column with one coordinate)
__device__ __forceinline__ int pv_rec_elem_index(int ei, const PvFusedOffsets& o, int cd) {
  const int HH = FD_H * FD_H;
  if (ei < HH) return o.W1 + ei;
  if (ei < 2 * HH) return o.W2 + (ei - HH);
  const int k = ei - 2 * HH, seg = k / FD_H, j = k % FD_H;
  if (seg == 0) return o.b1 + j;
  if (seg == 1) return o.b2 + j;
  if (seg == 2) return o.Wc + j * cd;
  if (seg == 3) return cd == 2 ? (int)(o.Wc + j * 2 + 1) : -1;
  if (seg == 4) return o.wo + j;
  return o.bo;
}
template <bool ADAM>
__device__ __forceinline__ void pv_sdec_fused_reduce_block_on(const float* __restrict__ part, int G_,
                                                              float* __restrict__ Gr, const PvFusedOffsets& o, int cd,
                                                              int dwo_slots, int block, f32x4 (*sm)[4][64], int fmt,
                                                              const PvRecAdam& ad) {
  const int HH = FD_H * FD_H;
  const int total = 2 * HH + 5 * FD_H + 1;          // the record is padded well past this: whole float4s are readable
  const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
  if (fmt != PV_REC_ROWMAJOR && block < pv_fused_reduce_mat_blocks(fmt)) {
    if (fmt == PV_REC_LANE_BF16) pv_sdec_fused_reduce_block_lane<PV_REC_LANE_BF16, ADAM>(part, G_, Gr, o, block, sm, ad);
    else pv_sdec_fused_reduce_block_lane<PV_REC_LANE_F32, ADAM>(part, G_, Gr, o, block, sm, ad);
    return;
  }
  // (lane-native formats: the blocks behind the matrices' take the vectors, which sit at float 2*H*H in every format)
  // Thread (chunk c, slice sl) sums its slice of the four floats at e; thread t then finalises the ONE float e0 + t of the block's 256
  // (the chunks sit in LDS as they were summed, [slice][chunk]: thread t loads word t of each slice)
  const int e0 = fmt != PV_REC_ROWMAJOR ? 2 * HH + (block - pv_fused_reduce_mat_blocks(fmt)) * 256 : block * 256;
  const int e = e0 + 4 * c, ef = e0 + (int)threadIdx.x;
  const int idx = ef < total ? pv_rec_elem_index(ef, o, cd) : -1;
  const int per = (G_ + 3) / 4;
  const int w0 = sl * per, w1 = min(G_, w0 + per);
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  PvRecOps qf = {0.0f, 0.0f, 0.0f};
  // (a thread without an element requests element 0's: a branch round the requests would cost the counted waits, as above)
  const auto request = [&]() { qf = pv_rec_request<ADAM>(Gr, max(idx, 0), ad); };
  if (e >= total) request();
  else {
    const bool slots = dwo_slots && e >= 2 * HH + 4 * FD_H && e < 2 * HH + 5 * FD_H;   // d(wo): 8 per-wave slots
    if (slots) {
      for (int w = w0; w < w1; ++w) {
        const float* p8 = part + (int64_t)w * FD_REC + 2 * HH + 6 * FD_H + (e - (2 * HH + 4 * FD_H));
        f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < FD_WAVES; ++k) a += *reinterpret_cast<const f32x4*>(p8 + k * FD_H);
        v += a;
      }
      request();
    } else {
      pv_rec_stream<f32x4>(part + e, w0, w1, [&](const f32x4 x) { v += x; }, request);
    }
  }
  sm[0][sl][c] = v;
  pv_lds_barrier();
  if (idx < 0) return;
  const float* lf = reinterpret_cast<const float*>(sm) + threadIdx.x;
  pv_rec_fin<ADAM>(Gr, idx, (lf[0] + lf[256]) + (lf[512] + lf[768]), qf, ad);
}
__device__ __forceinline__ void pv_sdec_fused_reduce_block(const float* __restrict__ part, int G_,
                                                           float* __restrict__ Gr, const PvFusedOffsets& o, int cd,
                                                           int dwo_slots, int block, f32x4 (*sm)[4][64], int fmt = PV_REC_ROWMAJOR,
                                                           const PvRecAdam& ad = PvRecAdam{}) {
  if (ad.on) pv_sdec_fused_reduce_block_on<true>(part, G_, Gr, o, cd, dwo_slots, block, sm, fmt, ad);
  else pv_sdec_fused_reduce_block_on<false>(part, G_, Gr, o, cd, dwo_slots, block, sm, fmt, ad);
}


