// pv_out_lik_mc_body.inc — pv_elementwise.hip's out_lik_mc kernel, included once per likelihood family with
//   OLM_KERNEL  the __global__'s name        OLM_CAT  0: the per-value likelihoods (pv_lik_any), 1: PV_LIK_CATEGORICAL
// so that the per-value instances keep their name and their code, and the categorical ones carry no run-time switch.
template <int C>
__global__ __launch_bounds__(256) void OLM_KERNEL(PvOutLik p) {
  constexpr bool CAT = OLM_CAT != 0;
  static_assert(C >= 2 && C <= PV_MAX_CHANNELS, "channels per row");
  __shared__ float red[4][64 * OL_MAXJ];
  __shared__ float redb[4][PV_MAX_CHANNELS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = p.H;
  float wo[C][OL_MAXJ], acc[C][OL_MAXJ];
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int jj = 0; jj < OL_MAXJ; ++jj) {
      const int j = lane + 64 * jj;
      wo[c][jj] = j < H ? p.wo[c * H + j] : 0.0f;
      acc[c][jj] = 0.0f;
    }
  }
  const float bo = (p.bo && lane < C) ? p.bo[lane] : 0.0f;
  float accb = 0.0f;                                  // lane c: sum over the wave's rows of dL/da_c
  const int64_t rbeg = (int64_t)blockIdx.x * OL_ROWS + wave * (OL_ROWS / 4);
  for (int i = 0; i < OL_ROWS / 4; ++i) {
    const int64_t row = rbeg + i;
    if (row >= p.M) break;
    const float* hr = p.h + row * p.ldh;
    float hv[OL_MAXJ];
#pragma unroll
    for (int jj = 0; jj < OL_MAXJ; ++jj) {
      const int j = lane + 64 * jj;
      hv[jj] = j < H ? hr[j] : 0.0f;
    }
    // (the lane index made opaque per row: hoisted out of the row loop, the C masks of `lane == c` would be scalar spills)
    int lv = lane;
    asm volatile("" : "+v"(lv));
    float a = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float dot = 0.0f;
#pragma unroll
      for (int jj = 0; jj < OL_MAXJ; ++jj) dot += hv[jj] * wo[c][jj];
      dot = pv_wave_sum(dot);
      if (lv == c) a = dot;
    }
    a += bo;
    float ll = 0.0f, dlda = 0.0f, locv = 0.0f;
    if (CAT) {
      float xw = 0.0f;                                   // the weighted observation of lane c's class
      if (lane < C) {
        xw = p.x ? p.x[(p.xmod > 0 ? row % p.xmod : row) * C + lane] : 0.0f;
        if (p.pw) xw *= p.pw[(p.pw_img ? row : row % p.N) * C + lane];
      }
      float mx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 0));
#pragma unroll
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), c)));
      const float e = expf(a - mx);                      // <= 1: no overflow at any logit
      float se = 0.0f, sx = 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        se += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), c));
        sx += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xw), c));
      }
      if (lane < C) {
        locv = e / se;
        ll = xw * (a - (mx + logf(se)));                 // log p_c = a_c - lse, never log(p_c): xw = 0 gives exactly 0
        dlda = locv * sx - xw;
        if (p.loc) p.loc[row * C + lane] = locv;
        if (p.sw) dlda *= p.sw[row / p.N];
      }
    } else if (lane < C) {
      const float x = p.x ? p.x[(p.xmod > 0 ? row % p.xmod : row) * C + lane] : 0.0f;
      pv_lik_any(a, x, p.lik, p.sigmoid_out, p.sig, ll, dlda, locv);
      if (p.loc) p.loc[row * C + lane] = locv;
      if (p.pw) {                                        // per-observation weight (pv_ivae_weighted_*)
        const float w = p.pw[(p.pw_img ? row : row % p.N) * C + lane];
        ll *= w;
        dlda *= w;
      }
      if (p.sw) dlda *= p.sw[row / p.N];
    }
    if (p.llrow) {
      float s = 0.0f;
#pragma unroll
      for (int c = 0; c < C; ++c) s += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ll), c));
      if (lane == 0) p.llrow[row] = s;
    }
    if (p.dpre) {
      float d[C];
#pragma unroll
      for (int c = 0; c < C; ++c) d[c] = __shfl(dlda, c);      // (vector registers: eight more scalars would spill)
      float* dr = p.dpre + row * p.ldh;
      const float* pr_ = p.hpre ? p.hpre + row * p.ldh : nullptr;
#pragma unroll
      for (int jj = 0; jj < OL_MAXJ; ++jj) {
        const int j = lane + 64 * jj;
        if (j < H) {
          float g = 0.0f;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            g += d[c] * wo[c][jj];
            acc[c][jj] += d[c] * hv[jj];
          }
          dr[j] = g * pv_act_grad2(hv[jj], pr_ ? pr_[j] : 0.0f, p.act_last);
        }
      }
      accb += dlda;
    }
  }
  if (!p.dpre) return;
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int jj = 0; jj < OL_MAXJ; ++jj) red[wave][lane + 64 * jj] = acc[c][jj];
    __syncthreads();
    for (int j = threadIdx.x; j < H; j += 256)
      p.part_dwo[((int64_t)blockIdx.x * C + c) * H + j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
    __syncthreads();
  }
  if (lane < C) redb[wave][lane] = accb;
  __syncthreads();
  if (threadIdx.x < C)
    p.part_dbo[(int64_t)blockIdx.x * C + threadIdx.x] =
        (redb[0][threadIdx.x] + redb[1][threadIdx.x]) + (redb[2][threadIdx.x] + redb[3][threadIdx.x]);
}

