// pv_linear.hip — the generic nn.Linear / kernel-3 convolution building blocks: GEMM problems (pv_gemm.hip) with fused epilogues.
// Declared in pv_linear.h for the orchestration units; pv_linear_* are the C entry points (include/pyroved_amd.h).
#include "pv_common.h"
#include "pv_linear.h"

int64_t gemm_ws_need(int64_t M, int64_t N, int64_t K) {
  const int s = pv_gemm_pick_splits((int)M, (int)N, (int)K);
  return s > 1 ? (int64_t)s * M * (N + 1) * (int64_t)sizeof(float) : 0;     // + row-sum partials
}

// y = act(x W^T + b)
int linear_fwd(const float* x, int64_t ldx, const float* W, const float* b, float* y, float* pre, int64_t ldy,
               int64_t M, int64_t K, int64_t N, int act, void* ws, int64_t wsb, hipStream_t s) {
  PvGemm g{};
  g.A = x; g.a_rs = ldx; g.a_cs = 1;
  g.B = W; g.b_rs = 1; g.b_cs = K;            // B(k,n) = W[n][k]
  g.C = y; g.ldc = ldy; g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.bias = b; g.act = act; g.pre = pre;
  return pv_gemm(g, pv_gemm_pick_splits((int)M, (int)N, (int)K), ws, wsb, s);
}

// dx = (dpre W) * act'(xact)
int linear_dgrad(const float* dpre, int64_t lddp, const float* W, float* dx, int64_t lddx, const float* xact,
                 const float* xpre, int64_t ldxa, int act_prev, int64_t M, int64_t K, int64_t N, void* ws, int64_t wsb,
                 hipStream_t s) {
  PvGemm g{};
  g.A = dpre; g.a_rs = lddp; g.a_cs = 1;      // (M, N)
  g.B = W; g.b_rs = K; g.b_cs = 1;            // B(n,k) = W[n][k]
  g.C = dx; g.ldc = lddx; g.M = (int)M; g.N = (int)K; g.K = (int)N;
  g.act = PV_ACT_NONE;
  if (act_prev != PV_ACT_NONE) { g.aux = xact; g.auxpre = xpre; g.ldaux = ldxa; g.act_aux = act_prev; }
  return pv_gemm(g, pv_gemm_pick_splits((int)M, (int)K, (int)N), ws, wsb, s);
}

// dw = dpre^T x ; db = colsum(dpre)
int linear_wgrad(const float* dpre, int64_t lddp, const float* x, int64_t ldx, float* dw, float* db, int64_t M,
                 int64_t K, int64_t N, void* ws, int64_t wsb, hipStream_t s) {
  if (dw) {
    PvGemm g{};
    g.A = dpre; g.a_rs = 1; g.a_cs = lddp;    // A(n, row) = dpre[row][n]
    g.B = x; g.b_rs = ldx; g.b_cs = 1;        // B(row, k) = x[row][k]
    g.C = dw; g.ldc = K; g.M = (int)N; g.N = (int)K; g.K = (int)M;
    g.act = PV_ACT_NONE;
    g.rowsumA = db;                            // db[n] = sum_rows dpre[row][n], fused into the same pass
    PV_TRY(pv_gemm(g, pv_gemm_pick_splits((int)N, (int)K, (int)M), ws, wsb, s));
    return 0;
  }
  if (db) PV_TRY(pv_colsum(dpre, lddp, M, (int)N, db, ws, wsb, s));
  return 0;
}

// ---- convolutions (kernel 3, padding 1, stride 1; channels-last) as GEMMs over an IMPLICIT im2col operand ----
// y[(b,y,x)][co] = act(sum_j patch[(b,y,x)][j] W[co][j] + b[co]),  j = ci*KK + tap;  W = the torch weight as it lies
int conv3_fwd(const float* in, int B, int H, int W_, int C, int nd, const float* W, const float* b, float* y, int Cout,
              int act, void* ws, int64_t wsb, hipStream_t s) {
  const int64_t rows = (int64_t)B * H * W_, K = (int64_t)C * (nd == 2 ? 9 : 3);
  PvGemm g{};
  g.A = in; g.a_rs = K; g.a_cs = 1; g.conv_a = 1; g.cH = H; g.cW = W_; g.cC = C; g.cnd = nd;
  g.B = W; g.b_rs = 1; g.b_cs = K;
  g.C = y; g.ldc = Cout; g.M = (int)rows; g.N = Cout; g.K = (int)K;
  g.bias = b; g.act = act;
  return pv_gemm(g, pv_gemm_pick_splits((int)rows, Cout, (int)K), ws, wsb, s);
}

// dw[co][j] = sum_rows dpre[row][co] patch[row][j] ; db[co] = sum_rows dpre[row][co]
int conv3_wgrad(const float* dpre, const float* in, int B, int H, int W_, int C, int nd, float* dw, float* db, int Cout,
                void* ws, int64_t wsb, hipStream_t s) {
  const int64_t rows = (int64_t)B * H * W_, K = (int64_t)C * (nd == 2 ? 9 : 3);
  PvGemm g{};
  g.A = dpre; g.a_rs = 1; g.a_cs = Cout;
  g.B = in; g.b_rs = K; g.b_cs = 1; g.conv_b = 1; g.cH = H; g.cW = W_; g.cC = C; g.cnd = nd;
  g.C = dw; g.ldc = K; g.M = Cout; g.N = (int)K; g.K = (int)rows;
  g.act = PV_ACT_NONE;
  g.rowsumA = db;
  return pv_gemm(g, pv_gemm_pick_splits(Cout, (int)K, (int)rows), ws, wsb, s);
}

// ---- building blocks -------------------------------------------------------------------------
extern "C" int64_t pv_linear_workspace_bytes(int64_t M, int64_t K, int64_t N) {
  if (M < 0 || K <= 0 || N <= 0) return PV_EINVAL;
  int64_t need = gemm_ws_need(M, N, K);
  const int64_t a = gemm_ws_need(M, K, N), b = gemm_ws_need(N, K, M), c = pv_colsum_ws(M, (int)N);
  if (a > need) need = a;
  if (b > need) need = b;
  if (c > need) need = c;
  return pv_align_up(need, 256);
}

extern "C" int pv_linear_fwd(const float* x, int64_t ldx, const float* w, const float* b, float* y, float* pre,
                             int64_t ldy, int64_t M, int64_t K, int64_t N, int act, void* ws, int64_t ws_bytes,
                             void* stream) {
  if (!x || !w || !y || M < 0 || K <= 0 || N <= 0) return PV_EINVAL;
  return linear_fwd(x, ldx, w, b, y, pre, ldy, M, K, N, act, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int pv_linear_bwd(const float* dpre, int64_t lddp, const float* x, int64_t ldx, const float* w, float* dx,
                             int64_t lddx, const float* xact, const float* xpre, int64_t ldxa, int act_prev, float* dw,
                             float* db, int64_t M, int64_t K, int64_t N, void* ws, int64_t ws_bytes, void* stream) {
  if (!dpre || M < 0 || K <= 0 || N <= 0) return PV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (dx) {
    if (!w) return PV_EINVAL;
    PV_TRY(linear_dgrad(dpre, lddp, w, dx, lddx, xact, xpre, ldxa, act_prev, M, K, N, ws, ws_bytes, s));
  }
  if (dw || db) {
    if (dw && !x) return PV_EINVAL;
    PV_TRY(linear_wgrad(dpre, lddp, x, ldx, dw, db, M, K, N, ws, ws_bytes, s));
  }
  return 0;
}
