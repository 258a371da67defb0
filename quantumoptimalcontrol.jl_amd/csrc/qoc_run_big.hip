// qoc_run_big.hip — the large-N batched-GEMM pipeline (qoc_bgemm.hpp), the GEMM-shaped order-3 gradient and the
// exact (Fréchet) gradient (qoc_frechet.hpp).
#include <type_traits>
#include "qoc_bgemm.hpp"
#include "qoc_frechet.hpp"
#include "qoc_internal.hpp"

#include <complex>

namespace qoc_host {

// =============================================================================================
// Large-N path: chunked batched-GEMM pipeline (N beyond the LDS-resident kernels).
//   propagate : per chunk of slices  k_form_norm -> Padé products (6 GEMMs for d = 13, fused
//               lincomb epilogues) -> Newton-Schulz solve of (V-U) X = (V+U) (all GEMM) ->
//               squarings;  then the forward chain as Nt batched GEMMs over the seeds.
//   sensitivity: backward chain as Nt batched U^H GEMMs; per chunk P_a = X^a x, Q_b = (X^H)^b λ,
//               W_a = sum_b Q_b/(a+b+1)!, M' = W P^H (one GEMM, K = order*m), dJdu = Re<A_j, M'>.
// =============================================================================================
static const double hPade3[4] = {120.0, 60.0, 12.0, 1.0};
static const double hPade5[6] = {30240.0, 15120.0, 3360.0, 420.0, 30.0, 1.0};
static const double hPade7[8] = {17297280.0, 8648640.0, 1995840.0, 277200.0, 25200.0, 1512.0, 56.0, 1.0};
static const double hPade9[10] = {17643225600.0, 8821612800.0, 2075673600.0, 302702400.0, 30270240.0,
                                  2162160.0, 110880.0, 3960.0, 90.0, 1.0};
static const double hPade13[14] = {64764752532480000.0, 32382376266240000.0, 7771770303897600.0,
                                   1187353796428800.0, 129060195264000.0, 10559470521600.0,
                                   670442572800.0, 33522128640.0, 1323241920.0, 40840800.0,
                                   960960.0, 16380.0, 182.0, 1.0};

size_t big_ws_elems_per_item(int N, int m) {
  const size_t NN = (size_t)N * N, Nm = (size_t)N * m;
  return std::max(8 * NN, 2 * NN + 11 * Nm);
}

Opd mk_opd(const void* base, size_t elem_off, size_t esz, long long inner, int per = 0, long long outer = 0,
           int u0 = 0) {
  Opd o;
  o.p = (const char*)base + elem_off * esz;
  o.inner = inner;
  o.per = per;
  o.outer = outer;
  o.u0 = u0;
  return o;
}

GemmArgs gemm_args(int M, int K, int Ncol, int nitems) {
  GemmArgs g;
  std::memset(&g, 0, sizeof(g));
  g.M = M;
  g.K = K;
  g.Ncol = Ncol;
  g.nitems = nitems;
  g.alpha1 = 1.0;
  return g;
}

template <typename T>
int big_gemm(qoc_ctx* c, int opa, int opb, GemmArgs g, int mode = 0) {
  g.tiles_m = (g.M + BG_BM - 1) / BG_BM;
  g.tiles = g.tiles_m * ((g.Ncol + BG_BN - 1) / BG_BN);
  const long long total = (long long)g.nitems * g.tiles;
  if (total <= 0 || total >= (1LL << 31)) return fail(c, QOC_ERR_ARG, "GEMM grid out of range");
  const dim3 grid((unsigned)total), blk(BG_THREADS);
  qoc_ctx::GMark gm{nullptr, nullptr, 8.0 * g.M * (double)g.K * g.Ncol * g.nitems};
  if (c->profiling) {
    gm.a = take_event(c);
    gm.b = take_event(c);
    (void)hipEventRecord(gm.a, c->stream);
  }
  // fp32 products with K % 16 == 0 and even M, Ncol: the LDS-DMA staged kernel (QOC_BGEMM_GLDS=0 keeps k_bgemm)
  static const bool glds_env = env_int("QOC_BGEMM_GLDS", 1) != 0;
  const bool glds = std::is_same<T, float>::value && mode == 0 && glds_env && g.K >= 16 && g.K % 16 == 0 && g.M % 2 == 0 &&
                    g.Ncol % 2 == 0 && g.M >= 2 && g.Ncol >= 2;
  if (glds) {
    if (opa == 0 && opb == 0) hipLaunchKernelGGL((k_bgemm_glds<0, 0>), grid, blk, 0, c->stream, g);
    else if (opa == 1 && opb == 0) hipLaunchKernelGGL((k_bgemm_glds<1, 0>), grid, blk, 0, c->stream, g);
    else if (opa == 0 && opb == 1) hipLaunchKernelGGL((k_bgemm_glds<0, 1>), grid, blk, 0, c->stream, g);
    else hipLaunchKernelGGL((k_bgemm_glds<1, 1>), grid, blk, 0, c->stream, g);
  } else if (mode == 1) hipLaunchKernelGGL((k_bgemm<T, 0, 0, true, 1, 2, 1>), grid, blk, 0, c->stream, g);
  else if (mode == 2) hipLaunchKernelGGL((k_bgemm<T, 0, 0, true, 1, 2, 2>), grid, blk, 0, c->stream, g);
  else if (opa == 0 && opb == 0) hipLaunchKernelGGL((k_bgemm<T, 0, 0>), grid, blk, 0, c->stream, g);
  else if (opa == 1 && opb == 0) hipLaunchKernelGGL((k_bgemm<T, 1, 0>), grid, blk, 0, c->stream, g);
  else if (opa == 0 && opb == 1) hipLaunchKernelGGL((k_bgemm<T, 0, 1>), grid, blk, 0, c->stream, g);
  else hipLaunchKernelGGL((k_bgemm<T, 1, 1>), grid, blk, 0, c->stream, g);
  HIPCHK(c, hipGetLastError());
  if (c->profiling) {
    (void)hipEventRecord(gm.b, c->stream);
    c->gmarks.push_back(gm);
  }
  return QOC_OK;
}

template <typename T>
int big_lincomb(qoc_ctx* c, LinArgs a) {
  const size_t total = (size_t)a.rows * a.cols * a.nitems;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL((k_lincomb<T>), dim3(blocks), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}

// exp(A_k) for units [u0, u0+cnt) -> d_U.  Workspace buffers w(i), i < 8, of cnt x N x N.
// Paterson-Stockmeyer degree m = 3r + 2 (r = 2..8): the largest ||A||_1 whose Taylor tail sum_{k>m} ||A||^k / k!
// is <= 2^-53 (fp64) or 2^-24 (fp32, the unit roundoff of the arithmetic the fp32 pipeline runs in)
static const double hTaylorTheta[7] = {0.069933, 0.247240, 0.553491, 0.978345, 1.504147, 2.113468, 2.791345};
static const double hTaylorTheta32[7] = {0.648322, 1.31065, 2.099345, 2.969587, 3.894655, 4.858047, 5.849147};

// T12 on the GEMM pipeline: Â = A / 2^s, Â2 = Â², A3 = Â2 Â, B_j = x_j0 I + x_j1 Â + x_j2 Â2 + x_j3 A3,
// A6 = B3 + B4², T12 = B1 + (B2 + A6) A6, then s squarings.  Each B_j comes out of the A3 product's epilogue
// (B1, B4, B3: its three outputs); B2 is carried as B2 = β B3 + (x_20 I + (x_21 − β x_31) Â + (x_22 − β x_32) Â2)
// with β = x_23 / x_33, so that B2 + A6 leaves the B4² product's epilogue next to A6 (three addends).
// Host copy of kT12 (qoc_expm.hpp).
static const double hT12[4][4] = {
    {1.0, 0.99999999999276613715098, -0.13243184210109929356121, -0.050548416421727518977426},
    {5.5174437753406856228547, 1.3093238729673181077940, 0.0043247187525051520919919, 0.0096586056829351321677927},
    {0.0, 1.3110895450078318461208e-12, 0.097250029534075019542638, 0.0068219250901116764187357},
    {0.0, 0.13181061013830184015682, 0.020278555405892590793357, 0.0067595184686308635977856}};

// Degree-8 Taylor polynomial in 3 products (the m = 8 scheme of Bader, Blanes & Casas 2019; coefficients re-derived
// by tools/derive_t8.py, exact to 60 digits):  A2 = Â², A4 = A2 (x1 Â + x2 A2),
// A8 = (x3 A2 + A4)(x4 I + x5 Â + x6 A2 + x7 A4),  T8 = I + Â + y2 A2 + A8 = Σ_{k<=8} Â^k / k!.
static const double hT8x[7] = {0.01992047682223989399948029, 0.004980119205559973499870072, 0.1225521150112074730916119,
                               2.974307204847626663750796,  0.8765009801785553359771326,  0.07665265321119146690319094,
                               1.0};
static const double hT8y2 = 0.1354923613528506316624289;
// largest ||A|| whose degree-8 Taylor tail Σ_{k>8} ||A||^k / k! is <= 2^-24 (fp32) / 2^-53 (fp64): PS r = 2's
static const double kTheta8_32 = 0.648322, kTheta8_64 = 0.069933;

template <typename T>
int t8_gemm_chunk(qoc_ctx* c, int N, int cnt, void* ws, size_t ws_items, const Opd& Asrc, const Opd& dest, int ts,
                  bool count_hist) {
  const size_t NN = (size_t)N * N, esz = c->esz;
  auto w = [&](int i) { return mk_opd(ws, (size_t)i * ws_items * NN, esz, (long long)NN); };
  if (count_hist) c->big_thist[8 * 64 + std::min(ts, 63)] += cnt;  // row 8: T8
  const double sc = std::ldexp(1.0, -ts);
  const double* x = hT8x;
  int r;
  GemmArgs g = gemm_args(N, N, N, cnt);  // A2 = sc² A A -> w1;  P = x1 Â + x2 A2 -> w2
  g.A = Asrc; g.B = Asrc; g.C1 = w(1); g.alpha1 = sc * sc;
  g.C2 = w(2); g.alpha2 = x[1] * sc * sc; g.nY = 1; g.Y[0] = Asrc; g.w2[0] = x[0] * sc;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  g = gemm_args(N, N, N, cnt);  // A4 = A2 P:  L = x3 A2 + A4 -> w3,  R = x7 A4 + x6 A2 + x5 Â + x4 I -> w4
  g.A = w(1); g.B = w(2);
  g.nY = 2; g.Y[0] = w(1); g.Y[1] = Asrc;
  g.C1 = w(3); g.alpha1 = 1.0; g.w1[0] = x[2];
  g.C2 = w(4); g.alpha2 = x[6]; g.w2[0] = x[5]; g.w2[1] = x[4] * sc; g.gamma2 = x[3];
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  g = gemm_args(N, N, N, cnt);  // T8 = L R + y2 A2 + Â + I
  g.A = w(3); g.B = w(4); g.C1 = ts == 0 ? dest : w(7);
  g.nY = 2; g.Y[0] = w(1); g.w1[0] = hT8y2; g.Y[1] = Asrc; g.w1[1] = sc; g.gamma1 = 1.0;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  int xb = 7;
  for (int q = 0; q < ts; ++q) {
    const int nb = xb == 7 ? 1 : 7;
    g = gemm_args(N, N, N, cnt);
    g.A = w(xb); g.B = w(xb); g.C1 = q == ts - 1 ? dest : w(nb);
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;
    xb = nb;
  }
  return QOC_OK;
}

template <typename T>
int t12_gemm_chunk(qoc_ctx* c, int N, int cnt, void* ws, size_t ws_items, const Opd& Asrc, const Opd& dest, int ts,
                   bool count_hist) {
  const size_t NN = (size_t)N * N, esz = c->esz;
  auto w = [&](int i) { return mk_opd(ws, (size_t)i * ws_items * NN, esz, (long long)NN); };
  if (count_hist) c->big_thist[kT12Row * 64 + std::min(ts, 63)] += cnt;
  const double sc = std::ldexp(1.0, -ts), (*x)[4] = hT12, beta = x[1][3] / x[2][3];
  int r;
  GemmArgs g = gemm_args(N, N, N, cnt);  // Â2 -> w1
  g.A = Asrc; g.B = Asrc; g.C1 = w(1); g.alpha1 = sc * sc;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  g = gemm_args(N, N, N, cnt);  // A3 = sc Â2 A:  B1 -> w2, B4 -> w3, B3 -> w4
  g.A = w(1); g.B = Asrc;
  g.nY = 2; g.Y[0] = Asrc; g.Y[1] = w(1);
  g.C1 = w(2); g.alpha1 = x[0][3] * sc; g.w1[0] = x[0][1] * sc; g.w1[1] = x[0][2]; g.gamma1 = x[0][0];
  g.C2 = w(3); g.alpha2 = x[3][3] * sc; g.w2[0] = x[3][1] * sc; g.w2[1] = x[3][2]; g.gamma2 = x[3][0];
  g.C3 = w(4); g.alpha3 = x[2][3] * sc; g.w3[0] = x[2][1] * sc; g.w3[1] = x[2][2]; g.gamma3 = x[2][0];
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  g = gemm_args(N, N, N, cnt);  // B4²:  A6 = B4² + B3 -> w5,  B2 + A6 -> w6
  g.A = w(3); g.B = w(3);
  g.nY = 3; g.Y[0] = w(4); g.Y[1] = Asrc; g.Y[2] = w(1);
  g.C1 = w(5); g.w1[0] = 1.0;
  g.C2 = w(6); g.alpha2 = 1.0; g.w2[0] = 1.0 + beta; g.w2[1] = (x[1][1] - beta * x[2][1]) * sc;
  g.w2[2] = x[1][2] - beta * x[2][2]; g.gamma2 = x[1][0];
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  g = gemm_args(N, N, N, cnt);  // T12 = (B2 + A6) A6 + B1
  g.A = w(6); g.B = w(5); g.C1 = ts == 0 ? dest : w(7);
  g.nY = 1; g.Y[0] = w(2); g.w1[0] = 1.0;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  int xb = 7;
  for (int q = 0; q < ts; ++q) {
    const int nb = xb == 7 ? 1 : 7;
    g = gemm_args(N, N, N, cnt);
    g.A = w(xb); g.B = w(xb); g.C1 = q == ts - 1 ? dest : w(nb);
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;
    xb = nb;
  }
  return QOC_OK;
}

// Taylor / Paterson-Stockmeyer exponential on the GEMM pipeline (the large-N analogue of k_expm ALG 1):
// degree m = 3r + 2 with (r, s) minimising 2 + r + s for the chunk's max norm; every B_i = c I + c' A + c'' A2
// is added in a GEMM epilogue, so the chunk costs exactly 2 + r + s GEMMs and no element-wise pass.
template <typename T>
int taylor_gemm_chunk(qoc_ctx* c, int N, int cnt, void* ws, size_t ws_items, const Opd& Asrc, const Opd& dest,
                      double nA, bool count_hist) {
  const size_t NN = (size_t)N * N, esz = c->esz;
  auto w = [&](int i) { return mk_opd(ws, (size_t)i * ws_items * NN, esz, (long long)NN); };
  int tr = 2, ts = 0, best = 1 << 30;
  const double* th = sizeof(T) == 4 ? hTaylorTheta32 : hTaylorTheta;
  for (int rr = 2; rr <= 8; ++rr) {
    const int ss = nA > th[rr - 2] ? (int)std::ceil(std::log2(nA / th[rr - 2])) : 0;
    if (2 + rr + ss < best || (2 + rr + ss == best && ss < ts)) {
      best = 2 + rr + ss;
      tr = rr;
      ts = ss;
    }
  }
  // Degree-12 Taylor in 4 products (the T12 scheme of k_expm_rr, coefficients kT12) when it needs fewer GEMMs:
  // 4 + s12 with θ12 = 1.5622 in fp32 (tail <= 2^-24) / kTheta12 in fp64.  Synthetic slices (||A||_1 in
  // (3.1, 4.2]): 6 GEMMs instead of Paterson-Stockmeyer's 7.
  const double th12 = sizeof(T) == 4 ? 1.562211457125874 : kTheta12;
  const int s12 = nA > th12 ? (int)std::ceil(std::log2(nA / th12)) : 0;
  // degree 8 in 3 products (T8) when 3 + s8 GEMMs beat both: synthetic slices (2-norm bound 0.58 <= θ8 = 0.648 in
  // fp32) need no squaring
  const double th8 = sizeof(T) == 4 ? kTheta8_32 : kTheta8_64;
  const int s8 = nA > th8 ? (int)std::ceil(std::log2(nA / th8)) : 0;
  const bool t12ok = !env_set("QOC_BIG_NO_T12");
  if (3 + s8 < best && (!t12ok || 3 + s8 <= 4 + s12) && !env_set("QOC_BIG_NO_T8"))
    return t8_gemm_chunk<T>(c, N, cnt, ws, ws_items, Asrc, dest, s8, count_hist);
  if (4 + s12 < best && t12ok) return t12_gemm_chunk<T>(c, N, cnt, ws, ws_items, Asrc, dest, s12, count_hist);
  if (count_hist) c->big_thist[(tr - 2) * 64 + std::min(ts, 63)] += cnt;
  static const double f[27] = {1.0, 1.0, 0.5, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320,
                               2.755731922398589e-06, 2.755731922398589e-07, 2.505210838544172e-08,
                               2.08767569878681e-09, 1.6059043836821613e-10, 1.1470745597729725e-11,
                               7.647163731819816e-13, 4.779477332387385e-14, 2.8114572543455206e-15,
                               1.5619206968586225e-16, 8.22063524662433e-18, 4.110317623312165e-19,
                               1.9572941063391263e-20, 8.896791392450574e-22, 3.8681701706306835e-23,
                               1.6117375710961184e-24, 6.446950284384474e-26, 2.4795962632247976e-27};
  const double sc = std::ldexp(1.0, -ts);
  int r;
  // Â2 = sc^2 A A -> w1
  GemmArgs g = gemm_args(N, N, N, cnt);
  g.A = Asrc; g.B = Asrc; g.C1 = w(1); g.alpha1 = sc * sc;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  // Â3 = sc Â2 A -> w2, and B_r = c_{3r} I + c_{3r+1} Â + c_{3r+2} Â2 -> w3 from the epilogue
  g = gemm_args(N, N, N, cnt);
  g.A = w(1); g.B = Asrc; g.C1 = w(2); g.alpha1 = sc;
  g.nY = 2; g.Y[0] = Asrc; g.Y[1] = w(1);
  g.C2 = w(3); g.alpha2 = 0.0; g.w2[0] = f[3 * tr + 1] * sc; g.w2[1] = f[3 * tr + 2]; g.gamma2 = f[3 * tr];
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  int cur = 3;
  for (int i = tr - 1; i >= 0; --i) {  // cur <- Â3 cur + B_i  (polynomials in A commute)
    const int nxt = cur == 3 ? 4 : 3;
    g = gemm_args(N, N, N, cnt);
    g.A = w(2); g.B = w(cur);
    g.C1 = (i == 0) ? (ts == 0 ? dest : w(6)) : w(nxt);
    g.nY = 2; g.Y[0] = Asrc; g.Y[1] = w(1);
    g.w1[0] = f[3 * i + 1] * sc; g.w1[1] = f[3 * i + 2]; g.gamma1 = f[3 * i];
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;
    cur = nxt;
  }
  int xb = 6;
  for (int q = 0; q < ts; ++q) {
    const int nb = xb == 6 ? 7 : 6;
    g = gemm_args(N, N, N, cnt);
    g.A = w(xb); g.B = w(xb); g.C1 = q == ts - 1 ? dest : w(nb);
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;
    xb = nb;
  }
  return QOC_OK;
}

// exp of cnt explicit n x n matrices (operand Asrc, chunk max 1-norm nA) -> dest, all GEMM:
// Padé (Higham 2005 degree / squarings for nA) + Newton-Schulz solve + squarings.  Workspace:
// 8 buffers of ws_items x n x n at ws; red >= cnt doubles.
template <typename T>
int expm_gemm_chunk(qoc_ctx* c, int N, int cnt, void* ws, size_t ws_items, double* red, const Opd& Asrc,
                    const Opd& dest, double nA, bool count_hist, double nA_exec = -1.0) {
  const size_t NN = (size_t)N * N, esz = c->esz;
  auto w = [&](int i) { return mk_opd(ws, (size_t)i * ws_items * NN, esz, (long long)NN); };
  int r;
  // Padé degree / squarings: the thresholds of k_expm (Higham 2005), one (d, s) per chunk chosen
  // from the chunk's largest norm (any degree >= the per-slice choice meets the same bound).  Counted
  // for the reference-equivalent accounting whichever algorithm runs.
  int d, sq = 0;
  if (nA <= 2.1) {
    d = nA > 0.95 ? 9 : nA > 0.25 ? 7 : nA > 0.015 ? 5 : 3;
  } else {
    d = 13;
    const double sl = std::log2(nA / 5.4);
    sq = sl > 0 ? (int)std::ceil(sl) : 0;
  }
  const int di = d == 3 ? 0 : d == 5 ? 1 : d == 7 ? 2 : d == 9 ? 3 : 4;
  if (count_hist) c->big_hist[di * 64 + std::min(sq, 63)] += cnt;
  // the executed Taylor scheme may use a tighter norm bound (nA_exec: the 2-norm bound of skew-Hermitian slices);
  // the Padé (d, s) above is the reference's 1-norm choice, kept for the reference-equivalent accounting
  if (c->expm_alg != 0)
    return taylor_gemm_chunk<T>(c, N, cnt, ws, ws_items, Asrc, dest, nA_exec >= 0.0 ? std::min(nA, nA_exec) : nA,
                                count_hist);
  const double* C = d == 3 ? hPade3 : d == 5 ? hPade5 : d == 7 ? hPade7 : d == 9 ? hPade9 : hPade13;
  const double sc = std::ldexp(1.0, -sq);
  GemmArgs g;
  // buffers: 0 A, 1 A2, 2 A4, 3 A6, 4 T1/A8, 5 T2, 6 U', 7 V
  g = gemm_args(N, N, N, cnt);
  g.A = Asrc; g.B = Asrc; g.C1 = w(1); g.alpha1 = sc * sc;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;  // A2
  if (d == 13) {
    g = gemm_args(N, N, N, cnt);
    g.A = w(1); g.B = w(1); g.C1 = w(2);
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;  // A4
    // A6 = A2 A4, with T1 = c13 A6 + c11 A4 + c9 A2 and T2 = c12 A6 + c10 A4 + c8 A2 from its epilogue
    g.A = w(1); g.B = w(2); g.C1 = w(3); g.C2 = w(4); g.C3 = w(5);
    g.nY = 2; g.Y[0] = w(2); g.Y[1] = w(1);
    g.alpha2 = C[13]; g.w2[0] = C[11]; g.w2[1] = C[9];
    g.alpha3 = C[12]; g.w3[0] = C[10]; g.w3[1] = C[8];
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;
    g = gemm_args(N, N, N, cnt);
    g.A = w(3); g.B = w(4); g.C1 = w(6);
    g.nY = 3; g.Y[0] = w(3); g.Y[1] = w(2); g.Y[2] = w(1);
    g.w1[0] = C[7]; g.w1[1] = C[5]; g.w1[2] = C[3]; g.gamma1 = C[1];
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;  // U' = A6 T1 + c7 A6 + c5 A4 + c3 A2 + c1 I
    g.B = w(5); g.C1 = w(7);
    g.w1[0] = C[6]; g.w1[1] = C[4]; g.w1[2] = C[2]; g.gamma1 = C[0];
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;  // V
  } else {
    // powers A^{2k} = A^{2k-2} A2 (oracle: P = P @ A2), buffers 1.. ; U', V as lincombs
    const int npow = d / 2;  // number of even powers beyond I: d=3:1, 5:2, 7:3, 9:4
    for (int k = 2; k <= npow; ++k) {
      g = gemm_args(N, N, N, cnt);
      g.A = w(k - 1); g.B = w(1); g.C1 = w(k);
      if ((r = big_gemm<T>(c, 0, 0, g))) return r;
    }
    LinArgs la;
    std::memset(&la, 0, sizeof(la));
    la.rows = N; la.cols = N; la.nitems = cnt; la.nt = npow;
    for (int k = 1; k <= npow; ++k) la.Y[k - 1] = w(k);
    la.out = w(6); la.dI = C[1];
    for (int k = 1; k <= npow; ++k) la.w[k - 1] = C[2 * k + 1];
    la.out2 = w(7); la.dI2 = C[0];
    for (int k = 1; k <= npow; ++k) la.w2[k - 1] = C[2 * k];
    if ((r = big_lincomb<T>(c, la))) return r;  // U', V in one pass
  }
  // U = (A/2^s) U';  P = V + U -> w1,  Q = V - U -> w2
  g = gemm_args(N, N, N, cnt);
  g.A = Asrc; g.B = w(6); g.C1 = w(1); g.C2 = w(2);
  g.alpha1 = sc; g.alpha2 = -sc;
  g.nY = 1; g.Y[0] = w(7); g.w1[0] = 1.0; g.w2[0] = 1.0;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  // Newton-Schulz for Q^{-1}:  Y0 = P / c0^2,  R = I - Q Y,  Y <- Y + Y R  (R_{k+1} = R_k^2).
  // For A = -i H dt, P = conj-adjoint partner of Q and R0 = I - QP/c0^2 is tiny; ||R0||_F (computed
  // in the GEMM epilogue) fixes the iteration count: smallest k with ||R0||^(2^k) <= tol.
  const double c0sq = C[0] * C[0];
  HIPCHK(c, hipMemsetAsync(red, 0, (size_t)cnt * sizeof(double), c->stream));
  g = gemm_args(N, N, N, cnt);
  g.A = w(2); g.B = w(1); g.C1 = w(3); g.alpha1 = -1.0 / c0sq; g.gamma1 = 1.0; g.sumsq = red;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;  // R0 -> w3
  std::vector<double> ss(cnt);
  HIPCHK(c, hipMemcpyAsync(ss.data(), red, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double e0 = 0.0;
  for (double v : ss) e0 = std::max(e0, std::sqrt(v));
  if (!(e0 < 0.9))
    return fail(c, QOC_ERR_UNSUPPORTED,
                "large-N solve: Newton-Schulz residual %.3g >= 0.9 (generators not skew-Hermitian?)", e0);
  // stop once the residual bound is below the GEMMs' own rounding level (fp32 K=256 dot products
  // carry ~1e-6 relative error; fp64 ~1e-15)
  const double tol = c->prec == QOC_FP64 ? 1e-16 : 1e-7;
  int iters = 1;
  for (double e = e0 * e0; e > tol && iters < 8; e *= e) ++iters;
  c->ns_iters += iters;
  // Y1 = (P + P R0)/c0^2 -> w4
  g = gemm_args(N, N, N, cnt);
  g.A = w(1); g.B = w(3); g.C1 = w(4); g.alpha1 = 1.0 / c0sq;
  g.nY = 1; g.Y[0] = w(1); g.w1[0] = 1.0 / c0sq;
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  int cur = 4;
  for (int it = 1; it < iters; ++it) {
    g = gemm_args(N, N, N, cnt);
    g.A = w(2); g.B = w(cur); g.C1 = w(3); g.alpha1 = -1.0; g.gamma1 = 1.0;
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;  // R = I - Q Y
    const int nxt = cur == 4 ? 5 : 4;
    g = gemm_args(N, N, N, cnt);
    g.A = w(cur); g.B = w(3); g.C1 = w(nxt);
    g.nY = 1; g.Y[0] = w(cur); g.w1[0] = 1.0;
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;  // Y <- Y + Y R
    cur = nxt;
  }
  // X = Y P, then s squarings; the last product lands in d_U
  g = gemm_args(N, N, N, cnt);
  g.A = w(cur); g.B = w(1); g.C1 = sq == 0 ? dest : w(6);
  if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  int xb = 6;
  for (int q = 0; q < sq; ++q) {
    const int nb = xb == 6 ? 7 : 6;
    g = gemm_args(N, N, N, cnt);
    g.A = w(xb); g.B = w(xb); g.C1 = q == sq - 1 ? dest : w(nb);
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;
    xb = nb;
  }
  return QOC_OK;
}

// A_k = A_0 + Σ_j u_jk A_j for units [u0, u0 + cnt) -> out, and (nmax set) the chunk's max 1-norm: the generators in
// registers per (column block, slice group) for nu <= 2 and N <= 512 (k_form_norm2), else one workgroup per slice
template <typename T>
static int form_norm(qoc_ctx* c, long long u0, int cnt, cx<T>* out, unsigned long long* nmax) {
  const int N = c->N;
  const dim3 g2((unsigned)((N + 3) / 4), (unsigned)((cnt + FN2_SG - 1) / FN2_SG));
  if (c->nu <= 2 && N <= 256)
    hipLaunchKernelGGL((k_form_norm2<T, 4>), g2, dim3(256), 0, c->stream, N, c->nu, u0, cnt, c->d_A.as<const cx<T>>(),
                       (const double*)c->d_u, out, nmax);
  else if (c->nu <= 2 && N <= 512)
    hipLaunchKernelGGL((k_form_norm2<T, 8>), g2, dim3(256), 0, c->stream, N, c->nu, u0, cnt, c->d_A.as<const cx<T>>(),
                       (const double*)c->d_u, out, nmax);
  else
    hipLaunchKernelGGL((k_form_norm<T>), dim3(cnt), dim3(256), 0, c->stream, N, c->nu, u0, c->d_A.as<const cx<T>>(),
                       (const double*)c->d_u, out, nmax);
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}

// dJdu[unit, j] = Re <A_j, M'_unit> for units [u0, u0 + cnt): the generators in registers per column block
// (k_gen_contract2 + k_gen_reduce, nu <= 2, N <= 512), else one workgroup per slice (k_gen_contract)
template <typename T>
static int gen_contract(qoc_ctx* c, long long u0, int cnt, const cx<T>* Mp, double* d_dJdu) {
  const int N = c->N, nu = c->nu;
  if (nu >= 1 && nu <= 2 && N <= 512) {
    const int ncb = (N + 3) / 4;
    const size_t need = (size_t)c->chunk * ncb * nu * sizeof(double);
    if (need > c->d_gc_part.bytes()) {
      if (c->d_gc_part) HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, c->d_gc_part.grow(need));
    }
    const dim3 g2((unsigned)ncb, (unsigned)((cnt + GC2_SG - 1) / GC2_SG));
    if (N <= 256)
      hipLaunchKernelGGL((k_gen_contract2<T, 4>), g2, dim3(256), 0, c->stream, N, nu, cnt, c->d_A.as<const cx<T>>(), Mp,
                         c->d_gc_part);
    else
      hipLaunchKernelGGL((k_gen_contract2<T, 8>), g2, dim3(256), 0, c->stream, N, nu, cnt, c->d_A.as<const cx<T>>(), Mp,
                         c->d_gc_part);
    HIPCHK(c, hipGetLastError());
    const unsigned rb = (unsigned)std::min<long long>(((long long)cnt * nu + 255) / 256, 1024);
    hipLaunchKernelGGL(k_gen_reduce, dim3(rb), dim3(256), 0, c->stream, cnt, nu, ncb, u0, c->d_gc_part, d_dJdu);
  } else {
    hipLaunchKernelGGL((k_gen_contract<T>), dim3(cnt), dim3(256), 0, c->stream, N, nu, u0, c->d_A.as<const cx<T>>(), Mp,
                       d_dJdu);
  }
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}

// exp(A_k) for units [u0, u0+cnt) -> d_U (forms A_k from the generators, chunk max norm, then the GEMM expm)
template <typename T>
int big_expm_chunk(qoc_ctx* c, long long u0, int cnt) {
  const int N = c->N;
  const size_t NN = (size_t)N * N, esz = c->esz;
  cx<T>* a0 = c->d_ws.as<cx<T>>();
  HIPCHK(c, hipMemsetAsync(c->d_red, 0, 2 * sizeof(double), c->stream));
  if (int r = form_norm<T>(c, u0, cnt, a0, c->d_red.as<unsigned long long>())) return r;
  if (c->big_rho_ok) {
    SpecBound sb{};
    for (int j = 0; j <= c->nu && j < 9; ++j) sb.rho[j] = c->big_rho[j];
    const unsigned blocks = (unsigned)std::min<long long>((cnt + 255) / 256, 1024);
    hipLaunchKernelGGL(k_spec_bound, dim3(blocks), dim3(256), 0, c->stream, c->nu, u0, cnt, (const double*)c->d_u, sb,
                       (unsigned long long*)(c->d_red + 1));
    HIPCHK(c, hipGetLastError());
  }
  double nA[2] = {0.0, 0.0};
  HIPCHK(c, hipMemcpyAsync(nA, c->d_red, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return expm_gemm_chunk<T>(c, N, cnt, c->d_ws, (size_t)c->chunk, c->d_red, mk_opd(c->d_ws, 0, esz, (long long)NN),
                            mk_opd(c->d_U, (size_t)u0 * NN, esz, (long long)NN), nA[0], true,
                            c->big_rho_ok ? nA[1] : -1.0);
}

template <typename T>
int big_forward(qoc_ctx* c) {
  const int N = c->N, m = c->m, Nt = c->Nt, B = c->B;
  const size_t NN = (size_t)N * N, Nm = (size_t)N * m, esz = c->esz;
  const long long units = (long long)B * Nt;
  int r;
  int mk = mark_begin(c, 0);
  for (long long u0 = 0; u0 < units; u0 += c->chunk) {
    const int cnt = (int)std::min<long long>(c->chunk, units - u0);
    if ((r = big_expm_chunk<T>(c, u0, cnt))) return r;
  }
  mark_end(c, mk);
  mk = mark_begin(c, 1);
  // x_0 for every seed
  LinArgs la;
  std::memset(&la, 0, sizeof(la));
  la.rows = N; la.cols = m; la.nitems = B; la.nt = 1; la.w[0] = 1.0;
  la.Y[0] = mk_opd(c->d_x0, 0, esz, c->x0_per_seed ? (long long)Nm : 0);
  la.out = mk_opd(c->d_X, 0, esz, (long long)(Nt + 1) * Nm);
  if ((r = big_lincomb<T>(c, la))) return r;
  // x_{k+1} = U_k x_k, batched over seeds
  for (int k = 0; k < Nt; ++k) {
    GemmArgs g = gemm_args(N, N, m, B);
    g.A = mk_opd(c->d_U, (size_t)k * NN, esz, (long long)Nt * NN);
    g.B = mk_opd(c->d_X, (size_t)k * Nm, esz, (long long)(Nt + 1) * Nm);
    g.C1 = mk_opd(c->d_X, (size_t)(k + 1) * Nm, esz, (long long)(Nt + 1) * Nm);
    if ((r = big_gemm<T>(c, 0, 0, g))) return r;
  }
  // costs
  const bool pen = c->mu != 0.0;
  if (pen) {
    hipLaunchKernelGGL((k_penalty_sum<T>), dim3(B), dim3(256), 0, c->stream, N, m, Nt, c->d_X.as<const cx<T>>(),
                       c->d_pmask, c->mu, c->d_J);
    HIPCHK(c, hipGetLastError());
  }
  if (c->cost_kind != QOC_COST_EXTERNAL) {
    hipLaunchKernelGGL((k_terminal_cost<T>), dim3(B), dim3(256), 0, c->stream, N, m, Nt, c->d_X.as<const cx<T>>(),
                       c->d_Xt.as<const cx<T>>(), c->cost_kind, c->cost_n, pen ? 1 : 0, c->d_J, c->d_coef, sectors(c));
    HIPCHK(c, hipGetLastError());
  } else if (!pen) {
    HIPCHK(c, hipMemsetAsync(c->d_J, 0, (size_t)B * sizeof(double), c->stream));
  }
  mark_end(c, mk);
  return QOC_OK;
}

template <typename T>
int big_backward(qoc_ctx* c, int order, double* d_dJdu) {
  const int N = c->N, m = c->m, Nt = c->Nt, B = c->B, nu = c->nu;
  const size_t NN = (size_t)N * N, Nm = (size_t)N * m, esz = c->esz;
  const bool pen = c->mu != 0.0;
  const unsigned eb = (unsigned)std::min<size_t>((Nm * B + 255) / 256, 8192);
  int r;
  int mk = mark_begin(c, 2);
  if (c->cost_kind != QOC_COST_EXTERNAL) {
    hipLaunchKernelGGL((k_lambda_final<T>), dim3(eb), dim3(256), 0, c->stream, N, m, Nt, B, c->d_Xt.as<const cx<T>>(),
                       (const cx<double>*)c->d_coef, c->d_L.as<cx<T>>(), sectors(c));
    HIPCHK(c, hipGetLastError());
  }
  if (pen) {
    hipLaunchKernelGGL((k_penalty_grad<T>), dim3(eb), dim3(256), 0, c->stream, N, m, Nt, B, Nt,
                       c->d_X.as<const cx<T>>(), c->d_pmask, 2.0 * c->mu, c->d_L.as<cx<T>>());
    HIPCHK(c, hipGetLastError());
  }
  if (c->src_on) {
    hipLaunchKernelGGL((k_add_source<T>), dim3(eb), dim3(256), 0, c->stream, N, m, Nt, B, Nt, c->d_src.as<const cx<T>>(),
                       c->d_L.as<cx<T>>());
    HIPCHK(c, hipGetLastError());
  }
  // λ_k = U_k^H λ_{k+1} (+ dL/dx(x_k))
  for (int k = Nt - 1; k >= 0; --k) {
    GemmArgs g = gemm_args(N, N, m, B);
    g.A = mk_opd(c->d_U, (size_t)k * NN, esz, (long long)Nt * NN);
    g.B = mk_opd(c->d_L, (size_t)(k + 1) * Nm, esz, (long long)(Nt + 1) * Nm);
    g.C1 = mk_opd(c->d_L, (size_t)k * Nm, esz, (long long)(Nt + 1) * Nm);
    if ((r = big_gemm<T>(c, 1, 0, g))) return r;
    if (pen) {
      hipLaunchKernelGGL((k_penalty_grad<T>), dim3(eb), dim3(256), 0, c->stream, N, m, Nt, B, k,
                         c->d_X.as<const cx<T>>(), c->d_pmask, 2.0 * c->mu, c->d_L.as<cx<T>>());
      HIPCHK(c, hipGetLastError());
    }
    if (c->src_on) {
      hipLaunchKernelGGL((k_add_source<T>), dim3(eb), dim3(256), 0, c->stream, N, m, Nt, B, k, c->d_src.as<const cx<T>>(),
                         c->d_L.as<cx<T>>());
      HIPCHK(c, hipGetLastError());
    }
  }
  mark_end(c, mk);
  mk = mark_begin(c, 3);
  if (order == QOC_DUKDP_EXACT) {
    r = frechet_grad<T>(c, d_dJdu);
    mark_end(c, mk);
    return r;
  }
  // gradient, per chunk of slice units
  const long long units = (long long)B * Nt;
  const int o = order;
  const size_t C = (size_t)c->chunk;
  const size_t offX = 0, offP = C * NN, offQ = offP + C * o * Nm, offW = offQ + C * (o > 1 ? o - 1 : 1) * Nm,
               offM = offW + C * o * Nm;
  static const double inv_fact[9] = {1.0, 1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320};
  // Order 3 with m close to N: the same M' from the co-state/state outer product G = λ_{k+1} x_k^H,
  //   M' = G + (Y G + G Y)/2 + (Y^2 G + Y G Y + G Y^2)/6,   Y = X^H,
  // as five products (G: N^2 m flops; T1 = G Y, S = Y G + T1, R = T1 Y/6 + G + S/2, M' = Y S/6 + R: N^3 each)
  // instead of seven N^2 m-GEMM equivalents; cheaper when 4 N < 6 m (synthetic: m = N).
  bool sandwich = o == 3 && 4 * N < 6 * m;
  if (env_set("QOC_GRAD_SANDWICH")) sandwich = o == 3 && env_int("QOC_GRAD_SANDWICH", 0) != 0;
  for (long long u0 = 0; u0 < units; u0 += c->chunk) {
    const int cnt = (int)std::min<long long>(c->chunk, units - u0);
    if (int r = form_norm<T>(c, u0, cnt, (cx<T>*)(c->d_ws.as<char>() + offX * esz), nullptr)) return r;
    const Opd Xk = mk_opd(c->d_ws, offX, esz, (long long)NN);
    if (sandwich) {  // workspace: X, then three N x N blocks per item (G / R, T1 / M', S) — 4 NN of the 8 NN
      const size_t offG = C * NN, offT = 2 * C * NN, offS = 3 * C * NN;
      const Opd Gk = mk_opd(c->d_ws, offG, esz, (long long)NN), Tk = mk_opd(c->d_ws, offT, esz, (long long)NN),
                Sk = mk_opd(c->d_ws, offS, esz, (long long)NN);
      GemmArgs g = gemm_args(N, m, N, cnt);  // G = λ x^H
      g.A = mk_opd(c->d_L, Nm, esz, (long long)Nm, Nt, (long long)(Nt + 1) * Nm, (int)u0);
      g.B = mk_opd(c->d_X, 0, esz, (long long)Nm, Nt, (long long)(Nt + 1) * Nm, (int)u0);
      g.C1 = Gk;
      if ((r = big_gemm<T>(c, 0, 1, g))) return r;
      g = gemm_args(N, N, N, cnt);  // T1 = G X^H
      g.A = Gk; g.B = Xk; g.C1 = Tk;
      if ((r = big_gemm<T>(c, 0, 1, g))) return r;
      g = gemm_args(N, N, N, cnt);  // S = X^H G + T1
      g.A = Xk; g.B = Gk; g.C1 = Sk; g.nY = 1; g.Y[0] = Tk; g.w1[0] = 1.0;
      if ((r = big_gemm<T>(c, 1, 0, g))) return r;
      g = gemm_args(N, N, N, cnt);  // R = T1 X^H / 6 + G + S / 2   (over G, element-wise in the epilogue)
      g.A = Tk; g.B = Xk; g.C1 = Gk; g.alpha1 = 1.0 / 6;
      g.nY = 2; g.Y[0] = Gk; g.w1[0] = 1.0; g.Y[1] = Sk; g.w1[1] = 0.5;
      if ((r = big_gemm<T>(c, 0, 1, g))) return r;
      g = gemm_args(N, N, N, cnt);  // M' = X^H S / 6 + R   (over T1)
      g.A = Xk; g.B = Sk; g.C1 = Tk; g.alpha1 = 1.0 / 6; g.nY = 1; g.Y[0] = Gk; g.w1[0] = 1.0;
      if ((r = big_gemm<T>(c, 1, 0, g))) return r;
      if ((r = gen_contract<T>(c, u0, cnt, (const cx<T>*)(c->d_ws.as<char>() + offT * esz), d_dJdu))) return r;
      continue;
    }
    auto Pa = [&](int a) { return mk_opd(c->d_ws, offP + a * Nm, esz, (long long)(o * Nm)); };
    auto Qb = [&](int b) {  // Q_0 = λ_{k+1} in place; Q_b (b >= 1) in the workspace
      if (b == 0) return mk_opd(c->d_L, Nm, esz, (long long)Nm, Nt, (long long)(Nt + 1) * Nm, (int)u0);
      return mk_opd(c->d_ws, offQ + (b - 1) * Nm, esz, (long long)((o - 1) * Nm));
    };
    auto Wa = [&](int a) { return mk_opd(c->d_ws, offW + a * Nm, esz, (long long)(o * Nm)); };
    const Opd xk = mk_opd(c->d_X, 0, esz, (long long)Nm, Nt, (long long)(Nt + 1) * Nm, (int)u0);
    LinArgs la;
    std::memset(&la, 0, sizeof(la));
    if (o == 1) {
      la.rows = N; la.cols = m; la.nitems = cnt; la.nt = 1; la.w[0] = 1.0;
      la.Y[0] = xk; la.out = Pa(0);
      if ((r = big_lincomb<T>(c, la))) return r;  // P_0 = x_k
    }
    for (int a = 1; a < o; ++a) {
      GemmArgs g = gemm_args(N, N, m, cnt);
      g.A = Xk; g.B = a == 1 ? xk : Pa(a - 1); g.C1 = Pa(a);
      if (a == 1) {  // P_0 = x_k copied into the stacked P from this GEMM's epilogue
        g.C2 = Pa(0); g.alpha2 = 0.0; g.nY = 1; g.Y[0] = xk; g.w2[0] = 1.0;
      }
      if ((r = big_gemm<T>(c, 0, 0, g))) return r;  // P_a = X P_{a-1}
    }
    if (o == 3) {
      // Q_1 = X^H λ  (+ W_2 = λ/6 from the epilogue);  X^H Q_1 -> W_0 = λ + Q_1/2 + Q_2/6, W_1 = λ/2 + Q_1/6
      GemmArgs g = gemm_args(N, N, m, cnt);
      g.A = Xk; g.B = Qb(0); g.C1 = Qb(1);
      g.C2 = Wa(2); g.alpha2 = 0.0; g.nY = 1; g.Y[0] = Qb(0); g.w2[0] = 1.0 / 6;
      if ((r = big_gemm<T>(c, 1, 0, g))) return r;
      g = gemm_args(N, N, m, cnt);
      g.A = Xk; g.B = Qb(1);
      g.nY = 2; g.Y[0] = Qb(0); g.Y[1] = Qb(1);
      g.C1 = Wa(0); g.alpha1 = 1.0 / 6; g.w1[0] = 1.0; g.w1[1] = 0.5;
      g.C2 = Wa(1); g.alpha2 = 0.0; g.w2[0] = 0.5; g.w2[1] = 1.0 / 6;
      if ((r = big_gemm<T>(c, 1, 0, g))) return r;
    } else {
    for (int b = 1; b < o; ++b) {
      GemmArgs g = gemm_args(N, N, m, cnt);
      g.A = Xk; g.B = Qb(b - 1); g.C1 = Qb(b);
      if ((r = big_gemm<T>(c, 1, 0, g))) return r;  // Q_b = X^H Q_{b-1}
    }
    for (int a = 0; a < o; a += 2) {  // W_a = sum_b Q_b/(a+b+1)!, two W's per pass
      std::memset(&la, 0, sizeof(la));
      la.rows = N; la.cols = m; la.nitems = cnt; la.nt = o - a;
      for (int b = 0; b < o - a; ++b) {
        la.Y[b] = Qb(b);
        la.w[b] = inv_fact[a + b + 1];
        la.w2[b] = b < o - a - 1 ? inv_fact[a + b + 2] : 0.0;
      }
      la.out = Wa(a);
      if (a + 1 < o) la.out2 = Wa(a + 1);
      if ((r = big_lincomb<T>(c, la))) return r;
    }
    }
    GemmArgs g = gemm_args(N, o * m, N, cnt);
    g.A = mk_opd(c->d_ws, offW, esz, (long long)(o * Nm));
    g.B = mk_opd(c->d_ws, offP, esz, (long long)(o * Nm));
    g.C1 = mk_opd(c->d_ws, offM, esz, (long long)NN);
    if ((r = big_gemm<T>(c, 0, 1, g))) return r;  // M' = W P^H
    if ((r = gen_contract<T>(c, u0, cnt, (const cx<T>*)(c->d_ws.as<char>() + offM * esz), d_dJdu))) return r;
  }
  mark_end(c, mk);
  return QOC_OK;
}

// Order-3 gradient of the LDS-resident path as GEMMs over every (seed, slice) at once.  With the state
// matrix Xall = [x_0 .. x_Nt] of all seeds (N x B(Nt+1)m, the d_X buffer as is) and
// X_k v = A0 v + sum_j u_jk A_j v = [A0 | A1 | ...] [v; u_1k v; ...]:
//   P1 = X Xall, P2 = X P1, Q1 = X^H Lsh (Lsh = λ_{k+1} columns), and from the epilogues
//   W2 = λ/6, W0 = λ + Q1/2 + Q2/6, W1 = λ/2 + Q1/6 (Q2 = X^H Q1 is never stored);
//   dJdu[k, j] = sum_a Re<W_a, A_j P_a>  (k_bgemm MODE 2 epilogue, [A1; A2; ...] x P_a).
// Same contraction as k_grad / the reference's expm_jacobian! order 3, on MFMA with the generators
// shared by every GEMM.
template <typename T>
int grad_gemm_o3(qoc_ctx* c, double* d_dJdu) {
  const int N = c->N, m = c->m, nu = c->nu, Nt = c->Nt;
  const size_t Nm = (size_t)N * m, esz = c->esz;
  const long long cols = (long long)c->B * (Nt + 1) * m - m;  // the last seed's x_Nt column block is unused
  const size_t bufN = (size_t)N * ((size_t)c->B * (Nt + 1) * m);
  auto buf = [&](int i) { return mk_opd(c->d_gws, (size_t)i * bufN, esz, 0); };
  const Opd Xall = mk_opd(c->d_X, 0, esz, 0), Lsh = mk_opd(c->d_L, Nm, esz, 0);
  const Opd P1 = buf(0), P2 = buf(1), Q1 = buf(2), W0 = buf(3), W1 = buf(4), W2 = buf(5);
  HIPCHK(c, hipMemsetAsync(d_dJdu, 0, (size_t)c->B * Nt * nu * sizeof(double), c->stream));
  auto comb = [&](const void* Gmat, const Opd& Bsrc) {
    GemmArgs g = gemm_args(N, (nu + 1) * N, (int)cols, 1);
    g.A = mk_opd(Gmat, 0, esz, 0);
    g.B = Bsrc;
    g.uc = c->d_u;
    g.kb = N;
    g.cm = m;
    g.sps = Nt + 1;
    g.cNt = Nt;
    g.cnu = nu;
    return g;
  };
  int r;
  GemmArgs g = comb(c->d_A, Xall);
  g.C1 = P1;
  if ((r = big_gemm<T>(c, 0, 0, g, 1))) return r;  // P1 = X x
  g = comb(c->d_A, P1);
  g.C1 = P2;
  if ((r = big_gemm<T>(c, 0, 0, g, 1))) return r;  // P2 = X P1
  g = comb(c->d_AH, Lsh);
  g.C1 = Q1;
  g.C2 = W2; g.alpha2 = 0.0; g.nY = 1; g.Y[0] = Lsh; g.w2[0] = 1.0 / 6;
  if ((r = big_gemm<T>(c, 0, 0, g, 1))) return r;  // Q1 = X^H λ, W2 = λ/6
  g = comb(c->d_AH, Q1);
  g.nY = 2; g.Y[0] = Lsh; g.Y[1] = Q1;
  g.C1 = W0; g.alpha1 = 1.0 / 6; g.w1[0] = 1.0; g.w1[1] = 0.5;
  g.C2 = W1; g.alpha2 = 0.0; g.w2[0] = 0.5; g.w2[1] = 1.0 / 6;
  if ((r = big_gemm<T>(c, 0, 0, g, 1))) return r;  // W0, W1 (Q2 consumed in the epilogue)
  const Opd Pa[3] = {Xall, P1, P2}, Wa[3] = {W0, W1, W2};
  for (int a = 0; a < 3; ++a) {
    GemmArgs h = gemm_args(nu * N, N, (int)cols, 1);
    h.A = mk_opd(c->d_Cst, 0, esz, 0);
    h.B = Pa[a];
    h.C1 = Pa[a];  // not written in MODE 2
    h.kb = N;
    h.cm = m;
    h.sps = Nt + 1;
    h.cNt = Nt;
    h.cnu = nu;
    h.dot = d_dJdu;
    h.Wd = Wa[a];
    if ((r = big_gemm<T>(c, 0, 0, h, 2))) return r;  // dJdu += Re<W_a, A_j P_a>
  }
  return QOC_OK;
}

// Exact gradient (QOC_DUKDP_EXACT): one Fréchet derivative per slice from the 2N x 2N block exponential
// (qoc_frechet.hpp), k_expm when 2N fits the LDS-resident kernel, the GEMM pipeline otherwise.
template <typename T>
int frechet_grad(qoc_ctx* c, double* d_dJdu) {
  const int N = c->N, n2 = 2 * N, nu = c->nu;
  const size_t NN = (size_t)N * N, BB = (size_t)n2 * n2, esz = c->esz;
  const long long units = (long long)c->B * c->Nt;
  const bool small = expm_supported(n2, c->prec);
  const size_t per_item = (small ? 2 : 10) * BB * esz + 3 * sizeof(double);
  size_t freeb = 0, totalb = 0;
  (void)hipMemGetInfo(&freeb, &totalb);
  const size_t budget = std::min<size_t>(4ull << 30, std::max<size_t>(freeb / 8, per_item));
  const int fch = (int)std::max<long long>(1, std::min<long long>({(long long)(budget / per_item), units, 16384LL}));
  const size_t need = (size_t)fch * per_item + nu * NN * esz + 64 * sizeof(double);
  HIPCHK(c, c->d_fws.grow(need));
  char* p = c->d_fws.as<char>();
  cx<T>* blocks = (cx<T>*)p;
  p += (size_t)fch * BB * esz;
  cx<T>* E = (cx<T>*)p;
  p += (size_t)fch * BB * esz;
  void* ws = nullptr;
  if (!small) {
    ws = p;
    p += 8 * (size_t)fch * BB * esz;
  }
  cx<T>* At = (cx<T>*)p;
  p += nu * NN * esz;
  double* alpha = (double*)p;
  p += (size_t)fch * sizeof(double);
  double* red = (double*)p;  // fch + 8 doubles
  hipLaunchKernelGGL((k_transpose_gens<T>), dim3(256), dim3(256), 0, c->stream, N, nu, c->d_A.as<const cx<T>>(), At);
  HIPCHK(c, hipGetLastError());
  int r;
  for (long long u0 = 0; u0 < units; u0 += fch) {
    const int cnt = (int)std::min<long long>(fch, units - u0);
    hipLaunchKernelGGL((k_frechet_build<T>), dim3(cnt), dim3(256), 0, c->stream, N, c->m, nu, c->Nt, u0,
                       c->d_A.as<const cx<T>>(), (const double*)c->d_u, c->d_X.as<const cx<T>>(), c->d_L.as<const cx<T>>(),
                       blocks, alpha);
    HIPCHK(c, hipGetLastError());
    if (small) {
      hipError_t e = launch_expm(c->prec, c->stream, n2, 0, cnt, nullptr, nullptr, blocks, E, nullptr, nullptr, nullptr,
                                 c->expm_alg, nullptr, c->d_ps);
      if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_expm (Frechet block): %s", hipGetErrorString(e));
    } else {
      HIPCHK(c, hipMemsetAsync(red, 0, sizeof(double), c->stream));
      hipLaunchKernelGGL((k_norm1_max<T>), dim3(cnt), dim3(256), 0, c->stream, n2, (const cx<T>*)blocks,
                         (unsigned long long*)red);
      HIPCHK(c, hipGetLastError());
      double nA = 0.0;
      HIPCHK(c, hipMemcpyAsync(&nA, red, sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if ((r = expm_gemm_chunk<T>(c, n2, cnt, ws, (size_t)fch, red, mk_opd(blocks, 0, esz, (long long)BB),
                                  mk_opd(E, 0, esz, (long long)BB), nA, false)))
        return r;
    }
    hipLaunchKernelGGL((k_frechet_contract<T>), dim3(cnt), dim3(256), 0, c->stream, N, nu, u0, (const cx<T>*)At,
                       (const cx<T>*)E, (const double*)alpha, d_dJdu);
    HIPCHK(c, hipGetLastError());
  }
  return QOC_OK;
}

// Extreme eigenvalues of H = i A (A skew-Hermitian, column-major interleaved N x N): Householder reduction of H to a
// Hermitian tridiagonal T (its off-diagonal moduli give a real symmetric tridiagonal with the same spectrum), then
// Sturm-count bisection for the smallest and the largest eigenvalue.  Backward stable: the interval is exact up to
// ~N eps ||H||, which the caller adds as a margin.
void herm_extremes(const double* A, int N, double& lmin, double& lmax) {
  using C = std::complex<double>;
  std::vector<C> H((size_t)N * N);
  auto h = [&](int r, int c) -> C& { return H[r + (size_t)N * c]; };
  for (int c = 0; c < N; ++c)
    for (int r = 0; r < N; ++r) {
      const C a(A[2 * (r + (size_t)N * c)], A[2 * (r + (size_t)N * c) + 1]);
      h(r, c) = C(0.0, 1.0) * a;  // H = i A
    }
  for (int c = 0; c < N; ++c)  // exact Hermitian symmetry
    for (int r = c; r < N; ++r) {
      const C v = 0.5 * (h(r, c) + std::conj(h(c, r)));
      h(r, c) = v;
      h(c, r) = std::conj(v);
    }
  std::vector<C> v(N), p(N), q(N);
  for (int k = 0; k + 2 < N; ++k) {
    double nx = 0.0;
    for (int i = k + 1; i < N; ++i) nx += std::norm(h(i, k));
    nx = std::sqrt(nx);
    if (nx == 0.0) continue;
    const C x0 = h(k + 1, k);
    const C alpha = -(std::abs(x0) > 0 ? x0 / std::abs(x0) : C(1.0)) * nx;
    for (int i = 0; i < N; ++i) v[i] = 0.0;
    for (int i = k + 1; i < N; ++i) v[i] = h(i, k);
    v[k + 1] -= alpha;
    double nv = 0.0;
    for (int i = k + 1; i < N; ++i) nv += std::norm(v[i]);
    nv = std::sqrt(nv);
    if (nv == 0.0) continue;
    for (int i = k + 1; i < N; ++i) v[i] /= nv;
    // H <- (I - 2 v v^H) H (I - 2 v v^H) = H - 2 v w^H - 2 w v^H, w = p - (v^H p) v, p = H v
    for (int i = k; i < N; ++i) {
      C s = 0.0;
      for (int j = k + 1; j < N; ++j) s += h(i, j) * v[j];
      p[i] = s;
    }
    C K = 0.0;
    for (int i = k + 1; i < N; ++i) K += std::conj(v[i]) * p[i];
    for (int i = k; i < N; ++i) q[i] = p[i] - K * v[i];
    for (int j = k; j < N; ++j)
      for (int i = k; i < N; ++i) h(i, j) -= 2.0 * (v[i] * std::conj(q[j]) + q[i] * std::conj(v[j]));
  }
  std::vector<double> d(N), e(N, 0.0);
  double gl = 1e300, gu = -1e300;
  for (int i = 0; i < N; ++i) {
    d[i] = h(i, i).real();
    if (i + 1 < N) e[i] = std::abs(h(i + 1, i));
  }
  for (int i = 0; i < N; ++i) {  // Gershgorin interval of T
    const double r = (i > 0 ? e[i - 1] : 0.0) + (i + 1 < N ? e[i] : 0.0);
    gl = std::min(gl, d[i] - r);
    gu = std::max(gu, d[i] + r);
  }
  auto count_below = [&](double x) {  // eigenvalues of T below x (Sturm: negative pivots of T - x I = L D L^T)
    int cnt = 0;
    double piv = 1.0;
    for (int i = 0; i < N; ++i) {
      piv = d[i] - x - (i > 0 ? e[i - 1] * e[i - 1] / piv : 0.0);
      if (piv == 0.0) piv = -1e-300;
      if (piv < 0.0) ++cnt;
    }
    return cnt;
  };
  auto bisect = [&](int target) {  // smallest x with count_below(x) > target: the (target+1)-th eigenvalue
    double lo = gl, hi = gu;
    for (int it = 0; it < 200 && hi - lo > 1e-15 * std::max(std::fabs(lo), std::fabs(hi)) + 1e-300; ++it) {
      const double mid = 0.5 * (lo + hi);
      (count_below(mid) > target ? hi : lo) = mid;
    }
    return 0.5 * (lo + hi);
  };
  lmin = bisect(0);
  lmax = bisect(N - 1);
}

// generator layouts of the GEMM-shaped gradient: [A0^H | A1^H | ...] and [A1; A2; ...]
hipError_t launch_gen_aux(qoc_ctx* c) {
  const size_t NN = (size_t)c->N * c->N;
  const unsigned blocks = (unsigned)std::min<size_t>(((c->nu + 1) * NN + 255) / 256, 2048);
  if (c->prec == QOC_FP64)
    hipLaunchKernelGGL((k_gen_aux<double>), dim3(blocks), dim3(256), 0, c->stream, c->N, c->nu,
                       c->d_A.as<const cx<double>>(), c->d_AH.as<cx<double>>(), c->d_Cst.as<cx<double>>());
  else
    hipLaunchKernelGGL((k_gen_aux<float>), dim3(blocks), dim3(256), 0, c->stream, c->N, c->nu,
                       c->d_A.as<const cx<float>>(), c->d_AH.as<cx<float>>(), c->d_Cst.as<cx<float>>());
  return hipGetLastError();
}

template int big_forward<double>(qoc_ctx*);
template int big_forward<float>(qoc_ctx*);
template int big_backward<double>(qoc_ctx*, int, double*);
template int big_backward<float>(qoc_ctx*, int, double*);
template int grad_gemm_o3<double>(qoc_ctx*, double*);
template int grad_gemm_o3<float>(qoc_ctx*, double*);
template int frechet_grad<double>(qoc_ctx*, double*);
template int frechet_grad<float>(qoc_ctx*, double*);

}  // namespace qoc_host
