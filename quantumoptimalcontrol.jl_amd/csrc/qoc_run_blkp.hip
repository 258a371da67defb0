// qoc_run_blkp.hip — stored / interpolating propagators for blocks of 5..16 rows (qoc_blkp.hpp; blkp_on,
// qoc_run_blk.hip).  The tunable bus' parity blocks: U_k per (seed, slice, live block) -- interpolated in u for one
// control (k_blkp_int), else on MFMA (k_blkp_exp) --, then the one-matvec chains (k_blkp_dual / k_blkp_chain) and the
// order-3 gradient on MFMA (k_blkp_grad).  QOC_BLKP=0 keeps the Chebyshev-action chains (k_blkrot_dual).
#include "qoc_blk_host.hpp"
#include "qoc_blkp.hpp"

namespace qoc_host {

// The state penalty as the stored / interpolating propagator chains take it (qoc_blkp.hpp BlkpPen) for the wave blocks
// `wrow` (16 rows each): the row masks from h_pen_rows, the column mask from h_pen_cols.  False: no penalised entry
// there (μ = 0, no column, or every penalised row in a dead block, whose x_k is zero): the eval is the unpenalised one.
static bool blkp_pen_masks(const qoc_ctx* c, const std::vector<int>& wrow, BlkpPen& pp) {
  pp = BlkpPen{};
  if (c->mu == 0.0 || wrow.size() > 16 * 8) return false;
  unsigned rows = 0;
  for (size_t e = 0; e < wrow.size(); ++e)
    if (wrow[e] >= 0 && std::find(c->h_pen_rows.begin(), c->h_pen_rows.end(), wrow[e]) != c->h_pen_rows.end()) {
      pp.prow[e / 16] |= (unsigned short)(1u << (e % 16));
      rows |= 1u;
    }
  for (int col : c->h_pen_cols)
    if (col >= 0 && col < std::min(c->m, 32)) pp.pcol |= 1u << col;
  return rows != 0 && pp.pcol != 0;
}
// the masks for the layout an eval runs on: every block with a co-state source (λ_k is then nonzero on every row),
// else the live blocks
static bool blkp_pen_active(const qoc_ctx* c, BlkpPen& pp) {
  std::vector<int> wl, dead;
  const bool part = !c->src_on && blk_live_rows(c, wl, dead);
  return blkp_pen_masks(c, part ? wl : c->h_wrow, pp);
}
// How a state penalty / co-state source runs on blocks of 5..16 rows:
//   0  none in effect (μ = 0 or no penalised entry in a live block, and no source): the unpenalised paths, same bits;
//   1  on the stored / interpolating propagator chains' PEN instantiations (blkp_forward, then blkp_backward);
//   2  on the Chebyshev block chains (QOC_BLKP_PEN=0, read per call; packed states; QOC_BLKP=0).
int blkp_pen_mode(const qoc_ctx* c) {
  if (c->mu == 0.0 && !c->src_on) return 0;
  if (env_int("QOC_BLKP_PEN", 1) == 0 || c->packed || !blkp_on(c)) return 2;
  if (c->src_on) return 1;
  BlkpPen pp;
  return blkp_pen_active(c, pp) ? 1 : 0;
}

// the dead rows' zeros in x_k and λ_k when the launch runs on the live blocks alone
// lam: the caller writes the co-states too (an eval, a grape_sensitivity); a propagate leaves d_L alone
static int blkp_zero_dead(qoc_ctx* c, const BlkArgs& bk, bool lam) {
  if (bk.nwb == c->nwb) return QOC_OK;
  return lam ? blk_zero_dead(c, {c->d_X, c->d_L}) : blk_zero_dead(c, {c->d_X});
}
// a forward from propagators formed without step records: d_steps still holds the last k_tchain_prep's records, not
// this u's (the Chebyshev backward re-preps first); ichain: the chains that ran (blkp_ichain_on), for qoc_get_info
static void blkp_forward_done(qoc_ctx* c, int ichain) {
  c->props_since_reset++;
  c->fwd.steps_old = true;
  c->fwd.formed_ichain = ichain;
}

// the propagator store d_blkU of at least `bytes` (reallocated when a larger batch part or block layout needs more);
// soft: a failed allocation is no error (returns 1: the caller takes the Chebyshev block chains instead)
static int blkp_ensure_store(qoc_ctx* c, size_t bytes, bool soft) {
  if (c->d_blkU.bytes() >= bytes) return QOC_OK;
  if (c->d_blkU) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
  }
  const hipError_t e = c->d_blkU.grow(bytes);
  if (e != hipSuccess) {
    if (soft) return 1;
    return fail(c, QOC_ERR_HIP, "stored block propagators (%zu bytes): %s", bytes, hipGetErrorString(e));
  }
  return QOC_OK;
}

// θ[r][s] of BlkpArgs::tail: the largest ρ with Σ_{k > 4r} ρ^k / k! <= 2^-53 2^-(s + tail) (bisection; the tail sum from
// its first term, exp((4r + 1) ln ρ - lgamma(4r + 2)), 40 terms)
static void blkp_theta_table(int tail, double (&theta)[BLKP_RMAX + 1][16]) {
  for (int r = 0; r <= BLKP_RMAX; ++r)
    for (int s = 0; s < 16; ++s) {
      if (r < BLKP_RMIN) {
        theta[r][s] = 0.0;
        continue;
      }
      const int m = 4 * r;
      const double tol = std::ldexp(1.0, -53 - s - tail);
      auto tailsum = [&](double rho) {
        double t = std::exp((m + 1) * std::log(rho) - std::lgamma(m + 2.0)), sum = 0.0;
        for (int k = m + 1; k < m + 41; ++k) {
          sum += t;
          t *= rho / (k + 1);
        }
        return sum;
      };
      double lo = 0.0, hi = 16.0;
      for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        (tailsum(mid) <= tol ? lo : hi) = mid;
      }
      theta[r][s] = lo;
    }
}

// The Chebyshev form's table (qoc_blkp.hpp blkp_cheb) for block size cm up to ρ_c = crmax: per grid point
// ρ_c = 2^((g - BLKP_CT_G0) / 4) the Bessel values J_k(ρ_c) (Miller's backward recurrence in long double, normalised
// by J_0 + 2 Σ J_2k = 1), the degree n with Σ_{k>n} 2 |J_k| <= 2^-57, and the series rewritten for block Clenshaw in
// Z = T_cm: c_k = (2 - δ_k0) (-i)^k J_k, then from the top block down a_{q,j} = 2 c_{cm q + j}, c_{cm q - j} -= c_{cm q + j}
// (j = 1..cm-1), a_{q,0} = c_{cm q}; β_{q,j} = i^j a_{q,j} is real for even cm.
static int blkp_cheb_table(qoc_ctx* c, int cm, double crmax) {
  if (c->d_blkp_ctab && c->ctab_cm == cm && c->ctab_rmax == crmax) return QOC_OK;
  const int gn = BLKP_CT_G0 + (int)std::lround(4.0 * std::log2(crmax)) + 1;
  std::vector<double> tab((size_t)gn * BLKP_CT_STRIDE, 0.0);
  typedef long double LD;
  for (int g = 0; g < gn; ++g) {
    const LD rc = std::pow((LD)2, (LD)(g - BLKP_CT_G0) / 4);
    const int K = 100, M = K + 60 + (int)(4 * rc);
    std::vector<LD> jb(M + 2, 0.0L);
    jb[M] = 1e-300L;
    for (int k = M; k >= 1; --k) jb[k - 1] = (2.0L * k / rc) * jb[k] - jb[k + 1];
    LD nrm = jb[0];
    for (int k = 2; k <= M; k += 2) nrm += 2 * jb[k];
    std::vector<LD> J(K + 1);
    for (int k = 0; k <= K; ++k) J[k] = jb[k] / nrm;
    int n = K;
    LD tail = 0;
    while (n > 0 && tail + 2 * std::fabs(J[n]) <= std::ldexp(1.0L, -57)) tail += 2 * std::fabs(J[n--]);
    const int Q = n <= cm - 1 ? 0 : (n - (cm - 1) + cm - 1) / cm;
    if (4 + (Q + 1) * cm > BLKP_CT_STRIDE) return fail(c, QOC_ERR_UNSUPPORTED, "Chebyshev table: degree %d at rho %g", n, (double)rc);
    const int L = cm * (Q + 1);
    std::vector<LD> cr(L, 0.0L), ci(L, 0.0L);  // c_k = (2 - δ) (-i)^k J_k
    for (int k = 0; k <= n && k < L; ++k) {
      const LD v = (k ? 2 : 1) * J[k];
      switch (k & 3) {
        case 0: cr[k] = v; break;
        case 1: ci[k] = -v; break;
        case 2: cr[k] = -v; break;
        default: ci[k] = v; break;
      }
    }
    double* row = tab.data() + (size_t)g * BLKP_CT_STRIDE;
    row[0] = (double)rc;
    row[1] = (double)(1.0L / rc);
    row[2] = Q;
    for (int qq = Q; qq >= 0; --qq)
      for (int jj = cm - 1; jj >= 0; --jj) {
        const int k = cm * qq + jj;
        LD ar = cr[k], ai = ci[k];
        if (qq > 0 && jj > 0) {
          ar *= 2;
          ai *= 2;
          cr[cm * qq - jj] -= cr[k];
          ci[cm * qq - jj] -= ci[k];
        }
        // β = i^j a (real)
        LD br = ar, bi = ai;
        for (int t = 0; t < (jj & 3); ++t) {
          const LD nr = -bi, ni = br;
          br = nr;
          bi = ni;
        }
        if (std::fabs(bi) > 1e-12L * (std::fabs(br) + 1e-300L) && std::fabs(bi) > 1e-300L)
          return fail(c, QOC_ERR_UNSUPPORTED, "Chebyshev table: complex coefficient (g %d, q %d, j %d)", g, qq, jj);
        row[4 + qq * cm + jj] = (double)br;
      }
  }
  if (c->d_blkp_ctab) HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, c->d_blkp_ctab.alloc(tab.size() * sizeof(double)));
  HIPCHK(c, hipMemcpy(c->d_blkp_ctab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  c->ctab_cm = cm;
  c->ctab_rmax = crmax;
  return QOC_OK;
}

// ---- one control: the propagators interpolated in u (qoc_blkp.hpp k_blkp_int) ----
typedef long double LD;
// exp(X) of an n x n complex matrix in long double (row-major, re / im apart): scaling to ||X||_1 <= 1/2, Taylor
// degree 30 (tail < 1e-40), squarings; 64-bit mantissas, so its own error (~1e-18) is far below the fp64 result
static void ld_expm(int n, const std::vector<LD>& Xr, const std::vector<LD>& Xi, std::vector<LD>& Er, std::vector<LD>& Ei) {
  LD n1 = 0;
  for (int c = 0; c < n; ++c) {
    LD sum = 0;
    for (int r = 0; r < n; ++r) sum += std::hypot(Xr[r * n + c], Xi[r * n + c]);
    n1 = std::max(n1, sum);
  }
  int s = 0;
  while (n1 > 0.5L && s < 60) {
    n1 *= 0.5L;
    ++s;
  }
  const LD sc = std::ldexp(1.0L, -s);
  std::vector<LD> Yr(n * n), Yi(n * n), Tr(n * n, 0), Ti(n * n, 0), Nr(n * n), Ni(n * n);
  for (int e = 0; e < n * n; ++e) {
    Yr[e] = Xr[e] * sc;
    Yi[e] = Xi[e] * sc;
  }
  Er.assign(n * n, 0);
  Ei.assign(n * n, 0);
  for (int d = 0; d < n; ++d) Tr[d * n + d] = Er[d * n + d] = 1;
  auto mul = [&](const std::vector<LD>& Ar, const std::vector<LD>& Ai, const std::vector<LD>& Br, const std::vector<LD>& Bi) {
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) {
        LD sr = 0, si = 0;
        for (int q = 0; q < n; ++q) {
          sr += Ar[r * n + q] * Br[q * n + c] - Ai[r * n + q] * Bi[q * n + c];
          si += Ar[r * n + q] * Bi[q * n + c] + Ai[r * n + q] * Br[q * n + c];
        }
        Nr[r * n + c] = sr;
        Ni[r * n + c] = si;
      }
  };
  for (int k = 1; k <= 30; ++k) {
    mul(Tr, Ti, Yr, Yi);
    for (int e = 0; e < n * n; ++e) {
      Tr[e] = Nr[e] / k;
      Ti[e] = Ni[e] / k;
      Er[e] += Tr[e];
      Ei[e] += Ti[e];
    }
  }
  for (int t = 0; t < s; ++t) {
    mul(Er, Ei, Er, Ei);
    Er = Nr;
    Ei = Ni;
  }
}

// the control range [lo, hi] of the batch in d_u (nu = 1): a partial min / max per block, finished on the host
static int blkp_urange(qoc_ctx* c, double& lo, double& hi) {
  const long long n = (long long)c->B * c->Nt * c->nu;
  const int grid = (int)std::max<long long>(1, std::min<long long>(256, (n + 255) / 256));
  if (!c->d_minmax) {
    HIPCHK(c, c->h_minmax.alloc(512 * sizeof(double)));
    HIPCHK(c, c->d_minmax.alloc(512 * sizeof(double)));
  }
  hipLaunchKernelGGL(k_minmax, dim3(grid), dim3(256), 0, c->stream, (const double*)c->d_u, n, c->d_minmax);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_minmax, c->d_minmax, 2 * grid * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  lo = c->h_minmax[0];
  hi = c->h_minmax[1];
  for (int b = 1; b < grid; ++b) {
    lo = std::min(lo, c->h_minmax[2 * b]);
    hi = std::max(hi, c->h_minmax[2 * b + 1]);
  }
  return QOC_OK;
}

// The coefficient matrices of exp(Ã_0 + u Ã_1) on [lo, hi] for every live wave block: the exponentials at NI
// Chebyshev points θ_k = π (k + 1/2) / NI in long double, M_i = (2 - δ_i0) / NI Σ_k F_k cos(i θ_k), D the last index
// whose tail max_{i > D} |M_i| is <= 2^-56 (the coefficients of an entire function fall super-exponentially; the
// aliasing of the NI-point transform is below the last ones).  Returns 1 when the series has not converged within NI
// points (a control range too wide) or the coefficients exceed the LDS.
static int blkp_interp_coeffs(qoc_ctx* c, const std::vector<int>& wrow, double lo, double hi) {
  constexpr int NI = 40;
  const int N = c->N, nwb = (int)(wrow.size() / 16);
  const size_t NN = (size_t)N * N;
  const LD pi = std::acos(-1.0L), mid = ((LD)lo + hi) / 2, half = ((LD)hi - lo) / 2;
  std::vector<std::vector<LD>> Mr((size_t)nwb * NI, std::vector<LD>(256, 0)), Mi = Mr;
  std::vector<LD> Xr(256), Xi(256), Er, Ei;
  for (int b = 0; b < nwb; ++b)
    for (int k = 0; k < NI; ++k) {
      const LD th = pi * (k + 0.5L) / NI, u = mid + half * std::cos(th);
      for (int r = 0; r < 16; ++r)
        for (int q = 0; q < 16; ++q) {
          const int row = wrow[16 * b + r], col = wrow[16 * b + q];
          LD vr = 0, vi = 0;
          if (row >= 0 && col >= 0) {
            for (int j = 0; j <= 1; ++j) {
              const double* a = c->h_gen.data() + 2 * (j * NN + row + (size_t)N * col);
              LD ar = a[0], ai = a[1];
              if (row == col) {
                ar -= c->tprm.mur[j];
                ai -= c->tprm.mui[j];
              }
              const LD f = j ? u : 1.0L;
              vr += f * ar;
              vi += f * ai;
            }
          }
          Xr[r * 16 + q] = vr;
          Xi[r * 16 + q] = vi;
        }
      ld_expm(16, Xr, Xi, Er, Ei);
      for (int i = 0; i < NI; ++i) {
        const LD w = std::cos(i * th) * (i ? 2.0L : 1.0L) / NI;
        auto& mr = Mr[(size_t)b * NI + i];
        auto& mi = Mi[(size_t)b * NI + i];
        for (int e = 0; e < 256; ++e) {
          mr[e] += w * Er[e];
          mi[e] += w * Ei[e];
        }
      }
    }
  // complex-symmetric generators on a block's rows (A_j^T = A_j: -i H Δt with H real symmetric) give symmetric
  // propagators: the coefficients are symmetrised (the long-double transform leaves the two triangles a rounding
  // apart), so every form gives U[r][c] = U[c][r] bit for bit, and the interpolating chains may form the upper triangle
  // alone (k_blkp_ichain SYM: block 0, its nl live rows first in the wave block, nl (nl + 1) / 2 <= 128)
  std::vector<char> bsym(nwb, 1);
  for (int b = 0; b < nwb; ++b) {
    for (int r = 0; r < 16 && bsym[b]; ++r)
      for (int q = r + 1; q < 16 && bsym[b]; ++q) {
        const int row = wrow[16 * b + r], col = wrow[16 * b + q];
        if (row < 0 || col < 0) continue;
        for (int j = 0; j <= 1; ++j) {
          const double* x = c->h_gen.data() + 2 * (j * NN + row + (size_t)N * col);
          const double* y = c->h_gen.data() + 2 * (j * NN + col + (size_t)N * row);
          if (x[0] != y[0] || x[1] != y[1]) bsym[b] = 0;
        }
      }
    if (!bsym[b]) continue;
    for (int i = 0; i < NI; ++i) {
      auto& mr = Mr[(size_t)b * NI + i];
      auto& mi = Mi[(size_t)b * NI + i];
      for (int r = 0; r < 16; ++r)
        for (int q = r + 1; q < 16; ++q) {
          const LD ar = (mr[r * 16 + q] + mr[q * 16 + r]) / 2, ai = (mi[r * 16 + q] + mi[q * 16 + r]) / 2;
          mr[r * 16 + q] = mr[q * 16 + r] = ar;
          mi[r * 16 + q] = mi[q * 16 + r] = ai;
        }
    }
  }
  int nl = 0;
  while (nl < 16 && wrow[nl] >= 0) ++nl;
  bool sym = nwb == 1 && bsym[0] && nl * (nl + 1) / 2 <= 128;
  for (int r = nl; r < 16 && sym; ++r) sym = wrow[r] < 0;
  // per block (its own degree: a block's propagators do not depend on the other blocks of the launch); the long-double
  // transform's own rounding leaves a floor near 1e-18 under the converged coefficients
  const LD tol = std::ldexp(1.0L, -56);
  if (nwb > 8) return 1;
  std::vector<int> Db(nwb);
  int D = 0;
  for (int b = 0; b < nwb; ++b) {
    std::vector<LD> mx(NI, 0);
    for (int i = 0; i < NI; ++i)
      for (int e = 0; e < 256; ++e)
        mx[i] = std::max(mx[i], std::max(std::fabs(Mr[(size_t)b * NI + i][e]), std::fabs(Mi[(size_t)b * NI + i][e])));
    if (mx[NI - 1] > tol || mx[NI - 2] > tol) return 1;
    int d = NI - 1;
    while (d > 0 && mx[d] <= tol) --d;
    Db[b] = d;
    D = std::max(D, d);
  }
  if (blkp_int_lds(1, D) > (size_t)150 * 1024) return 1;  // one block's coefficients per launch at least
  // The exact gradient's coefficients (qoc_blkp.hpp k_blkp_grad_exact): dU/du = e^{μ(u)} Σ_i T_i(ξ) N_i with
  // N_i = μ_1 M_i + xa M'_i, xa = dξ/du = 1 / half, and M' the differentiated series: M'_{i-1} = M'_{i+1} + 2 i M_i
  // downwards, M'_0 halved.  The series differentiated is the one the chains apply, i <= Db: the coefficients past it
  // are the long-double transform's floor (~2e-18), which the recurrence's factors 2 i xa would raise to ~1e-15 in
  // every N_i, above the 2^-56 the tail rule asks for, while what they still carry of the curve is below it.  Each
  // block's own degree Eb <= Db by the same tail rule; symmetrised M_i give symmetric N_i entry by entry.
  std::vector<std::vector<LD>> Gr((size_t)nwb * NI, std::vector<LD>(256, 0)), Gi = Gr;
  std::vector<int> Eb(nwb);
  int E = 0;
  {
    const LD m1r = c->tprm.mur[1], m1i = c->tprm.mui[1];
    for (int b = 0; b < nwb; ++b) {
      const int d = Db[b];
      for (int e = 0; e < 256; ++e) {
        LD pr[NI + 2] = {0}, pi2[NI + 2] = {0};
        for (int i = d; i >= 1; --i) {
          pr[i - 1] = pr[i + 1] + 2 * i * Mr[(size_t)b * NI + i][e];
          pi2[i - 1] = pi2[i + 1] + 2 * i * Mi[(size_t)b * NI + i][e];
        }
        pr[0] /= 2;
        pi2[0] /= 2;
        for (int i = 0; i <= d; ++i) {
          const LD mr = Mr[(size_t)b * NI + i][e], mi = Mi[(size_t)b * NI + i][e];
          Gr[(size_t)b * NI + i][e] = m1r * mr - m1i * mi + pr[i] / half;
          Gi[(size_t)b * NI + i][e] = m1r * mi + m1i * mr + pi2[i] / half;
        }
      }
      int dd = d;
      auto small = [&](int i) {
        for (int e = 0; e < 256; ++e)
          if (std::max(std::fabs(Gr[(size_t)b * NI + i][e]), std::fabs(Gi[(size_t)b * NI + i][e])) > tol) return false;
        return true;
      };
      while (dd > 0 && small(dd)) --dd;
      Eb[b] = dd;
      E = std::max(E, dd);
    }
  }
  std::vector<double2> h((size_t)nwb * (D + 1) * 256);
  for (int b = 0; b < nwb; ++b)
    for (int i = 0; i <= D; ++i)
      for (int p = 0; p < 256; ++p) {  // store position p = blkp_upos(r, col): col = 4 ((p >> 4) & 3) + (p >> 6)
        const int col = 4 * ((p >> 4) & 3) + (p >> 6), row = (p & 15) ^ col, ent = row * 16 + col;
        h[((size_t)b * (D + 1) + i) * 256 + p] =
            make_double2((double)Mr[(size_t)b * NI + i][ent], (double)Mi[(size_t)b * NI + i][ent]);
      }
  const size_t nfull = h.size();
  if (sym) {  // block 0's packed upper triangle after the full layout: [i][slot], slots past nl (nl + 1) / 2 zero
    h.resize(nfull + (size_t)(D + 1) * 128, make_double2(0.0, 0.0));
    for (int i = 0; i <= D; ++i)
      for (int a = 0; a < nl; ++a)
        for (int b2 = a; b2 < nl; ++b2)
          h[nfull + (size_t)i * 128 + blkp_sym_slot(a, b2, nl)] =
              make_double2((double)Mr[i][a * 16 + b2], (double)Mi[i][a * 16 + b2]);
  }
  // N_i after them in the same two layouts: [β][i][p] with stride E + 1, then (sym) block 0's packed upper triangle
  const size_t noff = h.size();
  h.resize(noff + (size_t)nwb * (E + 1) * 256 + (sym ? (size_t)(E + 1) * 128 : 0), make_double2(0.0, 0.0));
  for (int b = 0; b < nwb; ++b)
    for (int i = 0; i <= E; ++i)
      for (int p = 0; p < 256; ++p) {
        const int col = 4 * ((p >> 4) & 3) + (p >> 6), row = (p & 15) ^ col, ent = row * 16 + col;
        h[noff + ((size_t)b * (E + 1) + i) * 256 + p] =
            make_double2((double)Gr[(size_t)b * NI + i][ent], (double)Gi[(size_t)b * NI + i][ent]);
      }
  const size_t nsoff = noff + (size_t)nwb * (E + 1) * 256;
  if (sym)
    for (int i = 0; i <= E; ++i)
      for (int a = 0; a < nl; ++a)
        for (int b2 = a; b2 < nl; ++b2)
          h[nsoff + (size_t)i * 128 + blkp_sym_slot(a, b2, nl)] =
              make_double2((double)Gr[i][a * 16 + b2], (double)Gi[i][a * 16 + b2]);
  const size_t bytes = h.size() * sizeof(double2);
  if (c->d_blkp_M.bytes() < bytes) {
    if (c->d_blkp_M) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
    }
    HIPCHK(c, c->d_blkp_M.grow(bytes));
  }
  HIPCHK(c, hipMemcpy(c->d_blkp_M, h.data(), bytes, hipMemcpyHostToDevice));
  c->int_D = D;
  c->int_Db = Db;
  c->int_sym = sym;
  c->int_nl = nl;
  c->int_nfull = nfull;
  c->int_E = E;
  c->int_Eb = Eb;
  c->int_noff = noff;
  c->int_nsoff = nsoff;
  c->int_lo = lo;
  c->int_hi = hi;
  c->int_wrow = wrow;
  c->int_ok = true;
  return QOC_OK;
}

// the interpolation's launch arguments from the cached coefficients (c->int_*: valid for bk's layout)
static void blkp_interp_args(const qoc_ctx* c, const BlkArgs& bk, BlkpIntArgs& ia) {
  ia = BlkpIntArgs{};
  ia.nwb = bk.nwb;
  ia.D = c->int_D;
  for (int b = 0; b < bk.nwb && b < 8; ++b) ia.Db[b] = c->int_Db[b];
  ia.u = c->d_u;
  ia.xa = 2.0 / (c->int_hi - c->int_lo);
  ia.xb = -(c->int_hi + c->int_lo) / (c->int_hi - c->int_lo);
  for (int j = 0; j < 2; ++j) {
    ia.mur[j] = c->tprm.mur[j];
    ia.mui[j] = c->tprm.mui[j];
  }
  ia.skew = c->skew_exact && c->tprm.mur[0] == 0.0 && c->tprm.mur[1] == 0.0;
  ia.M = c->d_blkp_M;
  ia.Msym = c->int_sym && bk.nwb == 1 ? c->d_blkp_M + c->int_nfull : nullptr;
  ia.nl = ia.Msym ? c->int_nl : 0;
}

// 0: the formation interpolates (ia filled), 1: it forms the exponentials.  One control (nu = 1) and
// QOC_BLKP_INTERP != 0; the coefficients are recomputed when the batch's control range leaves the one they were made
// for (then widened by 5 % each side, so that an optimiser's drifting controls rarely trigger it) or the generators
// or the live-block layout changed.
static int blkp_interp_setup(qoc_ctx* c, const BlkArgs& bk, BlkpIntArgs& ia) {
  if (c->nu != 1 || env_int("QOC_BLKP_INTERP", 1) == 0) return 1;
  double lo, hi;
  int r = blkp_urange(c, lo, hi);
  if (r) return r;
  if (!std::isfinite(lo) || !std::isfinite(hi)) return 1;
  const std::vector<int>& wrow = bk.wrow == c->d_wrow_live ? c->h_wrow_live : c->h_wrow;  // the host copy of bk's rows
  if (wrow.size() != 16 * (size_t)bk.nwb) return 1;
  if (!(c->int_ok && lo >= c->int_lo && hi <= c->int_hi && wrow == c->int_wrow)) {
    // a range already found too wide (within the failed one, same layout and generators): no second attempt
    if (c->int_failed && lo <= c->int_fail_lo && hi >= c->int_fail_hi && wrow == c->int_wrow) return 1;
    const double w = std::max(hi - lo, 1e-3 * std::max(1.0, std::max(std::fabs(lo), std::fabs(hi))));
    r = blkp_interp_coeffs(c, wrow, lo - 0.05 * w, hi + 0.05 * w);
    if (r == 1) r = blkp_interp_coeffs(c, wrow, lo, hi);  // without the margin
    if (r) {
      c->int_ok = false;
      if (r == 1) {
        c->int_failed = true;
        c->int_fail_lo = lo;
        c->int_fail_hi = hi;
        c->int_wrow = wrow;
      }
      return r;
    }
    c->int_failed = false;
  }
  blkp_interp_args(c, bk, ia);
  return QOC_OK;
}

// The formation's arguments and launch shape, the chain kernels' chunk size
struct BlkpPlan {
  BlkpArgs a;
  void (*kern)(BlkpArgs);
  size_t lds;
  int per_cu;
  int ch;
  size_t clds;
  bool interp;  // the formation interpolates (k_blkp_int)
  BlkpIntArgs ia;
};
// form: the plan of a launch that forms propagators (the interpolation's setup reads the control range)
static int blkp_plan(qoc_ctx* c, const BlkArgs& bk, int parts, BlkpPlan& pl, bool form = true) {
  BlkpArgs& a = pl.a;
  a = BlkpArgs{};
  a.N = c->N;
  a.nu = c->nu;
  a.nwb = bk.nwb;
  a.skew = c->skew_exact && c->tprm.mur[0] == 0.0 && c->tprm.mur[1] == 0.0 && c->tprm.mur[2] == 0.0;
  a.four = env_int("QOC_BLKP_4M", 0) != 0;
  // one product more for one squaring fewer (default): each squaring doubles the rounding error a slice carries over
  // 2000 chained slices (tunable bus, all 512 seeds against the C port: max |ΔJ| 4.7e-12 with the fewest products,
  // 9.1e-13 with slack 1 at 11.75 instead of 10.75 products per unit; tools/blkp_accuracy.py)
  a.slack = std::max(0, env_int("QOC_BLKP_SLACK", 1));
  // the accurate (r, s) choice by default (BlkpArgs::rcap): pieces of norm <= 1, truncation 2^-3 ulp after the
  // squarings; QOC_BLKP_RCAP=0 keeps the fewest-products choice (QOC_BLKP_SLACK, QOC_BLKP_TAIL)
  a.rcap = std::max(0.0, env_dbl("QOC_BLKP_RCAP", 1.0));
  a.tail = std::max(0, env_int("QOC_BLKP_TAIL", a.rcap > 0.0 ? 3 : 0));
  if (a.tail > 0) blkp_theta_table(a.tail, a.theta);
  a.wrow = bk.wrow;
  a.At = c->d_At.as<const cx<double>>();
  a.u = c->d_u;
  for (int j = 0; j < 3; ++j) {
    a.mur[j] = j <= c->nu ? c->tprm.mur[j] : 0.0;
    a.mui[j] = j <= c->nu ? c->tprm.mui[j] : 0.0;
  }
  a.prods = c->d_terms;  // qoc_chain_terms: executed 16 x 16 complex products on this path
  pl.lds = (size_t)bk.nwb * 768 * sizeof(double2) + (size_t)(BLKP_WG / 64) * BLKP_TP * sizeof(double2);
  const bool occ3 = env_int("QOC_BLKP_OCC", 0) != 2;
  pl.kern = c->nu == 1 ? (occ3 ? k_blkp_exp<1, 3> : k_blkp_exp<1, 2>) : (occ3 ? k_blkp_exp<2, 3> : k_blkp_exp<2, 2>);
  // skew-Hermitian blocks: the Chebyshev form (QOC_BLKP_CHEB = block size 4 or 6, 0 off; QOC_BLKP_CRMAX the largest
  // ρ_c before a squaring, 8 or 16)
  int cm = env_int("QOC_BLKP_CHEB", 0);
  if (cm != 4 && cm != 6) cm = 0;
  if (!a.skew) cm = 0;
  if (cm) {
    const double crmax = env_dbl("QOC_BLKP_CRMAX", 0.0) >= 16.0 ? 16.0 : 8.0;
    if (int r = blkp_cheb_table(c, cm, crmax)) return r;
    a.ctab = c->d_blkp_ctab;
    a.cgn = BLKP_CT_G0 + (int)std::lround(4.0 * std::log2(crmax)) + 1;
    a.crmax = crmax;
    pl.kern = cm == 4 ? (c->nu == 1 ? k_blkp_exp<1, 3, 4> : k_blkp_exp<2, 3, 4>)
                      : (c->nu == 1 ? k_blkp_exp<1, 2, 6> : k_blkp_exp<2, 2, 6>);
  }
  HIPCHK(c, blk_lds_attr(pl.kern, pl.lds));
  const int waves = bk.nwb * c->m;
  int ch = blkp_chunk(waves, parts);
  const int chv = env_int("QOC_BLKP_CH", 0);
  if (chv == 1 || chv == 2 || chv == 4 || chv == 8) ch = chv;
  if (blkp_chain_lds(c->N, c->m, waves, ch) > 160 * 1024) ch = blkp_chunk(waves);
  pl.ch = ch;
  pl.clds = blkp_chain_lds(c->N, c->m, waves, ch);
  pl.per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pl.per_cu, (const void*)pl.kern, BLKP_WG, pl.lds) != hipSuccess ||
      pl.per_cu < 1)
    pl.per_cu = 2;
  if (parts > 1) pl.per_cu = std::min(pl.per_cu, 2);  // a chain workgroup fits beside the formation
  pl.interp = false;
  if (form) {
    const int ri = blkp_interp_setup(c, bk, pl.ia);
    if (ri > 1 || ri < 0) return ri;
    pl.interp = ri == 0;
    c->fwd.formed_D = pl.interp ? pl.ia.D : 0;
  }
  return QOC_OK;
}
// the formation of units [unit0, units) into UF (which holds unit ubase at its start)
static int blkp_launch_exp(qoc_ctx* c, BlkpPlan& pl, long long unit0, long long units, double2* UF, long long ubase) {
  if (pl.interp) {  // seed groups cover whole (seed, slice) slots: units are multiples of nwb
    BlkpIntArgs& ia = pl.ia;
    ia.slot0 = unit0 / ia.nwb;
    ia.slots = units / ia.nwb;
    ia.ubase = ubase;
    ia.UF = UF;
    // as many blocks per launch as their coefficients fit the LDS
    const int per = std::max(1, std::min(ia.nwb, (int)((size_t)150 * 1024 / blkp_int_lds(1, ia.D))));
    for (int b0 = 0; b0 < ia.nwb; b0 += per) {
      ia.beta0 = b0;
      ia.nb = std::min(per, ia.nwb - b0);
      // workgroups of 4 waves (QOC_BLKP_INT_WG=8: 8 waves), 4 units per wave (QOC_BLKP_INT_UPW=8: 8), up to 4
      // workgroups per CU in the grid (one holds the LDS at a time when the coefficients exceed 80 KB)
      const bool w8 = env_int("QOC_BLKP_INT_WG", 0) == 8, u8 = env_int("QOC_BLKP_INT_UPW", 0) == 8;
      const int iw = w8 ? 8 : 4, upw = u8 ? 8 : 4;
      auto kern = u8 ? (w8 ? k_blkp_int<8, 512> : k_blkp_int<8, 256>) : (w8 ? k_blkp_int<4, 512> : k_blkp_int<4, 256>);
      HIPCHK(c, blk_lds_attr(kern, blkp_int_lds(ia.nb, ia.D)));
      const long long items = (ia.slots - ia.slot0 + upw - 1) / upw * ia.nb;
      const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((items + iw - 1) / iw, (long long)c->ncu * 4));
      const int mk = mark_begin(c, 0);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * iw), blkp_int_lds(ia.nb, ia.D), c->stream, ia);
      mark_end(c, mk);
      HIPCHK(c, hipGetLastError());
    }
    return QOC_OK;
  }
  pl.a.unit0 = unit0;
  pl.a.units = units;
  pl.a.UF = UF;
  pl.a.ubase = ubase;
  const unsigned grid = (unsigned)std::max<long long>(
      1, std::min<long long>((units - unit0 + BLKP_WG / 64 - 1) / (BLKP_WG / 64), (long long)c->ncu * pl.per_cu));
  const int mk = mark_begin(c, 0);
  hipLaunchKernelGGL(pl.kern, dim3(grid), dim3(BLKP_WG), pl.lds, c->stream, pl.a);
  mark_end(c, mk);
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}
// one direction's chains for seeds [s0, s1) from the propagators in U (seed useed0's first)
// (pp: the PEN instantiation -- the forward's penalty sum, the backward's λ chain with sources --, or nullptr)
template <bool FWD>
static int blkp_launch_chain(qoc_ctx* c, const BlkpPlan& pl, const TChainArgs& g, const BlkArgs& bk, const double2* U,
                             int s0, int s1, int useed0, hipStream_t st, const int* stale, const BlkpPen* pp = nullptr) {
  auto chain = pl.ch == 8   ? (pp ? k_blkp_chain<FWD, 8, true> : k_blkp_chain<FWD, 8>)
               : pl.ch == 4 ? (pp ? k_blkp_chain<FWD, 4, true> : k_blkp_chain<FWD, 4>)
               : pl.ch == 2 ? (pp ? k_blkp_chain<FWD, 2, true> : k_blkp_chain<FWD, 2>)
                            : (pp ? k_blkp_chain<FWD, 1, true> : k_blkp_chain<FWD, 1>);
  HIPCHK(c, blk_lds_attr(chain, pl.clds));
  const int mk = mark_begin(c, FWD ? 1 : 2, st);
  hipLaunchKernelGGL(chain, dim3(s1 - s0), dim3(64 * bk.nwb * c->m), pl.clds, st, g, bk, U, s0, useed0, stale,
                     pp ? *pp : BlkpPen{});
  mark_end(c, mk, st);
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}
// the order-3 gradient from x_k, μ_{k+1} and the λ_N coefficients
// (lam: d_L holds λ_k itself, the PEN backward chains')
static int blkp_launch_grad(qoc_ctx* c, const BlkArgs& bk, double* d_dJdu, const int* stale, cx<double>* coef_out,
                            bool lam = false) {
  BlkpGradArgs ga{};
  ga.N = c->N;
  ga.m = c->m;
  ga.Nt = c->Nt;
  ga.nwb = bk.nwb;
  ga.wrow = bk.wrow;
  ga.A = c->d_A.as<const cx<double>>();
  ga.u = c->d_u;
  ga.X = c->d_X.as<const cx<double>>();
  ga.L = c->d_L.as<const cx<double>>();
  ga.coef = c->d_coef;
  ga.dJdu = d_dJdu;
  ga.tiles = (long long)c->B * ((c->Nt + 15) / 16);
  ga.stale = stale;
  ga.coef_out = coef_out;
  // generators diagonal on the live wave blocks' rows (QOC_BLKP_GDIAG=0: every product on MFMA)
  ga.diag = 0;
  if (env_int("QOC_BLKP_GDIAG", 1) != 0) {
    const std::vector<int>& wrow = bk.wrow == c->d_wrow_live ? c->h_wrow_live : c->h_wrow;
    const size_t NN = (size_t)c->N * c->N;
    for (int j = 1; j <= c->nu && wrow.size() == 16 * (size_t)bk.nwb; ++j) {
      bool dg = true;
      for (int w = 0; w < bk.nwb && dg; ++w)
        for (int r = 0; r < 16 && dg; ++r)
          for (int q = 0; q < 16 && dg; ++q) {
            const int row = wrow[16 * w + r], col = wrow[16 * w + q];
            if (row < 0 || col < 0 || row == col) continue;
            const double* z = c->h_gen.data() + 2 * (j * NN + row + (size_t)c->N * col);
            dg = z[0] == 0.0 && z[1] == 0.0;
          }
      if (dg) ga.diag |= 1u << j;
    }
  }
  const size_t glds = blkp_grad_lds(bk.nwb, c->nu);
  auto gk = c->nu == 1 ? (lam ? k_blkp_grad<1, true> : k_blkp_grad<1>) : (lam ? k_blkp_grad<2, true> : k_blkp_grad<2>);
  HIPCHK(c, blk_lds_attr(gk, glds));
  int gpc = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&gpc, (const void*)gk, 256, glds) != hipSuccess || gpc < 1) gpc = 2;
  const unsigned ggrid = (unsigned)std::max<long long>(1, std::min<long long>((ga.tiles + 3) / 4, (long long)c->ncu * gpc));
  const int mg = mark_begin(c, 3);
  hipLaunchKernelGGL(gk, dim3(ggrid), dim3(256), glds, c->stream, ga);
  mark_end(c, mg);
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}
// The exact gradient (QOC_DUKDP_EXACT) stays on these propagators where their interpolation applies: one control,
// QOC_BLKP_INTERP != 0 (and a converged series: known once the coefficients of the batch's range are formed);
// QOC_BLKP_EXACT=0 leaves it to the block exponential of the dense path
bool blkp_exact_on(const qoc_ctx* c) {
  return blkp_on(c) && c->nu == 1 && env_int("QOC_BLKP_INTERP", 1) != 0 && env_int("QOC_BLKP_EXACT", 1) != 0;
}
// the exact gradient from x_k, μ_{k+1} (lam: λ_{k+1}) and the cached derivative coefficients N_i of bk's layout
// (c->int_*: blkp_interp_coeffs), in place of blkp_launch_grad
static int blkp_launch_grad_exact(qoc_ctx* c, const BlkArgs& bk, double* d_dJdu, const int* stale, cx<double>* coef_out,
                                  bool lam = false) {
  const std::vector<int>& wrow = bk.wrow == c->d_wrow_live ? c->h_wrow_live : c->h_wrow;
  if (!(c->int_ok && wrow == c->int_wrow && (int)c->int_Eb.size() == bk.nwb && bk.nwb <= 8))
    return fail(c, QOC_ERR_STATE, "exact block gradient: no derivative coefficients for this block layout");
  BlkpGxArgs ga{};
  ga.N = c->N;
  ga.m = c->m;
  ga.Nt = c->Nt;
  ga.B = c->B;
  ga.nwb = bk.nwb;
  ga.E = c->int_E;
  for (int b = 0; b < bk.nwb; ++b) ga.Eb[b] = c->int_Eb[b];
  ga.wrow = bk.wrow;
  ga.u = c->d_u;
  ga.xa = 2.0 / (c->int_hi - c->int_lo);
  ga.xb = -(c->int_hi + c->int_lo) / (c->int_hi - c->int_lo);
  for (int j = 0; j < 2; ++j) {
    ga.mur[j] = c->tprm.mur[j];
    ga.mui[j] = c->tprm.mui[j];
  }
  ga.skew = c->skew_exact && c->tprm.mur[0] == 0.0 && c->tprm.mur[1] == 0.0;
  // complex-symmetric generators: the upper triangle alone (QOC_BLKP_ISYM=0: every entry)
  const bool sym = c->int_sym && bk.nwb == 1 && env_int("QOC_BLKP_ISYM", 1) != 0;
  ga.Nc = c->d_blkp_M + (sym ? c->int_nsoff : c->int_noff);
  ga.nl = sym ? c->int_nl : 0;
  ga.X = c->d_X.as<const cx<double>>();
  ga.L = c->d_L.as<const cx<double>>();
  ga.coef = c->d_coef;
  ga.dJdu = d_dJdu;
  ga.stale = stale;
  auto gk = sym ? (lam ? k_blkp_grad_exact<true, true> : k_blkp_grad_exact<false, true>)
                : (lam ? k_blkp_grad_exact<true, false> : k_blkp_grad_exact<false, false>);
  // 8 waves per workgroup, 4 where one block's coefficients leave no room for 8 waves' staging rows (E <= D: 148 KB at
  // the most); as many blocks per launch as fit the LDS beside them
  const int waves = blkp_gx_lds(1, ga.E, sym, BLKP_GX_WG / 64) <= (size_t)160 * 1024 ? BLKP_GX_WG / 64 : 4;
  const size_t room = (size_t)160 * 1024 - blkp_gx_lds(0, ga.E, sym, waves);
  const int per = std::max(1, std::min(bk.nwb, (int)(room / blkp_gx_lds(1, ga.E, sym, 0))));
  const long long items = (long long)c->B * ((c->Nt + BLKP_GX_UPW - 1) / BLKP_GX_UPW);
  for (int b0 = 0; b0 < bk.nwb; b0 += per) {
    ga.beta0 = b0;
    ga.nb = std::min(per, bk.nwb - b0);
    ga.accum = b0 > 0;
    ga.coef_out = b0 == 0 ? coef_out : nullptr;
    const size_t lds = blkp_gx_lds(ga.nb, ga.E, sym, waves);
    HIPCHK(c, blk_lds_attr(gk, lds));
    int gpc = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&gpc, (const void*)gk, 64 * waves, lds) != hipSuccess || gpc < 1) gpc = 1;
    const long long wgs = (items + waves - 1) / waves;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(wgs, (long long)c->ncu * gpc));
    const int mg = mark_begin(c, 3);
    hipLaunchKernelGGL(gk, dim3(grid), dim3(64 * waves), lds, c->stream, ga);
    mark_end(c, mg);
    HIPCHK(c, hipGetLastError());
  }
  return QOC_OK;
}
// the interpolating chains (k_blkp_ichain) apply: the interpolation (one control), one live wave block, one state
// column, and the block's coefficients in the LDS beside four waves' rows (QOC_BLKP_ICHAIN=0: the stored form)
constexpr int BLKP_ISL = 8;  // slices per chunk
static bool blkp_ichain_sym(const BlkpIntArgs& ia) {  // complex-symmetric generators: the upper triangle alone
  return ia.Msym && env_int("QOC_BLKP_ISYM", 1) != 0;
}
// 0: the stored form, 1: the interpolating chains (every entry), 2: the same on the upper triangle
static int blkp_ichain_on(const qoc_ctx* c, const BlkArgs& bk, const BlkpPlan& pl) {
  if (env_int("QOC_BLKP_ICHAIN", 1) == 0) return 0;
  const bool sym = pl.interp && blkp_ichain_sym(pl.ia);
  if (!(pl.interp && bk.nwb == 1 && c->m == 1 && blkp_ichain_lds(pl.ia.D, BLKP_ISL, 4, sym) <= 160 * 1024)) return 0;
  return sym ? 2 : 1;
}
// dual: the forward chain and the μ recurrence of every seed (one launch), else direction dir alone; the forward's
// terminal cost and λ_N coefficients by k_terminal_cost (64 threads: chain_costs as the one-wave chain workgroups run
// it, the same sums); stale: a queued stale-u flag (nonzero: nothing is written)
// pp: the PEN instantiations (one direction at a time): the forward leaves the seeds' penalty sums in J, which
// k_terminal_cost then adds the terminal cost to; the backward is the λ chain with sources
static int blkp_launch_ichain(qoc_ctx* c, const TChainArgs& gf, const TChainArgs& gb, const BlkArgs& bk,
                              const BlkpIntArgs& ia0, bool dual, int dir, const int* stale, const BlkpPen* pp = nullptr) {
  // the slices' e^{μ(u_k)} first (one sincos per (seed, slice) instead of one per chain wave)
  const size_t nph = (size_t)c->B * c->Nt;
  if (c->d_blkp_ph.bytes() < nph * sizeof(double2)) {
    if (c->d_blkp_ph) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_blkp_ph.grow(nph * sizeof(double2)));
  }
  BlkpIntArgs ia = ia0;
  ia.ph = c->d_blkp_ph;
  hipLaunchKernelGGL(k_blkp_phase, dim3((unsigned)std::min<size_t>((nph + 255) / 256, 4096)), dim3(256), 0, c->stream, ia,
                     (long long)nph);
  HIPCHK(c, hipGetLastError());
  // (the next chunk's interpolation interleaved with this chunk's steps measured slower: 2.45 ms at SL = 4, 2.68 ms at
  // SL = 8 with AGPR spills, against 1.95 ms in sequence; profiles/r06v_ichain_ab.txt)
  // complex-symmetric generators: the upper triangle alone (QOC_BLKP_ISYM=0: every entry)
  const bool sym = blkp_ichain_sym(ia);
  // two waves per (seed, direction) on one SIMD, taking alternate chunks (QOC_BLKP_IPAIR=0: one wave)
  const int pairs = (dual ? 2 : 1) * c->B;
  // pairs per workgroup: 4 (the two waves of a pair on one SIMD) unless that leaves CUs without one, then 2
  // (QOC_BLKP_IPW=2 on the dual launch: two workgroups per CU, the pairs' waves on different SIMDs; tests force either)
  const int npw = env_int("QOC_BLKP_IPW", pairs >= 4 * c->ncu ? 4 : 2) == 4 ? 4 : 2;
  const bool pair = env_int("QOC_BLKP_IPAIR", 1) != 0 && blkp_ipair_lds(ia.D, BLKP_ISL, sym, npw) <= 160 * 1024;
  auto kern = pp ? (pair ? (sym ? k_blkp_ichain2<BLKP_ISL, true, true> : k_blkp_ichain2<BLKP_ISL, false, true>)
                         : (sym ? k_blkp_ichain<BLKP_ISL, true, true> : k_blkp_ichain<BLKP_ISL, false, true>))
                   : (pair ? (sym ? k_blkp_ichain2<BLKP_ISL, true> : k_blkp_ichain2<BLKP_ISL, false>)
                           : (sym ? k_blkp_ichain<BLKP_ISL, true> : k_blkp_ichain<BLKP_ISL, false>));
  const size_t lds = pair ? blkp_ipair_lds(ia.D, BLKP_ISL, sym, npw) : blkp_ichain_lds(ia.D, BLKP_ISL, 4, sym);
  HIPCHK(c, blk_lds_attr(kern, lds));
  const int per = pair ? npw : 4;  // (seed, direction) pairs per workgroup
  const int mk = mark_begin(c, dual || dir == 0 ? 1 : 2);
  hipLaunchKernelGGL(kern, dim3((pairs + per - 1) / per), dim3(pair ? 128 * npw : 256), lds, c->stream, gf, gb, bk, ia,
                     0, c->B, dual ? 1 : 0, dir, stale, pp ? *pp : BlkpPen{});
  mark_end(c, mk);
  HIPCHK(c, hipGetLastError());
  if (dual || dir == 0) {
    hipLaunchKernelGGL(k_terminal_cost<double>, dim3(c->B), dim3(64), 0, c->stream, c->N, c->m, c->Nt,
                       (const cx<double>*)gf.X, (const cx<double>*)gf.Xt, gf.cost_kind, gf.n_norm, pp ? 1 : 0, gf.J,
                       gf.coef, gf.sc);
    HIPCHK(c, hipGetLastError());
  }
  return QOC_OK;
}
static int blkp_parts(const qoc_ctx* c) { return std::max(1, std::min(env_int("QOC_BLKP_PARTS", 4), c->B)); }

// qoc_eval_dev: U_k per (seed, slice, live block) on MFMA, the forward chain and the μ recurrence from the stored
// propagators, then the order-3 gradient.  The formation is MFMA-bound and the chains are bound by their propagator
// reads: the seeds go in `parts` groups, the chains of group p (second stream) beside the formation of group p + 1, with
// the formation at two workgroups per CU so that a chain workgroup fits beside them (QOC_BLKP_PARTS, default 4; 1: one
// formation, then the chains).  The propagators of two groups are held at a time (the formation of group p + 2 waits
// for the chains of group p): 2.1 GB at the tunable bus' B = 512 instead of every seed's 4.2 GB.  Returns 1 (nothing
// launched) when even that does not fit in the free HBM: the Chebyshev block chains then run.
int blkp_eval_concurrent(qoc_ctx* c, int order, double* d_dJdu, const BlkArgs& bk) {
  const bool exact = order == QOC_DUKDP_EXACT;
  TChainArgs gf = tchain_args(c);
  TChainArgs gb = tchain_args(c);
  gb.mu_mode = 1;
  int r;
  const int parts = blkp_parts(c);
  const long long per_seed = (long long)c->Nt * bk.nwb;  // units per seed
  const int gmax = (c->B + parts - 1) / parts;           // seeds of the largest group
  const int nslab = parts > 1 ? 2 : 1;
  const size_t slab = (size_t)gmax * per_seed * 256;      // double2 per slab
  BlkpPlan pl;
  if ((r = blkp_plan(c, bk, parts, pl))) return r;
  if (exact && !pl.interp) return 1;  // no curve to differentiate: the caller's dense path, nothing launched here
  const int ichain = blkp_ichain_on(c, bk, pl);
  if (ichain) {  // both chains interpolate their own propagators: nothing stored
    if ((r = blkp_zero_dead(c, bk, true))) return r;
    if ((r = blkp_launch_ichain(c, gf, gb, bk, pl.ia, true, 0, nullptr))) return r;
    blkp_forward_done(c, ichain);
    if ((r = exact ? blkp_launch_grad_exact(c, bk, d_dJdu, nullptr, c->d_coef_mu)
                   : blkp_launch_grad(c, bk, d_dJdu, nullptr, c->d_coef_mu)))
      return r;
    c->bwd.is_mu = true;
    c->bwd.route = 7;
    return QOC_OK;
  }
  if ((r = blkp_ensure_store(c, nslab * slab * sizeof(double2), true))) return r;  // 1: does not fit
  if ((r = blkp_zero_dead(c, bk, true))) return r;
  // events: [p] group p formed, [parts + p] group p's chains done, [2 parts] everything queued before
  if (parts > 1) {
    if ((r = ensure_stream2(c, 2 * parts + 1))) return r;
    HIPCHK(c, hipEventRecord(c->sync_ev[2 * parts], c->stream));  // the second stream after everything queued so far
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->sync_ev[2 * parts], 0));
  }
  hipStream_t cs = parts > 1 ? c->stream2 : c->stream;
  // QOC_BLKP_PRIO=1: the chain waves at the top issue priority.  Measured: each group's chains 1.63 -> 1.07 ms, the
  // formation beside them 1.85 -> 1.97 ms per group, and the formation is the critical path (8.72 vs 8.93 ms per
  // eval), so off by default
  const int cprio = env_int("QOC_BLKP_PRIO", 0);
  auto chain = pl.ch == 8 ? k_blkp_dual<8> : pl.ch == 4 ? k_blkp_dual<4> : pl.ch == 2 ? k_blkp_dual<2> : k_blkp_dual<1>;
  HIPCHK(c, blk_lds_attr(chain, pl.clds));
  const int waves = bk.nwb * c->m;
  for (int p = 0; p < parts; ++p) {
    const int s0 = (int)((long long)c->B * p / parts), s1 = (int)((long long)c->B * (p + 1) / parts);
    if (s1 <= s0) continue;
    double2* const U = c->d_blkU.as<double2>() + (size_t)(p % nslab) * slab;
    if (p >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, c->sync_ev[parts + p - 2], 0));  // slab p % 2 read out
    if ((r = blkp_launch_exp(c, pl, (long long)s0 * per_seed, (long long)s1 * per_seed, U, (long long)s0 * per_seed)))
      return r;
    if (parts > 1) {
      HIPCHK(c, hipEventRecord(c->sync_ev[p], c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->stream2, c->sync_ev[p], 0));
    }
    const int mk = mark_begin(c, 1, cs);
    hipLaunchKernelGGL(chain, dim3(2 * (s1 - s0)), dim3(64 * waves), pl.clds, cs, gf, gb, bk, (const double2*)U, s0, s0,
                       cprio);
    mark_end(c, mk, cs);
    HIPCHK(c, hipGetLastError());
    if (parts > 1) HIPCHK(c, hipEventRecord(c->sync_ev[parts + p], c->stream2));
  }
  if (parts > 1) {  // the gradient (and everything after it on the engine stream) after the last chains
    HIPCHK(c, hipEventRecord(c->sync_ev[2 * parts], c->stream2));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->sync_ev[2 * parts], 0));
  }
  blkp_forward_done(c, 0);
  if ((r = exact ? blkp_launch_grad_exact(c, bk, d_dJdu, nullptr, c->d_coef_mu)
                 : blkp_launch_grad(c, bk, d_dJdu, nullptr, c->d_coef_mu)))
    return r;
  c->bwd.is_mu = true;
  c->bwd.route = 7;
  return QOC_OK;
}

// the stored-propagator eval applies (blocks of 5..16 rows with a live-wave layout that fits the chain and gradient
// kernels)
bool blkp_fits_nwb(const qoc_ctx* c, int nwb) {
  const int waves = nwb * c->m;
  return waves <= 8 && blkp_chain_lds(c->N, c->m, waves, blkp_chunk(waves)) <= 160 * 1024 &&
         blkp_grad_lds(nwb, c->nu) <= 160 * 1024;
}

// propagate on stored propagators (the reference's own structure, src/gradient_computations.jl:17-29): every U_k of
// the live blocks formed on MFMA, the forward chain from them (seed groups pipelined as in the eval), states in d_X;
// the propagators stay for grape_sensitivity (every seed's: 4.2 GB at the tunable bus' B = 512).  Built-in costs; a
// state penalty's sum is the chains' own (their PEN instantiations; QOC_BLKP_PEN=0: the Chebyshev block chains take a
// penalised propagate); QOC_BLKP_SPLIT=0 keeps the Chebyshev block chains.  Returns 1 (nothing launched) when it does
// not apply.
int blkp_forward(qoc_ctx* c) {
  const int pmode = blkp_pen_mode(c);
  if (env_int("QOC_BLKP_SPLIT", 1) == 0 || !blkp_on(c) || (c->mu != 0.0 && pmode == 2) ||
      (c->cost_kind != QOC_COST_TRACE && c->cost_kind != QOC_COST_ZCAL))
    return 1;
  BlkArgs bk = blk_args(c);
  int r = blk_live(c, bk, pmode == 1 && c->src_on);  // a co-state source: every block live
  if (r) return r;
  if (!blkp_fits_nwb(c, bk.nwb)) return 1;
  // the penalised forward: the chains' PEN instantiations add the penalty sum to J
  BlkpPen pp;
  const BlkpPen* const pen = pmode == 1 && blkp_pen_active(c, pp) ? &pp : nullptr;
  const long long per_seed = (long long)c->Nt * bk.nwb;
  const int parts = blkp_parts(c);
  BlkpPlan pl;
  if ((r = blkp_plan(c, bk, parts, pl))) return r;
  const TChainArgs gf = tchain_args(c);
  const int ichain = blkp_ichain_on(c, bk, pl);
  // what either end leaves for grape_sensitivity (blkp_backward_ok, blkp_backward)
  auto done = [&]() {
    blkp_forward_done(c, ichain);
    c->fwd.kind = 2;
    c->fwd.ichain = ichain != 0;
    c->fwd.nwb = bk.nwb;
    c->fwd.interp = pl.interp;
    return QOC_OK;
  };
  if (ichain) {  // the forward chain interpolates its propagators; grape_sensitivity's μ recurrence will too
    if ((r = blkp_zero_dead(c, bk, false))) return r;
    if ((r = blkp_launch_ichain(c, gf, gf, bk, pl.ia, false, 0, nullptr, pen))) return r;
    return done();
  }
  if ((r = blkp_ensure_store(c, (size_t)c->B * per_seed * 256 * sizeof(double2), true))) return r;
  if ((r = blkp_zero_dead(c, bk, false))) return r;
  if (parts > 1) {
    if ((r = ensure_stream2(c, parts + 1))) return r;
    HIPCHK(c, hipEventRecord(c->sync_ev[parts], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->sync_ev[parts], 0));
  }
  hipStream_t cs = parts > 1 ? c->stream2 : c->stream;
  double2* const U = c->d_blkU.as<double2>();
  for (int p = 0; p < parts; ++p) {
    const int s0 = (int)((long long)c->B * p / parts), s1 = (int)((long long)c->B * (p + 1) / parts);
    if (s1 <= s0) continue;
    if ((r = blkp_launch_exp(c, pl, (long long)s0 * per_seed, (long long)s1 * per_seed, U, 0))) return r;
    if (parts > 1) {
      HIPCHK(c, hipEventRecord(c->sync_ev[p], c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->stream2, c->sync_ev[p], 0));
    }
    if ((r = blkp_launch_chain<true>(c, pl, gf, bk, U, s0, s1, 0, cs, nullptr, pen))) return r;
  }
  if (parts > 1) {
    HIPCHK(c, hipEventRecord(c->sync_ev[parts], c->stream2));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->sync_ev[parts], 0));
  }
  return done();
}

bool blkp_backward_ok(const qoc_ctx* c, int order) {
  // the exact gradient: the derivative of the curve the propagate interpolated on (blkp_exact_on)
  const bool ord_ok = order == 3 || (order == QOC_DUKDP_EXACT && blkp_exact_on(c) && c->fwd.interp);
  if (!(c->fwd.kind == 2 && ord_ok && (c->cost_kind == QOC_COST_TRACE || c->cost_kind == QOC_COST_ZCAL) &&
        (c->fwd.ichain || c->d_blkU)))
    return false;
  const int pmode = blkp_pen_mode(c);
  if (pmode == 2) return false;                                                   // the Chebyshev block chains
  return !(pmode == 1 && c->src_on && !blkp_fits_nwb(c, c->nwb));  // a co-state source: every block's waves
}

// grape_sensitivity after blkp_forward: the μ recurrence from the stored propagators (μ_N = X_target, λ_k = coef ⊙ μ_k,
// src/penalty_fcns.jl:19-22, 35-40), then the order-3 gradient; stale: the device flag of a queued stale-u check.
// With a state penalty or a co-state source (blkp_pen_mode 1) the chains' PEN instantiations run λ_k itself,
// λ_N = coef ⊙ X_target + s_N, λ_k = U_k^H λ_{k+1} + s_k (src/gradient_computations.jl:46-58), and the gradient reads it
// as it is.  A source counts every block live; where the propagate ran on other wave blocks (the live ones alone, or
// the interpolating chains of one block) the propagators of this layout are formed first, from the propagate's u.
int blkp_backward(qoc_ctx* c, int order, double* d_dJdu, const int* stale) {
  const bool exact = order == QOC_DUKDP_EXACT;
  const int pmode = blkp_pen_mode(c);
  BlkArgs bk = blk_args(c);
  int r = blk_live(c, bk, c->src_on);
  if (r) return r;
  if ((r = blk_coef_mu(c))) return r;
  BlkpPen pp;
  const bool lam = pmode == 1;
  if (lam) blkp_pen_active(c, pp);  // (no penalised entry: empty masks, the caller's source alone)
  const BlkpPen* const pen = lam ? &pp : nullptr;
  TChainArgs gb = tchain_args(c);
  gb.mu_mode = lam ? 0 : 1;
  if (bk.nwb != c->fwd.nwb) {  // the propagators of this layout
    BlkpPlan pl;
    if ((r = blkp_plan(c, bk, 1, pl))) return r;  // (with this layout's N_i when it interpolates)
    if (exact && !pl.interp) return 1;            // this layout's series did not converge: nothing launched
    const long long units = (long long)c->B * c->Nt * bk.nwb;
    if ((r = blkp_ensure_store(c, (size_t)units * 256 * sizeof(double2), false))) return r;
    if ((r = blkp_launch_exp(c, pl, 0, units, c->d_blkU.as<double2>(), 0))) return r;
    c->fwd.ichain = false;  // the forward's leftovers are now the stored propagators of this layout
    c->fwd.formed_ichain = 0;
    c->fwd.nwb = bk.nwb;
  }
  // the dead rows of d_L (a no-op unless a sourced backward, or co-states from before x0 or the target moved to another
  // block, left λ there).  k_zero_rows reads no stale flag, and a refused call must leave the last grape_sensitivity's
  // co-states as they are: when there is something to zero, the host waits for the check first
  if (stale && bk.nwb != c->nwb && blk_dead_pending(c, c->d_L))
    if (const int w = wait_stale_check(c)) return w;
  if ((r = blkp_zero_dead(c, bk, true))) return r;
  if (c->fwd.ichain) {  // the propagate interpolated: the μ recurrence from the same coefficients (the same u)
    BlkpIntArgs ia;
    blkp_interp_args(c, bk, ia);
    if ((r = blkp_launch_ichain(c, gb, gb, bk, ia, false, 1, stale, pen))) return r;
  } else {
    BlkpPlan pl;
    if ((r = blkp_plan(c, bk, 1, pl, false))) return r;
    if ((r = blkp_launch_chain<false>(c, pl, gb, bk, c->d_blkU.as<const double2>(), 0, c->B, 0, c->stream, stale, pen)))
      return r;
  }
  if ((r = exact ? blkp_launch_grad_exact(c, bk, d_dJdu, stale, lam ? nullptr : c->d_coef_mu, lam)
                 : blkp_launch_grad(c, bk, d_dJdu, stale, lam ? nullptr : c->d_coef_mu, lam)))
    return r;
  if (c->src_on) c->dead_dirty = true;  // λ_k is nonzero on the rows of blocks that carry no state
  c->bwd = {};  // (backward() resets after the split paths: they state the whole record)
  c->bwd.is_mu = !lam;
  c->bwd.route = 7;
  return QOC_OK;
}

}  // namespace qoc_host
