// qoc_run_grad.hip — launches of the fused order-3 gradient (qoc_grad_rr.hpp: k_grad_rr_q / _p / _s / _c) and of the
// exact gradient as a series on the same tiles (k_grad_rr_xn / _xq / _xp).
#include "qoc_grad_rr.hpp"
#include "qoc_internal.hpp"

namespace qoc_host {

// Fused order-3 gradient (qoc_grad_rr.hpp): k_grad_rr_q (co-state side -> W0, W1 in the state layout)
// then k_grad_rr_p (state side + contraction -> dJdu).  Persistent grids of 4-wave workgroups.
template <typename T, int NT, int KS, int NU>
int grad_rr_launch(qoc_ctx* c, double* d_dJdu, hipStream_t st, int k0, int nk, int mode) {
  using G = GradRR<T, NT>;
  const int N = c->N, m = c->m, Nt = c->Nt, B = c->B;
  const size_t lds = G::lds_bytes(N, NU);
  const long long units = (long long)B * nk, ntiles = (units + 16 / m - 1) / (16 / m);
  const int per_cu = lds <= 80 * 1024 ? 2 : 1;
  const int grid = (int)std::max<long long>(1, std::min<long long>((ntiles + 3) / 4, (long long)c->ncu * per_cu));
  const size_t bufN = (size_t)N * ((size_t)B * (Nt + 1) * m);
  cx<T>* W0 = c->d_gws.as<cx<T>>();
  cx<T>* W1 = W0 + bufN;
  // mode 0: q + p;  1: state side only (k_grad_rr_s -> P1, P2 in d_pws);  2: q + p reading P1, P2
  cx<T>* P1 = c->d_pws.as<cx<T>>();
  cx<T>* P2 = P1 ? P1 + bufN : nullptr;
  if (mode == 1) {
    HIPCHK(c, hipFuncSetAttribute((const void*)k_grad_rr_s<T, NT, KS, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_grad_rr_s<T, NT, KS, NU>), dim3(grid), dim3(256), lds, st, N, m, Nt, B, k0, nk,
                       c->d_A.as<const cx<T>>(), c->d_u, c->d_X.as<const cx<T>>(), P1, P2);
    HIPCHK(c, hipGetLastError());
    return QOC_OK;
  }
  HIPCHK(c, hipFuncSetAttribute((const void*)k_grad_rr_q<T, NT, KS, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_grad_rr_q<T, NT, KS, NU>), dim3(grid), dim3(256), lds, st, N, m, Nt, B, k0, nk,
                     c->d_A.as<const cx<T>>(), c->d_u, c->d_L.as<const cx<T>>(), W0, W1);
  HIPCHK(c, hipGetLastError());
  if (mode == 2) {
    HIPCHK(c, hipFuncSetAttribute((const void*)k_grad_rr_p<T, NT, KS, NU, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_grad_rr_p<T, NT, KS, NU, true>), dim3(grid), dim3(256), lds, st, N, m, Nt, B, k0, nk,
                       c->d_A.as<const cx<T>>(), c->d_u, c->d_X.as<const cx<T>>(), c->d_L.as<const cx<T>>(), (const cx<T>*)W0,
                       (const cx<T>*)W1, d_dJdu, (const cx<T>*)P1, (const cx<T>*)P2);
  } else {
    HIPCHK(c, hipFuncSetAttribute((const void*)k_grad_rr_p<T, NT, KS, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_grad_rr_p<T, NT, KS, NU>), dim3(grid), dim3(256), lds, st, N, m, Nt, B, k0, nk,
                       c->d_A.as<const cx<T>>(), c->d_u, c->d_X.as<const cx<T>>(), c->d_L.as<const cx<T>>(), (const cx<T>*)W0,
                       (const cx<T>*)W1, d_dJdu);
  }
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}

template <typename T, int NT, int NU>
int grad_rr_nt(qoc_ctx* c, double* d_dJdu, hipStream_t st, int k0, int nk, int mode) {
  const int ks = sizeof(T) == 8 ? (c->N + 3) / 4 : 4 * NT;
  if constexpr (sizeof(T) == 8) {
    if (ks == 4 * NT - 3) return grad_rr_launch<T, NT, 4 * NT - 3, NU>(c, d_dJdu, st, k0, nk, mode);
    if (ks == 4 * NT - 2) return grad_rr_launch<T, NT, 4 * NT - 2, NU>(c, d_dJdu, st, k0, nk, mode);
    if (ks == 4 * NT - 1) return grad_rr_launch<T, NT, 4 * NT - 1, NU>(c, d_dJdu, st, k0, nk, mode);
  }
  return grad_rr_launch<T, NT, 4 * NT, NU>(c, d_dJdu, st, k0, nk, mode);
}

template <typename T>
int grad_rr_o3(qoc_ctx* c, double* d_dJdu, hipStream_t st, int k0, int nk, int mode) {
  const int NT = (c->N + 15) / 16;
  if (c->nu == 1) {
    if (NT == 1) return grad_rr_nt<T, 1, 1>(c, d_dJdu, st, k0, nk, mode);
    if (NT == 2) return grad_rr_nt<T, 2, 1>(c, d_dJdu, st, k0, nk, mode);
    return grad_rr_nt<T, 3, 1>(c, d_dJdu, st, k0, nk, mode);
  }
  if (NT == 1) return grad_rr_nt<T, 1, 2>(c, d_dJdu, st, k0, nk, mode);
  if (NT == 2) return grad_rr_nt<T, 2, 2>(c, d_dJdu, st, k0, nk, mode);
  return grad_rr_nt<T, 3, 2>(c, d_dJdu, st, k0, nk, mode);
}

// k_grad_rr_c over the units of slices [k0, k0 + nk) (fp64: the captures come from the MFMA chains)
template <int NT, int KS, int NU>
int grad_cap_launch(qoc_ctx* c, double* d_dJdu, hipStream_t st, int k0, int nk, bool mu_mode) {
  using G = GradRR<double, NT>;
  const int N = c->N, m = c->m, Nt = c->Nt, B = c->B;
  const size_t lds = G::lds_bytes(N, NU);
  const long long units = (long long)B * nk, ntiles = (units + 16 / m - 1) / (16 / m);
  // as many resident workgroups as the kernel's registers and LDS allow (N <= 16: 3 per CU; the loads of a tile
  // are waited for before its contractions, so resident waves are the memory-level parallelism)
  HIPCHK(c, hipFuncSetAttribute((const void*)k_grad_rr_c<NT, KS, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  static int occ = 0;  // per instantiation (lds depends on N, fixed by the instantiation up to 3 rows)
  int per_cu = occ;
  if (per_cu < 1) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_grad_rr_c<NT, KS, NU>, 256, lds) !=
            hipSuccess ||
        per_cu < 1)
      per_cu = lds <= 80 * 1024 ? 2 : 1;
    occ = per_cu;
  }
  const int grid = (int)std::max<long long>(1, std::min<long long>((ntiles + 3) / 4, (long long)c->ncu * per_cu));
  const size_t bufN = (size_t)N * ((size_t)B * (Nt + 1) * m);
  GradCapArgs a{};
  a.N = N;
  a.m = m;
  a.Nt = Nt;
  a.B = B;
  a.k0 = k0;
  a.nk = nk;
  a.Agen = c->d_A;
  a.u = c->d_u;
  a.X = c->d_X;
  a.L = c->d_L;
  a.F1 = c->d_pws;
  a.F2 = c->d_pws.as<const cx<double>>() + bufN;
  a.G1 = c->d_gws;
  a.G2 = c->d_gws.as<const cx<double>>() + bufN;
  a.steps = c->d_steps.as<const double>();
  for (int j = 0; j < 3; ++j) {
    a.mur[j] = j <= c->nu ? c->tprm.mur[j] : 0.0;
    a.mui[j] = j <= c->nu ? c->tprm.mui[j] : 0.0;
  }
  a.kappa = c->fwd.steps_cheb ? 2.0 : 1.0;
  a.coef = mu_mode ? c->d_coef : nullptr;
  a.rsec_mask = 0;
  if (c->packed)
    for (int r = 0; r < N && r < 64; ++r) a.rsec_mask |= (unsigned long long)(c->h_rsec[r] & 1) << r;
  a.dJdu = d_dJdu;
  hipLaunchKernelGGL((k_grad_rr_c<NT, KS, NU>), dim3(grid), dim3(256), lds, st, a);
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}

template <int NT, int NU>
int grad_cap_nt(qoc_ctx* c, double* d_dJdu, hipStream_t st, int k0, int nk, bool mu_mode) {
  const int ks = (c->N + 3) / 4;
  if (ks == 4 * NT - 3) return grad_cap_launch<NT, 4 * NT - 3, NU>(c, d_dJdu, st, k0, nk, mu_mode);
  if (ks == 4 * NT - 2) return grad_cap_launch<NT, 4 * NT - 2, NU>(c, d_dJdu, st, k0, nk, mu_mode);
  if (ks == 4 * NT - 1) return grad_cap_launch<NT, 4 * NT - 1, NU>(c, d_dJdu, st, k0, nk, mu_mode);
  return grad_cap_launch<NT, 4 * NT, NU>(c, d_dJdu, st, k0, nk, mu_mode);
}

int grad_rr_cap(qoc_ctx* c, double* d_dJdu, hipStream_t st, int k0, int nk, bool mu_mode) {
  if (c->prec != QOC_FP64 || !c->d_pws || !c->d_gws) return fail(c, QOC_ERR_STATE, "captured gradient: no captures");
  const int NT = (c->N + 15) / 16;
  if (c->nu == 1) {
    if (NT == 1) return grad_cap_nt<1, 1>(c, d_dJdu, st, k0, nk, mu_mode);
    if (NT == 2) return grad_cap_nt<2, 1>(c, d_dJdu, st, k0, nk, mu_mode);
    return grad_cap_nt<3, 1>(c, d_dJdu, st, k0, nk, mu_mode);
  }
  if (NT == 1) return grad_cap_nt<1, 2>(c, d_dJdu, st, k0, nk, mu_mode);
  if (NT == 2) return grad_cap_nt<2, 2>(c, d_dJdu, st, k0, nk, mu_mode);
  return grad_cap_nt<3, 2>(c, d_dJdu, st, k0, nk, mu_mode);
}

// ---- the exact gradient as a series (k_grad_rr_xn / _xq / _xp) ----
template <int NT, int KS, int NU>
int gradx_launch(qoc_ctx* c, const GradXArgs& a, hipStream_t st) {
  using G = GradRR<double, NT>;
  const size_t lds = G::lds_bytes(a.N, NU);
  const long long units = (long long)a.B * a.nk, ntiles = (units + 16 / a.m - 1) / (16 / a.m);
  const int per_cu = lds <= 80 * 1024 ? 2 : 1;
  const int grid = (int)std::max<long long>(1, std::min<long long>((ntiles + 3) / 4, (long long)c->ncu * per_cu));
  HIPCHK(c, hipFuncSetAttribute((const void*)k_grad_rr_xq<double, NT, KS, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_grad_rr_xq<double, NT, KS, NU>), dim3(grid), dim3(256), lds, st, a);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipFuncSetAttribute((const void*)k_grad_rr_xp<double, NT, KS, NU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_grad_rr_xp<double, NT, KS, NU>), dim3(grid), dim3(256), lds, st, a);
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}

template <int NT, int NU>
int gradx_nt(qoc_ctx* c, const GradXArgs& a, hipStream_t st) {
  const int ks = (a.N + 3) / 4;
  if (ks == 4 * NT - 3) return gradx_launch<NT, 4 * NT - 3, NU>(c, a, st);
  if (ks == 4 * NT - 2) return gradx_launch<NT, 4 * NT - 2, NU>(c, a, st);
  if (ks == 4 * NT - 1) return gradx_launch<NT, 4 * NT - 1, NU>(c, a, st);
  return gradx_launch<NT, 4 * NT, NU>(c, a, st);
}

// Route (include/qoc.h QOC_DUKDP_EXACT): fp64 dense contexts the fused kernels fit, exponential propagation.  Block
// contexts keep frechet_grad on every leg that reaches dense_gradient: it is the second implementation their tests
// compare against.  The term counts are read back once (16 bytes, one stream synchronisation): the routing decision
// and the workspace size depend on the largest one.
template <typename T>
int grad_rr_exact(qoc_ctx* c, double* d_dJdu) {
  if constexpr (sizeof(T) != 8) {
    return 1;
  } else {
    if (!c->exact_series || !c->grad_rr || c->prop_method != QOC_PROP_EXPM || blk_active(c)) return 1;
    const int N = c->N, m = c->m, Nt = c->Nt, B = c->B, nu = c->nu;
    const long long units = (long long)B * Nt;
    if (!c->d_xn) HIPCHK(c, c->d_xn.alloc(2 * sizeof(unsigned long long) + (size_t)units * sizeof(int)));
    // ρ_k: the chain prep's bound of Ã_k, spectral half-widths where the Chebyshev chains apply, else 1-norms
    const bool cheb = c->chain_mode == 1 && c->cheb && tchain_mf(c);
    GradXCount cn{};
    cn.nu = nu;
    cn.units = units;
    cn.u = c->d_u;
    for (int j = 0; j <= nu; ++j) cn.rho[j] = cheb ? c->tprm.rad[j] : c->tprm.nrm[j];
    cn.nterm = (int*)(c->d_xn + 2);
    cn.stat = c->d_xn;
    HIPCHK(c, hipMemsetAsync(c->d_xn, 0, 2 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_grad_rr_xn, dim3((unsigned)std::min<long long>((units + 255) / 256, 1024)), dim3(256), 0,
                       c->stream, cn);
    HIPCHK(c, hipGetLastError());
    unsigned long long h[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->d_xn, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int nmax = (int)h[0];
    if (nmax > GRADX_NMAX) {
      ++c->xs_stats[3];
      return 1;
    }
    if (nmax < 1) return fail(c, QOC_ERR_STATE, "exact series: no term counts");
    if (!c->xws_budget) {
      if (env_set("QOC_GRAD_EXACT_WS_MB")) {
        c->xws_budget = (size_t)std::max(1, env_int("QOC_GRAD_EXACT_WS_MB", 1)) << 20;
      } else {
        size_t freeb = 0, totalb = 0;
        (void)hipMemGetInfo(&freeb, &totalb);
        c->xws_budget = std::max<size_t>(std::min<size_t>(2ull << 30, freeb / 8), 1);
      }
    }
    // slices per range: nmax R(b) of B nk units each within the budget (one slice when even that exceeds it)
    const size_t per_slice = (size_t)nmax * B * N * m * c->esz;
    const int nk_r = (int)std::max<size_t>(1, std::min<size_t>(c->xws_budget / per_slice, (size_t)Nt));
    const size_t need = per_slice * nk_r;
    HIPCHK(c, c->d_fws.grow(need));
    GradXArgs a{};
    a.N = N;
    a.m = m;
    a.Nt = Nt;
    a.B = B;
    a.nmax = nmax;
    a.Agen = c->d_A;
    a.u = c->d_u;
    a.X = c->d_X;
    a.L = c->d_L;
    a.R = c->d_fws;
    a.nterm = cn.nterm;
    for (int j = 0; j < 3; ++j) {
      a.mur[j] = j <= nu ? c->tprm.mur[j] : 0.0;
      a.mui[j] = j <= nu ? c->tprm.mui[j] : 0.0;
    }
    double f = 1.0;
    for (int b = 0; b < GRADX_NMAX; ++b) {
      f /= (double)(b + 1);
      a.c[b] = f;  // 1 / (b+1)!
    }
    a.dJdu = d_dJdu;
    const int NT = (N + 15) / 16;
    for (int k0 = 0; k0 < Nt; k0 += nk_r) {
      a.k0 = k0;
      a.nk = std::min(nk_r, Nt - k0);
      int r;
      if (nu == 1) r = NT == 1 ? gradx_nt<1, 1>(c, a, c->stream) : NT == 2 ? gradx_nt<2, 1>(c, a, c->stream) : gradx_nt<3, 1>(c, a, c->stream);
      else r = NT == 1 ? gradx_nt<1, 2>(c, a, c->stream) : NT == 2 ? gradx_nt<2, 2>(c, a, c->stream) : gradx_nt<3, 2>(c, a, c->stream);
      if (r) return r;
    }
    c->xs_stats[0] += units;
    c->xs_stats[1] += (long long)h[1];
    c->xs_stats[2] = std::max<long long>(c->xs_stats[2], nmax);
    return QOC_OK;
  }
}

template int grad_rr_exact<double>(qoc_ctx*, double*);
template int grad_rr_exact<float>(qoc_ctx*, double*);
template int grad_rr_o3<double>(qoc_ctx*, double*, hipStream_t, int, int, int);
template int grad_rr_o3<float>(qoc_ctx*, double*, hipStream_t, int, int, int);

}  // namespace qoc_host
