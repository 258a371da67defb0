// qoc_run_ode.hip — the fixed-step Tsit5 path (qoc_ode.hpp: k_ode_pwc, k_ode_envelope; qoc_ode_grad.hpp: the
// envelope run's discrete adjoint) and the terminal-cost kernel of the paths without a fused forward epilogue.
#include "qoc_bgemm.hpp"
#include "qoc_internal.hpp"
#include "qoc_ode.hpp"
#include "qoc_ode_grad.hpp"

namespace qoc_host {

// ---- ODE path (fixed-step Tsit5, qoc_ode.hpp) ------------------------------------------------
// k_ode_pwc instantiation by N: register-resident rows up to 48 (fp64) / 64 (fp32), LDS beyond
template <typename T>
void launch_ode_pwc(qoc_ctx* c, int adjoint, cx<T>* S, const unsigned char* pmask, double two_mu) {
  const int N = c->N, W = std::min(c->m, 4);
  const size_t lds = (((size_t)N * N * c->esz + 15) & ~(size_t)15) + (size_t)W * 64 * c->esz;
  auto go = [&](auto kern) {
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(c->B), dim3(64 * W), lds, c->stream, N, c->m, c->nu, c->Nt, c->nsub, adjoint,
                       c->d_A.as<const cx<T>>(), (const double*)c->d_u, c->d_x0.as<const cx<T>>(), c->x0_per_seed, S,
                       c->d_X.as<const cx<T>>(), pmask, two_mu);
  };
  if (c->ode_kernel == 1) go(k_ode_pwc<T, 0>);
  else if (N <= 16) go(k_ode_pwc<T, 16>);
  else if (N <= 32) go(k_ode_pwc<T, 32>);
  else if (N <= 48) go(k_ode_pwc<T, 48>);
  else if (sizeof(T) == 4) go(k_ode_pwc<T, 64>);
  else go(k_ode_pwc<T, 0>);
}

template <typename T>
int ode_forward(qoc_ctx* c) {
  int mk = mark_begin(c, 1);
  launch_ode_pwc<T>(c, 0, c->d_X.as<cx<T>>(), nullptr, 0.0);
  HIPCHK(c, hipGetLastError());
  const bool pen = c->mu != 0.0;
  if (pen) {
    hipLaunchKernelGGL((k_penalty_sum<T>), dim3(c->B), dim3(256), 0, c->stream, c->N, c->m, c->Nt,
                       c->d_X.as<const cx<T>>(), c->d_pmask, c->mu, c->d_J);
    HIPCHK(c, hipGetLastError());
  }
  if (c->cost_kind != QOC_COST_EXTERNAL) {
    hipLaunchKernelGGL((k_terminal_cost<T>), dim3(c->B), dim3(256), 0, c->stream, c->N, c->m, c->Nt,
                       c->d_X.as<const cx<T>>(), c->d_Xt.as<const cx<T>>(), c->cost_kind, c->cost_n, pen ? 1 : 0, c->d_J,
                       c->d_coef, sectors(c));
    HIPCHK(c, hipGetLastError());
  } else if (!pen) {
    HIPCHK(c, hipMemsetAsync(c->d_J, 0, (size_t)c->B * sizeof(double), c->stream));
  }
  mark_end(c, mk);
  return QOC_OK;
}

template <typename T>
int ode_adjoint(qoc_ctx* c) {
  const int N = c->N, m = c->m, Nt = c->Nt, B = c->B;
  const size_t Nm = (size_t)N * m;
  const bool pen = c->mu != 0.0;
  const unsigned eb = (unsigned)std::min<size_t>((Nm * B + 255) / 256, 8192);
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
  launch_ode_pwc<T>(c, 1, c->d_L.as<cx<T>>(), pen ? c->d_pmask : nullptr, 2.0 * c->mu);
  HIPCHK(c, hipGetLastError());
  mark_end(c, mk);
  return QOC_OK;
}

hipError_t launch_envelope(qoc_ctx* c, int kind, const double* dP, int np, double dt, long long nsteps) {
  const size_t lds = (size_t)(c->nu + 1) * c->N * c->N * c->esz;
  const int W = std::min(c->m, 4);
  hipError_t e;
  if (c->prec == QOC_FP64) {
    e = hipFuncSetAttribute((const void*)k_ode_envelope<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_ode_envelope<double>), dim3(c->B), dim3(64 * W), lds, c->stream, c->N, c->m, c->nu, c->Nt,
                       kind, dP, np, dt, nsteps, c->d_A.as<const cx<double>>(), c->d_x0.as<const cx<double>>(),
                       c->x0_per_seed, c->d_X.as<cx<double>>());
  } else {
    e = hipFuncSetAttribute((const void*)k_ode_envelope<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_ode_envelope<float>), dim3(c->B), dim3(64 * W), lds, c->stream, c->N, c->m, c->nu, c->Nt,
                       kind, dP, np, dt, nsteps, c->d_A.as<const cx<float>>(), c->d_x0.as<const cx<float>>(),
                       c->x0_per_seed, c->d_X.as<cx<float>>());
  }
  return hipGetLastError();
}

// J and the λ_N coefficients of the stored x_N (no state penalty)
hipError_t launch_terminal_cost(qoc_ctx* c) {
  if (c->prec == QOC_FP64)
    hipLaunchKernelGGL((k_terminal_cost<double>), dim3(c->B), dim3(256), 0, c->stream, c->N, c->m, c->Nt,
                       c->d_X.as<const cx<double>>(), c->d_Xt.as<const cx<double>>(), c->cost_kind, c->cost_n, 0, c->d_J,
                       c->d_coef, sectors(c));
  else
    hipLaunchKernelGGL((k_terminal_cost<float>), dim3(c->B), dim3(256), 0, c->stream, c->N, c->m, c->Nt,
                       c->d_X.as<const cx<float>>(), c->d_Xt.as<const cx<float>>(), c->cost_kind, c->cost_n, 0, c->d_J,
                       c->d_coef, sectors(c));
  return hipGetLastError();
}

// ---- qoc_eval_envelope: checkpoint spacing, workspace, launches (qoc_ode_grad.hpp) ----
// The spacing C: 1 (every x_n stored, no segment re-run) while the checkpoints fit the workspace budget, else the
// smallest spacing that does (QOC_ENV_WS_MB sets the budget, read at the first call); QOC_ENV_CKPT forces it.  Either is bounded by the LDS ring of C x N per column wave
// beside the generators; a forced spacing beyond that runs at the bound.  The conjugate-transposed generator copies
// are kept when both sets take at most 64 KiB: a function of N and nu alone, so that the spacing does not decide
// which mat-vec runs.  The workspace grows when a call needs more and stays with the context.
int env_grad_plan(qoc_ctx* c, long long nsteps, EnvGradPlan* pl) {
  const size_t gen = (size_t)(c->nu + 1) * c->N * c->N * sizeof(cx<double>);
  const int W = std::min(c->m, 4);
  pl->W = W;
  pl->tr = 2 * gen <= 64 * 1024;
  const size_t fixed = (pl->tr ? 2 : 1) * gen + (size_t)W * 64 * sizeof(double);
  const size_t per_c = (size_t)W * c->N * sizeof(cx<double>);
  if (fixed + per_c > 160 * 1024)
    return fail(c, QOC_ERR_UNSUPPORTED, "generators (%zu B) leave no LDS for the adjoint's state ring", gen);
  const long long c_lds = (long long)((160 * 1024 - fixed) / per_c);
  const size_t per_ckpt = (size_t)c->B * c->m * 2 * c->N * sizeof(cx<double>);
  if (!c->env_budget) {
    size_t freeb = 0, totalb = 0;
    (void)hipMemGetInfo(&freeb, &totalb);
    c->env_budget = std::max<size_t>(std::min<size_t>(1ull << 30, freeb / 4), 1);
    if (env_set("QOC_ENV_WS_MB")) c->env_budget = std::max<size_t>((size_t)(env_dbl("QOC_ENV_WS_MB", 0.0) * 1048576.0), 1);
  }
  long long C = 1;
  if (c->env_ckpt > 0) {
    C = std::min<long long>(c->env_ckpt, c_lds);
  } else {
    const long long fit = std::max<long long>(1, (long long)(c->env_budget / per_ckpt));  // checkpoints that fit
    C = std::max<long long>(1, (nsteps + fit - 1) / fit);
    if (C > c_lds)
      return fail(c, QOC_ERR_UNSUPPORTED,
                  "%lld steps need a checkpoint spacing of %lld in a workspace of %zu MiB; the LDS ring holds %lld",
                  nsteps, C, c->env_budget >> 20, c_lds);
  }
  pl->C = (int)C;
  pl->nseg = (int)((nsteps + C - 1) / C);
  pl->lds = fixed + (size_t)pl->C * per_c;
  const size_t need = std::max<size_t>(1, (size_t)pl->nseg) * per_ckpt;
  if (need > c->d_env_ws.bytes()) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_env_ws.grow(need));
  }
  return QOC_OK;
}

hipError_t launch_envelope_ckpt(qoc_ctx* c, int kind, const double* dP, int np, double dt, long long nsteps,
                                const EnvGradPlan& pl) {
  const size_t lds = (size_t)(c->nu + 1) * c->N * c->N * sizeof(cx<double>);
  hipError_t e = hipFuncSetAttribute((const void*)k_ode_envelope_ckpt, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ode_envelope_ckpt, dim3(c->B), dim3(64 * pl.W), lds, c->stream, c->N, c->m, c->nu, c->Nt, kind,
                     dP, np, dt, nsteps, pl.C, pl.nseg, c->d_A.as<const cx<double>>(), c->d_x0.as<const cx<double>>(),
                     c->x0_per_seed, c->d_X.as<cx<double>>(), c->d_env_ws.as<cx<double>>());
  return hipGetLastError();
}

// d_lam: the caller's λ_N (B x N x m, QOC_COST_EXTERNAL) or nullptr: λ_N from d_coef and the target
hipError_t launch_envelope_grad(qoc_ctx* c, int kind, const double* dP, int np, double dt, long long nsteps,
                                const EnvGradPlan& pl, const void* d_lam, double* d_dJdp) {
  auto go = [&](auto kern) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(c->B), dim3(64 * pl.W), pl.lds, c->stream, c->N, c->m, kind, dP, np, dt, nsteps, pl.C,
                       pl.nseg, c->d_A.as<const cx<double>>(), c->d_env_ws.as<const cx<double>>(), c->d_Xt.as<const cx<double>>(),
                       (const cx<double>*)c->d_coef, (const cx<double>*)d_lam, d_dJdp);
    return hipGetLastError();
  };
  if (c->nu == 1) return pl.tr ? go(k_ode_envelope_grad<1, true>) : go(k_ode_envelope_grad<1, false>);
  return pl.tr ? go(k_ode_envelope_grad<2, true>) : go(k_ode_envelope_grad<2, false>);
}

template int ode_forward<double>(qoc_ctx*);
template int ode_forward<float>(qoc_ctx*);
template int ode_adjoint<double>(qoc_ctx*);
template int ode_adjoint<float>(qoc_ctx*);

}  // namespace qoc_host
