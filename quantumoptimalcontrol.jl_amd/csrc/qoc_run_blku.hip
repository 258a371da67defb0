// qoc_run_blku.hip — block propagators for blocks of <= 4 rows (qoc_blku.hpp), the default for them: formed per
// (slice, block) apart from the serial chain, which then runs one NB x NB matvec per slice (blku_on, qoc_run_blk.hip).
#include "qoc_blk_host.hpp"
#include "qoc_blku.hpp"

namespace qoc_host {

struct BlkuShape {
  int C, CW, W, S, ustg;
  size_t lds;
};
// Waves per workgroup: CW chain waves (one lane per state element), in the fused backward one staging wave, and FW
// worker waves (formation, in the fused backward also the contraction).  The workers are the critical path (their
// chunk of formation + contraction takes longer than the chain's C matvecs), so FW takes every wave slot left:
// 8 waves per CU at the kernels' > 128 VGPRs (2 per SIMD), shared by the B / CUs workgroups a CU holds at once
// (QOC_BLKU_FW / QOC_BLKU_GFW override FW).  C: the most slices per chunk (a power of two <= 64: chunks never
// straddle k_blku_rec's 64-slice (J, P) groups) whose LDS fits those workgroups (QOC_BLKU_C / QOC_BLKU_GC override
// it).  S: the prefix-product group (QOC_BLKU_S; 1 by default: the chains are store- or latency-bound at S = 1 and
// the scans cost the workers more than they save).
static BlkuShape blku_shape(const qoc_ctx* c, bool fused, bool storeu = false) {
  BlkuShape s{};
  const int NB = c->blk_nb;
  s.CW = (c->nblk * c->m * (NB == 2 ? 2 : 4) + 63) / 64;  // one chain lane per state element (qoc_blku.hpp)
  const int per_cu = std::max(1, std::min(3, (c->B + c->ncu - 1) / std::max(1, c->ncu)));
  // the fused backward's staging waves: with stored propagators one more, unless one wave can hold a chunk's records,
  // x_k and propagators (QOC_BLKU_USTG=1: then the freed wave slot is a worker's)
  s.ustg = storeu && env_int("QOC_BLKU_USTG", 0) == 1 ? 1 : 2;
  int stg = fused ? (storeu && s.ustg == 2 ? 2 : 1) : 0;
  // waves per workgroup at most: the kernels' launch bound (blku_max_threads: 12 waves for blocks of 2 rows), shared
  // by the workgroups of a CU
  const int wcap = blku_max_threads(NB) / 64;
  // the fused backward needs at least one worker wave (the contraction runs on workers only): with the second
  // staging wave that would not fit (blocks of 4 rows, nblk m > 16: CW = 2 within 4 waves), one stager copies all
  if (fused && stg == 2 && s.CW + stg + 1 > wcap) {
    s.ustg = 1;
    stg = 1;
  }
  const int wmax = std::max(s.CW + stg + 1, wcap / per_cu);
  int fw = env_int(fused ? "QOC_BLKU_GFW" : "QOC_BLKU_FW", wmax - s.CW - stg);
  fw = std::max(1, std::min(fw, wcap - s.CW - stg));
  s.W = s.CW + stg + fw;
  s.S = env_int("QOC_BLKU_S", 1) >= 2 && NB < 4 ? 2 : 1;
  const size_t budget = (size_t)156 * 1024 / per_cu;
  const int gw = fused ? fw : 0;
  s.C = 64;
  // the stager's registers: x_k and the stored propagators of one chunk
  auto stage_ok = [&](int C) { return !fused || std::max(C * c->N * c->m, C * NB * NB * c->nblk) <= BLKU_XMAX * 64; };
  auto fits = [&](int C) { return blku_lds(c->N, c->m, NB, c->nblk, C, gw) <= budget && stage_ok(C); };
  if (!fused) {
    while (s.C > 4 && !fits(s.C)) s.C >>= 1;
  } else {
    // the fused backward: the largest C that fits, then within [Cmax / 2, Cmax] the C whose wave-iterations of the
    // contraction (ceil(C / UPW), UPW = 64 / nblk slices each) come out most even over the fw workers: the fewest
    // iterations of the busiest worker per slice (ties: the larger C, fewer chunk barriers)
    while (s.C > 4 && !fits(s.C)) --s.C;
    const int upw = std::max(1, 64 / std::max(1, c->nblk)), cmax = s.C;
    auto per_slice = [&](int C) { return (double)(((C + upw - 1) / upw + fw - 1) / fw) / C; };
    for (int C = cmax; C >= std::max(4, cmax / 2); --C)
      if (per_slice(C) < per_slice(s.C) - 1e-12) s.C = C;
  }
  if (const char* cenv = fused ? "QOC_BLKU_GC" : "QOC_BLKU_C"; env_set(cenv)) {
    // an override is clamped to what fits (the stager's registers and the LDS budget), never an invalid launch
    const int want = std::min(env_int(cenv, 0), 64);
    int q = 1;
    if (fused) {
      q = std::max(1, want);
      while (q > 1 && !fits(q)) --q;
    } else {
      while (q * 2 <= want && fits(q * 2)) q *= 2;
    }
    s.C = q;
  }
  s.C = std::max(s.C, s.S);
  s.lds = blku_lds(c->N, c->m, NB, c->nblk, s.C, gw);
  s.W = std::min(s.W, wcap);  // never above the launch bound (a larger launch faults)
  if (fused && s.W < s.CW + stg + 1) s.W = 0;  // no worker wave: not launchable (blku_fused_ok refuses it)
  return s;
}

static int blku_ntp(const qoc_ctx* c) { return (c->Nt + BLKU_RECBLK - 1) / BLKU_RECBLK * BLKU_RECBLK; }

static BlkuParams blku_params(const qoc_ctx* c, const BlkuShape& s, double* d_dJdu = nullptr) {
  BlkuParams p{};
  for (int j = 0; j < 3; ++j) {
    const bool on = j <= c->nu;
    // skew-Hermitian generators: spectral half-widths (the 2-norm bound of Ã_k); otherwise the shifted 1-norms
    p.rad[j] = on ? (c->cheb_ok ? c->tprm.rad[j] : c->tprm.nrm[j]) : 0.0;
    p.mur[j] = on ? c->tprm.mur[j] : 0.0;
    p.mui[j] = on ? c->tprm.mui[j] : 0.0;
  }
  p.theta_cap = c->tprm.theta[17];
  p.C = s.C;
  p.CW = s.CW;
  p.Ntp = blku_ntp(c);
  p.rec = c->d_blkrec;
  p.terms = c->d_terms;
  p.dJdu = d_dJdu;
  return p;
}

// the step records of every (seed, slice) of the current u (k_blku_rec); count: add Σ P 2^J to the terms counter
static int blku_records(qoc_ctx* c, BlkuParams& bp, bool count, const double* d_u = nullptr) {
  const long long total = (long long)c->B * blku_ntp(c);
  if (!c->d_blkrec) HIPCHK(c, c->d_blkrec.alloc((size_t)total * BLKU_REC * sizeof(double)));
  bp.rec = c->d_blkrec;
  BlkuParams rp = bp;
  rp.terms = count ? c->d_terms : nullptr;
  const int mk = mark_begin(c, 0);
  hipLaunchKernelGGL(k_blku_rec, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, rp,
                     d_u ? d_u : (const double*)c->d_u, c->nu, c->Nt, total, c->d_blkrec);
  mark_end(c, mk);
  HIPCHK(c, hipGetLastError());
  return QOC_OK;
}

template <typename F>
static hipError_t blku_dispatch(const qoc_ctx* c, F&& f) {
  using std::integral_constant;
  switch (c->blk_nb) {
    case 2: return f(integral_constant<int, 2>());
    case 3: return f(integral_constant<int, 3>());
    case 4: return f(integral_constant<int, 4>());
  }
  return hipErrorInvalidValue;
}

// the prefix-product group size as a compile-time constant (1, or 2 for blocks of <= 3 rows)
template <int NB, typename F>
static hipError_t blku_sdispatch(int S, F&& f) {
  using std::integral_constant;
  if constexpr (NB <= 3)
    if (S == 2) return f(integral_constant<int, 2>());
  return f(integral_constant<int, 1>());
}

static hipError_t blku_launch_fwd_g(qoc_ctx* c, const TChainArgs& g, const BlkuShape& s, const BlkuParams& bp) {
  const BlkArgs bk = blk_args(c);
  return blku_dispatch(c, [&](auto NB_) {
    constexpr int NB = decltype(NB_)::value;
    return blku_sdispatch<NB>(s.S, [&](auto S_) {
      constexpr int S = decltype(S_)::value;
      const hipError_t q = blk_lds_attr(k_blku_fwd<NB, S>, s.lds);
      if (q != hipSuccess) return q;
      hipLaunchKernelGGL((k_blku_fwd<NB, S>), dim3(c->B), dim3(64 * s.W), s.lds, c->stream, g, bk, bp);
      return hipGetLastError();
    });
  });
}

static hipError_t blku_launch_fwd(qoc_ctx* c, const BlkuShape& s, const BlkuParams& bp) {
  return blku_launch_fwd_g(c, tchain_args(c), s, bp);
}

int blku_forward(qoc_ctx* c) {
  const BlkuShape s = blku_shape(c, false);
  BlkuParams bp = blku_params(c, s);
  int r = blku_records(c, bp, true);
  if (r) return r;
  const int mk = mark_begin(c, 1);
  const hipError_t e = blku_launch_fwd(c, s, bp);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blku_fwd launch: %s", hipGetErrorString(e));
  c->props_since_reset++;
  return QOC_OK;
}

// the order-o gradient from d_X and d_L (mu_mode: d_L holds μ, λ = coef ⊙ μ with the coefficients in d_coef)
static int blku_grad(qoc_ctx* c, int order, bool mu_mode, double* d_dJdu) {
  const TChainArgs g = tchain_args(c);
  const BlkArgs bk = blk_args(c);
  const long long units = (long long)c->B * c->Nt;
  const int upw = 64 / blku_nbp(c->nblk);  // units per wave (blocks on power-of-two lane groups)
  if (upw < 1) return fail(c, QOC_ERR_UNSUPPORTED, "block gradient: %d blocks exceed one wave", c->nblk);
  const long long waves = (units + upw - 1) / upw;
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((waves + 3) / 4, (long long)c->ncu * 8));
  const size_t glds = blku_grad_lds(c->blk_nb, c->nblk);
  const int mk = mark_begin(c, 3);
  // the column count as a compile-time constant (operand prefetch) for blocks of 2 rows with m = 2 (cavity)
  const bool m2 = c->blk_nb == 2 && c->m == 2 && !env_is("QOC_BLKU_GRAD_PF", "0");
  const hipError_t e = blku_dispatch(c, [&](auto NB_) {
    constexpr int NB = decltype(NB_)::value;
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), glds, c->stream, g, bk, units, (int)mu_mode, d_dJdu);
      return hipGetLastError();
    };
    auto by_m = [&](auto ORD_) {
      constexpr int ORD = decltype(ORD_)::value;
      if constexpr (NB == 2) {
        if (m2) return launch(k_blku_grad<NB, ORD, 2>);
      }
      return launch(k_blku_grad<NB, ORD, 0>);
    };
    return blk_order_dispatch(order, by_m);
  });
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blku_grad launch: %s", hipGetErrorString(e));
  return QOC_OK;
}

// the plain backward chain (λ_Nt -> λ_0 into d_L; add: the penalty / co-state source after every slice)
static hipError_t blku_launch_bwd(qoc_ctx* c, const TChainArgs& g, const BlkuShape& s, const BlkuParams& bp, bool add) {
  const BlkArgs bk = blk_args(c);
  return blku_dispatch(c, [&](auto NB_) {
    constexpr int NB = decltype(NB_)::value;
    auto launch = [&](auto kern) {
      const hipError_t q = blk_lds_attr(kern, s.lds);
      if (q != hipSuccess) return q;
      hipLaunchKernelGGL(kern, dim3(c->B), dim3(64 * s.W), s.lds, c->stream, g, bk, bp);
      return hipGetLastError();
    };
    if (add) return launch(k_blku_bwd<NB, 1, true>);  // additions after every slice: no prefix groups
    return blku_sdispatch<NB>(s.S, [&](auto S_) { return launch(k_blku_bwd<NB, decltype(S_)::value, false>); });
  });
}

// The fused backward (k_blku_bwdg): orders 1..4 without a penalty or co-state source.  λ stays in the workgroups;
// qoc_get_costates recomputes it on demand from a copy of this evaluation's u and λ_N coefficients (blku_costates).
static bool blku_fused_ok(const qoc_ctx* c, int order) {
  return order >= 1 && order <= BLK_ORDMAX && c->mu == 0.0 && !c->src_on && !env_is("QOC_BLKU_FUSED", "0") &&
         blku_shape(c, true, false).W > 0;
}

static int blku_bwdg(qoc_ctx* c, int order, double* d_dJdu, const double2* Uin = nullptr) {
  const TChainArgs g = tchain_args(c);
  const BlkArgs bk = blk_args(c);
  const BlkuShape s = blku_shape(c, true, Uin != nullptr);
  if (s.W <= 0) return fail(c, QOC_ERR_UNSUPPORTED, "fused block backward: no worker wave fits the launch bound");
  BlkuParams bp = blku_params(c, s, d_dJdu);  // the records are current (the caller's)
  bp.Uin = Uin;
  bp.ustg = s.ustg;
  const int mk = mark_begin(c, 2);
  const hipError_t e = blku_dispatch(c, [&](auto NB_) {
    constexpr int NB = decltype(NB_)::value;
    return blku_sdispatch<NB>(s.S, [&](auto S_) {
      constexpr int S = decltype(S_)::value;
      return blk_order_dispatch(order, [&](auto ORD_) {
        constexpr int ORD = decltype(ORD_)::value;
        const hipError_t q = blk_lds_attr(k_blku_bwdg<NB, S, ORD>, s.lds);
        if (q != hipSuccess) return q;
        hipLaunchKernelGGL((k_blku_bwdg<NB, S, ORD>), dim3(c->B), dim3(64 * s.W), s.lds, c->stream, g, bk, bp);
        return hipGetLastError();
      });
    });
  });
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blku_bwdg launch: %s", hipGetErrorString(e));
  // what qoc_get_costates needs to rebuild λ: this u and the λ_N coefficients (external λ_N stays in d_L)
  const size_t nu_t = (size_t)c->B * c->nu * c->Nt, ncf = (size_t)c->B * 2 * c->m;
  if (!c->d_u_lam) {
    HIPCHK(c, c->d_coef_lam.alloc(ncf * sizeof(cx<double>)));
    HIPCHK(c, c->d_u_lam.alloc(nu_t * sizeof(double)));
  }
  HIPCHK(c, hipMemcpyAsync(c->d_u_lam, c->d_u, nu_t * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_coef_lam, c->d_coef, ncf * sizeof(cx<double>), hipMemcpyDeviceToDevice, c->stream));
  c->bwd.lazy = true;
  c->bwd.route = 5;
  return QOC_OK;
}

// the block forward chain on d_u into d_X, J and the coefficients into scratch
static int blku_states_of(qoc_ctx* c, const double* d_u) {
  if (!c->d_J_scr) {
    HIPCHK(c, c->d_coef_scr.alloc((size_t)c->B * 2 * c->m_user * sizeof(cx<double>)));
    HIPCHK(c, c->d_J_scr.alloc((size_t)c->B * sizeof(double)));
  }
  TChainArgs g = tchain_args(c);
  g.J = c->d_J_scr;
  g.coef = c->d_coef_scr;
  g.pmask = nullptr;
  g.u = d_u;
  const BlkuShape s = blku_shape(c, false);
  BlkuParams bp = blku_params(c, s);
  int r = blku_records(c, bp, false, d_u);
  if (r) return r;
  const hipError_t e = blku_launch_fwd_g(c, g, s, bp);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blku_fwd launch (states): %s", hipGetErrorString(e));
  return QOC_OK;
}

// x_k of the last segmented eval: the block forward chain on the u it left in d_u (the eval's own J and coefficients
// stay as they were)
int blku_states(qoc_ctx* c) {
  if (!c->fwd.lazy) return QOC_OK;
  const int r = blku_states_of(c, c->d_u);
  if (r == QOC_OK) c->fwd.lazy = false;
  return r;
}

// qoc_get_costates after a fused backward: the plain backward chain from the saved u and coefficients into d_L
// After a penalised segmented eval λ_k carries the source 2 μ x_k[P, C], so the states of the saved u are rebuilt
// first (into d_X, which then counts as lazy again: the last propagate's u may be another).  qoc_set_state_penalty
// materialises before it changes the penalty, so the one in force here is the eval's.
int blku_costates(qoc_ctx* c) {
  if (!c->bwd.lazy) return QOC_OK;
  TChainArgs g = tchain_args(c);
  g.coef = c->d_coef_lam;
  g.u = c->d_u_lam;
  g.src = nullptr;  // (a lazily kept λ never had one: the paths that leave it decline a co-state source)
  int r = QOC_OK;
  if (g.pmask) {
    if ((r = blku_states_of(c, c->d_u_lam))) return r;
    c->fwd.lazy = true;
  }
  const BlkuShape s = blku_shape(c, false);
  BlkuParams bp = blku_params(c, s);
  r = blku_records(c, bp, false, c->d_u_lam);
  if (r) return r;
  const hipError_t e = blku_launch_bwd(c, g, s, bp, g.pmask != nullptr);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blku_bwd launch: %s", hipGetErrorString(e));
  c->bwd.lazy = false;
  return QOC_OK;
}

// grape_sensitivity: the fused backward when it applies; otherwise λ by the plain backward chain (penalty, co-state
// source and an external λ_N included), then the block gradient for orders 1..4 or the dense exact (Fréchet) one
int blku_backward(qoc_ctx* c, int order, double* d_dJdu) {
  const TChainArgs g = tchain_args(c);
  const BlkuShape s = blku_shape(c, false);
  BlkuParams bp = blku_params(c, s);
  int r = blku_records(c, bp, false);  // the u of the last propagate (stale-checked by the caller)
  if (r) return r;
  if (blku_fused_ok(c, order)) return blku_bwdg(c, order, d_dJdu);
  const int mk = mark_begin(c, 2);
  const hipError_t e = blku_launch_bwd(c, g, s, bp, g.pmask || g.src);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blku_bwd launch: %s", hipGetErrorString(e));
  if (order == QOC_DUKDP_EXACT) return dense_gradient<double>(c, order, d_dJdu);
  return blku_grad(c, order, false, d_dJdu);
}

// qoc_eval_dev (built-in cost, no penalty, no co-state source): the step records once, the forward chain (J and the
// λ_N coefficients), then the fused backward -- x_k is written once and read once, λ never leaves the workgroups
int blku_eval_concurrent(qoc_ctx* c, int order, double* d_dJdu) {
  BlkuShape s = blku_shape(c, false);
  // the forward's prefix groups apart from the backward's (QOC_BLKU_FS; the stored propagators are the plain ones)
  if (env_set("QOC_BLKU_FS")) {
    s.S = env_int("QOC_BLKU_FS", 0) >= 2 && c->blk_nb < 4 ? 2 : 1;
    s.C = std::max(s.C, s.S);
  }
  BlkuParams bp = blku_params(c, s);
  int r = blku_records(c, bp, true);
  if (r) return r;
  // the forward also stores the block propagators for the fused backward (which then forms none; its S = 1 only:
  // with prefix groups its chunks hold products); QOC_BLKU_STOREU=0 keeps the backward forming its own
  const bool fused = blku_fused_ok(c, order);
  const bool storeu = fused && blku_shape(c, true, true).S == 1 && !env_is("QOC_BLKU_STOREU", "0");
  const size_t ubytes = (size_t)c->B * c->Nt * c->blk_nb * c->blk_nb * c->nblk * sizeof(double2);
  if (storeu && c->d_blkU.bytes() < ubytes) {  // a new block layout (qoc_set_generators) may need more
    if (c->d_blkU) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_blkU.grow(ubytes));
  }
  bp.Uout = storeu ? c->d_blkU.as<double2>() : nullptr;
  const int mk = mark_begin(c, 1);
  const hipError_t e = blku_launch_fwd(c, s, bp);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blku_fwd launch: %s", hipGetErrorString(e));
  c->props_since_reset++;
  if (fused) {
    r = blku_bwdg(c, order, d_dJdu, storeu ? c->d_blkU.as<const double2>() : nullptr);
  } else {
    const int mb = mark_begin(c, 2);
    const hipError_t eb = blku_launch_bwd(c, tchain_args(c), s, bp, false);
    mark_end(c, mb);
    if (eb != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blku_bwd launch: %s", hipGetErrorString(eb));
    r = blku_grad(c, order, false, d_dJdu);
  }
  if (r) return r;
  if (!fused) c->bwd.route = 4;  // the block chains' eval, λ in HBM
  return QOC_OK;
}

}  // namespace qoc_host
