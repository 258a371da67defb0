// qoc_run_blkseg.hip — the segmented block eval (qoc_blkseg.hpp): its launch shape, its parameters and the launches of
// the fused eval and of its forward and backward halves.
#include <cstring>

#include "qoc_blkseg_host.hpp"

namespace qoc_host {

// One workgroup per seed with W waves (8 at one seed per CU, fewer when several seeds share a CU: 8 wave slots at the
// kernel's <= 256 VGPRs), UPW = 64 / nblk segments per wave, S = W UPW segments of L = ceil(Nt / S) slices (then S
// trimmed so that no segment is empty).  QOC_BLKSEG_W / QOC_BLKSEG_S override the waves / cap the segments.
// Derived once per context and again when one of its inputs changes (qoc_ctx::seg_key): every eval asks for it, some
// twice, and the B = 1 plumbing latency is host time.  With a generator ensemble set the launch has B E workgroups, which
// is what the waves-per-workgroup rule counts, and E is part of the key.  The sizes are compared here, not invalidated by their setters:
// m moves with the state packing and the blocks with every qoc_set_generators, and a missed setter would launch a
// stale shape.  The cache is the context's (mutable members: blkseg_ok, a predicate on a const context, fills it
// too); like the rest of a context it is for one host thread at a time.  The reference returned stays valid until
// the next call with other sizes.
// The state penalty in the form the segmented eval takes (BlksegParams::prow / pcol): whether the eval is a penalised
// one (μ != 0 with at least one row and one column; otherwise the unpenalised kernel computes the same J and dJdu).
// The masks are the context's, derived on first use after qoc_set_state_penalty or a new block layout dropped them.
static bool blkseg_pen(const qoc_ctx* c) {
  if (c->mu == 0.0) return false;
  if (!c->seg_pen_valid) {
    c->seg_prow[0] = c->seg_prow[1] = c->seg_prow[2] = 0;
    c->seg_pcol = 0;
    const int NB = c->blk_nb;
    if (NB >= 2 && NB <= 3 && c->nblk <= 32 && (int)c->h_brow.size() == c->nblk * NB)
      for (int r : c->h_pen_rows)
        for (int q = 0; q < c->nblk * NB; ++q)
          if (c->h_brow[q] == r) c->seg_prow[q % NB] |= 1u << (q / NB);
    for (int col : c->h_pen_cols)
      if (col >= 0 && col < 32) c->seg_pcol |= 1u << col;
    c->seg_pen_valid = true;
  }
  return (c->seg_prow[0] | c->seg_prow[1] | c->seg_prow[2]) != 0 && c->seg_pcol != 0;
}

static const BlksegShape& blkseg_shape(const qoc_ctx* c) {
  const bool pen = blkseg_pen(c);
  const int key[9] = {c->B, c->Nt, c->N, c->m, c->nu, c->blk_nb, c->nblk, pen ? 1 : 0, c->ens_E};
  if (std::equal(key, key + 9, c->seg_key)) return c->seg_shape;
  BlksegShape& s = c->seg_shape;
  s = BlksegShape{};
  const long long wgs = (long long)c->B * std::max(1, c->ens_E);
  const int per_cu = (int)std::max<long long>(1, std::min<long long>(8, (wgs + c->ncu - 1) / std::max(1, c->ncu)));
  // ensemble launches keep at least 4 waves: at 8 workgroups per CU (B E = 2048; cavity Nt = 1000 and zz Nt = 500, order 3
  // and exact) 4 waves measured 1.5-1.8 x the rule's single wave and 1.1-1.4 x two ("Ensemble evals"); the
  // plain eval's rule is untouched
  const int wdef = c->ens_E > 0 ? std::max(4, 8 / per_cu) : 8 / per_cu;
  s.W = std::max(1, std::min(8, env_int("QOC_BLKSEG_W", wdef)));
  s.UPW = 64 / std::max(1, c->nblk);
  int S = std::max(1, std::min(s.W * s.UPW, c->Nt));
  S = std::max(1, std::min(S, env_int("QOC_BLKSEG_S", S)));
  s.L = (c->Nt + S - 1) / S;
  s.S = (c->Nt + s.L - 1) / s.L;
  s.W = (s.S + s.UPW - 1) / s.UPW;
  s.RB = blkseg_rb(s.UPW, c->nu);
  // blocks of 2 rows: up to 8 slice-steps per reduction when the LDS holds them (cavity: 0.0727 -> 0.0715 ms per launch,
  // the same sums in the same order, profiles/bench_r06zl_*); QOC_BLKSEG_RB overrides (up to 64 / (UPW nu))
  const int rbmax = std::max(1, 64 / (s.UPW * std::max(1, c->nu)));
  if (c->blk_nb == 2) {
    const int rb8 = std::min(8, rbmax);
    if (blkseg_lds(c->N, c->m, c->nu, c->blk_nb, c->nblk, c->Nt, s.S, s.W, rb8, pen) <= BLKSEG_LDS_MAX) s.RB = rb8;
  }
  if (env_set("QOC_BLKSEG_RB")) s.RB = std::max(1, std::min(env_int("QOC_BLKSEG_RB", 0), rbmax));
  s.lds = blkseg_lds(c->N, c->m, c->nu, c->blk_nb, c->nblk, c->Nt, s.S, s.W, s.RB, pen);
  std::copy(key, key + 9, c->seg_key);
  return s;
}

// The segmented eval applies to block propagators of blocks of <= 3 rows with exactly skew-Hermitian generators
// (unitary slices), the built-in costs with or without the state penalty (the kernel's PEN instantiations;
// QOC_BLKSEG_PEN=0 leaves a penalised eval to the k_blku_* chains) and no co-state source (an arbitrary dL/dx needs
// x_k); QOC_BLKSEG=0 keeps the forward + fused backward of k_blku_*.  The exact (Fréchet) gradient is the kernel's
// ORD 0 instantiation (the whole series of the contraction); QOC_BLKSEG_EXACT=0 leaves an exact eval to the rebuilt
// x_k / λ_k and the dense Fréchet kernel (dense_gradient), the second implementation the tests compare against.
bool blkseg_ok(const qoc_ctx* c, int order) {
  if (!blku_on(c) || (c->blk_nb != 2 && c->blk_nb != 3) || !c->skew_exact || c->nblk > 32) return false;
  const bool exact = order == QOC_DUKDP_EXACT;
  if ((!exact && (order < 1 || order > BLK_ORDMAX)) || c->src_on) return false;
  if (exact && env_is("QOC_BLKSEG_EXACT", "0")) return false;
  if (c->cost_kind != QOC_COST_TRACE && c->cost_kind != QOC_COST_ZCAL) return false;
  if (env_is("QOC_BLKSEG", "0")) return false;
  if (c->mu != 0.0 && (env_is("QOC_BLKSEG_PEN", "0") || c->m > 32)) return false;  // (the column mask has 32 bits)
  return blkseg_shape(c).lds <= BLKSEG_LDS_MAX;
}

static int ensure_lazy_bufs(qoc_ctx* c) {
  const size_t nu_t = (size_t)c->B * c->nu * c->Nt, ncf = (size_t)c->B * 2 * c->m_user;
  if (!c->d_u_lam) {
    HIPCHK(c, c->d_coef_lam.alloc(ncf * sizeof(cx<double>)));
    HIPCHK(c, c->d_u_lam.alloc(nu_t * sizeof(double)));
  }
  return QOC_OK;
}

// the launch parameters every mode shares; the best-(J, seed) epilogue's buffers on first use
static int blkseg_params(qoc_ctx* c, const BlksegShape& s, BlksegParams& sp) {
  sp = BlksegParams{};
  for (int j = 0; j < 3; ++j) {
    const bool on = j <= c->nu;
    sp.rad[j] = on ? c->tprm.rad[j] : 0.0;  // skew-Hermitian: spectral half-widths of the shifted generators
    sp.mur[j] = on ? c->tprm.mur[j] : 0.0;
    sp.mui[j] = on ? c->tprm.mui[j] : 0.0;
  }
  sp.theta_cap = c->tprm.theta[17];
  sp.S = s.S;
  sp.L = s.L;
  sp.UPW = s.UPW;
  sp.RB = s.RB;
  sp.gtab = c->d_gtab;
  sp.terms = c->d_terms;
  if (blkseg_pen(c)) {  // (else zeros: the unpenalised kernel reads none of them)
    sp.pen_mu = c->mu;
    for (int i = 0; i < 3; ++i) sp.prow[i] = c->seg_prow[i];
    sp.pcol = c->seg_pcol;
  }
  // the best (J, seed) for qoc_allgather_best_dev, found by the launch's last workgroup
  if (!c->d_best) {  // no communicator yet: this context alone (the epilogue's own layout)
    HIPCHK(c, c->d_best.alloc(6 * sizeof(double)));
    c->world = 1;
    c->rank = 0;
  }
  if (!c->d_done) {
    HIPCHK(c, c->d_done.alloc(sizeof(unsigned int)));
    HIPCHK(c, hipMemsetAsync(c->d_done, 0, sizeof(unsigned int), c->stream));
  }
  sp.done = c->d_done;
  sp.best = c->d_best + 2 + 2 * c->rank;
  sp.seed_offset = c->seed_offset;
  // one rank: the pick after the (identity) exchange is done here, when a buffer is registered
  const bool direct = c->world == 1 && c->best_out;
  sp.best_res = direct ? c->d_best + 2 + 2 * c->world : nullptr;
  sp.best_out = direct ? c->best_out : nullptr;
  c->jbest.direct = direct;
  return QOC_OK;
}

// blk_lds_attr for the segmented eval's kernels without a runtime call per launch: a context sets a kernel's limit
// once (seg_attr), to the most the eval ever asks for (BLKSEG_LDS_MAX less the kernel's static LDS) and not to its own
// size, because the limit belongs to the kernel, not to the context: another context with a smaller shape must not
// lower it
static hipError_t blkseg_lds_attr(qoc_ctx* c, int nb, int ord, int mode, bool pen, const void* kern, size_t lds) {
  bool& set = c->seg_attr[nb - 2][ord == 0 ? BLK_ORDMAX : ord - 1][mode][pen ? 1 : 0];  // (ORD 0: the exact slot)
  if (lds <= 65536 || set) return hipSuccess;
  hipFuncAttributes fa{};
  hipError_t e = hipFuncGetAttributes(&fa, kern);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BLKSEG_LDS_MAX - fa.sharedSizeBytes));
  set = e == hipSuccess;
  return e;
}

// the ensemble launch: B E workgroups of the fused kernel's ENS instantiation, J and the coefficients into the
// ensemble's workspace (sp.dJdu is the caller's to point there)
static hipError_t blkseg_launch_ens(qoc_ctx* c, int order, const BlksegShape& s, const BlksegParams& sp) {
  TChainArgs g = tchain_args(c);
  g.J = c->d_ens_J;
  g.coef = c->d_ens_coef;
  const BlkArgs bk = blk_args(c);
  return blkseg_dispatch(c->blk_nb, order, [&](auto NB_, auto ORD_) {
    constexpr int NB = decltype(NB_)::value, ORD = decltype(ORD_)::value;
    auto launch = [&](auto PEN_) {
      constexpr bool PEN = decltype(PEN_)::value;
      if constexpr (PEN && NB == 3) {  // (the two-launch form: blkseg_ens_ok declines)
        return hipErrorInvalidValue;
      } else {
        auto kern = k_blkseg_eval<NB, ORD, 8, BLKSEG_FUSED, PEN, true>;
        bool& set = c->seg_attr_ens[NB - 2][ORD == 0 ? BLK_ORDMAX : ORD - 1][PEN ? 1 : 0];
        if (s.lds > 65536 && !set) {
          hipFuncAttributes fa{};
          hipError_t e = hipFuncGetAttributes(&fa, (const void*)kern);
          if (e != hipSuccess) return e;
          e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(BLKSEG_LDS_MAX - fa.sharedSizeBytes));
          if (e != hipSuccess) return e;
          set = true;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)(c->B * c->ens_E)), dim3(64 * s.W), s.lds, c->stream, g, bk, sp);
        return hipGetLastError();
      }
    };
    if (sp.pen_mu != 0.0) return launch(std::true_type());
    return launch(std::false_type());
  });
}

template <int MODE>
static hipError_t blkseg_launch(qoc_ctx* c, int order, const BlksegShape& s, const BlksegParams& sp) {
  const TChainArgs g = tchain_args(c);
  const BlkArgs bk = blk_args(c);
  return blkseg_dispatch(c->blk_nb, MODE == BLKSEG_FWD ? 1 : order, [&](auto NB_, auto ORD_) {
    constexpr int NB = decltype(NB_)::value, ORD = decltype(ORD_)::value;
    // the forward half has no gradient: one instantiation (ORD 1) serves every order
    if constexpr (MODE == BLKSEG_FWD && ORD != 1) {
      return hipErrorInvalidValue;
    } else {
      auto launch = [&](auto PEN_) {
        constexpr bool PEN = decltype(PEN_)::value;
        // blocks of 3 rows: the penalised eval runs as the forward and the backward half (blkseg_eval), so the fused
        // penalised kernel, which does not fit its registers there, is never built
        if constexpr (PEN && NB == 3 && MODE == BLKSEG_FUSED) {
          return hipErrorInvalidValue;
        } else {
          auto kern = k_blkseg_eval<NB, ORD, 8, MODE, PEN>;
          const hipError_t q = blkseg_lds_attr(c, NB, ORD, MODE, PEN, (const void*)kern, s.lds);
          if (q != hipSuccess) return q;
          hipLaunchKernelGGL(kern, dim3(c->B), dim3(64 * s.W), s.lds, c->stream, g, bk, sp);
          return hipGetLastError();
        }
      };
      // the penalised instantiation when the launch carries a penalty (blkseg_params)
      if (sp.pen_mu != 0.0) return launch(std::true_type());
      return launch(std::false_type());
    }
  });
}

int blkseg_eval(qoc_ctx* c, int order, const double* d_u, double* d_J, double* d_dJdu) {
  if (blkseg_pen(c) && c->blk_nb == 3) {
    // Blocks of 3 rows with the penalty: the two halves as two launches (G and D at the segment ends through HBM).
    // In one kernel the penalised phases 1-2 and phase 3 together spill (416 bytes per lane at order 3), and the two
    // launches measured faster than that kernel (zz, B = 512: 4.4M against 4.0M evals/s); J and dJdu are bitwise the
    // same, and each half is within its registers.  The eval leaves no split forward behind.
    int r = blkseg_forward(c, d_u, d_J);
    if (r) return r;
    c->fwd.kind = 0;
    c->props_since_reset--;  // (counted by the caller)
    return blkseg_backward(c, order, d_dJdu, nullptr);
  }
  const BlksegShape s = blkseg_shape(c);
  int r = ensure_lazy_bufs(c);
  if (r) return r;
  BlksegParams sp;
  if ((r = blkseg_params(c, s, sp))) return r;
  sp.u = d_u;
  sp.u_copy = d_u != c->d_u ? c->d_u : nullptr;
  sp.u_copy2 = c->d_u_lam;  // the co-states' rebuild (blku_costates) reads this copy and d_coef_lam
  sp.J2 = d_J && d_J != c->d_J ? d_J : nullptr;
  sp.coef2 = c->d_coef_lam;
  sp.dJdu = d_dJdu;
  const int mk = mark_begin(c, 2);
  const hipError_t e = blkseg_launch<BLKSEG_FUSED>(c, order, s, sp);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blkseg_eval launch: %s", hipGetErrorString(e));
  c->fwd.lazy = true;
  c->bwd.lazy = true;
  c->bwd.route = 6;
  c->jbest.ready = true;
  return QOC_OK;
}

bool blkseg_ens_ok(const qoc_ctx* c, int order) {
  if (c->ens_E < 1 || !blkseg_ok(c, order)) return false;
  return !(blkseg_pen(c) && c->blk_nb == 3);  // (G and D per seed through HBM: not part of the ensemble eval)
}

// When a MAX or CVaR eval takes route 2 (the forward half for every (pulse, member), the backward half where ω is not
// 0) instead of the fused launch, from the sweeps of tools/bench_ensemble_risk.py on an MI355X ("Ensemble
// evals"): at most ENS_SKIP_TAU of the members can carry weight, and the launch has at least ENS_SKIP_WG_PER_CU
// workgroups per compute unit.  With fewer the skipped workgroups free compute units that have nothing else to do,
// and the second launch and the round trip of G through HBM cost 3-12 %; at E = 8 one active member of 8 wins every
// repeat from 4 workgroups per CU on (1.05-1.44 x), two of 8 lose on the cavity at 4 per CU.  QOC_ENS_SKIP=0|1
// forces a route.
constexpr double ENS_SKIP_TAU = 0.125;
constexpr long long ENS_SKIP_WG_PER_CU = 4;

EnsPlan blkseg_ens_plan(qoc_ctx* c, int E, const double* w, int kind, double param) {
  EnsPlan pl;
  if (E < 1 || kind == QOC_ENS_MEAN) return pl;
  pl.om_bytes = (size_t)c->B * E * sizeof(double);
  if (kind == QOC_ENS_MAX || kind == QOC_ENS_CVAR) {
    // n_act: the most members that can carry weight whatever the costs: 1 + the largest k for which the k smallest
    // positive weights sum to less than α W (the worst case puts the lightest members first)
    int n_act = 1;
    if (kind == QOC_ENS_CVAR) {
      double W = 0.0;
      std::vector<double> pos;
      for (int e = 0; e < E; ++e) {
        W += w[e];
        if (w[e] > 0.0) pos.push_back(w[e]);
      }
      std::sort(pos.begin(), pos.end());
      const double aW = param * W;
      double acc = 0.0;
      int k = 0;
      for (double x : pos) {
        acc += x;
        if (!(acc < aW)) break;
        ++k;
      }
      n_act = std::min(1 + k, (int)pos.size());
    }
    const bool filled = (long long)c->B * E >= ENS_SKIP_WG_PER_CU * std::max(1, c->ncu);
    pl.route = filled && (double)n_act / E <= ENS_SKIP_TAU ? 2 : 1;
    if (env_is("QOC_ENS_SKIP", "0")) pl.route = 1;
    if (env_is("QOC_ENS_SKIP", "1")) pl.route = 2;
  }
  if (pl.route == 2) {  // G at every segment's end per (pulse, member), and D behind it when the eval is penalised
    const int E_ctx = c->ens_E;
    c->ens_E = E;  // (the launch shape counts B E workgroups)
    const BlksegShape s = blkseg_shape(c);
    c->ens_E = E_ctx;
    pl.gseg_bytes = (blkseg_pen(c) ? 2 : 1) * (size_t)c->B * E * s.S * c->nblk * c->blk_nb * c->blk_nb * sizeof(double2);
  }
  return pl;
}

// One eval of every pulse over the ensemble.  Under the mean: the fused kernel on B E (pulse, member) workgroups writes
// the members' J, coefficients and dJdu into the ensemble's workspace (and u into d_u, by member 0's workgroups, when
// the caller's buffer is another one), then k_ens_reduce forms the weighted sums in d_J (and the caller's J) and
// d_dJdu.  Under another objective (qoc_set_ensemble_objective) k_ens_weights forms the per-pulse member weights ω and
// J̄ from the member costs and k_ens_reduce_w the ω-weighted gradient; route 1 has the fused launch in front of them,
// route 2 the forward half for every workgroup, k_ens_weights, then the backward half, which returns at once where
// ω is 0.  Nothing lazy is kept and the best-pair epilogue is off: k_argmin_seed picks from d_J.
int blkseg_eval_ens(qoc_ctx* c, int order, const double* d_u, double* d_J, double* d_dJdu) {
  const BlksegShape s = blkseg_shape(c);
  BlksegParams sp;
  int r = blkseg_params(c, s, sp);
  if (r) return r;
  const int kind = c->ens_obj;
  const int route = kind == QOC_ENS_MEAN ? 1 : c->ens_route;
  const size_t gcount = (size_t)c->B * c->ens_E * s.S * c->nblk * c->blk_nb * c->blk_nb;
  if (kind != QOC_ENS_MEAN && !c->d_ens_om)
    return fail(c, QOC_ERR_STATE, "the ensemble objective's workspace is missing");
  if (route == 2) {
    // (the setters sized G for the shape and the penalty of their time; a penalty set since may need D behind it)
    const size_t gbytes = (blkseg_pen(c) ? 2 : 1) * gcount * sizeof(double2);
    if (c->d_ens_gseg.bytes() < gbytes) {  // (the new one first: a failure leaves the old one in place)
      DevBuf<double2> q;
      HIPCHK(c, q.alloc(gbytes));
      if (c->d_ens_gseg) HIPCHK(c, hipStreamSynchronize(c->stream));
      c->d_ens_gseg.adopt(std::move(q));
    }
  }
  sp.u = d_u;
  sp.u_copy = d_u != c->d_u ? c->d_u : nullptr;
  sp.dJdu = c->d_ens_g;
  sp.done = nullptr;
  sp.best = sp.best_res = sp.best_out = nullptr;
  sp.gtab = c->d_ens_gtab;
  sp.E = c->ens_E;
  sp.ens = c->d_ens_prm;
  c->jbest.direct = false;
  const int mk = mark_begin(c, 2);
  hipError_t e;
  if (route == 2) {
    sp.gseg = c->d_ens_gseg;
    sp.dseg = c->d_ens_gseg + gcount;
    e = blkseg_launch_ens_half(c, BLKSEG_FWD, 1, s, sp);
    if (e == hipSuccess) e = ens_weights_launch(c, d_J);
    if (e == hipSuccess) {
      sp.u_copy = nullptr;  // (written by the forward half)
      sp.omega = c->d_ens_om;
      e = blkseg_launch_ens_half(c, BLKSEG_BWD, order, s, sp);
    }
    if (e == hipSuccess) e = ens_reduce_w_launch(c, d_dJdu);
  } else {
    e = blkseg_launch_ens(c, order, s, sp);
    if (e == hipSuccess && kind != QOC_ENS_MEAN) {
      e = ens_weights_launch(c, d_J);
      if (e == hipSuccess) e = ens_reduce_w_launch(c, d_dJdu);
    } else if (e == hipSuccess) {
      const int n = c->Nt * c->nu;
      const bool vec = c->nu == 2 && (reinterpret_cast<size_t>(d_dJdu) & 15) == 0;
      const long long thr = std::max<long long>((long long)c->B * (vec ? n / 2 : n), c->B);
      const unsigned grid = (unsigned)((thr + 255) / 256);
      double* const J2 = d_J && d_J != c->d_J ? d_J : nullptr;
      if (vec)
        hipLaunchKernelGGL(k_ens_reduce<true>, dim3(grid), dim3(256), 0, c->stream, c->B, c->ens_E, n, c->d_ens_w,
                           c->d_ens_g, c->d_ens_J, d_dJdu, c->d_J, J2);
      else
        hipLaunchKernelGGL(k_ens_reduce<false>, dim3(grid), dim3(256), 0, c->stream, c->B, c->ens_E, n, c->d_ens_w,
                           c->d_ens_g, c->d_ens_J, d_dJdu, c->d_J, J2);
      e = hipGetLastError();
    }
  }
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blkseg_eval (ensemble) launch: %s", hipGetErrorString(e));
  c->ens_costs = true;
  c->ens_last_route = route;
  return QOC_OK;
}

bool blkseg_ts_ok(const qoc_ctx* c, int order) { return c->ts_on && c->ens_E == 0 && blkseg_ok(c, order); }

// G (and D behind it when the eval is penalised) at every segment's end: the buffer the forward half writes
static int blkseg_gseg_buf(qoc_ctx* c, const BlksegShape& s, size_t& gcount) {
  gcount = (size_t)c->B * s.S * c->nblk * c->blk_nb * c->blk_nb;
  const size_t gbytes = (blkseg_pen(c) ? 2 : 1) * gcount * sizeof(double2);
  if (c->d_gseg.bytes() < gbytes) {  // a new block layout (qoc_set_generators) or a penalty may need more
    if (c->d_gseg) HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->d_gseg.grow(gbytes));
  }
  return QOC_OK;
}

// One eval under a per-seed time scale (qoc_set_time_scale): the TS instantiations read τ_b from d_ts and write J,
// dJdu at fixed τ and dJ/dτ (d_ts + B); one fused launch, or the two halves for penalised blocks of 3 rows (as
// blkseg_eval).  u goes into d_u when the caller's buffer is another one.  Nothing lazy is kept (the k_blku_* rebuild
// chains know nothing of τ), the last backward's record stands, and the launch's own epilogue leaves the best
// (J, seed).
int blkseg_eval_ts(qoc_ctx* c, int order, const double* d_u, double* d_J, double* d_dJdu) {
  const BlksegShape s = blkseg_shape(c);
  const bool halves = blkseg_pen(c) && c->blk_nb == 3;
  size_t gcount = 0;
  int r;
  if (halves && (r = blkseg_gseg_buf(c, s, gcount))) return r;
  BlksegParams sp;
  if ((r = blkseg_params(c, s, sp))) return r;
  sp.u = d_u;
  sp.u_copy = d_u != c->d_u ? c->d_u : nullptr;
  sp.J2 = d_J && d_J != c->d_J ? d_J : nullptr;
  sp.dJdu = d_dJdu;
  sp.tau = c->d_ts;
  sp.dJdtau = c->d_ts + c->B;
  const int mk = mark_begin(c, 2);
  hipError_t e;
  if (halves) {
    sp.gseg = c->d_gseg;
    sp.dseg = c->d_gseg + gcount;
    e = blkseg_launch_ts(c, BLKSEG_FWD, 1, s, sp);
    if (e == hipSuccess) {
      sp.u_copy = nullptr;  // (written by the forward half)
      sp.J2 = nullptr;
      e = blkseg_launch_ts(c, BLKSEG_BWD, order, s, sp);
    }
  } else {
    e = blkseg_launch_ts(c, BLKSEG_FUSED, order, s, sp);
  }
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blkseg_eval (time scale) launch: %s", hipGetErrorString(e));
  c->jbest.ready = true;
  c->ts_grad = true;
  return QOC_OK;
}

// propagate on the segmented eval (the reference's f, examples/ipopt_callbacks_exp.jl:11-19): J, the λ_N coefficients
// and G at every segment's end, x_k rebuilt on demand.  Applies where the fused eval does (any order: the forward half
// has none) unless QOC_BLKSEG_SPLIT=0.
bool blkseg_split_ok(const qoc_ctx* c) {
  return !env_is("QOC_BLKSEG_SPLIT", "0") && blkseg_ok(c, 3);
}

int blkseg_forward(qoc_ctx* c, const double* d_u, double* d_J) {
  const BlksegShape s = blkseg_shape(c);
  int r = ensure_lazy_bufs(c);
  if (r) return r;
  size_t gcount = 0;
  if ((r = blkseg_gseg_buf(c, s, gcount))) return r;
  BlksegParams sp;
  if ((r = blkseg_params(c, s, sp))) return r;
  sp.u = d_u;
  sp.u_copy = d_u != c->d_u ? c->d_u : nullptr;  // the backward half and the stale check read d_u
  sp.J2 = d_J && d_J != c->d_J ? d_J : nullptr;
  sp.gseg = c->d_gseg;  // (the co-states' rebuild source stays the last grape_sensitivity's: the backward writes it)
  sp.dseg = c->d_gseg + gcount;
  const int mk = mark_begin(c, 1);
  const hipError_t e = blkseg_launch<BLKSEG_FWD>(c, 1, s, sp);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blkseg_eval (forward) launch: %s", hipGetErrorString(e));
  c->fwd.lazy = true;
  c->fwd.kind = 1;
  c->jbest.ready = true;
  c->props_since_reset++;
  return QOC_OK;
}

// grape_sensitivity after blkseg_forward (the reference's f_grad, :21-31): phase 3 from the stored G; the co-states are
// rebuilt on demand from the forward's copies of u and the λ_N coefficients
int blkseg_backward(qoc_ctx* c, int order, double* d_dJdu, const int* stale) {
  const BlksegShape s = blkseg_shape(c);
  BlksegParams sp;
  int r = blkseg_params(c, s, sp);
  if (r) return r;
  if ((r = ensure_lazy_bufs(c))) return r;
  sp.u = c->d_u;
  sp.u_copy2 = c->d_u_lam;  // λ_k rebuilt on demand from this u and the forward's λ_N coefficients
  sp.coef2 = c->d_coef_lam;
  sp.dJdu = d_dJdu;
  sp.gseg = c->d_gseg;
  sp.dseg = c->d_gseg + (size_t)c->B * s.S * c->nblk * c->blk_nb * c->blk_nb;
  sp.stale = stale;
  const int mk = mark_begin(c, 2);
  const hipError_t e = blkseg_launch<BLKSEG_BWD>(c, order, s, sp);
  mark_end(c, mk);
  if (e != hipSuccess) return fail(c, QOC_ERR_HIP, "k_blkseg_eval (backward) launch: %s", hipGetErrorString(e));
  c->bwd = {};  // (backward() resets after the split paths: they state the whole record)
  c->bwd.lazy = true;
  c->bwd.route = 6;
  return QOC_OK;
}

}  // namespace qoc_host
