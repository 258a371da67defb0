// qoc_opt.hpp — device-resident multi-start optimiser: one projected L-BFGS / augmented-Lagrangian state machine per
// seed (the per-seed form of qoc_amd/optimize.py minimize_batched, the stand-in for the Ipopt
// multi-start of examples/zz_coupling_ipopt_exp.jl:56-80).
//
// A tick: the caller evaluates all B trial points in one batch, then every seed consumes its own (f, grad) and does
// exactly one of: accept the trial (update its pairs, new direction, new trial), reject it (halve the step), or end
// an augmented-Lagrangian round.  No seed waits for another and no decision is taken on the host.
//
// One wave per seed; lane l holds variables l, l + 64, l + 128, l + 192 (n <= 256).  Every dot product, norm and max is
// a per-lane partial in that fixed order followed by a fixed xor butterfly, so a seed's iterates depend on nothing but
// its own data: not on B, its position in the batch or the workgroup it lands in.  All state is fp64.  Floating-point
// contraction is off inside these functions and the FMAs are spelled out, so the fused step and the ask/tell step run
// the same arithmetic.
#pragma once
#include "qoc_common.hpp"

namespace qoc {

constexpr int OPT_MAX_N = 256;   // variables per seed
constexpr int OPT_MAX_MEM = 16;  // L-BFGS pairs
constexpr int OPT_R = OPT_MAX_N / WAVE;
constexpr int OPT_INIT = 0, OPT_LS = 1, OPT_DONE = 2;
// per-seed records: doubles (merit at x, step, last violation, 1 / s'y and s'y / y'y per pair) and ints
enum { OD_PHI = 0, OD_ALPHA = 1, OD_PREV_VIOL = 2, OD_RINV = 4, OD_GAM = 4 + OPT_MAX_MEM, OD_STRIDE = 4 + 2 * OPT_MAX_MEM };
enum { OI_PHASE = 0, OI_LS = 1, OI_HEAD = 2, OI_IT = 3, OI_VALID = 4, OI_STRIDE = 8 };

struct OptParams {
  int n, ns, nu, max_iter, memory, outer_iters, max_ls;
  double lower, upper, gu0, gu1, rho0, gtol;
};

// the duration form (qoc_opt_create_duration): the last variable is a gate duration τ with bounds of its own; kappa is
// the weight of τ in f = J + kappa τ, used by the fused step only
struct OptDur {
  double tau_lo, tau_hi, kappa;
};

struct OptState {
  double *x, *gx, *d, *xt;  // B x n: iterate, merit gradient there, direction, trial
  double *S, *Y;            // B x memory x n
  double* rec;              // B x OD_STRIDE
  double *f, *g, *lam, *rho;  // B, B x 2, B x 2, B: objective and constraints at x, multipliers, penalty
  int* irec;                  // B x OI_STRIDE
  int *evals, *iters, *rounds, *converged, *done, *fails;  // B each
  int* ndone;                                              // seeds that are DONE
  int* host_done;                                          // its host-mapped mirror
};

__device__ __forceinline__ double opt_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double opt_wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}
// sum_i a_i b_i over the wave's variables: FMA chain over the lane's own, then the butterfly
__device__ __forceinline__ double opt_dot(const double (&a)[OPT_R], const double (&b)[OPT_R]) {
  double p = 0.0;
#pragma unroll
  for (int r = 0; r < OPT_R; ++r) p = fma(a[r], b[r], p);
  return opt_wave_sum(p);
}
__device__ __forceinline__ double opt_clamp(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// the finished-seed count, mirrored to the host word as the stale-u flag is (k_compare_u_flags): the value is the one
// before this launch's own seeds finish, so the host sees the count with a lag of one tick
__device__ __forceinline__ void opt_mirror_done(const OptState& st) {
  const int v = __hip_atomic_load(st.ndone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(st.host_done, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One tick of seed b, run by one full wave.  f_in, grad[0..n): the objective and its gradient at the seed's trial
// st.xt; the next trial is written to st.xt (and to xt_out when given, e.g. LDS).  A DONE seed returns at once.
// DUR: variable n - 1 is the duration: clamped to [D.tau_lo, D.tau_hi] instead of the scalar bounds and left out of
// the two spline norms and their Jacobians (n - 1 = ns nu would read as s = 0, j = nu); everything else runs over all n.
template <bool DUR = false>
__device__ __forceinline__ void opt_tell(const OptParams& P, const OptState& st, int b, int lane, double f_in,
                                         const double* grad, double* xt_out, const OptDur D = OptDur{}) {
#pragma clang fp contract(off)
  const int n = P.n, m = P.memory;
  const int nc = DUR ? n - 1 : n;  // variables the spline norms run over
  // bounds of the variable in register row r of this lane
  auto lo_of = [&](int r) -> double {
    if constexpr (DUR) return lane + WAVE * r == nc ? D.tau_lo : P.lower;
    return P.lower;
  };
  auto hi_of = [&](int r) -> double {
    if constexpr (DUR) return lane + WAVE * r == nc ? D.tau_hi : P.upper;
    return P.upper;
  };
  int* ir = st.irec + (size_t)b * OI_STRIDE;
  double* dr = st.rec + (size_t)b * OD_STRIDE;
  const int phase = ir[OI_PHASE];
  if (phase == OPT_DONE) return;
  double* xb = st.x + (size_t)b * n;
  double* gxb = st.gx + (size_t)b * n;
  double* db = st.d + (size_t)b * n;
  double* xtb = st.xt + (size_t)b * n;
  double* Sb = st.S + (size_t)b * m * n;
  double* Yb = st.Y + (size_t)b * m * n;
  const bool cons = P.ns > 0;

  // everything the tick may read, loaded up front: the loads overlap instead of queueing behind the decisions
  double xt[OPT_R], gp[OPT_R], x[OPT_R], gx[OPT_R], dv[OPT_R];
#pragma unroll
  for (int r = 0; r < OPT_R; ++r) {
    const int i = lane + WAVE * r;
    xt[r] = i < n ? xtb[i] : 0.0;
    gp[r] = i < n ? grad[i] : 0.0;
    x[r] = i < n ? xb[i] : 0.0;
    gx[r] = i < n ? gxb[i] : 0.0;
    dv[r] = i < n ? db[i] : 0.0;
  }
  int ls = ir[OI_LS], head = ir[OI_HEAD], it = ir[OI_IT];
  unsigned valid = (unsigned)ir[OI_VALID];
  double alpha = dr[OD_ALPHA];
  const double phi_x = dr[OD_PHI];
  // merit phi = f + sum(a^2 - lam^2) / (2 rho), a = max(lam + rho (g - g_U), 0), and its gradient; the constraints
  // and their Jacobian as in k_spline_constraints (a zero norm has a zero gradient)
  double phi = f_in, g0 = 0.0, g1 = 0.0;
  const double lam0 = cons ? st.lam[2 * b] : 0.0, lam1 = cons ? st.lam[2 * b + 1] : 0.0, rho = cons ? st.rho[b] : 0.0;
  if (cons) {
    const int ns = P.ns;
    double dl[OPT_R], dq[OPT_R], xc[OPT_R];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int r = 0; r < OPT_R; ++r) {
      const int i = lane + WAVE * r;
      const int s = i % ns;
      if constexpr (DUR) xc[r] = i < nc ? xt[r] : 0.0;
      else xc[r] = xt[r];
      dl[r] = (i < nc && s > 0) ? xt[r] - xtb[i - 1] : 0.0;
      dq[r] = (i < nc && s + 1 < ns) ? xtb[i + 1] - xt[r] : 0.0;
      s0 = fma(xc[r], xc[r], s0);
      s1 = fma(dl[r], dl[r], s1);
    }
    g0 = sqrt(opt_wave_sum(s0));
    g1 = sqrt(opt_wave_sum(s1));
    const double a0 = fmax(lam0 + rho * (g0 - P.gu0), 0.0);
    const double a1 = fmax(lam1 + rho * (g1 - P.gu1), 0.0);
    phi = f_in + ((a0 * a0 - lam0 * lam0) + (a1 * a1 - lam1 * lam1)) / (2.0 * rho);
#pragma unroll
    for (int r = 0; r < OPT_R; ++r) {
      const double j0 = g0 > 0.0 ? xc[r] / g0 : 0.0;
      const double j1 = g1 > 0.0 ? (dl[r] - dq[r]) / g1 : 0.0;
      gp[r] = gp[r] + (a0 * j0 + a1 * j1);
    }
  }

  double gv0 = g0, gv1 = g1;  // constraint values at x
  bool newdir = false, took = false;
  // the pair stored in this tick: its scalars are used from registers (lane 0's stores are for the next tick)
  int new_slot = -1;
  double new_rinv = 0.0, new_gam = 1.0;
  if (lane == 0) st.evals[b] += 1;

  if (phase == OPT_INIT) {  // first eval of a round, at xt = x: a fresh history
#pragma unroll
    for (int r = 0; r < OPT_R; ++r) {
      x[r] = xt[r];
      gx[r] = gp[r];
    }
    valid = 0;
    head = 0;
    it = 0;
    newdir = took = true;
  } else {
    double s[OPT_R];
#pragma unroll
    for (int r = 0; r < OPT_R; ++r) s[r] = xt[r] - x[r];
    const bool ok = (phi <= phi_x + 1e-4 * opt_dot(gx, s)) && isfinite(phi);
    if (ok) {  // Armijo: accept, update the pairs
      double y[OPT_R];
#pragma unroll
      for (int r = 0; r < OPT_R; ++r) y[r] = gp[r] - gx[r];
      const double sy = opt_dot(s, y), ss = opt_dot(s, s), yy = opt_dot(y, y);
      const bool upd = sy > 1e-12 * sqrt(ss) * sqrt(yy);
      if (upd) {
#pragma unroll
        for (int r = 0; r < OPT_R; ++r) {
          const int i = lane + WAVE * r;
          if (i < n) {
            Sb[(size_t)head * n + i] = s[r];
            Yb[(size_t)head * n + i] = y[r];
          }
        }
        new_slot = head;
        new_rinv = 1.0 / sy;
        new_gam = yy > 0.0 ? sy / yy : 1.0;
        if (lane == 0) {
          dr[OD_RINV + head] = new_rinv;
          dr[OD_GAM + head] = new_gam;
        }
        valid |= 1u << head;
      } else {
        valid &= ~(1u << head);
      }
      head = head + 1 == m ? 0 : head + 1;
#pragma unroll
      for (int r = 0; r < OPT_R; ++r) {
        x[r] = xt[r];
        gx[r] = gp[r];
      }
      it += 1;
      if (lane == 0) st.iters[b] += 1;
      newdir = took = true;
    } else {
      ls += 1;
      if (ls == P.max_ls) {  // the line search failed: restart from steepest descent at x
        head = head + 1 == m ? 0 : head + 1;
        valid = 0;
        it += 1;
        if (lane == 0) st.fails[b] += 1;
        if (cons) {
          gv0 = st.g[2 * b];
          gv1 = st.g[2 * b + 1];
        }
        newdir = true;
      } else {
        alpha = alpha * 0.5;
#pragma unroll
        for (int r = 0; r < OPT_R; ++r) xt[r] = opt_clamp(x[r] + alpha * dv[r], lo_of(r), hi_of(r));
      }
    }
  }
  // x changed (INIT or accepted): its merit, gradient, objective and constraints
  if (took) {
#pragma unroll
    for (int r = 0; r < OPT_R; ++r) {
      const int i = lane + WAVE * r;
      if (i < n) {
        xb[i] = x[r];
        gxb[i] = gx[r];
      }
    }
    if (lane == 0) {
      dr[OD_PHI] = phi;
      st.f[b] = f_in;
      st.g[2 * b] = g0;
      st.g[2 * b + 1] = g1;
    }
  }

  int next = OPT_LS;
  if (newdir) {
    bool end_round = it == P.max_iter;
    double q[OPT_R];
    bool fr[OPT_R];
    double pgn = 0.0;
    if (!end_round) {
#pragma unroll
      for (int r = 0; r < OPT_R; ++r) {
        fr[r] = !((x[r] <= lo_of(r) && gx[r] > 0.0) || (x[r] >= hi_of(r) && gx[r] < 0.0));
        q[r] = fr[r] ? gx[r] : 0.0;
        pgn = fmax(pgn, fabs(q[r]));
      }
      pgn = opt_wave_max(pgn);
      const bool conv = pgn <= P.gtol;
      if (lane == 0) st.converged[b] = conv ? 1 : 0;
      end_round = conv;
    }
    if (!end_round) {
      // two-loop recursion on q, newest pair first
      double al[OPT_MAX_MEM];
      double w[OPT_R];
#pragma unroll
      for (int r = 0; r < OPT_R; ++r) w[r] = q[r];
#pragma unroll
      for (int i = 0; i < OPT_MAX_MEM; ++i) {
        al[i] = 0.0;
        if (i < m) {
          int slot = head - 1 - i;
          if (slot < 0) slot += m;
          if ((valid >> slot) & 1u) {
            double sv[OPT_R], yv[OPT_R];
#pragma unroll
            for (int r = 0; r < OPT_R; ++r) {
              const int k = lane + WAVE * r;
              sv[r] = k < n ? Sb[(size_t)slot * n + k] : 0.0;
              yv[r] = k < n ? Yb[(size_t)slot * n + k] : 0.0;
            }
            const double a = (slot == new_slot ? new_rinv : dr[OD_RINV + slot]) * opt_dot(sv, w);
            al[i] = a;
#pragma unroll
            for (int r = 0; r < OPT_R; ++r) w[r] = w[r] - a * yv[r];
          }
        }
      }
      const int newest = head == 0 ? m - 1 : head - 1;
      const double gamma = ((valid >> newest) & 1u) ? (newest == new_slot ? new_gam : dr[OD_GAM + newest]) : 1.0;
#pragma unroll
      for (int r = 0; r < OPT_R; ++r) w[r] = gamma * w[r];
#pragma unroll
      for (int i = OPT_MAX_MEM - 1; i >= 0; --i) {
        if (i < m) {
          int slot = head - 1 - i;
          if (slot < 0) slot += m;
          if ((valid >> slot) & 1u) {
            double sv[OPT_R], yv[OPT_R];
#pragma unroll
            for (int r = 0; r < OPT_R; ++r) {
              const int k = lane + WAVE * r;
              sv[r] = k < n ? Sb[(size_t)slot * n + k] : 0.0;
              yv[r] = k < n ? Yb[(size_t)slot * n + k] : 0.0;
            }
            const double bb = (slot == new_slot ? new_rinv : dr[OD_RINV + slot]) * opt_dot(yv, w);
            const double cf = al[i] - bb;
#pragma unroll
            for (int r = 0; r < OPT_R; ++r) w[r] = w[r] + cf * sv[r];
          }
        }
      }
      double d[OPT_R];
#pragma unroll
      for (int r = 0; r < OPT_R; ++r) d[r] = fr[r] ? -w[r] : 0.0;
      const double desc = opt_dot(d, gx);
      if (!(desc < 0.0)) {  // not a descent direction: steepest descent, forget the pairs
#pragma unroll
        for (int r = 0; r < OPT_R; ++r) d[r] = -q[r];
        valid = 0;
      }
      alpha = valid == 0 ? fmin(1.0 / fmax(pgn, 1e-12), 1.0) : 1.0;
      ls = 0;
#pragma unroll
      for (int r = 0; r < OPT_R; ++r) {
        const int i = lane + WAVE * r;
        if (i < n) db[i] = d[r];
        xt[r] = opt_clamp(x[r] + alpha * d[r], lo_of(r), hi_of(r));
      }
    } else {
      // end of the round: the trial goes back to x
#pragma unroll
      for (int r = 0; r < OPT_R; ++r) xt[r] = x[r];
      bool done = true;
      if (cons) {
        const double t0 = gv0 - P.gu0, t1 = gv1 - P.gu1;
        const double viol = fmax(fmax(t0, 0.0), fmax(t1, 0.0));
        const int round = st.rounds[b];
        double rn = rho;
        if (round > 0 && viol > 0.25 * dr[OD_PREV_VIOL]) rn = rho * 10.0;
        done = round + 1 >= (P.outer_iters > 1 ? P.outer_iters : 1);
        if (lane == 0) {
          st.lam[2 * b] = fmax(lam0 + rho * t0, 0.0);
          st.lam[2 * b + 1] = fmax(lam1 + rho * t1, 0.0);
          st.rho[b] = rn;
          dr[OD_PREV_VIOL] = viol;
          st.rounds[b] = round + 1;
        }
      } else if (lane == 0) {
        st.rounds[b] = 1;
      }
      next = done ? OPT_DONE : OPT_INIT;
      if (done && lane == 0) {
        st.done[b] = 1;
        atomicAdd(st.ndone, 1);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < OPT_R; ++r) {
    const int i = lane + WAVE * r;
    if (i < n) {
      xtb[i] = xt[r];
      if (xt_out) xt_out[i] = xt[r];
    }
  }
  if (lane == 0) {
    ir[OI_PHASE] = next;
    ir[OI_LS] = ls;
    ir[OI_HEAD] = head;
    ir[OI_IT] = it;
    ir[OI_VALID] = (int)valid;
    dr[OD_ALPHA] = alpha;
  }
}

// x = xt = clamp(c0), every seed in INIT with zero multipliers and counters
template <bool DUR>
__device__ __forceinline__ void opt_start(int B, const OptParams& P, const OptState& st, const double* __restrict__ c0,
                                          const OptDur D = OptDur{}) {
  const long long total = (long long)B * P.n;
  const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (g == 0) {
    *st.ndone = 0;
    __hip_atomic_store(st.host_done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (g >= total) return;
  double v;
  if constexpr (DUR)
    v = g % P.n == P.n - 1 ? opt_clamp(c0[g], D.tau_lo, D.tau_hi) : opt_clamp(c0[g], P.lower, P.upper);
  else
    v = opt_clamp(c0[g], P.lower, P.upper);
  st.x[g] = v;
  st.xt[g] = v;
  st.gx[g] = 0.0;
  st.d[g] = 0.0;
  if (g % P.n == 0) {
    const int b = (int)(g / P.n);
    for (int i = 0; i < OD_STRIDE; ++i) st.rec[(size_t)b * OD_STRIDE + i] = 0.0;
    for (int i = 0; i < OI_STRIDE; ++i) st.irec[(size_t)b * OI_STRIDE + i] = 0;
    st.f[b] = 0.0;
    st.g[2 * b] = st.g[2 * b + 1] = 0.0;
    st.lam[2 * b] = st.lam[2 * b + 1] = 0.0;
    st.rho[b] = P.rho0;
    st.evals[b] = st.iters[b] = st.rounds[b] = st.converged[b] = st.done[b] = st.fails[b] = 0;
  }
}
static __global__ void k_opt_start(int B, OptParams P, OptState st, const double* __restrict__ c0) {
  opt_start<false>(B, P, st, c0);
}
static __global__ void k_opt_start_dur(int B, OptParams P, OptDur D, OptState st, const double* __restrict__ z0) {
  opt_start<true>(B, P, st, z0, D);
}

// generic ask/tell step: four seeds per workgroup, one wave each
static __global__ __launch_bounds__(256) void k_opt_tell(int B, OptParams P, OptState st, const double* f,
                                                         const double* grad) {
  if (blockIdx.x == 0 && threadIdx.x == 0) opt_mirror_done(st);
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  opt_tell(P, st, b, threadIdx.x & 63, f[b], grad + (size_t)b * P.n, nullptr);
}
// the same with the last variable a duration; the caller's f and grad are complete (D.kappa is not used)
static __global__ __launch_bounds__(256) void k_opt_tell_dur(int B, OptParams P, OptDur D, OptState st, const double* f,
                                                             const double* grad) {
  if (blockIdx.x == 0 && threadIdx.x == 0) opt_mirror_done(st);
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  opt_tell<true>(P, st, b, threadIdx.x & 63, f[b], grad + (size_t)b * P.n, nullptr, D);
}

// the fused per-tick step of the spline form, one workgroup per seed: dJdc = Bs' dJdu' in k_spline_grad's summation
// order (lane-strided over k, then the butterfly), wave 0 runs the seed's state machine with the spline constraints,
// then all waves write u = transpose(Bs xt) of the new trial in k_spline_u's order.  A DONE seed's u already is its
// iterate's.
static __global__ __launch_bounds__(256) void k_opt_step_spline(OptParams P, OptState st, int Nt,
                                                                const double* __restrict__ Bs,
                                                                const double* __restrict__ dJdu,
                                                                const double* __restrict__ J, double* __restrict__ u) {
#pragma clang fp contract(off)
  __shared__ double s_g[OPT_MAX_N], s_xt[OPT_MAX_N];
  const int b = blockIdx.x, ns = P.ns, nu = P.nu, nc = P.n;
  if (b == 0 && threadIdx.x == 0) opt_mirror_done(st);
  if (st.irec[(size_t)b * OI_STRIDE + OI_PHASE] == OPT_DONE) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double* gb = dJdu + (size_t)b * nu * Nt;
  // a wave takes four outputs at a time (o, o + 4, o + 8, o + 12): their loads and butterflies are in flight together
  for (int o0 = wave; o0 < nc; o0 += 16) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const double* bp[4];
    const double* gp4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = o0 + 4 * q < nc ? o0 + 4 * q : o0;  // a slot past the end repeats the first (not stored)
      bp[q] = Bs + (size_t)Nt * (o % ns);
      gp4[q] = gb + o / ns;
    }
    for (int k = lane; k < Nt; k += 64) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = fma(bp[q][k], gp4[q][(size_t)k * nu], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = opt_wave_sum(acc[q]);
      if (lane == 0 && o0 + 4 * q < nc) s_g[o0 + 4 * q] = v;
    }
  }
  __syncthreads();
  if (wave == 0) opt_tell(P, st, b, lane, J[b], s_g, s_xt);
  __syncthreads();
  double* ub = u + (size_t)b * nu * Nt;
  for (int e = threadIdx.x; e < Nt * nu; e += 256) {
    const int j = e % nu, k = e / nu;
    double acc = 0.0;
    for (int s = 0; s < ns; ++s) acc = fma(Bs[k + (size_t)Nt * s], s_xt[s + ns * j], acc);
    ub[e] = acc;
  }
}

// the fused per-tick step of the duration form, z_b = [c_b, τ_b] with rows of stride n = ns nu + 1: k_opt_step_spline
// with the gradient's last entry dJ/dτ + kappa, the objective J + kappa τ at the trial's τ (a product, then a sum: the
// bits of torch's J + kappa * tau), and the next trial's τ written into the context's time-scale buffer beside its u
static __global__ __launch_bounds__(256) void k_opt_step_spline_dur(OptParams P, OptDur D, OptState st, int Nt,
                                                                    const double* __restrict__ Bs,
                                                                    const double* __restrict__ dJdu,
                                                                    const double* __restrict__ J,
                                                                    const double* __restrict__ dJdtau,
                                                                    double* __restrict__ u, double* __restrict__ tau) {
#pragma clang fp contract(off)
  __shared__ double s_g[OPT_MAX_N], s_xt[OPT_MAX_N];
  const int b = blockIdx.x, ns = P.ns, nu = P.nu, nc = P.n - 1;
  if (b == 0 && threadIdx.x == 0) opt_mirror_done(st);
  if (st.irec[(size_t)b * OI_STRIDE + OI_PHASE] == OPT_DONE) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double* gb = dJdu + (size_t)b * nu * Nt;
  for (int o0 = wave; o0 < nc; o0 += 16) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const double* bp[4];
    const double* gp4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = o0 + 4 * q < nc ? o0 + 4 * q : o0;  // a slot past the end repeats the first (not stored)
      bp[q] = Bs + (size_t)Nt * (o % ns);
      gp4[q] = gb + o / ns;
    }
    for (int k = lane; k < Nt; k += 64) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = fma(bp[q][k], gp4[q][(size_t)k * nu], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v = opt_wave_sum(acc[q]);
      if (lane == 0 && o0 + 4 * q < nc) s_g[o0 + 4 * q] = v;
    }
  }
  if (threadIdx.x == 0) s_g[nc] = dJdtau[b] + D.kappa;
  __syncthreads();
  if (wave == 0) {
    const double kt = D.kappa * st.xt[(size_t)b * P.n + nc];
    opt_tell<true>(P, st, b, lane, J[b] + kt, s_g, s_xt, D);
  }
  __syncthreads();
  double* ub = u + (size_t)b * nu * Nt;
  for (int e = threadIdx.x; e < Nt * nu; e += 256) {
    const int j = e % nu, k = e / nu;
    double acc = 0.0;
    for (int s = 0; s < ns; ++s) acc = fma(Bs[k + (size_t)Nt * s], s_xt[s + ns * j], acc);
    ub[e] = acc;
  }
  if (threadIdx.x == 0) tau[b] = s_xt[nc];
}

// u = transpose(Bs c_b) in k_spline_u's order and tau[b] = z[b n + ns nu] from rows z_b = [c_b, τ_b] of stride
// n = ns nu + 1: the controls and time scale of the duration form's start and closing eval
static __global__ void k_spline_u_tau(int B, int Nt, int ns, int nu, const double* __restrict__ Bs,
                                      const double* __restrict__ z, double* __restrict__ u, double* __restrict__ tau) {
#pragma clang fp contract(off)
  const long long total = (long long)B * Nt * nu;
  const int n = ns * nu + 1;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(g % nu);
    const long long bk = g / nu;
    const int k = (int)(bk % Nt);
    const int b = (int)(bk / Nt);
    const double* cb = z + (size_t)b * n + (size_t)ns * j;
    double acc = 0.0;
    for (int s = 0; s < ns; ++s) acc = fma(Bs[k + (size_t)Nt * s], cb[s], acc);
    u[g] = acc;
    if (j == 0 && k == 0) tau[b] = z[(size_t)b * n + n - 1];
  }
}

// f_b = J_b + kappa τ_b at the iterates, for a run in which no seed took an eval (max_ticks = 0)
static __global__ void k_opt_f_dur(int B, int n, double kappa, const double* __restrict__ J, const double* __restrict__ x,
                                   double* __restrict__ f) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double kt = kappa * x[(size_t)b * n + n - 1];
  f[b] = J[b] + kt;
}

}  // namespace qoc

// host object behind qoc_opt (include/qoc.h)
struct qoc_opt {
  int dev = 0, B = 0, order = 3;
  bool dur = false;  // qoc_opt_create_duration: the last variable is a duration with the bounds in D
  qoc::OptDur D{};
  qoc::OptParams P{};
  qoc::OptState st{};
  int* h_done = nullptr;  // host-mapped word behind st.host_done
  hipEvent_t ev = nullptr;
  std::vector<void*> allocs;
};
