// qoc_ode_grad.hpp — J and dJ/dp of the continuous-envelope run (qoc_eval_envelope): the discrete adjoint of the
// fixed-step Tsit5 scheme of k_ode_envelope (qoc_ode.hpp), i.e. the derivative of the J that kernel's states give.
//
// FSAL only saves an evaluation, so a step is a plain six-stage explicit Runge-Kutta with b = row 7 of the tableau:
//   X_i = x_n + h Σ_{j<i} a_ij k_j,  k_i = A(t_i) X_i,  x_{n+1} = x_n + h Σ_i b_i k_i,   A(t) = A0 + Σ_j c_j(t; p) A_j.
// Reverse sweep of one step with ℓ = λ_{n+1} (dJ = Re<λ, dx>), i = 6..1:
//   κ_i = h (b_i ℓ + Σ_{j>i} a_ji ξ_j),  ξ_i = A(t_i)^H κ_i,  dJ/dp_q += Σ_j ∂c_j/∂p_q(t_i) Re<κ_i, A_j X_i>,
//   λ_n = ℓ + Σ_i ξ_i.
//
//   k_ode_envelope_ckpt: k_ode_envelope's forward (same step, same right-hand side) that also writes (x_n, k1_n) every
//                        C steps: the checkpoints.  k1_n is the FSAL stage the forward carried into step n, so a
//                        restart from a checkpoint repeats the forward's arithmetic and its x_n bit for bit.
//   k_ode_envelope_grad: per column wave, segments from the last to the first: reload the checkpoint, re-run the
//                        segment's steps keeping x_n in a wave-private LDS ring, then walk the steps backwards.  A
//                        reverse step recomputes the six X_i and v_ji = A_j X_i from x_n (k_1 = A(t_n) x_n, whatever
//                        the spacing), runs the κ / ξ recurrence and adds the contraction.  λ never leaves registers.
//
// Layout as k_ode_envelope: one workgroup per seed, wave w owns columns w, w + W, ..., lane = row (N <= 64), the
// nu + 1 generators in LDS.  A^H κ: lane l needs column l of the column-major generator.  With TR the workgroup keeps
// conjugate-transposed copies (conflict-free, the forward's mat-vec); without, lane l reads its column in place: 16
// contiguous bytes per lane and row, lanes N * 16 bytes apart (conflict-free for odd N, 16-way at N = 64).  Both run
// the same sums in the same order.
// Parameters: lane q owns parameter q (np <= 64).  s_ji = Re Σ_rows conj(κ_i) v_ji is reduced over the wave (a
// butterfly over the first 2^ceil(log2 N) lanes, then a broadcast of lane 0), and lane q adds ∂c_j/∂p_q(t_i) s_ji to
// its accumulator; the waves' accumulators meet in LDS and are added in wave order: no atomics, repeatable bits.
#pragma once
#include "qoc_ode.hpp"

namespace qoc {

// k_ode_envelope's right-hand side: (A0 + Σ_j c_j(t) A_j) y
template <typename T>
__device__ __forceinline__ cx<T> envelope_rhs(int N, int nu, const cx<T>* __restrict__ G, int kind,
                                              const double* __restrict__ p, int np, cx<T> y, double t, int lane) {
  const size_t NN = (size_t)N * N;
  double cc[2] = {0, 0};
  envelope_dev(kind, p, np, t, cc);
  cx<T> r = ode_matvec<T>(N, G, y, lane);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j < nu) {
      const cx<T> v = ode_matvec<T>(N, G + (size_t)(j + 1) * NN, y, lane);
      r.r += (T)cc[j] * v.r;
      r.i += (T)cc[j] * v.i;
    }
  }
  return r;
}

// y_lane = Σ_r conj(M[r + N lane]) x_r: M^H x with M read in place (ode_matvec's loop on the lane's column)
template <typename T>
__device__ __forceinline__ cx<T> ode_matvec_h(int N, const cx<T>* __restrict__ M, cx<T> x, int lane) {
  cx<T> y0 = {0, 0}, y1 = {0, 0};
  const cx<T>* __restrict__ mc = M + (size_t)N * (lane < N ? lane : 0);
  int j = 0;
  for (; j + 8 <= N; j += 8) {
    cx<T> a[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = mc[j + t];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const T xr = bcast(x.r, j + t), xi = bcast(x.i, j + t);
      cx<T>& y = (t & 1) ? y1 : y0;
      y.r += a[t].r * xr + a[t].i * xi;
      y.i += a[t].r * xi - a[t].i * xr;
    }
  }
  for (; j < N; ++j) {
    const T xr = bcast(x.r, j), xi = bcast(x.i, j);
    const cx<T> a = mc[j];
    y0.r += a.r * xr + a.i * xi;
    y0.i += a.r * xi - a.i * xr;
  }
  return cx<T>{y0.r + y1.r, y0.i + y1.i};
}

// ∂c_j/∂p_q(t), j = 0, 1, for the lane's own parameter q (zero for q >= np and for parameters the pulse does not
// read).  ∂/∂p_0 of DRAG (tgate) and of the sine basis (Tgate) is the partial derivative of the formula: the
// integration horizon is an argument of its own.  The tunable bus takes the branch of cos_envelope that t lies in
// (the envelope is C^1 in t_plateau and t_rise_fall); at cos θ = 0 its sqrt|cos θ| has no derivative and the result
// is not finite.
__device__ __forceinline__ void envelope_grad_dev(int kind, const double* __restrict__ p, int np, double t, int q,
                                                  double (&dc)[2]) {
  dc[0] = 0;
  dc[1] = 0;
  if (q >= np) return;
  if (kind == ENV_TUNABLE_BUS) {
    if (q > 4) return;
    const double tp = p[0], trf = p[1];
    double d, d_tp = 0, d_trf = 0;
    if (t > trf / 2 && t <= trf / 2 + tp) {
      d = 1.0;
    } else if (t <= trf / 2) {
      const double a = 2 * M_PI * t / trf;
      d = 0.5 * (1 - cos(a));
      d_trf = -0.5 * sin(a) * a / trf;
    } else {
      const double a = 2 * M_PI * (t - tp) / trf;
      d = 0.5 * (1 - cos(a));
      d_tp = -0.5 * sin(a) * 2 * M_PI / trf;
      d_trf = -0.5 * sin(a) * a / trf;
    }
    const double cw = cos(p[3] * t), sw = sin(p[3] * t);
    const double phi = M_PI * (p[2] + p[4] * d * cw);
    const double cph = cos(phi);
    const double c = sqrt(fabs(cph));
    const double dc_dphi = -sin(phi) * (cph < 0 ? -1.0 : 1.0) / (2 * c);
    double dphi;
    if (q == 0) dphi = M_PI * p[4] * cw * d_tp;
    else if (q == 1) dphi = M_PI * p[4] * cw * d_trf;
    else if (q == 2) dphi = M_PI;
    else if (q == 3) dphi = -M_PI * p[4] * d * t * sw;
    else dphi = M_PI * d * cw;
    dc[0] = dc_dphi * dphi;
  } else if (kind == ENV_DRAG) {
    if (q > 3) return;
    const double tg = p[0], sg = p[1], A = p[2], xi = p[3];
    const double x = t - tg / 2, s2 = sg * sg, s3 = s2 * sg;
    const double tmp = exp(-x * x / (2 * s2)), e0 = exp(-tg * tg / (8 * s2));
    if (q == 0) {
      dc[0] = A * (tmp * x / (2 * s2) + e0 * tg / (4 * s2));
      dc[1] = A * xi * tmp / (2 * s2) * (1 - x * x / s2);
    } else if (q == 1) {
      dc[0] = A * (tmp * x * x / s3 - e0 * tg * tg / (4 * s3));
      dc[1] = A * xi * x * tmp / s3 * (2 - x * x / s2);
    } else if (q == 2) {
      dc[0] = tmp - e0;
      dc[1] = -xi * x / s2 * tmp;
    } else {
      dc[1] = -A * x / s2 * tmp;
    }
  } else {
    const double T = p[0];
    if (q == 0) {
      double ox = 0, oy = 0;
      for (int k = 1; 2 * k + 1 <= np; ++k) {
        const double w = M_PI * k * t / T;
        const double dk = -cos(w) * w / T;
        ox += p[2 * k - 1] * dk;
        oy += p[2 * k] * dk;
      }
      dc[0] = ox;
      dc[1] = oy;
    } else {
      const int k = (q + 1) >> 1;
      if (2 * k + 1 <= np) dc[(q & 1) ? 0 : 1] = sin(M_PI * k * t / T);
    }
  }
}

// Checkpoint (b, seg, col): x then k1, N elements each.
__device__ __forceinline__ size_t env_ckpt_off(int N, int m, int nseg, int b, int seg, int col) {
  return (((size_t)b * nseg + seg) * m + col) * 2 * N;
}

// k_ode_envelope with checkpoints: (x_n, k1_n) at n = 0, C, 2C, ... < nsteps.
__global__ __launch_bounds__(256) void k_ode_envelope_ckpt(int N, int m, int nu, int Nt, int kind,
                                                           const double* __restrict__ P, int np, double dt,
                                                           long long nsteps, int C, int nseg,
                                                           const cx<double>* __restrict__ Agen,
                                                           const cx<double>* __restrict__ x0, int x0_per_seed,
                                                           cx<double>* __restrict__ S, cx<double>* __restrict__ ckpt) {
  typedef double T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cx<T>* G = reinterpret_cast<cx<T>*>(smem);  // (nu + 1) generators
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
  const size_t NN = (size_t)N * N, Nm = (size_t)N * m;
  for (size_t e = tid; e < (size_t)(nu + 1) * NN; e += blockDim.x) G[e] = Agen[e];
  cx<T>* Sb = S + (size_t)b * (Nt + 1) * Nm;
  const cx<T>* x0b = x0 + (x0_per_seed ? (size_t)b * Nm : 0);
  for (size_t o = tid; o < Nm; o += blockDim.x) Sb[o] = x0b[o];
  const double* p = P + (size_t)b * np;
  __syncthreads();
  for (int col = wave; col < m; col += W) {
    cx<T> x = lane < N ? x0b[(size_t)N * col + lane] : cx<T>{0, 0};
    auto rhs = [&](cx<T> y, double t) __attribute__((always_inline)) {
      return envelope_rhs<T>(N, nu, G, kind, p, np, y, t, lane);
    };
    cx<T> k1 = rhs(x, 0.0);
    int seg = 0, left = 0;  // left: steps until the next checkpoint
    for (long long s = 0; s < nsteps; ++s) {
      if (left == 0) {
        if (lane < N) {
          cx<T>* ck = ckpt + env_ckpt_off(N, m, nseg, b, seg, col);
          ck[lane] = x;
          ck[N + lane] = k1;
        }
        ++seg;
        left = C;
      }
      --left;
      tsit5_step<T>(x, k1, (T)dt, (double)s * dt, rhs);
    }
    if (lane < N) Sb[(size_t)Nt * Nm + (size_t)N * col + lane] = x;
  }
}

// Σ over the lanes < n2 (a power of two >= N; lanes in [N, n2) pass zero), the same value in every lane
__device__ __forceinline__ double env_wave_sum(double v, int n2) {
  for (int off = n2 >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return bcast(v, 0);
}

// dJdp[b][q] for the run of k_ode_envelope_ckpt.  λ_N = coef ⊙ X_target (k_terminal_cost's coefficients of the
// stored x(tgate)) or the caller's lam (B x N x m).  LDS: generators | their conjugate transposes (TR) | W rings of
// C x N | W x 64 doubles.
template <int NU, bool TR>
__global__ __launch_bounds__(256) void k_ode_envelope_grad(int N, int m, int kind, const double* __restrict__ P, int np,
                                                           double dt, long long nsteps, int C, int nseg,
                                                           const cx<double>* __restrict__ Agen,
                                                           const cx<double>* __restrict__ ckpt,
                                                           const cx<double>* __restrict__ Xt,
                                                           const cx<double>* __restrict__ coef,
                                                           const cx<double>* __restrict__ lam,
                                                           double* __restrict__ dJdp) {
  typedef double T;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
  const size_t NN = (size_t)N * N;
  cx<T>* G = reinterpret_cast<cx<T>*>(smem);
  cx<T>* GH = G + (size_t)(NU + 1) * NN;  // TR only
  cx<T>* ring = (TR ? GH + (size_t)(NU + 1) * NN : GH) + (size_t)wave * C * N;
  double* red = reinterpret_cast<double*>((TR ? GH + (size_t)(NU + 1) * NN : GH) + (size_t)W * C * N);
  for (size_t e = tid; e < (size_t)(NU + 1) * NN; e += blockDim.x) {
    const cx<T> a = Agen[e];
    G[e] = a;
    if (TR) {
      const size_t g = e / NN, o = e - g * NN, r = o % N, c = o / N;
      GH[g * NN + c + N * r] = cx<T>{a.r, -a.i};
    }
  }
  const double* p = P + (size_t)b * np;
  int n2 = 1;
  while (n2 < N) n2 <<= 1;
  const T h = (T)dt;
  __syncthreads();
  auto rhs = [&](cx<T> y, double t) __attribute__((always_inline)) {
    return envelope_rhs<T>(N, NU, G, kind, p, np, y, t, lane);
  };
  auto mv_h = [&](int g, cx<T> y) __attribute__((always_inline)) {
    if (TR) return ode_matvec<T>(N, GH + (size_t)g * NN, y, lane);
    return ode_matvec_h<T>(N, G + (size_t)g * NN, y, lane);
  };
  double acc = 0;  // dJ/dp_lane over this wave's columns
  for (int col = wave; col < m; col += W) {
    cx<T> l = {0, 0};  // λ_{n+1}
    if (lane < N) {
      if (lam) {
        l = lam[((size_t)b * m + col) * N + lane];
      } else {
        const cx<double> cf = coef[(size_t)b * 2 * m + col], t = Xt[(size_t)N * col + lane];
        l = cx<T>{cf.r * t.r - cf.i * t.i, cf.r * t.i + cf.i * t.r};
      }
    }
    for (int seg = nseg - 1; seg >= 0; --seg) {
      const long long s0 = (long long)seg * C;
      const int len = (int)((nsteps - s0 < C) ? nsteps - s0 : C);
      {  // the segment's x_n, n = s0 .. s0 + len - 1, as the forward formed them
        const cx<T>* ck = ckpt + env_ckpt_off(N, m, nseg, b, seg, col);
        cx<T> x = lane < N ? ck[lane] : cx<T>{0, 0};
        cx<T> k1 = lane < N ? ck[N + lane] : cx<T>{0, 0};
        if (lane < N) ring[lane] = x;
        for (int i = 1; i < len; ++i) {
          tsit5_step<T>(x, k1, h, (double)(s0 + i - 1) * dt, rhs);
          if (lane < N) ring[(size_t)i * N + lane] = x;
        }
      }
      for (int i = len - 1; i >= 0; --i) {
        const double tn = (double)(s0 + i) * dt;
        const cx<T> xn = lane < N ? ring[(size_t)i * N + lane] : cx<T>{0, 0};
        // stages: k_i, v_ji = A_j X_i and the envelope values
        cx<T> k[6], v[6][NU];
        double cc[6][2];
#pragma unroll
        for (int i6 = 0; i6 < 6; ++i6) {
          cx<T> X = xn;
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            if (j < i6) {
              const T a = (T)kTsitA[i6][j] * h;
              X.r += a * k[j].r;
              X.i += a * k[j].i;
            }
          }
          cc[i6][0] = 0;
          cc[i6][1] = 0;
          envelope_dev(kind, p, np, tn + kTsitC[i6] * (double)h, cc[i6]);
          cx<T> r = ode_matvec<T>(N, G, X, lane);
#pragma unroll
          for (int j = 0; j < NU; ++j) {
            v[i6][j] = ode_matvec<T>(N, G + (size_t)(j + 1) * NN, X, lane);
            r.r += (T)cc[i6][j] * v[i6][j].r;
            r.i += (T)cc[i6][j] * v[i6][j].i;
          }
          k[i6] = r;
        }
        // reverse: κ_i, the contraction, ξ_i (stored over k_i, no longer needed)
        cx<T> ln = l;
#pragma unroll
        for (int i6 = 5; i6 >= 0; --i6) {
          const T bi = (T)kTsitA[6][i6] * h;
          cx<T> kap = {bi * l.r, bi * l.i};
#pragma unroll
          for (int j = 5; j > 0; --j) {
            if (j > i6) {
              const T a = (T)kTsitA[j][i6] * h;
              kap.r += a * k[j].r;
              kap.i += a * k[j].i;
            }
          }
          double dc[2];
          envelope_grad_dev(kind, p, np, tn + kTsitC[i6] * (double)h, lane, dc);
#pragma unroll
          for (int j = 0; j < NU; ++j) {
            const double s = env_wave_sum(lane < N ? kap.r * v[i6][j].r + kap.i * v[i6][j].i : 0.0, n2);
            acc += dc[j] * s;
          }
          cx<T> xi = mv_h(0, kap);
#pragma unroll
          for (int j = 0; j < NU; ++j) {
            const cx<T> w = mv_h(j + 1, kap);
            xi.r += (T)cc[i6][j] * w.r;
            xi.i += (T)cc[i6][j] * w.i;
          }
          k[i6] = xi;
          ln.r += xi.r;
          ln.i += xi.i;
        }
        l = ln;
      }
    }
  }
  red[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave == 0 && lane < np) {
    double g = 0;
    for (int w = 0; w < W; ++w) g += red[w * 64 + lane];
    dJdp[(size_t)b * np + lane] = g;
  }
}

}  // namespace qoc
