// qoc_blkseg.hpp — one evaluation (propagate + J + grape_sensitivity) on block propagators with the time axis cut
// into segments, so that the serial depth per seed is about 2 Nt / S + log2 S instead of 2 Nt.
//
// The reference's two chains are serial in k (src/gradient_computations.jl:27-29 forward, :52-58 co-states); only
// the exponentials are parallel (:17-25).  With generators whose invariant blocks have <= 3 rows (qoc_blk.hpp: cavity
// 20 blocks of 2, zz 3 blocks of 3) every U_k is block-diagonal, and one block of it costs as much to form as to
// apply.  One workgroup per seed; lane (s, β) owns block β of segment s = slices [s L, s L + L):
//   phase 0  step records of every slice (e^{μ_k}, 2^-J u_k) into LDS, J and the Taylor degree P from the seed's
//            largest ρ_k (one pair for the whole seed: every lane runs the same term loop);
//   phase 1  the segment product P_s = U_{sL+L-1} .. U_{sL} on the block (U_k formed per slice, the k_blku_* block
//            exponential: Taylor polynomial in the Cayley-Hamilton basis with the phase folded in);
//   phase 2  inclusive prefix products Q_s = P_s .. P_0 over the segments (a Hillis-Steele scan inside each wave,
//            then the earlier waves' totals; one workgroup barrier),
//            x_N = Q_{S-1} x_0, the terminal cost J and λ_N (chain_costs, src/penalty_fcns.jl:15-42), then
//            G_N = Σ_c x_N,c λ_N,c^H per block;
//   phase 3  every segment backwards from its end, with G_k = Σ_c x_k,c λ_k,c^H instead of the states: because U_k is
//            unitary (skew-Hermitian generators; the host checks them exactly),
//              K_k = Σ_c x_k λ_{k+1}^H = U_k^H G_{k+1},    G_k = K_k U_k,
//            and G at the segment's end is Q_s G_0 Q_s^H with G_0 = Q_{S-1}^H G_N Q_{S-1}.  The gradient of the slice is
//            the trace form of expm_jacobian! + _compute_u_sensitivity (:177-223, blku_contract) on K_k:
//              dJ/du_jk = Re tr(A_j M_k),  M = Σ_{a+b<ORD} X^b K X^a / (a+b+1)!,  X = A_k,
//            summed over the slice's blocks (a wave-private LDS slot, fixed order: no atomics).
//            ORD 0 is the exact (Fréchet) gradient, dUkdp_order = QOC_DUKDP_EXACT: the whole series
//              M = Σ_{a,b >= 0} X^b K X^a / (a+b+1)! = ∫_0^1 e^{sX} K e^{(1-s)X} ds
//            on the same K_k and X, so that dJdu is the derivative of the J this kernel computes.  Blocks of 2 rows
//            without halvings: closed form from the cos ω, sinc ω and e^{μ_k} e^{it} the propagator was formed from
//            (sk2_contract_exact); otherwise the recurrence as a rolled loop to a term count chosen per seed in
//            phase 0 (seg_contract_exact, blkseg_exact_terms).  Nothing else of the kernel depends on ORD.
// Blocks of 2 rows whose control blocks have zero diagonals and no shifts (the cavity's class, ZD below) and no
// halvings: U_k = z V_k with one unimodular constant z per block and V_k in SU(2), and both slice loops run on V_k
// alone (sk2_form_v): phase 1 multiplies SU(2) matrices in 4 reals, phase 3 moves Ĝ = z̄ G (the same K_k), and the
// traces need two of K's four Pauli components.  z enters once per lane: z^Nt on x_N (the only quantity of phase 2
// that sees the phase), z̄ on G at the segment's end.
// Neither x_k, λ_k nor U_k go to HBM: the launch reads u and writes J, the λ_N coefficients and dJdu.  qoc_get_states
// and qoc_get_costates rebuild x_k / λ_k on demand with the k_blku_* chains (qoc_run_blku.hip).
//
// The reference's own call form runs the two halves apart: Ipopt's f calls propagate, its f_grad grape_sensitivity
// (examples/ipopt_callbacks_exp.jl:11-31; f alone in every line-search trial).  MODE splits the launch at the end of
// phase 2 (BLKSEG_FWD: phases 0-2, which also write G at every segment's end, Q_s G_0 Q_s^H, to HBM: S nblk NB^2
// complex per seed, 31 KB at cavity size) and BLKSEG_BWD (phase 0's records and (J, P) again -- the same arithmetic on
// the same u, so the same values -- then phase 3 from those G): bitwise the fused launch's J and dJdu.
//
// The guard-state penalty (the PEN instantiations; setup_state_penalty, src/penalty_fcns.jl:1-11, consumed at
// src/gradient_computations.jl:47-49,55-57): L(x) = μ Σ_{i in P, c in C} |x_ic|^2 on all Nt + 1 states, and the source
// 2 μ x_k[P, C] of every λ_k.  No state comes back for it.  Per block, with Π the 0/1 projector on its rows in P,
// D_k = Σ_{c in C} x_k,c x_k,c^H and W_k = U_{k-1} .. U_0 (unitary): D_k = W_k D_0 W_k^H moves by the same
// conjugation as G, G_k = K_k U_k + 2 μ D_k Π, and with R_k = W_k^H Π W_k the frame of time 0 has
// W_k^H (K_k U_k) W_k = G~_N,cost + 2 μ D_0 Σ_{j > k} R_j and Σ_k L(x_k) = μ tr(D_0 Σ_{k=0}^{Nt} R_k).
//   phase 1  beside P_s, H_s = Σ V^H Π V over the running product V after each slice (one outer product per
//            penalised row), then H'_s = P_s H_s P_s^H;
//   phase 2  T_s = Q_s^H H'_s Q_s = Σ_{k in (kb, ke]} R_k; suffix sums of T over the segments (additions only: a scan
//            inside each wave through the lanes' rows of the segment products' area, then the later waves' totals);
//            D_0 from x_0 before x_N overwrites it; J += μ Σ_blocks Re tr(D_0 (Π + Σ_s T_s)) before J is published;
//            at the segment's end G = Q_s (G_0 + 2 μ D_0 Σ_{s' > s} T_s') Q_s^H (without the end's own source) and
//            D = Q_s D_0 Q_s^H;
//   phase 3  per slice G += 2 μ D Π (the source of λ_{k+1}), D <- U_k^H D U_k, then K_k and G_k as before.  D lives
//            in the lane's own row of the segment products' area (free by then), not in registers.
// BLKSEG_FWD also writes D at the segment ends (dseg, behind gseg).  The λ_N coefficients stay the cost's alone; the
// co-states' rebuild (blku_costates) adds the sources from rebuilt states.  Lanes of blocks without a row in P skip
// all of it (uniform control flow apart).  Extra LDS: D_0 per block.  Blocks of 3 rows: the fused penalised kernel
// does not fit 256 VGPRs (it spills), so the host runs the penalised eval as BLKSEG_FWD + BLKSEG_BWD, which do
// (qoc_run_blkseg.hip blkseg_eval), and BLKSEG_FUSED with PEN is built for blocks of 2 rows only.
#pragma once
#include "qoc_blku.hpp"

namespace qoc {

struct BlksegParams {
  double rad[3];               // ρ_k = rad[0] + Σ_j |u_jk| rad[j] (spectral half-widths of the shifted generators)
  double mur[3], mui[3];       // shifts μ_j: Ã_j = A_j - μ_j I, e^{μ_k} = exp(μ_0 + Σ_j u_jk μ_j)
  double theta_cap;            // ρ / 2^J <= theta_cap
  int S;                       // segments per seed
  int L;                       // slices per segment (S L >= Nt; the last segment may be shorter)
  int UPW;                     // segments per wave (64 / nblk)
  int RB;                      // slice-steps per block-sum reduction (blkseg_rb)
  const double* u;             // B x Nt x nu controls (the caller's buffer)
  double* u_copy;              // copies of u written by the launch (the stale check, the lazy rebuilds), or nullptr
  double* u_copy2;
  double* J2;                  // a second copy of J (the caller's), or nullptr
  cx<double>* coef2;           // a second copy of the λ_N coefficients (the lazy co-states), or nullptr
  double* dJdu;                // B x Nt x nu
  unsigned long long* terms;   // Σ P 2^J per pass over the slices (executed Taylor terms), nullptr: not counted
  // the best (J, global seed) of this launch for qoc_allgather_best_dev (the last workgroup to publish its J reduces
  // them; done counts the published ones and is reset by that workgroup), or nullptr
  unsigned int* done;
  double* best;
  long long seed_offset;
  // nothing to exchange (one rank): the final pair also into the context's result slot and the registered output
  // (qoc_set_best_output), or nullptr
  double* best_res;
  double* best_out;
  // the split launches: G at every segment's end, B x [NB^2][S][nblk] complex (written by BLKSEG_FWD, read by
  // BLKSEG_BWD); stale: the stale-u flag of the check queued before BLKSEG_BWD (nonzero: the launch writes nothing)
  double2* gseg;
  const int* stale;
  // the shifted generators' blocks, block-major [nblk][3][NB^2] (zeros for j > nu and for a padded row): built by the
  // host where the block layout and the shifted generators are established, copied to LDS by the prologue
  const double2* gtab;
  // the guard-state penalty (PEN instantiations; setup_state_penalty, src/penalty_fcns.jl:1-11): L(x) = pen_mu
  // Σ_{i in P, c in C} |x_ic|^2 summed over the Nt + 1 states.  prow[i]: bit β set when row i of block β is in P (never
  // a padding row); pcol: bit c set when column c is in C; dseg: D = Σ_{c in C} x_c x_c^H per block at every segment's
  // end, laid out like gseg (written by BLKSEG_FWD, read by BLKSEG_BWD)
  double pen_mu;
  unsigned int prow[3];
  unsigned int pcol;
  double2* dseg;
  // ensemble launches (the ENS instantiations; 0 / nullptr otherwise): E generator sets per pulse, workgroup v =
  // pulse * E + member; member e reads the table gtab + e * 3 nblk NB^2 and its nine scalars ens[9 e ..] =
  // rad[3] | mur[3] | mui[3] in place of the ones above
  int E;
  const double* ens;
  // the member-aware backward half (BLKSEG_BWD with ENS): ω[B][E] of k_ens_weights; workgroup v returns at once when
  // omega[v] == 0 and leaves its row of dJdu as it was (nullptr: every workgroup runs)
  const double* omega;
  // the per-seed time scale (the TS instantiations; nullptr otherwise): seed b runs on tau[b] times the generators
  // (the table and the nine scalars above, scaled in the prologue) and leaves dJ/dτ_b at fixed u in dJdtau[b]
  const double* tau;
  double* dJdtau;
};
enum { BLKSEG_FUSED = 0, BLKSEG_FWD = 1, BLKSEG_BWD = 2 };

// LDS, in doubles: shifted generator blocks [nblk][3][E] complex | step records [Nt][4] | segment products [S][E][nblk]
// complex | G_0 [E][nblk] complex | x_0 then x_N (N m complex) | X_target (N m complex) | λ_N coefficients (2 m
// complex) | scratch (24) |
// per-wave partial sums [W][RB][64][2] | dJdu [Nt][nu] | penalised shapes: D_0 [E][nblk] complex
__host__ __device__ inline size_t blkseg_off_rec(int NB, int nblk) { return (size_t)6 * NB * NB * nblk; }
__host__ __device__ inline size_t blkseg_off_slot(int NB, int nblk, int Nt) { return blkseg_off_rec(NB, nblk) + 4 * (size_t)Nt; }
__host__ __device__ inline size_t blkseg_off_g0(int NB, int nblk, int Nt, int S) {
  return blkseg_off_slot(NB, nblk, Nt) + (size_t)2 * S * NB * NB * nblk;
}
__host__ __device__ inline size_t blkseg_off_xN(int NB, int nblk, int Nt, int S) {
  return blkseg_off_g0(NB, nblk, Nt, S) + (size_t)2 * NB * NB * nblk;
}
__host__ __device__ inline size_t blkseg_off_xt(int N, int m, int NB, int nblk, int Nt, int S) {
  return blkseg_off_xN(NB, nblk, Nt, S) + (size_t)2 * N * m;
}
__host__ __device__ inline size_t blkseg_off_cf(int N, int m, int NB, int nblk, int Nt, int S) {
  return blkseg_off_xt(N, m, NB, nblk, Nt, S) + (size_t)2 * N * m;
}
__host__ __device__ inline size_t blkseg_off_red(int N, int m, int NB, int nblk, int Nt, int S) {
  return blkseg_off_cf(N, m, NB, nblk, Nt, S) + (size_t)4 * m;
}
__host__ __device__ inline size_t blkseg_off_wred(int N, int m, int NB, int nblk, int Nt, int S) {
  return blkseg_off_red(N, m, NB, nblk, Nt, S) + 32;  // red[0..23]: reductions, red[24..31]: wave progress
}
__host__ __device__ inline size_t blkseg_off_dJ(int N, int m, int NB, int nblk, int Nt, int S, int W, int RB) {
  return blkseg_off_wred(N, m, NB, nblk, Nt, S) + (size_t)128 * W * RB;
}
// (D_0 starts on a 16-byte boundary)
__host__ __device__ inline size_t blkseg_off_d0(int N, int m, int nu, int NB, int nblk, int Nt, int S, int W, int RB) {
  return (blkseg_off_dJ(N, m, NB, nblk, Nt, S, W, RB) + (size_t)Nt * nu + 1) & ~(size_t)1;
}
__host__ __device__ inline size_t blkseg_lds(int N, int m, int nu, int NB, int nblk, int Nt, int S, int W, int RB,
                                             bool pen = false) {
  if (pen) return (blkseg_off_d0(N, m, nu, NB, nblk, Nt, S, W, RB) + (size_t)2 * NB * NB * nblk) * sizeof(double);
  return (blkseg_off_dJ(N, m, NB, nblk, Nt, S, W, RB) + (size_t)Nt * nu) * sizeof(double);
}
// the most LDS a launch may take (dynamic plus the kernel's static share): the shape falls back or the eval declines
constexpr size_t BLKSEG_LDS_MAX = (size_t)160 * 1024;
// slice-steps whose block sums are reduced together (phase 3): as many as the reducing lanes of one wave allow
// (RB x segments per wave x controls <= 64), at most 4
__host__ __device__ inline int blkseg_rb(int upw, int nu) {
  const int r = 64 / (upw * (nu > 0 ? nu : 1));
  return r < 1 ? 1 : r > 4 ? 4 : r;
}

// Diagnostic per-wave stamps (tools/blkseg_probe.hip, -DQOC_PROBE): workgroup 7, wave w: phase 1 ends at
// g_segw[w], phase 3 at g_segw[16 + w] (cycles from the workgroup's start)
#ifdef QOC_PROBE
static __device__ unsigned long long g_segw[32];
#define SEGW_SET(slot, v)                                                        \
  do {                                                                           \
    if (blockIdx.x == 7 && (threadIdx.x & 63) == 0) g_segw[slot] = (v);          \
  } while (0)
static __device__ int g_seg_noturn, g_seg_turnmode;
#define SEG_TURNS (!g_seg_noturn)
#define SEG_TURNMODE g_seg_turnmode
#else
#define SEG_TURNS true
#define SEG_TURNMODE 1
#define SEGW_SET(slot, v) \
  do {                    \
  } while (0)
#endif

// launch bounds: WMAX = 8 waves (2 per SIMD, <= 256 VGPRs: the lane's generator blocks in registers) or 12 (3 per
// SIMD, <= 168 VGPRs: generator blocks read from LDS where used)

// c = a b, c = a^H b, c = a b^H on NB x NB complex blocks (row-major)
template <int NB, bool AH, bool BH>
__device__ __forceinline__ void seg_mm(const double (&ar)[NB * NB], const double (&ai)[NB * NB], const double (&br)[NB * NB],
                                       const double (&bi)[NB * NB], double (&cr)[NB * NB], double (&ci)[NB * NB]) {
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const int ea = AH ? q * NB + i : i * NB + q, eb = BH ? k * NB + q : q * NB + k;
        const double xr = ar[ea], xi = AH ? -ai[ea] : ai[ea];
        const double yr = br[eb], yi = BH ? -bi[eb] : bi[eb];
        sr = fma(xr, yr, fma(-xi, yi, sr));
        si = fma(xr, yi, fma(xi, yr, si));
      }
      cr[i * NB + k] = sr;
      ci[i * NB + k] = si;
    }
}

// cos x and sin x / x as polynomials in x^2 (Horner, a fixed degree BLKSEG_KMAX = 9: the terms of exp(B) up to
// B^19, whose tail is below 2^-53 for every |x| <= θ_cap ≈ 0.98, so at least the Taylor polynomial's degree P; a
// fixed count keeps the loop free of branches and uniform masks)
constexpr int BLKSEG_KMAX = 9;
struct BlksegTrig {
  double c[BLKSEG_KMAX + 1];  // (-1)^k / (2k)!
  double s[BLKSEG_KMAX + 1];  // (-1)^k / (2k+1)!
  double d[BLKSEG_KMAX + 1];  // (-1)^k 2 (k+1) / (2k+3)!: (sin x / x - cos x) / x^2 (the exact contraction's s3)
};
// The series degree K (terms up to x^(2K+1)) a seed needs: the first omitted term ρ^(2K+2) / (2K+2)! below 2^-53 for
// every |x| <= ρ (both ω and |t| are bounded by the seed's largest ρ_k: the eigenvalues i(t ± ω) of a shifted block lie
// within [-ρ, ρ]).  K = 5 up to ρ = 0.24, 7 up to 0.66, else 9 (covers θ_cap ≈ 0.98); the bounds leave margin
// (exact limits 0.248 / 0.684 / 1.32).
__host__ __device__ constexpr int blkseg_series_k(double rho) { return rho <= 0.24 ? 5 : rho <= 0.66 ? 7 : BLKSEG_KMAX; }
// blkseg_exact_terms, the exact gradient's term-count rule (seg_contract_exact), lives in qoc_common.hpp: the dense
// series kernels (qoc_grad_rr.hpp) share it.
constexpr BlksegTrig blkseg_trig() {
  BlksegTrig t{};
  double f = 1.0;  // 1 / n!
  for (int n = 0; n <= 2 * BLKSEG_KMAX + 1; ++n) {
    if (n > 0) f /= n;
    const double sg = (n / 2) % 2 ? -1.0 : 1.0;
    if (n % 2 == 0) t.c[n / 2] = sg * f;
    else t.s[n / 2] = sg * f;
  }
  // s3 = (sinc - cos) / x^2 = 1/3 - x^2/30 + x^4/840 - ..: its own series, because the difference cancels at small x.
  // The term dropped after degree K, 2 (K+2) x^(2K+2) / (2K+5)!, is below the cosine's x^(2K+2) / (2K+2)!, so the
  // degree classes of blkseg_series_k hold for it as they stand.
  double f3 = 1.0 / 6.0;  // 1 / (2k+3)!
  for (int k = 0; k <= BLKSEG_KMAX; ++k) {
    t.d[k] = (k % 2 ? -1.0 : 1.0) * 2.0 * (k + 1) * f3;
    f3 /= (double)((2 * k + 4) * (2 * k + 5));
  }
  return t;
}

// Â = 2^-J Ã_k on the lane's block and U_k = e^{μ_k} (p(Â))^{2^J} for NV slices at once (independent recurrences
// interleaved); rk[v]: the slice's record [Re e^μ, Im e^μ, 2^-J u_1, 2^-J u_2]; gen(j, e): entry e of Ã_j's block.
// P and J are uniform over the workgroup (k_blkseg_eval's phase 0).
template <int NB, int NV, typename GEN>
__device__ __forceinline__ void seg_form(GEN&& gen, const double* const (&rk)[NV], double s0, int P, int J,
                                         double (&ar)[NV][NB * NB], double (&ai)[NV][NB * NB], double (&ur)[NV][NB * NB],
                                         double (&ui)[NV][NB * NB]) {
  constexpr int E = NB * NB;
  double pr[NV], pi[NV], qr[NV], qi[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const double2 ph = *reinterpret_cast<const double2*>(rk[v]);
    const double2 su = *reinterpret_cast<const double2*>(rk[v] + 2);
    qr[v] = ph.x;
    qi[v] = ph.y;
    pr[v] = J ? 1.0 : ph.x;
    pi[v] = J ? 0.0 : ph.y;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double2 g0 = gen(0, e), g1 = gen(1, e), g2 = gen(2, e);
      ar[v][e] = fma(su.y, g2.x, fma(su.x, g1.x, s0 * g0.x));
      ai[v][e] = fma(su.y, g2.y, fma(su.x, g1.y, s0 * g0.y));
    }
  }
  if constexpr (NB == 2) {
    if (J == 0) {
      // blocks of 2 rows without halvings: the closed form.  Â is exactly skew-Hermitian (the host checks the
      // generators exactly; the scaled sums keep it so): Â = i t I + B with Â_00 = i (t + a), Â_11 = i (t - a),
      // B_01 = Â_01, B_10 = Â_10 = -conj(Â_01), B^2 = -ω^2 I, ω^2 = a^2 + |Â_01|^2, so
      //   exp(Â) = e^{i t} (cos ω I + (sin ω / ω) B)
      // with |t|, ω <= ρ <= θ_cap (the eigenvalues i (t ± ω) of Â lie within ±i ρ_k): both series to degree 19,
      // beyond the Taylor polynomial's P, so U_k agrees with it to rounding
      constexpr BlksegTrig T = blkseg_trig();
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const double t = 0.5 * (ai[v][0] + ai[v][3]), a = 0.5 * (ai[v][0] - ai[v][3]);
        const double w = fma(a, a, fma(ar[v][1], ar[v][1], ai[v][1] * ai[v][1])), t2 = t * t;
        double cw = 0.0, sw = 0.0, ct = 0.0, st = 0.0;
#pragma unroll
        for (int k = BLKSEG_KMAX; k >= 0; --k) {
          cw = fma(cw, w, T.c[k]);
          sw = fma(sw, w, T.s[k]);
          ct = fma(ct, t2, T.c[k]);
          st = fma(st, t2, T.s[k]);
        }
        st *= t;  // sin t
        // z = e^{μ_k} e^{i t};  U = z cos ω I + z sinc ω B
        const double zr = qr[v] * ct - qi[v] * st, zi = fma(qr[v], st, qi[v] * ct);
        const double cr = zr * cw, ci = zi * cw, sr = zr * sw, si = zi * sw;
        ur[v][0] = fma(-si, a, cr);
        ui[v][0] = fma(sr, a, ci);
        ur[v][3] = fma(si, a, cr);
        ui[v][3] = fma(-sr, a, ci);
        ur[v][1] = fma(sr, ar[v][1], -si * ai[v][1]);
        ui[v][1] = fma(sr, ai[v][1], si * ar[v][1]);
        ur[v][2] = fma(sr, ar[v][2], -si * ai[v][2]);
        ui[v][2] = fma(sr, ai[v][2], si * ar[v][2]);
      }
      return;
    }
  }
  blku_taylor<NB, NV>(ar, ai, P, pr, pi, nullptr, ur, ui);
  if (J) {  // squarings on the phase-free polynomial, then the phase
    for (int q = 0; q < J; ++q)
#pragma unroll
      for (int v = 0; v < NV; ++v) blku_square<NB>(ur[v], ui[v]);
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double vr = ur[v][e], vi = ui[v][e];
        ur[v][e] = qr[v] * vr - qi[v] * vi;
        ui[v][e] = qr[v] * vi + qi[v] * vr;
      }
  }
}

// Re tr(A_j M) for j = 1, 2 with M = Σ_{a+b<ORD} X^b K X^a / (a+b+1)! (blku_contract's recurrence: L_0 = R_0 = K,
// R_n = R_{n-1} X, L_n = X L_{n-1} + R_n, M = Σ_n L_n / (n+1)!) from the slice's X = A_k and the shifted generator
// blocks: A_j = Ã_j + μ_j I, so Re tr(A_j M) = Re tr(Ã_j M) + Re(μ_j tr M).  The traces are accumulated order by
// order (Re tr(A_j L_n) / (n+1)!), so that M is never held: three NB x NB matrices live (K -> L, R, X) instead of
// four.  K is overwritten.
template <int NB, typename GEN>
__device__ __forceinline__ void seg_trace(GEN&& gen, const double (&Lr)[NB * NB], const double (&Li)[NB * NB], double f,
                                          double m1r, double m1i, double m2r, double m2i, double& acc1, double& acc2) {
  double a1 = 0.0, a2 = 0.0, tr = 0.0, ti = 0.0;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    tr += Lr[i * NB + i];
    ti += Li[i * NB + i];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const double2 g1 = gen(1, i * NB + q), g2 = gen(2, i * NB + q);
      a1 = fma(g1.x, Lr[q * NB + i], fma(-g1.y, Li[q * NB + i], a1));
      a2 = fma(g2.x, Lr[q * NB + i], fma(-g2.y, Li[q * NB + i], a2));
    }
  }
  acc1 = fma(f, fma(m1r, tr, fma(-m1i, ti, a1)), acc1);
  acc2 = fma(f, fma(m2r, tr, fma(-m2i, ti, a2)), acc2);
}

// MACC: accumulate M = Σ_n L_n / (n+1)! and take the traces once (fewer flops, one more live matrix: blocks of 2
// rows); otherwise the traces order by order (blocks of 3 rows, where the registers are short)
template <int NB, int ORD, bool MACC, typename GEN>
__device__ __forceinline__ void seg_contract(GEN&& gen, const double (&xr_)[NB * NB], const double (&xi_)[NB * NB],
                                             double (&Lr)[NB * NB], double (&Li)[NB * NB], double m1r, double m1i,
                                             double m2r, double m2i, double& acc1, double& acc2) {
  constexpr int E = NB * NB;
  constexpr double invf[6] = {1.0, 1.0, 0.5, 1.0 / 6, 1.0 / 24, 1.0 / 120};
  acc1 = acc2 = 0.0;
  double Mr[MACC ? E : 1], Mi[MACC ? E : 1];
  if constexpr (MACC) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      Mr[e] = Lr[e];
      Mi[e] = Li[e];
    }
  } else {
    seg_trace<NB>(gen, Lr, Li, 1.0, m1r, m1i, m2r, m2i, acc1, acc2);
  }
  if constexpr (ORD > 1) {
    double Rr[E], Ri[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      Rr[e] = Lr[e];
      Ri[e] = Li[e];
    }
#pragma unroll
    for (int n = 1; n < ORD; ++n) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {  // R_n = R_{n-1} X, row by row in place
        double tr[NB], ti[NB];
#pragma unroll
        for (int kk = 0; kk < NB; ++kk) {
          double sr = 0.0, si = 0.0;
#pragma unroll
          for (int q = 0; q < NB; ++q) {
            sr = fma(Rr[i * NB + q], xr_[q * NB + kk], fma(-Ri[i * NB + q], xi_[q * NB + kk], sr));
            si = fma(Rr[i * NB + q], xi_[q * NB + kk], fma(Ri[i * NB + q], xr_[q * NB + kk], si));
          }
          tr[kk] = sr;
          ti[kk] = si;
        }
#pragma unroll
        for (int kk = 0; kk < NB; ++kk) {
          Rr[i * NB + kk] = tr[kk];
          Ri[i * NB + kk] = ti[kk];
        }
      }
#pragma unroll
      for (int kk = 0; kk < NB; ++kk) {  // L_n = X L_{n-1} + R_n, column by column in place
        double tr[NB], ti[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          double sr = Rr[i * NB + kk], si = Ri[i * NB + kk];
#pragma unroll
          for (int q = 0; q < NB; ++q) {
            sr = fma(xr_[i * NB + q], Lr[q * NB + kk], fma(-xi_[i * NB + q], Li[q * NB + kk], sr));
            si = fma(xr_[i * NB + q], Li[q * NB + kk], fma(xi_[i * NB + q], Lr[q * NB + kk], si));
          }
          tr[i] = sr;
          ti[i] = si;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          Lr[i * NB + kk] = tr[i];
          Li[i * NB + kk] = ti[i];
          if constexpr (MACC) {
            Mr[i * NB + kk] = fma(invf[n + 1], tr[i], Mr[i * NB + kk]);
            Mi[i * NB + kk] = fma(invf[n + 1], ti[i], Mi[i * NB + kk]);
          }
        }
      }
      if constexpr (!MACC) seg_trace<NB>(gen, Lr, Li, invf[n + 1], m1r, m1i, m2r, m2i, acc1, acc2);
    }
  }
  if constexpr (MACC) seg_trace<NB>(gen, Mr, Mi, 1.0, m1r, m1i, m2r, m2i, acc1, acc2);
}

// ---- blocks of 2 rows, exactly skew-Hermitian: [[i d0, r + i q], [-r + i q, i d1]] (4 reals instead of 8) ----
struct Sk2 {
  double d0, d1, r, q;
};
__device__ __forceinline__ Sk2 sk2_of(const double2 (&e)[4]) { return Sk2{e[0].y, e[3].y, e[1].x, e[1].y}; }

// cos t and sin t of the block's mean diagonal t = (d0 + d1) / 2 (sk2_form's series)
template <int K = BLKSEG_KMAX>
__device__ __forceinline__ void sk2_phase(double d0, double d1, double& ct, double& st) {
  constexpr BlksegTrig T = blkseg_trig();
  const double t = 0.5 * (d0 + d1), t2 = t * t;
  ct = T.c[K];  // (the Horner chains start at the top coefficient: fma(0, x, c) = c)
  st = T.s[K];
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    ct = fma(ct, t2, T.c[k]);
    st = fma(st, t2, T.s[k]);
  }
  st *= t;
}
// ZD with constant shifts: z = e^{μ_0} e^{it} of the lane's block, the same in every slice (rec[0..1]: e^{μ_0})
template <int K = BLKSEG_KMAX>
__device__ __forceinline__ void sk2_z(const Sk2& g0, const double* rec, double& zr, double& zi) {
  double ct, st;
  sk2_phase<K>(g0.d0, g0.d1, ct, st);
  const double2 ph = *reinterpret_cast<const double2*>(rec);
  zr = ph.x * ct - ph.y * st;
  zi = fma(ph.x, st, ph.y * ct);
}
// Â = Ã_0 + u_1 Ã_1 + u_2 Ã_2 (no halvings) and U = e^{μ_k} exp(Â) in the closed form of seg_form (ph = e^{μ_k}).
// EX (the exact contraction, sk2_contract_exact): also hands out ex = [cos ω, sinc ω, s3(ω), Re z, Im z], s3 from a
// third Horner chain beside the two
template <int K = BLKSEG_KMAX, bool EX = false>
__device__ __forceinline__ void sk2_form(const Sk2 (&g)[3], double2 ph, double2 u, Sk2& ah, double (&ur)[4],
                                         double (&ui)[4], double* ex = nullptr) {
  constexpr BlksegTrig T = blkseg_trig();
  ah.d0 = fma(u.y, g[2].d0, fma(u.x, g[1].d0, g[0].d0));
  ah.d1 = fma(u.y, g[2].d1, fma(u.x, g[1].d1, g[0].d1));
  ah.r = fma(u.y, g[2].r, fma(u.x, g[1].r, g[0].r));
  ah.q = fma(u.y, g[2].q, fma(u.x, g[1].q, g[0].q));
  const double a = 0.5 * (ah.d0 - ah.d1);
  const double w = fma(a, a, fma(ah.r, ah.r, ah.q * ah.q));
  double cw = T.c[K], sw = T.s[K], s3 = EX ? T.d[K] : 0.0, ct, st;
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    cw = fma(cw, w, T.c[k]);
    sw = fma(sw, w, T.s[k]);
    if constexpr (EX) s3 = fma(s3, w, T.d[k]);
  }
  sk2_phase<K>(ah.d0, ah.d1, ct, st);
  // z = e^{μ_k} e^{it}
  const double zr = ph.x * ct - ph.y * st, zi = fma(ph.x, st, ph.y * ct);
  const double cr = zr * cw, ci = zi * cw, sr = zr * sw, si = zi * sw;
  if constexpr (EX) {
    ex[0] = cw;
    ex[1] = sw;
    ex[2] = s3;
    ex[3] = zr;
    ex[4] = zi;
  }
  ur[0] = fma(-si, a, cr);
  ui[0] = fma(sr, a, ci);
  ur[3] = fma(si, a, cr);
  ui[3] = fma(-sr, a, ci);
  ur[1] = fma(sr, ah.r, -si * ah.q);  // z sinc(ω) (r + i q)
  ui[1] = fma(sr, ah.q, si * ah.r);
  ur[2] = fma(-sr, ah.r, -si * ah.q);  // z sinc(ω) (-r + i q)
  ui[2] = fma(sr, ah.q, -si * ah.r);
}
// ZD: the control generators' blocks have zero diagonals and no shifts, and Re μ_0 = 0, so Â's diagonal is Ã_0's and
// z = e^{μ_k} e^{it} is one unimodular constant of the lane's block (sk2_z) in every slice: U_k = z V_k with
//   V_k = cos ω I + sinc ω (Â - i t I) = [[α, β], [-β̄, ᾱ]] in SU(2),  α = cos ω + i sinc ω a,  β = sinc ω (r + i q)
// (a = a0, the block's constant half-difference).  The slice loops run on V alone, v = (Re α, Im α, Re β, Im β):
// products of SU(2) matrices stay of that form in phase 1, and phase 3 moves Ĝ = z̄ G, for which K_k = U_k^H G_{k+1} =
// V_k^H Ĝ_{k+1} (the same K) and Ĝ_k = K_k V_k.  z enters once per lane: z^Nt on x_N, z̄ on G at the segment's end.
// EX: ex = [cos ω, sinc ω, s3(ω), Re z, Im z] as sk2_form's (zr, zi: the lane's z)
template <int K = BLKSEG_KMAX, bool EX = false>
__device__ __forceinline__ void sk2_form_v(const Sk2 (&g)[3], double2 u, double a0, Sk2& ah, double (&v)[4],
                                           double zr = 1.0, double zi = 0.0, double* ex = nullptr) {
  constexpr BlksegTrig T = blkseg_trig();
  ah.d0 = g[0].d0;  // (u_j times a zero diagonal adds nothing)
  ah.d1 = g[0].d1;
  ah.r = fma(u.y, g[2].r, fma(u.x, g[1].r, g[0].r));
  ah.q = fma(u.y, g[2].q, fma(u.x, g[1].q, g[0].q));
  const double w = fma(a0, a0, fma(ah.r, ah.r, ah.q * ah.q));
  double cw = T.c[K], sw = T.s[K], s3 = EX ? T.d[K] : 0.0;
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    cw = fma(cw, w, T.c[k]);
    sw = fma(sw, w, T.s[k]);
    if constexpr (EX) s3 = fma(s3, w, T.d[k]);
  }
  if constexpr (EX) {
    ex[0] = cw;
    ex[1] = sw;
    ex[2] = s3;
    ex[3] = zr;
    ex[4] = zi;
  }
  v[0] = cw;
  v[1] = sw * a0;
  v[2] = sw * ah.r;
  v[3] = sw * ah.q;
}
// the 2 x 2 matrix of v: [[α, β], [-β̄, ᾱ]] (negations only)
__device__ __forceinline__ void sk2_expand(const double (&v)[4], double (&mr)[4], double (&mi)[4]) {
  mr[0] = v[0];
  mi[0] = v[1];
  mr[1] = v[2];
  mi[1] = v[3];
  mr[2] = -v[2];
  mi[2] = v[3];
  mr[3] = v[0];
  mi[3] = -v[1];
}
// p <- v p on SU(2) matrices in that form (p = (Re p, Im p, Re y, Im y)): p' = α p - β ȳ, y' = α y + β p̄
__device__ __forceinline__ void sk2_vmul(const double (&v)[4], const double (&p)[4], double (&t)[4]) {
  t[0] = fma(v[0], p[0], fma(-v[1], p[1], fma(-v[2], p[2], -v[3] * p[3])));
  t[1] = fma(v[0], p[1], fma(v[1], p[0], fma(v[2], p[3], -v[3] * p[2])));
  t[2] = fma(v[0], p[2], fma(-v[1], p[3], fma(v[2], p[0], v[3] * p[1])));
  t[3] = fma(v[0], p[3], fma(v[1], p[2], fma(-v[2], p[1], v[3] * p[0])));
}

// ---- phase 3 of the phase-free loops in the Pauli basis (orders 1..3, no penalty) ----
// V = v0 I + i n.σ with v = (v0, n3, n2, n1) as sk2_form_v returns it, and Ĝ = g0 I + g.σ (g0 complex, g a complex
// 3-vector), carried doubled as gp = (2 Re g0, 2 Im g0, 2 Re g[1..3], 2 Im g[1..3]): every map below is linear in Ĝ,
// and sk2_contract_pauli takes K doubled.  With d = n.g and t = n x g
//   K = V^H Ĝ:    k0 = v0 g0 - i d,  k = v0 g - i g0 n + t
//   Ĝ' = V^H Ĝ V: g0' = g0 (nothing to compute),  g' = g + 2 (v0 t + n x t)   (|V| = 1 used: v0² + |n|² = 1)
// t is shared between K and the rotation and no matrix is formed: 30 + 22 fp64 instructions at order 3 against the
// two general 2 x 2 products' 64 and the seven additions that turned K into its Pauli components (DESIGN.md §4 round
// 10; checked against the matrix products in tests/test_blkseg_pauli_algebra.py).
// The doubled Pauli components of a 2 x 2 matrix (row-major entries)
__device__ __forceinline__ void sk2_pauli_of(const double (&mr)[4], const double (&mi)[4], double (&gp)[8]) {
  gp[0] = mr[0] + mr[3];
  gp[1] = mi[0] + mi[3];
  gp[2] = mr[1] + mr[2];
  gp[3] = mi[2] - mi[1];
  gp[4] = mr[0] - mr[3];
  gp[5] = mi[1] + mi[2];
  gp[6] = mr[1] - mr[2];
  gp[7] = mi[0] - mi[3];
}
// t = n x g (tc = Re t[1..3], Im t[1..3]) and the doubled Pauli components of K = V^H Ĝ that the order-ORD contraction
// reads, kc = (Re k0, Im k0, Re k1, Im k1, Re k2, Im k2, Im k3): order 1 Im k1, Im k2; order 2 also Re k0, Re k1,
// Re k2; order 3 also Im k0, Im k3.  The others are left alone.
template <int ORD>
__device__ __forceinline__ void sk2_pauli_k(const double (&v)[4], const double (&gp)[8], double (&tc)[6],
                                            double (&kc)[7]) {
  const double v0 = v[0], n1 = v[3], n2 = v[2], n3 = v[1];
  const double* a = gp + 1;  // a[1..3] = 2 Re g, b[1..3] = 2 Im g
  const double* b = gp + 4;
  tc[0] = fma(n2, a[3], -n3 * a[2]);
  tc[1] = fma(n3, a[1], -n1 * a[3]);
  tc[2] = fma(n1, a[2], -n2 * a[1]);
  tc[3] = fma(n2, b[3], -n3 * b[2]);
  tc[4] = fma(n3, b[1], -n1 * b[3]);
  tc[5] = fma(n1, b[2], -n2 * b[1]);
  kc[3] = fma(v0, b[1], fma(-gp[0], n1, tc[3]));
  kc[5] = fma(v0, b[2], fma(-gp[0], n2, tc[4]));
  if constexpr (ORD >= 2) {
    const double di = fma(n3, b[3], fma(n2, b[2], n1 * b[1]));
    kc[0] = fma(v0, gp[0], di);
    kc[2] = fma(v0, a[1], fma(gp[1], n1, tc[0]));
    kc[4] = fma(v0, a[2], fma(gp[1], n2, tc[1]));
  }
  if constexpr (ORD >= 3) {
    const double dr = fma(n3, a[3], fma(n2, a[2], n1 * a[1]));
    kc[1] = fma(v0, gp[1], -dr);
    kc[6] = fma(v0, b[3], fma(-gp[0], n3, tc[5]));
  }
}
// g' = g + 2 (v0 t + n x t) on the six reals of g (gn = gp[2..7] rotated; g0 stays)
__device__ __forceinline__ void sk2_pauli_rot(const double (&v)[4], const double (&tc)[6], const double (&gp)[8],
                                              double (&gn)[6]) {
  const double w0 = 2.0 * v[0], m1 = 2.0 * v[3], m2 = 2.0 * v[2], m3 = 2.0 * v[1];
#pragma unroll
  for (int c = 0; c < 2; ++c) {  // real and imaginary parts
    const double t1 = tc[3 * c], t2 = tc[3 * c + 1], t3 = tc[3 * c + 2];
    gn[3 * c] = fma(m2, t3, fma(-m3, t2, fma(w0, t1, gp[2 + 3 * c])));
    gn[3 * c + 1] = fma(m3, t1, fma(-m1, t3, fma(w0, t2, gp[3 + 3 * c])));
    gn[3 * c + 2] = fma(m1, t2, fma(-m2, t1, fma(w0, t3, gp[4 + 3 * c])));
  }
}

// R <- R X in place, X skew-Hermitian (x0, x1, yr + i yq): 12 FMAs per row instead of 16
__device__ __forceinline__ void sk2_rx(double (&Rr)[4], double (&Ri)[4], const Sk2& x) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double p0r = Rr[2 * i], p0i = Ri[2 * i], p1r = Rr[2 * i + 1], p1i = Ri[2 * i + 1];
    Rr[2 * i] = fma(-p0i, x.d0, fma(-p1r, x.r, -p1i * x.q));
    Ri[2 * i] = fma(p0r, x.d0, fma(p1r, x.q, -p1i * x.r));
    Rr[2 * i + 1] = fma(p0r, x.r, fma(-p0i, x.q, -p1i * x.d1));
    Ri[2 * i + 1] = fma(p0r, x.q, fma(p0i, x.r, p1r * x.d1));
  }
}
// L <- X L + R in place, X skew-Hermitian
__device__ __forceinline__ void sk2_xlr(double (&Lr)[4], double (&Li)[4], const double (&Rr)[4], const double (&Ri)[4],
                                        const Sk2& x) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double c0r = Lr[k], c0i = Li[k], c1r = Lr[2 + k], c1i = Li[2 + k];
    Lr[k] = fma(-x.d0, c0i, fma(x.r, c1r, fma(-x.q, c1i, Rr[k])));
    Li[k] = fma(x.d0, c0r, fma(x.r, c1i, fma(x.q, c1r, Ri[k])));
    Lr[2 + k] = fma(-x.r, c0r, fma(-x.q, c0i, fma(-x.d1, c1i, Rr[2 + k])));
    Li[2 + k] = fma(-x.r, c0i, fma(x.q, c0r, fma(x.d1, c1r, Ri[2 + k])));
  }
}
// Re tr(A_j M) for j = 1, 2 with M = Σ_{a+b<ORD} X^b K X^a / (a+b+1)! (seg_contract's recurrence on skew X) and
// A_j = Ã_j + i m_j I: -(d0 + m) Im M00 - (d1 + m) Im M11 + r (Re M10 - Re M01) - q (Im M10 + Im M01); e_j = (d0 + m,
// d1 + m, r, q) of each generator.  K is overwritten.
template <int ORD>
__device__ __forceinline__ void sk2_contract(const Sk2& x, const Sk2& e1, const Sk2& e2, double (&Lr)[4],
                                             double (&Li)[4], double& acc1, double& acc2) {
  constexpr double invf[6] = {1.0, 1.0, 0.5, 1.0 / 6, 1.0 / 24, 1.0 / 120};
  double Mr[4], Mi[4], Rr[4], Ri[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    Mr[e] = Rr[e] = Lr[e];
    Mi[e] = Ri[e] = Li[e];
  }
#pragma unroll
  for (int n = 1; n < ORD; ++n) {
    sk2_rx(Rr, Ri, x);
    sk2_xlr(Lr, Li, Rr, Ri, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      Mr[e] = fma(invf[n + 1], Lr[e], Mr[e]);
      Mi[e] = fma(invf[n + 1], Li[e], Mi[e]);
    }
  }
  const double dr = Mr[2] - Mr[1], di = Mi[2] + Mi[1];
  acc1 = fma(-e1.d0, Mi[0], fma(-e1.d1, Mi[3], fma(e1.r, dr, -e1.q * di)));
  acc2 = fma(-e2.d0, Mi[0], fma(-e2.d1, Mi[3], fma(e2.r, dr, -e2.q * di)));
}

// The same traces for ORD <= 3 in the Pauli basis.  With X = i(x0 I + x.σ) (x real: x0 = (d0 + d1)/2, x = (q, r,
// (d0 - d1)/2)), K = k0 I + k.σ (complex) and A_j = i(a0 I + a.σ), Re tr(A_j M) = -2 (a0 Im m0 + a.Im m), and the
// order-ORD M = Σ_{a+b<ORD} X^b K X^a / (a+b+1)! has (d = x.k, ω² = |x|²)
//   ORD 2: Im m0 = Im k0 + x0 Re k0 + Re d,  Im m = Im k + x0 Re k + Re k0 x
//   ORD 3: Im m0 = (1 - (x0² + ω²)/2) Im k0 + x0 (Re k0 - Im d) + Re d,
//          Im m = (1 - x0²/2 - ω²/6) Im k + x0 Re k + (Re k0 - x0 Im k0 - Im d / 3) x
// (the Pauli products (x.σ)(k.σ)(x.σ) = 2 (x.k) x.σ - ω² k.σ etc.; checked against the matrix recurrence in numpy).
// ~73 flops instead of sk2_contract's 224 at order 3.  aj: the generators' Pauli vectors times 2 (pre-scaled so that
// the K components below can stay doubled: 2 k0 = K00 + K11, ...) times the trace's -1/2 (sk2_pauli2).
// CX: X's diagonal is the same in every slice (zero-diagonal controls, zero control shifts): x0, x3 and x0² come
// precomputed (x0c, x3c, x02c: the same values)
// The CX traces from K's doubled Pauli components as they are, kc = (Re k0, Im k0, Re k1, Im k1, Re k2, Im k2, Im k3)
// (sk2_pauli_k forms them without a matrix); order 1 reads Im k1, Im k2, order 2 also Re k0, Re k1, Re k2, order 3 all.
// Zero-diagonal controls without shifts: a1[0] = a1[3] = a2[0] = a2[3] = 0 exactly, so m0 and m3 (and Re d, 2 Re k3
// and al0, which feed nothing else) are not formed: they entered the sums as products with exact zeros added to
// finite values, so the traces are the same bits
template <int ORD>
__device__ __forceinline__ void sk2_contract_pauli_k(double x1, double x2, const double (&a1)[4],
                                                     const double (&a2)[4], const double (&kc)[7], double& acc1,
                                                     double& acc2, double x0c, double x3c, double x02c) {
  static_assert(ORD >= 1 && ORD <= 3, "Pauli form for orders 1..3");
  const double k1i = kc[3], k2i = kc[5];
  double m1, m2;
  if constexpr (ORD == 1) {
    m1 = k1i;
    m2 = k2i;
  } else {
    const double k0r = kc[0], k1r = kc[2], k2r = kc[4];
    if constexpr (ORD == 2) {
      m1 = fma(x0c, k1r, fma(k0r, x1, k1i));
      m2 = fma(x0c, k2r, fma(k0r, x2, k2i));
    } else {
      const double k0i = kc[1], k3i = kc[6];
      const double di = fma(x3c, k3i, fma(x2, k2i, x1 * k1i));
      const double w = fma(x3c, x3c, fma(x2, x2, x1 * x1));
      const double al1 = fma(-0.5, x02c, fma(-1.0 / 6.0, w, 1.0));
      const double c = fma(-x0c, k0i, fma(-1.0 / 3.0, di, k0r));
      m1 = fma(al1, k1i, fma(x0c, k1r, c * x1));
      m2 = fma(al1, k2i, fma(x0c, k2r, c * x2));
    }
  }
  acc1 = fma(a1[2], m2, a1[1] * m1);
  acc2 = fma(a2[2], m2, a2[1] * m1);
}
template <int ORD, bool CX = false>
__device__ __forceinline__ void sk2_contract_pauli(const Sk2& x, const double (&a1)[4], const double (&a2)[4],
                                                   const double (&Kr)[4], const double (&Ki)[4], double& acc1,
                                                   double& acc2, double x0c = 0.0, double x3c = 0.0,
                                                   double x02c = 0.0) {
  static_assert(ORD >= 1 && ORD <= 3, "Pauli form for orders 1..3");
  // doubled Pauli components of K: 2k0 = K00 + K11, 2k1 = K01 + K10, 2k2 = i (K01 - K10), 2k3 = K00 - K11
  const double k0i = Ki[0] + Ki[3], k1i = Ki[1] + Ki[2], k2i = Kr[1] - Kr[2], k3i = Ki[0] - Ki[3];
  if constexpr (CX) {
    double kc[7] = {0.0, k0i, 0.0, k1i, 0.0, k2i, k3i};
    if constexpr (ORD >= 2) {
      kc[0] = Kr[0] + Kr[3];
      kc[2] = Kr[1] + Kr[2];
      kc[4] = Ki[2] - Ki[1];
    }
    sk2_contract_pauli_k<ORD>(x.q, x.r, a1, a2, kc, acc1, acc2, x0c, x3c, x02c);
    return;
  }
  double m0, m1, m2, m3;  // 2 Im m
  if constexpr (ORD == 1) {
    m0 = k0i;
    m1 = k1i;
    m2 = k2i;
    m3 = k3i;
  } else {
    const double k0r = Kr[0] + Kr[3], k1r = Kr[1] + Kr[2], k2r = Ki[2] - Ki[1], k3r = Kr[0] - Kr[3];
    const double x0 = CX ? x0c : 0.5 * (x.d0 + x.d1), x1 = x.q, x2 = x.r, x3 = CX ? x3c : 0.5 * (x.d0 - x.d1);
    const double dr = fma(x3, k3r, fma(x2, k2r, x1 * k1r)), di = fma(x3, k3i, fma(x2, k2i, x1 * k1i));
    if constexpr (ORD == 2) {
      m0 = fma(x0, k0r, k0i + dr);
      m1 = fma(x0, k1r, fma(k0r, x1, k1i));
      m2 = fma(x0, k2r, fma(k0r, x2, k2i));
      m3 = fma(x0, k3r, fma(k0r, x3, k3i));
    } else {
      const double w = fma(x3, x3, fma(x2, x2, x1 * x1)), x02 = CX ? x02c : x0 * x0;
      const double al0 = fma(-0.5, x02 + w, 1.0), al1 = fma(-0.5, x02, fma(-1.0 / 6.0, w, 1.0));
      m0 = fma(al0, k0i, fma(x0, k0r - di, dr));
      const double c = fma(-x0, k0i, fma(-1.0 / 3.0, di, k0r));
      m1 = fma(al1, k1i, fma(x0, k1r, c * x1));
      m2 = fma(al1, k2i, fma(x0, k2r, c * x2));
      m3 = fma(al1, k3i, fma(x0, k3r, c * x3));
    }
  }
  // -2 a.Im m: aj holds -(2 a) / 2 (sk2_pauli2), m holds 2 Im m, so the trace is aj.m
  acc1 = fma(a1[3], m3, fma(a1[2], m2, fma(a1[1], m1, a1[0] * m0)));
  acc2 = fma(a2[3], m3, fma(a2[2], m2, fma(a2[1], m1, a2[0] * m0)));
}
// doubled Pauli vector of an Sk2 generator block times -1/2 (sk2_contract_pauli's aj: the trace's -1/2 folded in
// where the vector is built, once per lane; a power of two, so every product and sum rounds as before)
__device__ __forceinline__ void sk2_pauli2(const Sk2& e, double (&a)[4]) {
  a[0] = -0.5 * (e.d0 + e.d1);
  a[1] = -0.5 * (2.0 * e.q);
  a[2] = -0.5 * (2.0 * e.r);
  a[3] = -0.5 * (e.d0 - e.d1);
}

// The exact (Fréchet) traces in the same basis: the whole series M = Σ_{a,b >= 0} X^b K X^a / (a+b+1)! =
// ∫_0^1 e^{sX} K e^{(1-s)X} ds.  With z = e^{i x0} (sk2_form's e^{μ_k} e^{it}: x0 = t + Im μ_k), d = x.k and
// s3 = (sinc ω - cos ω) / ω²,
//   M = z { [cos ω k0 + i sinc ω d] I + [sinc ω k + (i sinc ω k0 - s3 d) x].σ }
// (e^{sX} = e^{i s x0} (cos sω + i sin sω x.σ / ω); the products of sines and cosines integrate to sinc, cos and s3;
// at ω -> 0 it reduces to the order-3 form above).  ex: sk2_form's [cos ω, sinc ω, s3, Re z, Im z].  CX: x3 precomputed.
template <bool CX = false>
__device__ __forceinline__ void sk2_contract_exact(const Sk2& x, const double (&a1)[4], const double (&a2)[4],
                                                   const double (&Kr)[4], const double (&Ki)[4], const double (&ex)[5],
                                                   double& acc1, double& acc2, double x3c = 0.0) {
  const double cw = ex[0], sw = ex[1], s3 = ex[2], zr = ex[3], zi = ex[4];
  const double k0i = Ki[0] + Ki[3], k1i = Ki[1] + Ki[2], k2i = Kr[1] - Kr[2], k3i = Ki[0] - Ki[3];
  const double k0r = Kr[0] + Kr[3], k1r = Kr[1] + Kr[2], k2r = Ki[2] - Ki[1], k3r = Kr[0] - Kr[3];
  const double x1 = x.q, x2 = x.r, x3 = CX ? x3c : 0.5 * (x.d0 - x.d1);
  const double dr = fma(x3, k3r, fma(x2, k2r, x1 * k1r)), di = fma(x3, k3i, fma(x2, k2i, x1 * k1i));
  // n = M / z (doubled, like K): n0 = cos ω k0 + i sinc ω d, n = sinc ω k + c x with c = i sinc ω k0 - s3 d
  const double cr = -fma(sw, k0i, s3 * dr), ci = fma(sw, k0r, -s3 * di);
  // 2 Im m = Re z Im n + Im z Re n
  const double m1 = fma(zr, fma(sw, k1i, ci * x1), zi * fma(sw, k1r, cr * x1));
  const double m2 = fma(zr, fma(sw, k2i, ci * x2), zi * fma(sw, k2r, cr * x2));
  if constexpr (CX) {  // a1[0] = a1[3] = a2[0] = a2[3] = 0 exactly (sk2_contract_pauli): n0, m0 and m3 are not formed
    acc1 = fma(a1[2], m2, a1[1] * m1);
    acc2 = fma(a2[2], m2, a2[1] * m1);
  } else {
    const double n0r = fma(cw, k0r, -sw * di), n0i = fma(cw, k0i, sw * dr);
    const double m0 = fma(zr, n0i, zi * n0r);
    const double m3 = fma(zr, fma(sw, k3i, ci * x3), zi * fma(sw, k3r, cr * x3));
    acc1 = fma(a1[3], m3, fma(a1[2], m2, fma(a1[1], m1, a1[0] * m0)));
    acc2 = fma(a2[3], m3, fma(a2[2], m2, fma(a2[1], m1, a2[0] * m0)));
  }
}

// ---- the exact traces on the generic path (blocks of 3 rows; blocks of 2 rows with halvings) ----
// R <- R X, row by row in place
template <int NB>
__device__ __forceinline__ void seg_rx(double (&Rr)[NB * NB], double (&Ri)[NB * NB], const double (&xr_)[NB * NB],
                                       const double (&xi_)[NB * NB]) {
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    double tr[NB], ti[NB];
#pragma unroll
    for (int kk = 0; kk < NB; ++kk) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        sr = fma(Rr[i * NB + q], xr_[q * NB + kk], fma(-Ri[i * NB + q], xi_[q * NB + kk], sr));
        si = fma(Rr[i * NB + q], xi_[q * NB + kk], fma(Ri[i * NB + q], xr_[q * NB + kk], si));
      }
      tr[kk] = sr;
      ti[kk] = si;
    }
#pragma unroll
    for (int kk = 0; kk < NB; ++kk) {
      Rr[i * NB + kk] = tr[kk];
      Ri[i * NB + kk] = ti[kk];
    }
  }
}
// L <- X L + R, column by column in place
template <int NB>
__device__ __forceinline__ void seg_xlr(double (&Lr)[NB * NB], double (&Li)[NB * NB], const double (&Rr)[NB * NB],
                                        const double (&Ri)[NB * NB], const double (&xr_)[NB * NB],
                                        const double (&xi_)[NB * NB]) {
#pragma unroll
  for (int kk = 0; kk < NB; ++kk) {
    double tr[NB], ti[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      double sr = Rr[i * NB + kk], si = Ri[i * NB + kk];
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        sr = fma(xr_[i * NB + q], Lr[q * NB + kk], fma(-xi_[i * NB + q], Li[q * NB + kk], sr));
        si = fma(xr_[i * NB + q], Li[q * NB + kk], fma(xi_[i * NB + q], Lr[q * NB + kk], si));
      }
      tr[i] = sr;
      ti[i] = si;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      Lr[i * NB + kk] = tr[i];
      Li[i * NB + kk] = ti[i];
    }
  }
}
// Re tr(A_j M) for j = 1, 2 with the whole series M = Σ_n L_n / (n+1)! (seg_contract's recurrence), nex orders in a
// rolled loop (nex uniform over the workgroup: blkseg_exact_terms of the seed's largest ρ_k).  The scalar part of
// X = A_k = Ã_k + μ_k I commutes, M(A_k; K) = e^{μ_k} M(Ã_k; K) = M(Ã_k; e^{μ_k} K): x is the shifted Ã_k, whose
// spectral half-width the records bound, and K takes the factor (er, ei) = e^{μ_k} first, so that the real traces of
// seg_trace serve.  The traces are accumulated order by order (three matrices live: K -> L, R, X).  genf(): the generator blocks' accessor, made anew in every pass so that the
// blocks read from LDS are not hoisted out of the loop.  K is overwritten.
template <int NB, typename GENF>
__device__ __forceinline__ void seg_contract_exact(GENF&& genf, const double (&xr_)[NB * NB], const double (&xi_)[NB * NB],
                                                   double (&Lr)[NB * NB], double (&Li)[NB * NB], int nex, double er,
                                                   double ei, double m1r, double m1i, double m2r, double m2i,
                                                   double& acc1, double& acc2) {
  constexpr int E = NB * NB;
  double Rr[E], Ri[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const double vr = Lr[e], vi = Li[e];
    Lr[e] = Rr[e] = er * vr - ei * vi;
    Li[e] = Ri[e] = fma(er, vi, ei * vr);
  }
  acc1 = acc2 = 0.0;
  seg_trace<NB>(genf(), Lr, Li, 1.0, m1r, m1i, m2r, m2i, acc1, acc2);
  double f = 1.0;  // 1 / (n+1)!
#pragma unroll 1
  for (int n = 1; n < nex; ++n) {
    seg_rx<NB>(Rr, Ri, xr_, xi_);
    seg_xlr<NB>(Lr, Li, Rr, Ri, xr_, xi_);
    f /= (double)(n + 1);
    seg_trace<NB>(genf(), Lr, Li, f, m1r, m1i, m2r, m2i, acc1, acc2);
  }
}

__device__ __forceinline__ double block_max(double v, double* scratch) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) scratch[w] = v;
  __syncthreads();
  double s = scratch[0];
  const int nw = (blockDim.x + 63) >> 6;
  for (int i = 1; i < nw; ++i) s = fmax(s, scratch[i]);
  __syncthreads();
  return s;
}

// wave-private LDS traffic between lanes of one wave: program order is LDS order within a wave; this keeps the
// compiler from moving accesses across the exchange
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Waves w, w + 4, w + 8 of a workgroup share a SIMD, and the oldest one wins the VALU issue arbitration: it would
// finish its segments far ahead and leave its partners alone on the SIMD at the end of each phase.  The partners
// take the priority in turns, one slice-step each.
__device__ __forceinline__ void seg_turn(int grp, int ngrp, int jj) {
  if ((grp + jj) % ngrp == 0) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}
// SIMD partners by progress (QOC_PROBE builds: g_seg_turnmode 1): each wave posts its step count in LDS and runs the
// next step at the higher issue priority when its partner (w ^ 4) is ahead (ties: the younger wave, which loses the
// arbitration otherwise).  The partner's count is read at the end of a step for the next one.  DEFER: it stays in the
// vector register it was loaded into until the next step makes it uniform, so that the read's latency hides behind
// the step; otherwise the readfirstlane follows the read and waits for it at once (an LDS round trip per step).  The
// deferred form costs one vector register over the loops: the instances that have none to give (blocks of 3 rows at
// 256 VGPRs with scratch, the forward half) keep the other.
template <bool DEFER>
struct SegProg {
  int* prog;
  int partner, other;  // other: the partner's count (DEFER: as loaded, uniform in value but not yet scalar)
  bool on, young;
  __device__ __forceinline__ void step(int t) {
    if (!on) return;
    const int o = DEFER ? __builtin_amdgcn_readfirstlane(other) : other;
    if (o > t || (o == t && young)) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
    prog[threadIdx.x >> 6] = t;
    other = DEFER ? prog[partner] : __builtin_amdgcn_readfirstlane(prog[partner]);
  }
};

// ---- the guard-state penalty (PEN) ----
// H += Σ_{i in pm} v_i^H v_i over the penalised rows v_i of the running product V (V^H Π V, Π the block's projector)
template <int NB>
__device__ __forceinline__ void seg_pen_acc(int pm, const double (&vr)[NB * NB], const double (&vi)[NB * NB],
                                            double (&hr)[NB * NB], double (&hi)[NB * NB]) {
#pragma unroll
  for (int i = 0; i < NB; ++i)
    if ((pm >> i) & 1) {
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int q = 0; q < NB; ++q) {
          const double ar = vr[i * NB + a], ai = vi[i * NB + a], br = vr[i * NB + q], bi = vi[i * NB + q];
          hr[a * NB + q] = fma(ar, br, fma(ai, bi, hr[a * NB + q]));
          hi[a * NB + q] = fma(ar, bi, fma(-ai, br, hi[a * NB + q]));
        }
    }
}
// One slice of the penalty in phase 3, D in LDS (entry e at dp[e stride]): G += f D Π on the penalised columns of D
// (the source 2 μ x_k[P, C] of λ_k in G_k = Σ_c x_k λ_k^H), then D <- U^H D U.  D is read column by column (T = D U
// accumulated) and written back row by row (U^H T), so that beside U and G only T is live.
// CF: the factor is complex, f + i fi (the phase-free loops: G stands for Ĝ = z̄ G, the source becomes z̄ 2 μ D Π, and
// U for V, which conjugates D as U does)
template <int NB, bool CF = false>
__device__ __forceinline__ void seg_pen_step(int pm, double f, double2* dp, int stride, const double (&ur)[NB * NB],
                                             const double (&ui)[NB * NB], double (&gr)[NB * NB], double (&gi)[NB * NB],
                                             double fi = 0.0) {
  double tr[NB * NB], ti[NB * NB];
#pragma unroll
  for (int e = 0; e < NB * NB; ++e) tr[e] = ti[e] = 0.0;
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    double2 c[NB];
#pragma unroll
    for (int a = 0; a < NB; ++a) c[a] = dp[(a * NB + q) * stride];
    if ((pm >> q) & 1) {
#pragma unroll
      for (int a = 0; a < NB; ++a) {
        if constexpr (CF) {
          gr[a * NB + q] = fma(f, c[a].x, fma(-fi, c[a].y, gr[a * NB + q]));
          gi[a * NB + q] = fma(f, c[a].y, fma(fi, c[a].x, gi[a * NB + q]));
        } else {
          gr[a * NB + q] = fma(f, c[a].x, gr[a * NB + q]);
          gi[a * NB + q] = fma(f, c[a].y, gi[a * NB + q]);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        tr[a * NB + j] = fma(c[a].x, ur[q * NB + j], fma(-c[a].y, ui[q * NB + j], tr[a * NB + j]));
        ti[a * NB + j] = fma(c[a].x, ui[q * NB + j], fma(c[a].y, ur[q * NB + j], ti[a * NB + j]));
      }
  }
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        sr = fma(ur[q * NB + i], tr[q * NB + j], fma(ui[q * NB + i], ti[q * NB + j], sr));
        si = fma(ur[q * NB + i], ti[q * NB + j], fma(-ui[q * NB + i], tr[q * NB + j], si));
      }
      dp[(i * NB + j) * stride] = make_double2(sr, si);
    }
}

// a value every lane of the wave holds alike, moved to scalar registers
__device__ __forceinline__ double seg_uniform(double x) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll)), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// a value computed alike in every lane (a product of uniform values, say), moved to scalar registers: through an
// opaque vector register, because the compiler drops the readfirstlane of a value it knows to be uniform and then
// keeps the result in vector registers
__device__ __forceinline__ double seg_scalar(double x) {
  const long long b = __double_as_longlong(x);
  int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
  asm volatile("" : "+v"(lo), "+v"(hi));
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// One workgroup per seed (blockIdx.x), W = blockDim / 64 waves, UPW segments of nblk lanes per wave (lanes past
// UPW nblk idle).  ORD: the gradient's order 1..4, or 0 for the exact one (the header comment's phase 3).
// Built-in costs only (TRACE / ZCAL), no co-state source, unpacked states, skew-Hermitian generators
// (the host's blkseg_ok).  PEN: with the state penalty on the rows P and columns C of sp.prow / sp.pcol (the header
// comment's penalty section); PEN = false is the unpenalised kernel, instruction for instruction.
// ENS: one workgroup per (pulse, member of a generator ensemble), blockIdx.x = v = pulse * E + member.  The pulse selects the row of u (and of a per-seed x_0), the member its generator table and nine scalars
// (uniform loads in the prologue); every output (J, the coefficients, dJdu) is indexed by v and goes to the ensemble's
// workspace, u_copy is written by member 0's workgroups alone, and the second copies and the best-pair epilogue are
// off.  Phases 1-3 are the same code; ENS = false is the kernel without any of it.  The halves under ENS (the risk
// objectives' route 2, qoc_run_blkseg_ens.hip): BLKSEG_FWD writes J, the coefficients, G and D indexed by v;
// BLKSEG_BWD of a workgroup whose member weight sp.omega[v] is exactly 0 returns before it reads anything else.
// TS: the gate duration as a per-seed variable.  Seed b runs on τ_b (A_0 + Σ_j u_jk A_j), τ_b = sp.tau[b]: the
// prologue multiplies the nine scalars and every table entry on its way to LDS by τ_b, so that ρ, J, P, the series
// class, e^{μ_k}, z and the exact term count follow from the seed's own scaled values and phases 1-3 run as they are
// (seeds of any durations share a launch); θ_cap is not scaled.  With U_k = exp(τ A_k) and [A_k, U_k] = 0,
//   dJ/dτ = Σ_k Re⟨λ_{k+1}, A_k x_{k+1}⟩ = Σ_k Σ_blocks Re tr(A_k G_{k+1}) = Σ_k Σ_blocks Re tr(A_k K_k U_k):
// phase 3 adds Re tr(X_k K_k U_k) per lane and slice, X_k = τ A_k as the loop holds it (unshifted, un-halved) and
// K_k U_k = G_k before its own penalty source; the phase-free loops carry z̄ G, so they add the complex trace and z
// is applied once per lane.  One fixed-order reduction over lanes and waves follows (no atomics), and
// dJdtau[b] = sum / τ_b: the exact derivative of the computed J at every ORD.  BLKSEG_FWD with TS only scales.
template <int NB, int ORD, int WMAX, int MODE = BLKSEG_FUSED, bool PEN = false, bool ENS = false, bool TS = false>
__global__ __launch_bounds__(64 * WMAX) void k_blkseg_eval(const TChainArgs g, const BlkArgs bk, const BlksegParams sp_) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  static_assert(!ENS || MODE != BLKSEG_FWD || ORD == 1, "the forward half has one instantiation");
  static_assert(!ENS || MODE == BLKSEG_FUSED || !(PEN && NB == 3), "penalised blocks of 3 rows have no ensemble eval");
  static_assert(!(ENS && TS), "a time scale and a generator ensemble do not combine");
  // the launch's parameters: the kernel argument itself, or a copy with (ENS) the member's table and scalars or (TS)
  // the seed's scaled scalars
  BlksegParams spm;
  double tau = 1.0;
  if constexpr (TS) {
    tau = seg_uniform(sp_.tau[blockIdx.x]);
    spm = sp_;
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // (the products are vector results: back to scalar registers, where the plain kernel has them)
      spm.rad[j] = seg_scalar(sp_.rad[j] * tau);
      spm.mur[j] = seg_scalar(sp_.mur[j] * tau);
      spm.mui[j] = seg_scalar(sp_.mui[j] * tau);
    }
  }
  int ens_p = blockIdx.x;
  if constexpr (ENS) {
    const int v = blockIdx.x, Ee = sp_.E;
    if constexpr (MODE == BLKSEG_BWD) {  // a member without weight in this pulse's objective: nothing to compute
      if (sp_.omega && sp_.omega[v] == 0.0) return;
    }
    ens_p = v / Ee;
    const int e = v - ens_p * Ee;
    spm = sp_;
    const double* const q = sp_.ens + 9 * (size_t)e;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      spm.rad[j] = seg_uniform(q[j]);
      spm.mur[j] = seg_uniform(q[3 + j]);
      spm.mui[j] = seg_uniform(q[6 + j]);
    }
    spm.gtab = sp_.gtab + (size_t)e * 3 * NB * NB * bk.nblk;
    spm.u_copy = e == 0 ? sp_.u_copy : nullptr;
    spm.u_copy2 = nullptr;
    spm.J2 = nullptr;
    spm.coef2 = nullptr;
    spm.done = nullptr;
  }
  const BlksegParams& sp = ENS || TS ? spm : sp_;
  const int bp = ENS ? ens_p : (int)blockIdx.x;  // the pulse: the row of u, of its copy and of a per-seed x_0
  if constexpr (MODE == BLKSEG_BWD) {  // a stale u (the check queued before this launch): leave every output alone
    if (sp.stale && *sp.stale != 0) return;
  }
  constexpr int E = NB * NB;
  // the lane's generator blocks in registers (blocks of 2 rows at <= 8 waves), else from LDS where used; blocks of 2
  // rows keep Â for X = A_k and accumulate M in the contraction
  constexpr bool GREG = NB == 2 && WMAX <= 8;
  constexpr bool XA = NB == 2;
  constexpr int NV1 = NB == 2 ? 2 : 1;  // slices formed at once in phase 1
  const int N = g.N, m = g.m, nu = g.nu, Nt = g.Nt, nblk = bk.nblk, S = sp.S, L = sp.L;
  const int tid = threadIdx.x, nthr = blockDim.x, w = tid >> 6, l = tid & 63, W = nthr >> 6;
  const int b = blockIdx.x;
  const size_t Nm = (size_t)N * m;
  BK_T(t0);
  double* const lds = reinterpret_cast<double*>(smem);
  double2* const gsh = reinterpret_cast<double2*>(lds);
  double* const rec = lds + blkseg_off_rec(NB, nblk);
  double2* const slot = reinterpret_cast<double2*>(lds + blkseg_off_slot(NB, nblk, Nt));
  double2* const g0s = reinterpret_cast<double2*>(lds + blkseg_off_g0(NB, nblk, Nt, S));
  double* const xN = lds + blkseg_off_xN(NB, nblk, Nt, S);
  double2* const xtl = reinterpret_cast<double2*>(lds + blkseg_off_xt(N, m, NB, nblk, Nt, S));
  cx<double>* const cf = reinterpret_cast<cx<double>*>(lds + blkseg_off_cf(N, m, NB, nblk, Nt, S));
  double* const red = lds + blkseg_off_red(N, m, NB, nblk, Nt, S);
  double* const wred = lds + blkseg_off_wred(N, m, NB, nblk, Nt, S);
  const int RB = sp.RB;
  double* const dJ = lds + blkseg_off_dJ(N, m, NB, nblk, Nt, S, W, RB);
  double2* const d0s = reinterpret_cast<double2*>(lds + blkseg_off_d0(N, m, nu, NB, nblk, Nt, S, W, RB));  // (PEN)

  // ---- the lane's unit: block beta of segment s = w UPW + uw ----
  const int uw = l / nblk;
  const bool lact = uw < sp.UPW;
  const int beta = lact ? l - uw * nblk : 0;
  // PEN: the penalised rows of the lane's block (bit i: row i), 0 for lanes without a segment; lanes of blocks without
  // a penalised row skip all of the penalty's arithmetic
  int pm = 0;
  if constexpr (PEN) {
    if (lact && w * sp.UPW + uw < S)
#pragma unroll
      for (int i = 0; i < NB; ++i) pm |= (int)((sp.prow[i] >> beta) & 1u) << i;
  }
  constexpr int PE = PEN ? NB * NB : 1;
  // ---- prologue: generator blocks, x_0, X_target, the seed's largest ρ_k ----
  // Every global read of the prologue is issued before the first wait, so that they share one round trip instead of
  // four in a row: each thread's first entry of the packed generator table, of x_0 and of X_target, the rows of its
  // lane's block and its first two slices of u (at cavity size that is all there is); then the LDS stores, and what
  // longer arrays have left in plain loops.
  const int ntab = 3 * E * nblk;
  const double2* const x0g = reinterpret_cast<const double2*>(g.x0) + (g.x0_per_seed ? (size_t)bp * Nm : 0);
  const double2* const xtg = reinterpret_cast<const double2*>(g.Xt);
  const double* ub = sp.u + (size_t)bp * Nt * nu;
  // two controls in an aligned buffer: one 16-byte load per slice
  const bool u16 = nu == 2 && (reinterpret_cast<size_t>(ub) & 15) == 0;
  auto load_u = [&](int k) -> double2 {
    if (u16) return reinterpret_cast<const double2*>(ub)[k];
    return make_double2(nu > 0 ? ub[(size_t)k * nu] : 0.0, nu > 1 ? ub[(size_t)k * nu + 1] : 0.0);
  };
  const bool hasx = MODE != BLKSEG_BWD && (size_t)tid < Nm;
  double2 tab0 = make_double2(0.0, 0.0), x00 = tab0, xt0 = tab0, ua = tab0, ubb = tab0;
  if (tid < ntab) tab0 = sp.gtab[tid];
  if (hasx) {
    x00 = x0g[tid];
    xt0 = xtg[tid];
  }
  if (tid < Nt) ua = load_u(tid);
  if (tid + nthr < Nt) ubb = load_u(tid + nthr);
  int brw[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) brw[i] = bk.brow[beta * NB + i];
  {
    if constexpr (TS) {  // the scaled blocks: nothing downstream sees an unscaled entry
      if (tid < ntab) gsh[tid] = make_double2(tab0.x * tau, tab0.y * tau);
      for (int q = tid + nthr; q < ntab; q += nthr) {
        const double2 v = sp.gtab[q];
        gsh[q] = make_double2(v.x * tau, v.y * tau);
      }
    } else {
    if (tid < ntab) gsh[tid] = tab0;
    for (int q = tid + nthr; q < ntab; q += nthr) gsh[q] = sp.gtab[q];
    }
    if constexpr (MODE != BLKSEG_BWD) {
      double2* const xN2 = reinterpret_cast<double2*>(xN);
      if (hasx) {
        xN2[tid] = x00;
        xtl[tid] = xt0;
      }
      for (size_t o = (size_t)tid + nthr; o < Nm; o += nthr) {
        xN2[o] = x0g[o];
        xtl[o] = xtg[o];
      }
    }
  }
  // one pass over u: ρ_k, the copies of u (the stale check, the lazy rebuilds) and the records
  // [Re e^{μ_k}, Im e^{μ_k}, u_1k, u_2k] (e^{μ_k} does not depend on J; u is scaled by 2^-J below when J > 0)
  double rmax = 0.0;
  // controls without shifts: e^{μ_k} = e^{μ_0} in every slice (the same value), one exp and sincos per thread
  const bool cmu = sp.mur[1] == 0.0 && sp.mur[2] == 0.0 && sp.mui[1] == 0.0 && sp.mui[2] == 0.0;
  double2 emu0 = make_double2(1.0, 0.0);
  if (cmu) {
    const double er = exp(sp.mur[0]);
    double sn, cs;
    sincos(sp.mui[0], &sn, &cs);
    emu0 = make_double2(er * cs, er * sn);
  }
  auto slice = [&](int k, double2 uk) {
    const double u1 = uk.x, u2 = uk.y;
    for (int j = 0; j < nu; ++j) {
      const double v = j ? u2 : u1;
      if (sp.u_copy) sp.u_copy[((size_t)bp * Nt + k) * nu + j] = v;
      if (sp.u_copy2) sp.u_copy2[((size_t)bp * Nt + k) * nu + j] = v;
    }
    rmax = fmax(rmax, fma(fabs(u2), sp.rad[2], fma(fabs(u1), sp.rad[1], sp.rad[0])));
    double2* r = reinterpret_cast<double2*>(rec + 4 * (size_t)k);
    if (cmu) {  // uniform
      r[0] = emu0;
    } else {
      const double mr = fma(u2, sp.mur[2], fma(u1, sp.mur[1], sp.mur[0]));
      const double mi = fma(u2, sp.mui[2], fma(u1, sp.mui[1], sp.mui[0]));
      const double er = exp(mr);
      double sn, cs;
      sincos(mi, &sn, &cs);
      r[0] = make_double2(er * cs, er * sn);
    }
    r[1] = make_double2(u1, u2);
  };
  if (tid < Nt) slice(tid, ua);
  if (tid + nthr < Nt) slice(tid + nthr, ubb);
  for (int k = tid + 2 * nthr; k < Nt; k += nthr) slice(k, load_u(k));
  rmax = block_max(rmax, red);  // (its barriers also publish the records)
  // J: the fewest halvings with ρ / 2^J <= θ_cap; P: the smallest degree whose tail bound
  // b^{P+1} / (P+1)! / (1 - b / (P+2)) is <= 2^-53 (b = ρmax / 2^J; every slice's ρ_k is <= ρmax)
  int J = 0;
  double s0 = 1.0;
  while (rmax * s0 > sp.theta_cap && J < 60) {
    s0 *= 0.5;
    ++J;
  }
  int P = 0;
  {
    const double bb = rmax * s0, tol = 1.1102230246251565e-16;
    constexpr BlkuCoef K = blku_coef();
    double term = bb;
#pragma unroll
    for (int q = 0; q < BLKU_TMAX; ++q) {
      if (!(term > tol * fma(-bb, K.inv[q + 2], 1.0))) break;
      P = q + 1;
      term *= bb * K.inv[q + 2];
    }
  }
  P = __builtin_amdgcn_readfirstlane(P);
  J = __builtin_amdgcn_readfirstlane(J);
  // the exact gradient's series length on the generic path (uniform: one seed per workgroup)
  int nex = 1;
  if constexpr (ORD == 0) nex = __builtin_amdgcn_readfirstlane(blkseg_exact_terms(rmax));
  if (tid < 8) reinterpret_cast<int*>(red + 24)[tid] = 0;  // wave progress (SegProg)
  if (J) {  // the records hold 2^-J u (exact scaling)
    for (int k = tid; k < Nt; k += nthr) {
      rec[4 * (size_t)k + 2] *= s0;
      rec[4 * (size_t)k + 3] *= s0;
    }
  }
  __syncthreads();
  BK_T(t1);
  BK_ADD(0, t1 - t0);

  const int s = w * sp.UPW + uw;
  const bool sact = lact && s < S;
  const int kb = sact ? s * L : 0;
  const int ke = sact ? min(kb + L, Nt) : 0;
  double2 greg[GREG ? 3 : 1][GREG ? E : 1];
  if constexpr (GREG) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int e = 0; e < E; ++e) greg[j][e] = gsh[(beta * 3 + j) * E + e];
  }
  // the generator blocks (blocks of 3 rows: read from LDS where used, through an opaque copy of the block index made
  // inside each loop, so that the compiler does not hoist all 3 E of them into registers and spill)
  auto gen_at = [&](int bc) {
    return [&, bc](int j, int e) -> double2 {
      if constexpr (GREG) return greg[j][e];
      else return gsh[(bc * 3 + j) * E + e];
    };
  };
  auto opaque = [](int v) {
    asm volatile("" : "+v"(v));
    return v;
  };

  // SIMD partners (w, w + 4) alternate the issue priority (seg_turn); QOC_PROBE builds: g_seg_noturn turns it off
  const int grp = __builtin_amdgcn_readfirstlane(w >> 2), ngrp = (W + 3) >> 2;
  const bool turns = ngrp > 1 && SEG_TURNS && SEG_TURNMODE == 0;
  SegProg<NB == 2 && MODE != BLKSEG_FWD> sprog;
  sprog.prog = reinterpret_cast<int*>(red + 24);
  sprog.partner = __builtin_amdgcn_readfirstlane(w ^ 4);
  sprog.on = ngrp > 1 && SEG_TURNS && SEG_TURNMODE == 1 && sprog.partner < W;
  sprog.young = grp == 1;
  sprog.other = 0;
  // ---- phase 1: the segment product P_s = U_{ke-1} .. U_{kb} ----
  double qr[E], qi[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    qr[e] = e % (NB + 1) == 0 ? 1.0 : 0.0;
    qi[e] = 0.0;
  }
  // PEN: H_s = Σ V^H Π V over the running product V after each slice of the segment (the states x_{kb+1} .. x_{ke} in
  // the frame of the segment's start); later T_s, its suffix sums and X_s (phase 2)
  double Hr[PE], Hi[PE];
#pragma unroll
  for (int e = 0; e < PE; ++e) Hr[e] = Hi[e] = 0.0;
  // every segment but the last has L slices; below Lf (the last one's length) no lane of a segment is past its end,
  // so those steps need no selects
  const int Lf = Nt - (S - 1) * L;
  // the fast path (blocks of 2 rows, no halvings): skew-Hermitian blocks in 4 reals, the closed-form exponential
  const bool fast = NB == 2 && J == 0;
  Sk2 gk[3];
  if constexpr (NB == 2) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double2 e4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) e4[e] = gsh[(beta * 3 + j) * E + e];
      gk[j] = sk2_of(e4);
    }
  }
  // the control generators' blocks without diagonal (cavity, zz: drives between levels): Â's diagonal is Ã_0's in
  // every slice, so e^{it} of the block's mean diagonal is computed once per lane (uniform over the workgroup)
  const bool zdl = NB != 2 || (gk[1].d0 == 0.0 && gk[1].d1 == 0.0 && gk[2].d0 == 0.0 && gk[2].d1 == 0.0);
  // With Re μ_0 = 0 besides (skew-Hermitian generators: always), z = e^{μ_0} e^{it} is one unimodular constant per
  // lane and the fast path's loops run phase-free on SU(2) (sk2_form_v); otherwise the general 2-row form runs, which
  // computes the same z in every slice.
  const bool zd = __syncthreads_and(zdl ? 1 : 0) != 0 && cmu && sp.mur[0] == 0.0;
  const double za0 = NB == 2 ? 0.5 * (gk[0].d0 - gk[0].d1) : 0.0;  // ZD: the blocks' constant half-difference
  // the fast path's series degree (uniform per seed: one loop instance per degree class)
  const int ksel = __builtin_amdgcn_readfirstlane(blkseg_series_k(rmax * s0));
  // ZD on the fast path: the running product of phase 1 as (p, y) of [[p, y], [-ȳ, p̄]], and the lane's z (formed where
  // it is used, for x_N and before phase 3, the same value both times: not live across the loops)
  const bool su = fast && zd;
  double pq[4] = {1.0, 0.0, 0.0, 0.0};
  auto lane_z = [&](double& zr, double& zi) {
    zr = 1.0;
    zi = 0.0;
    if constexpr (NB == 2) {
      if (su) {
        if (ksel == 5) sk2_z<5>(gk[0], rec, zr, zi);
        else if (ksel == 7) sk2_z<7>(gk[0], rec, zr, zi);
        else sk2_z<BLKSEG_KMAX>(gk[0], rec, zr, zi);
      }
    }
  };
  // the records of the lane's segment: the no-select steps address them from a per-lane base (one address
  // instruction per read; the shared base plus kb took a scalar that the loops had to fetch back from a spill)
  const double* const reck = rec + 4 * (size_t)kb;
  auto p1_fast = [&](int jj, auto SEL_, auto K_, auto ZD_) {
    constexpr bool SEL = decltype(SEL_)::value;
    constexpr int KS = decltype(K_)::value;
    constexpr bool ZD = decltype(ZD_)::value;
    if constexpr (NB == 2) {
    if constexpr (ZD) {
      double vv[2][4];
      bool act[2];
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int k = kb + jj + v;
        act[v] = !SEL || (sact && jj + v < L && k < ke);
        const double* r = SEL ? rec + 4 * (size_t)(act[v] ? k : 0) : reck + 4 * (size_t)(jj + v);
        Sk2 ah;
        sk2_form_v<KS>(gk, *reinterpret_cast<const double2*>(r + 2), za0, ah, vv[v]);
      }
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        double t[4];
        sk2_vmul(vv[v], pq, t);
#pragma unroll
        for (int e = 0; e < 4; ++e) pq[e] = !SEL || act[v] ? t[e] : pq[e];
        if constexpr (PEN) {
          if (pm && (!SEL || act[v])) {
            double wr_[4], wi_[4];
            sk2_expand(pq, wr_, wi_);
            seg_pen_acc<NB>(pm, wr_, wi_, Hr, Hi);
          }
        }
      }
    } else {
      double ur[2][4], ui[2][4];
      bool act[2];
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int k = kb + jj + v;
        act[v] = !SEL || (sact && jj + v < L && k < ke);
        const double* r = SEL ? rec + 4 * (size_t)(act[v] ? k : 0) : reck + 4 * (size_t)(jj + v);
        Sk2 ah;
        sk2_form<KS>(gk, *reinterpret_cast<const double2*>(r), *reinterpret_cast<const double2*>(r + 2), ah, ur[v],
                     ui[v]);
      }
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        double tr[4], ti[4];
        seg_mm<2, false, false>(ur[v], ui[v], qr, qi, tr, ti);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          qr[e] = !SEL || act[v] ? tr[e] : qr[e];
          qi[e] = !SEL || act[v] ? ti[e] : qi[e];
        }
        if constexpr (PEN) {
          if (pm && (!SEL || act[v])) seg_pen_acc<NB>(pm, qr, qi, Hr, Hi);
        }
      }
    }
    }  // NB == 2
  };
  auto loop1z = [&](auto K_, auto ZD_) {
    // the pairs wholly below Lf in a loop of their own (no selects, and nothing of the select variant's to merge at
    // the loop's head), then the tail with the selects (no iterations when Lf = L is even)
    int jj = 0;
    for (; jj + 1 < Lf; jj += 2) {
      if (turns) seg_turn(grp, ngrp, jj >> 1);
      sprog.step(jj >> 1);
      p1_fast(jj, std::false_type(), K_, ZD_);
    }
    for (; jj < L; jj += 2) {
      if (turns) seg_turn(grp, ngrp, jj >> 1);
      sprog.step(jj >> 1);
      p1_fast(jj, std::true_type(), K_, ZD_);
    }
    // ZD: the segment product without its phase z^(ke - kb), as a matrix for phase 2 (negations only); everything
    // there but x_N is invariant to the phase
    if constexpr (NB == 2) {
      if constexpr (decltype(ZD_)::value) sk2_expand(pq, qr, qi);
    }
  };
  auto loop1 = [&](auto K_) {
    if (zd) loop1z(K_, std::true_type());
    else loop1z(K_, std::false_type());
  };
  // G at the end of the lane's segment (phase 3's start): formed here, or read back (BLKSEG_BWD)
  double Gr[E], Gi[E];
  auto gseg_at = [&](int e) -> double2& { return sp.gseg[(((size_t)b * E + e) * S + s) * nblk + beta]; };
  // PEN: D at the lane's current slice (phase 3) lives in the lane's own row dl_at of the segment products' LDS area,
  // which is free after phase 2: held in registers across the contraction it would not fit beside G, U and K
  auto dl_at = [&](int e) -> double2& { return slot[((size_t)s * E + e) * nblk + beta]; };
  auto dseg_at = [&](int e) -> double2& { return sp.dseg[(((size_t)b * E + e) * S + s) * nblk + beta]; };
  if constexpr (MODE == BLKSEG_BWD) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double2 v = sact ? gseg_at(e) : make_double2(0.0, 0.0);
      Gr[e] = v.x;
      Gi[e] = v.y;
    }
    if constexpr (PEN) {
      if (pm)
#pragma unroll
        for (int e = 0; e < E; ++e) dl_at(e) = dseg_at(e);
    }
    // the co-states' rebuild source (blku_costates): this u (copied in the prologue) and the forward's λ_N coefficients
    if (sp.coef2 && tid < 2 * m) sp.coef2[(size_t)b * 2 * m + tid] = g.coef[(size_t)b * 2 * m + tid];
  } else {
  if (fast) {
    if (ksel == 5) loop1(std::integral_constant<int, 5>());
    else if (ksel == 7) loop1(std::integral_constant<int, 7>());
    else loop1(std::integral_constant<int, BLKSEG_KMAX>());
  } else {
    for (int jj = 0; jj < L; jj += NV1) {
      if (turns) seg_turn(grp, ngrp, jj / NV1);
      sprog.step(jj / NV1);
      const double* rk[NV1];
      bool act[NV1];
#pragma unroll
      for (int v = 0; v < NV1; ++v) {
        const int k = kb + jj + v;
        act[v] = sact && jj + v < L && k < ke;
        rk[v] = rec + 4 * (size_t)(act[v] ? k : 0);
      }
      double ar[NV1][E], ai[NV1][E], ur[NV1][E], ui[NV1][E];
      seg_form<NB, NV1>(gen_at(GREG ? beta : opaque(beta)), rk, s0, P, J, ar, ai, ur, ui);
#pragma unroll
      for (int v = 0; v < NV1; ++v) {
        double tr[E], ti[E];
        seg_mm<NB, false, false>(ur[v], ui[v], qr, qi, tr, ti);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          qr[e] = act[v] ? tr[e] : qr[e];
          qi[e] = act[v] ? ti[e] : qi[e];
        }
        if constexpr (PEN) {
          if (pm && act[v]) seg_pen_acc<NB>(pm, qr, qi, Hr, Hi);
        }
      }
    }
  }
  if constexpr (PEN) {
    if (pm) {  // to the frame of the segment's end, where the inclusive prefix Q_s applies: H' = P_s H_s P_s^H
      double tr[E], ti[E];
      seg_mm<NB, false, false>(qr, qi, Hr, Hi, tr, ti);
      seg_mm<NB, false, true>(tr, ti, qr, qi, Hr, Hi);
    }
    // D_0 = Σ_{c in C} x_0,c x_0,c^H of every block (the first segment's lanes), before x_N overwrites x_0 (after the
    // scan's workgroup barrier below)
    if (w == 0 && l < nblk) {
      double dr[E], di[E];
#pragma unroll
      for (int e = 0; e < E; ++e) dr[e] = di[e] = 0.0;
      if (pm)
        for (int c = 0; c < m; ++c) {
          if (!((sp.pcol >> c) & 1u)) continue;
          double xr[NB], xi[NB];
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            const size_t o = 2 * ((size_t)c * N + max(brw[i], 0));
            xr[i] = brw[i] >= 0 ? xN[o] : 0.0;
            xi[i] = brw[i] >= 0 ? xN[o + 1] : 0.0;
          }
#pragma unroll
          for (int a = 0; a < NB; ++a)
#pragma unroll
            for (int q = 0; q < NB; ++q) {
              dr[a * NB + q] = fma(xr[a], xr[q], fma(xi[a], xi[q], dr[a * NB + q]));
              di[a * NB + q] = fma(xi[a], xr[q], fma(-xr[a], xi[q], di[a * NB + q]));
            }
        }
#pragma unroll
      for (int e = 0; e < E; ++e) d0s[e * nblk + beta] = make_double2(dr[e], di[e]);
    }
  }

  if (turns || sprog.on) __builtin_amdgcn_s_setprio(0);
  BK_T(t2);
  BK_ADD(1, t2 - t1);
  SEGW_SET(w, t2 - t0);
  // ---- phase 2: prefix products Q_s = P_s .. P_0 ----
  // Two levels: a Hillis-Steele scan over the UPW segments of each wave through its own slot rows (one wave's LDS
  // accesses are ordered, so the rounds need wave syncs only), then every lane multiplies by the product of the
  // earlier waves' totals T_v (the local Q of their last segments), read after the one workgroup barrier.  Lanes of
  // segments past S hold the identity (phase 1 left their P = I), so the last wave's scan needs no masks.  14 of the
  // 15 barriers of the plain scan over 84 segments (zz) are gone.
  auto slot_at = [&](int ss, int e) -> double2& { return slot[((size_t)ss * E + e) * nblk + beta]; };
  const int UPW = sp.UPW, uw0 = lact ? uw : 0;
  if (sact)
#pragma unroll
    for (int e = 0; e < E; ++e) slot_at(s, e) = make_double2(qr[e], qi[e]);
  wave_lds_sync();
  for (int d = 1; d < UPW; d <<= 1) {
    const bool take = sact && uw0 >= d;
    double tr[E], ti[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double2 v = take ? slot_at(s - d, e) : make_double2(0.0, 0.0);
      tr[e] = v.x;
      ti[e] = v.y;
    }
    wave_lds_sync();
    if (take) {
      double cr[E], ci[E];
      seg_mm<NB, false, false>(qr, qi, tr, ti, cr, ci);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        qr[e] = cr[e];
        qi[e] = ci[e];
        slot_at(s, e) = make_double2(cr[e], ci[e]);
      }
    }
    wave_lds_sync();
  }
  lds_barrier();
  if (sact && w > 0) {  // E_w = T_{w-1} .. T_0, then Q_s = Q_s(local) E_w
    double er[E], ei[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double2 v = slot_at(UPW - 1, e);
      er[e] = v.x;
      ei[e] = v.y;
    }
    for (int v = 1; v < w; ++v) {
      double tr[E], ti[E], cr[E], ci[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double2 x = slot_at(v * UPW + UPW - 1, e);
        tr[e] = x.x;
        ti[e] = x.y;
      }
      seg_mm<NB, false, false>(tr, ti, er, ei, cr, ci);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        er[e] = cr[e];
        ei[e] = ci[e];
      }
    }
    double cr[E], ci[E];
    seg_mm<NB, false, false>(qr, qi, er, ei, cr, ci);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      qr[e] = cr[e];
      qi[e] = ci[e];
    }
  }
  if constexpr (PEN) {
    if (pm) {  // T_s = Q_s^H H'_s Q_s = Σ_{k in (kb, ke]} R_k, R_k = W_k^H Π W_k: the segment's sum in the frame of time 0
      double tr[E], ti[E];
      seg_mm<NB, true, false>(qr, qi, Hr, Hi, tr, ti);
      seg_mm<NB, false, false>(tr, ti, qr, qi, Hr, Hi);
    }
  }
  // x_N = Q_{S-1} x_0 on each block (the last segment's lanes), in place in xN
  const bool last = sact && s == S - 1;
  if (last) {
    // ZD: the block's phase over all slices, z^Nt by square-and-multiply (x_N is the one quantity that sees it)
    double znr = 1.0, zni = 0.0;
    if (su) {
      double br, bi;
      lane_z(br, bi);
      for (int n = Nt; n > 0; n >>= 1) {
        if (n & 1) {
          const double t = znr * br - zni * bi;
          zni = fma(znr, bi, zni * br);
          znr = t;
        }
        const double t = br * br - bi * bi;
        bi = 2.0 * (br * bi);
        br = t;
      }
    }
    for (int c = 0; c < m; ++c) {
      double xr[NB], xi[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const size_t o = 2 * ((size_t)c * N + max(brw[i], 0));
        xr[i] = brw[i] >= 0 ? xN[o] : 0.0;
        xi[i] = brw[i] >= 0 ? xN[o + 1] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        double yr = 0.0, yi = 0.0;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
          yr = fma(qr[i * NB + q], xr[q], fma(-qi[i * NB + q], xi[q], yr));
          yi = fma(qr[i * NB + q], xi[q], fma(qi[i * NB + q], xr[q], yi));
        }
        if (su) {
          const double t = yr * znr - yi * zni;
          yi = fma(yr, zni, yi * znr);
          yr = t;
        }
        if (brw[i] >= 0) {
          const size_t o = 2 * ((size_t)c * N + brw[i]);
          xN[o] = yr;
          xN[o + 1] = yi;
        }
      }
    }
  }
  __syncthreads();
  if constexpr (PEN) {
    // inclusive suffix sums of T over the segments of each wave, through the lanes' own rows of the segment products'
    // area (every wave is past its reads of the products: the barrier above); additions only, wave syncs only
    if (pm)
#pragma unroll
      for (int e = 0; e < E; ++e) slot_at(s, e) = make_double2(Hr[e], Hi[e]);
    wave_lds_sync();
    for (int d = 1; d < UPW; d <<= 1) {
      const bool take = pm && uw0 + d < UPW && s + d < S;
      double tr[E], ti[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double2 v = take ? slot_at(s + d, e) : make_double2(0.0, 0.0);
        tr[e] = v.x;
        ti[e] = v.y;
      }
      wave_lds_sync();
      if (take) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          Hr[e] += tr[e];
          Hi[e] += ti[e];
          slot_at(s, e) = make_double2(Hr[e], Hi[e]);
        }
      }
      wave_lds_sync();
    }
  }
  // J and the λ_N coefficients (src/penalty_fcns.jl:15-42)
  chain_costs<double>(N, m, reinterpret_cast<const cx<double>*>(xtl), [&](int q) { return cx<double>{xN[2 * q], xN[2 * q + 1]}; },
                      g.cost_kind, g.n_norm, 0.0, red, red + 16, cf, g.sc);
  __syncthreads();
  if (tid < 2 * m) {
    g.coef[(size_t)b * 2 * m + tid] = cf[tid];
    if (sp.coef2) sp.coef2[(size_t)b * 2 * m + tid] = cf[tid];
  }
  // PEN: the sum over the later waves' totals (the suffix sums of their first segments), waves in order
  auto later_waves = [&](double (&ar)[E], double (&ai)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) ar[e] = ai[e] = 0.0;
    for (int v = w + 1; v < W; ++v)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double2 x = slot_at(v * UPW, e);
        ar[e] += x.x;
        ai[e] += x.y;
      }
  };
  if constexpr (PEN) {
    // the first segment's lanes take their block's share of Σ_k L(x_k) / μ = Re tr(D_0 (Π + Σ_s T_s)) (Π: the state
    // x_0 itself); Σ_s T_s = the lane's own suffix sum (read back from its row: H is not kept in registers) plus the
    // later waves' totals
    double pj = 0.0;
    if (pm && s == 0) {
      double ar[E], ai[E];
      later_waves(ar, ai);
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int q = 0; q < NB; ++q) {
          const double2 d0 = d0s[(a * NB + q) * nblk + beta], h = slot_at(0, q * NB + a);
          const double mr = h.x + ar[q * NB + a] + (a == q && ((pm >> a) & 1) ? 1.0 : 0.0);
          const double mi = h.y + ai[q * NB + a];
          pj = fma(d0.x, mr, fma(-d0.y, mi, pj));
        }
    }
    if (w == 0) {  // the blocks' shares to the first thread, summed there in block order
      if (l < nblk) wred[l] = pj;
      wave_lds_sync();
    }
  }
  if (tid == 0) {
    double Jv = red[16];
    if constexpr (PEN) {
      double ps = 0.0;
      for (int q = 0; q < nblk; ++q) ps += wred[q];
      Jv = fma(sp.pen_mu, ps, Jv);
    }
    // J is the one value other workgroups read in this launch (publish): stored write-through at agent scope (sc1),
    // so the hand-off needs no release fence (no L2 write-back of everything this XCD holds dirty)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(g.J + b),
                       (unsigned long long)__double_as_longlong(Jv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sp.J2) sp.J2[b] = Jv;
  }
  // J is published after the cost: before the barrier that precedes G_0 when no waves share a SIMD within the
  // workgroup (early: all waves wait for the fences together), else after the last barrier before phase 3, so that
  // only wave 0 (one of the fast waves, seg_turn) waits for them.  The last workgroup to publish finds the best
  // (J, seed) of the launch (k_argmin_seed's order: NaN never wins, ties go to the lower seed).  The hand-off is the
  // write-through form of the guide's counter recipe (cdna_hip_programming.md, split-K combine / Guideline 16 R1):
  // J stored sc1, vmcnt(0), relaxed agent counter add; the last adder acquires and then reads every J.
  // This hand-off leans on gfx950's memory subsystem (the write-through sc1 store is complete at vmcnt(0), before the
  // counter add), not on a release/acquire pair, which would write back the whole L2 of the XCD; the build targets
  // gfx950 only (the check below keeps another target from compiling it silently).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_blkseg_eval's best-(J, seed) hand-off is written for gfx950"
#endif
  const bool early = W <= 4;
  auto publish = [&]() {
    if (ENS || w != 0 || !sp.done) return;
    unsigned int prev = 0;
    if (l == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the sc1 J store has reached memory
      prev = __hip_atomic_fetch_add(sp.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    prev = __shfl(prev, 0);
    if (prev == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      double bv = __builtin_inf();
      long long bi = -1;
      for (int e = l; e < (int)gridDim.x; e += 64) {
        // agent-scope atomic loads (sc1 on gfx950): the other workgroups' J stores were write-through at agent scope
        const double v = __longlong_as_double((long long)__hip_atomic_load(
            reinterpret_cast<unsigned long long*>(g.J + e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (v < bv || (v == bv && e < bi)) {
          bv = v;
          bi = e;
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const long long oi = __shfl_xor(bi, off);
        if (ov < bv || (ov == bv && oi >= 0 && (bi < 0 || oi < bi))) {
          bv = ov;
          bi = oi;
        }
      }
      if (l == 0) {
        const double bs = bi >= 0 ? (double)(bi + sp.seed_offset) : -1.0;
        sp.best[0] = bv;
        sp.best[1] = bs;
        if (sp.best_res) {
          sp.best_res[0] = bv;
          sp.best_res[1] = bs;
        }
        if (sp.best_out) {
          sp.best_out[0] = bv;
          sp.best_out[1] = bs;
        }
        *sp.done = 0;  // ready for the next launch (the kernel boundary orders it)
      }
    }
  };
  if (early) publish();
  // G_N = Σ_c x_N λ_N^H on each block, G_0 = Q_{S-1}^H G_N Q_{S-1}
  if (last) {
    const cx<double>* Xt = reinterpret_cast<const cx<double>*>(xtl);  // (the prologue's LDS copy)
    double gr[E], gi[E];
#pragma unroll
    for (int e = 0; e < E; ++e) gr[e] = gi[e] = 0.0;
    for (int c = 0; c < m; ++c) {
      double2 xv[NB], lv[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int r = brw[i];
        const size_t o = (size_t)c * N + max(r, 0);
        const cx<double> f = lam_coef(cf, g.sc, m, max(r, 0), c), t = Xt[o];
        xv[i] = r >= 0 ? make_double2(xN[2 * o], xN[2 * o + 1]) : make_double2(0.0, 0.0);
        lv[i] = r >= 0 ? make_double2(f.r * t.r - f.i * t.i, f.r * t.i + f.i * t.r) : make_double2(0.0, 0.0);
      }
      blku_kacc<NB>(gr, gi, xv, lv);
    }
    double tr[E], ti[E], cr[E], ci[E];
    seg_mm<NB, true, false>(qr, qi, gr, gi, tr, ti);
    seg_mm<NB, false, false>(tr, ti, qr, qi, cr, ci);
#pragma unroll
    for (int e = 0; e < E; ++e) g0s[e * nblk + beta] = make_double2(cr[e], ci[e]);
  }
  if constexpr (PEN) {
    // X_s = Σ_{s' > s} T_s' into H: the next segment's suffix sum within the wave plus the later waves' totals, in a
    // fixed order (read here, after the last segment's work above, so that X is not live across it; the rows are
    // overwritten only behind the barrier below)
    if (pm) {
      later_waves(Hr, Hi);
      if (uw0 + 1 < UPW && s + 1 < S)
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double2 x = slot_at(s + 1, e);
          Hr[e] += x.x;
          Hi[e] += x.y;
        }
    }
  }
  __syncthreads();
  // G at the segment's end: Q_s G_0 Q_s^H
  {
    double hr[E], hi[E], tr[E], ti[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double2 v = g0s[e * nblk + beta];
      hr[e] = v.x;
      hi[e] = v.y;
    }
    if constexpr (PEN) {
      // (entry by entry, each stored or added at once, and the three parts kept apart: few matrices live at a time)
      if (pm) {
        double dr[E], di[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double2 v = d0s[e * nblk + beta];
          dr[e] = v.x;
          di[e] = v.y;
        }
        // D at the segment's end, Q_s D_0 Q_s^H: phase 3's start, in the lane's LDS row (fused) or to HBM (forward)
        seg_mm<NB, false, false>(qr, qi, dr, di, tr, ti);
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int q = 0; q < NB; ++q) {
              sr = fma(tr[i * NB + q], qr[j * NB + q], fma(ti[i * NB + q], qi[j * NB + q], sr));
              si = fma(ti[i * NB + q], qr[j * NB + q], fma(-tr[i * NB + q], qi[j * NB + q], si));
            }
            if constexpr (MODE == BLKSEG_FWD) dseg_at(i * NB + j) = make_double2(sr, si);
            else dl_at(i * NB + j) = make_double2(sr, si);
          }
        __builtin_amdgcn_sched_barrier(0);
        // the later segments' sources in the frame of time 0: G_0 + 2 μ D_0 X_s
        const double f = 2.0 * sp.pen_mu;
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int q = 0; q < NB; ++q) {
              sr = fma(dr[i * NB + q], Hr[q * NB + j], fma(-di[i * NB + q], Hi[q * NB + j], sr));
              si = fma(dr[i * NB + q], Hi[q * NB + j], fma(di[i * NB + q], Hr[q * NB + j], si));
            }
            hr[i * NB + j] = fma(f, sr, hr[i * NB + j]);
            hi[i * NB + j] = fma(f, si, hi[i * NB + j]);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    seg_mm<NB, false, false>(qr, qi, hr, hi, tr, ti);
    seg_mm<NB, false, true>(tr, ti, qr, qi, Gr, Gi);
  }

  if (!early) publish();
  BK_T(t2e);
  BK_ADD(2, t2e - t2);
  if constexpr (MODE == BLKSEG_FWD) {  // the forward half ends here: G to HBM for the backward launch
    if (sact)
#pragma unroll
      for (int e = 0; e < E; ++e) gseg_at(e) = make_double2(Gr[e], Gi[e]);
    if (sp.terms && tid == 0) atomicAdd(sp.terms + b % TERM_SLOTS, (unsigned long long)Nt * ((unsigned long long)P << J));
    return;
  }
  }  // MODE != BLKSEG_BWD
  BK_T(t3);
  // ---- phase 3: each segment backwards, the gradient of every slice ----
  const double mu1r = sp.mur[1], mu1i = sp.mui[1], mu2r = sp.mur[2], mu2i = sp.mui[2];
  // PEN, one slice: G_{k+1} takes the source of λ_{k+1}, 2 μ D_{k+1} Π; then D_k = U_k^H D_{k+1} U_k.  D is read from
  // and written back to the lane's LDS row through an opaque copy of the segment index, so that the compiler does not
  // promote the row to registers over the loop (where it would be live across the contraction)
  const double pen2 = PEN ? 2.0 * sp.pen_mu : 0.0;
  auto pen_step = [&](const double (&ur)[E], const double (&ui)[E]) {
    seg_pen_step<NB>(pm, pen2, slot + (size_t)opaque(s) * E * nblk + beta, nblk, ur, ui, Gr, Gi);
  };
  // ZD on the fast path: the loop moves Ĝ = z̄ G (sk2_form_v), from here on in Gr, Gi; the fused launch and the
  // backward half (G back from HBM) do the same operations on the same G.  The penalty's source turns with it.
  double zr, zi;
  lane_z(zr, zi);
  if (su) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double t = fma(zr, Gr[e], zi * Gi[e]);
      Gi[e] = fma(zr, Gi[e], -zi * Gr[e]);
      Gr[e] = t;
    }
  }
  const double pen2r = pen2 * zr, pen2i = -pen2 * zi;
  auto pen_step_v = [&](const double (&ur)[E], const double (&ui)[E]) {
    seg_pen_step<NB, true>(pm, pen2r, slot + (size_t)opaque(s) * E * nblk + beta, nblk, ur, ui, Gr, Gi, pen2i);
  };
  double* const wr = wred + 128 * RB * w;
  // the slices' sums over their blocks: each step's partial sums go to slot (L - 1 - jj) % RB of a wave-private
  // area; every RB steps (and after the last) one lane per (step, segment of the wave, control) adds its nblk
  // entries in a fixed order
  const int nrl = sp.UPW * max(nu, 1);  // reducing lanes per step
  const int rq = l / nrl, rrem = l - rq * nrl, ro = rrem / max(nu, 1), rj = rrem - ro * max(nu, 1);
  int rslot = 0;  // (L - 1 - jj) % RB as a counter (jj runs down from L - 1 by one)
  auto reduce = [&](int jj, double acc1, double acc2) {
    const int r = rslot;
    rslot = r == RB - 1 ? 0 : r + 1;
    *reinterpret_cast<double2*>(wr + 128 * r + 2 * l) = make_double2(acc1, acc2);
    if (r == RB - 1 || jj == 0) {  // uniform
      wave_lds_sync();
      if (rq <= r) {  // slot rq holds step jj + r - rq
        const int ss = w * sp.UPW + ro, kk = ss * L + jj + r - rq;
        if (ss < S && kk < Nt) {
          const double* src = wr + 128 * rq + 2 * ro * nblk + rj;
          double sum = 0.0;
          for (int q = 0; q < nblk; ++q) sum += src[2 * q];
          dJ[(size_t)kk * nu + rj] = sum;
        }
      }
      wave_lds_sync();
    }
  };
  double pa1[4] = {0, 0, 0, 0}, pa2[4] = {0, 0, 0, 0};  // the generators' (A_j = Ã_j + i m_j I) doubled Pauli vectors times -1/2
  // ZD: X's diagonal in every slice (Ã_0's plus i Im μ_0) and its Pauli components
  const double zxd0 = NB == 2 ? gk[0].d0 + sp.mui[0] : 0.0, zxd1 = NB == 2 ? gk[0].d1 + sp.mui[0] : 0.0;
  const double zx0 = 0.5 * (zxd0 + zxd1), zx3 = 0.5 * (zxd0 - zxd1), zx02 = zx0 * zx0;
  if constexpr (NB == 2) {
    sk2_pauli2(Sk2{gk[1].d0 + mu1i, gk[1].d1 + mu1i, gk[1].r, gk[1].q}, pa1);
    sk2_pauli2(Sk2{gk[2].d0 + mu2i, gk[2].d1 + mu2i, gk[2].r, gk[2].q}, pa2);
  }
  // TS: the lane's Σ_k tr(X_k K_k U_k) over its slices (the imaginary part in the phase-free loops only, where the
  // trace is of z̄ G and z turns it back at the end)
  double tsr = 0.0, tsi = 0.0;
  // upre: the slice's controls where the caller has read them already (the no-select loop's read-ahead)
  auto p3_fast = [&](int jj, auto SEL_, auto K_, auto ZD_, const double2* upre = nullptr) {
    constexpr bool SEL = decltype(SEL_)::value;
    constexpr int KS = decltype(K_)::value;
    constexpr bool ZD = decltype(ZD_)::value;
    if constexpr (NB == 2) {
      const int k = kb + jj;
      const bool act = !SEL || (sact && k < ke);
      const double* r = SEL ? rec + 4 * (size_t)(act ? k : 0) : reck + 4 * (size_t)jj;
      const double2 u = upre ? *upre : *reinterpret_cast<const double2*>(r + 2);
      Sk2 ah;
      double ur[4], ui[4], ex[5];
      if constexpr (ZD) {  // V_k as a matrix (negations only) and Ĝ in Gr, Gi: the same K_k
        double vv[4];
        sk2_form_v<KS, ORD == 0>(gk, u, za0, ah, vv, zr, zi, ex);
        sk2_expand(vv, ur, ui);
      } else {
        sk2_form<KS, ORD == 0>(gk, *reinterpret_cast<const double2*>(r), u, ah, ur, ui, ex);
      }
      if constexpr (PEN) {
        // G_{k+1} takes the source of λ_{k+1}, 2 μ D_{k+1} Π; then D_k = U_k^H D_{k+1} U_k
        if (pm && (!SEL || act)) {
          if constexpr (ZD) pen_step_v(ur, ui);
          else pen_step(ur, ui);
        }
      }
      // K_k = U_k^H G_{k+1}, G_k = K_k U_k (ZD: K_k = V_k^H Ĝ_{k+1}, Ĝ_k = K_k V_k)
      double Kr[4], Ki[4], tr[4], ti[4];
      seg_mm<2, true, false>(ur, ui, Gr, Gi, Kr, Ki);
      seg_mm<2, false, false>(Kr, Ki, ur, ui, tr, ti);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Gr[e] = !SEL || act ? tr[e] : Gr[e];
        Gi[e] = !SEL || act ? ti[e] : Gi[e];
      }
      // X = A_k = Â + μ_k I (skew: μ_k = i (Im μ_0 + u_1 Im μ_1 + u_2 Im μ_2))
      // (ZD: μ_k = i Im μ_0, the same value)
      const double mki = ZD ? sp.mui[0] : fma(u.y, mu2i, fma(u.x, mu1i, sp.mui[0]));
      const Sk2 x{ah.d0 + mki, ah.d1 + mki, ah.r, ah.q};
      if constexpr (TS) {
        // tr(X_k K_k U_k) on the skew X = [[i d0, r + i q], [-r + i q, i d1]]; t = K_k U_k (ZD: z̄ times it).  Lanes
        // without a segment are dropped at the reduction.
        const double t_re = fma(-x.d0, ti[0], fma(-x.d1, ti[3], fma(x.r, tr[2] - tr[1], -x.q * (ti[2] + ti[1]))));
        tsr += !SEL || act ? t_re : 0.0;
        if constexpr (ZD) {
          const double t_im = fma(x.d0, tr[0], fma(x.d1, tr[3], fma(x.r, ti[2] - ti[1], x.q * (tr[2] + tr[1]))));
          tsi += !SEL || act ? t_im : 0.0;
        }
      }
      double acc1, acc2;
      if constexpr (ORD == 0) {
        sk2_contract_exact<ZD>(x, pa1, pa2, Kr, Ki, ex, acc1, acc2, zx3);
      } else if constexpr (ORD <= 3) {
        sk2_contract_pauli<ORD, ZD>(x, pa1, pa2, Kr, Ki, acc1, acc2, zx0, zx3, zx02);
      } else {
        const Sk2 e1{gk[1].d0 + mu1i, gk[1].d1 + mu1i, gk[1].r, gk[1].q};
        const Sk2 e2{gk[2].d0 + mu2i, gk[2].d1 + mu2i, gk[2].r, gk[2].q};
        sk2_contract<ORD>(x, e1, e2, Kr, Ki, acc1, acc2);
      }
      reduce(jj, !SEL || act ? acc1 : 0.0, !SEL || act ? acc2 : 0.0);
    }
  };
  // The same step of the phase-free loops in the Pauli basis (PAU: orders 1..3 without the penalty, whose step works
  // on the matrices G and D): Ĝ as gp, K's components and the rotation from sk2_pauli_k / sk2_pauli_rot.  g0 (gp[0..1])
  // is the same in every slice.  The fused, backward, ensemble and time-scale instances all take this form.
  constexpr bool PAU = NB == 2 && !PEN && ORD >= 1 && ORD <= 3;
  double gp[8];
  auto p3_pauli = [&](int jj, auto SEL_, auto K_, const double2* upre = nullptr) {
    constexpr bool SEL = decltype(SEL_)::value;
    constexpr int KS = decltype(K_)::value;
    if constexpr (PAU) {
      const int k = kb + jj;
      const bool act = !SEL || (sact && k < ke);
      const double* r = SEL ? rec + 4 * (size_t)(act ? k : 0) : reck + 4 * (size_t)jj;
      const double2 u = upre ? *upre : *reinterpret_cast<const double2*>(r + 2);
      Sk2 ah;
      double vv[4], tc[6], kc[7], gn[6];
      sk2_form_v<KS>(gk, u, za0, ah, vv);
      sk2_pauli_k<ORD>(vv, gp, tc, kc);
      sk2_pauli_rot(vv, tc, gp, gn);
#pragma unroll
      for (int e = 0; e < 6; ++e) gp[2 + e] = !SEL || act ? gn[e] : gp[2 + e];
      if constexpr (TS) {
        // tr(X_k Ĝ_k) = i (x0 2 g0 + x . 2 g) on the doubled components, X = i (x0 I + x.σ), x = (q, r, x3): the
        // quantity the matrix form sums.  Lanes without a segment are dropped at the reduction.
        const double t_re = -fma(ah.q, gn[3], fma(ah.r, gn[4], fma(zx3, gn[5], zx0 * gp[1])));
        const double t_im = fma(ah.q, gn[0], fma(ah.r, gn[1], fma(zx3, gn[2], zx0 * gp[0])));
        tsr += !SEL || act ? t_re : 0.0;
        tsi += !SEL || act ? t_im : 0.0;
      }
      double acc1, acc2;
      sk2_contract_pauli_k<ORD>(ah.q, ah.r, pa1, pa2, kc, acc1, acc2, zx0, zx3, zx02);
      reduce(jj, !SEL || act ? acc1 : 0.0, !SEL || act ? acc2 : 0.0);
    }
  };
  auto loop3z = [&](auto K_, auto ZD_) {
    constexpr bool PZ = PAU && decltype(ZD_)::value;
    auto p3 = [&](int jj, auto SEL_, const double2* upre = nullptr) {
      if constexpr (PZ) p3_pauli(jj, SEL_, K_, upre);
      else p3_fast(jj, SEL_, K_, ZD_, upre);
    };
    // Ĝ (behind the z̄ turn, fused or back from HBM) to its Pauli components, once per lane; nothing below reads G
    if constexpr (PAU) {
      if constexpr (PZ) sk2_pauli_of(Gr, Gi, gp);
    }
    // the steps at and above Lf first, with the selects (none when Lf = L), then the rest in a loop of their own
    int jj = L - 1;
    for (; jj >= Lf; --jj) {
      if (turns) seg_turn(grp, ngrp, jj);
      sprog.step(L + (L - 1 - jj));
      p3(jj, std::true_type());
    }
    // ZD: the slice's controls are read one step ahead (the next step's while this one runs: the read's latency
    // stood at the head of every step), the last step reads its own again
    constexpr bool PRE = decltype(ZD_)::value;
    double2 un = make_double2(0.0, 0.0);
    if (PRE && jj >= 0) {
      un = *reinterpret_cast<const double2*>(reck + 4 * (size_t)jj + 2);
      // This first read is waited for here, once, in front of the loop.  Left pending into the loop's head it made
      // the compiler wait at the top of every step, in front of the first formation FMA, for everything but the newest
      // read: the partner's count of SegProg::step, just issued, among it.
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0), the other counters left alone
    }
    for (; jj >= 0; --jj) {
      if (turns) seg_turn(grp, ngrp, jj);
      sprog.step(L + (L - 1 - jj));
      const double2 uc = un;
      if constexpr (PRE) {
        un = *reinterpret_cast<const double2*>(reck + 4 * (size_t)max(jj - 1, 0) + 2);
        __builtin_amdgcn_sched_barrier(0);
      }
      p3(jj, std::false_type(), PRE ? &uc : nullptr);
    }
  };
  auto loop3 = [&](auto K_) {
    if (zd) loop3z(K_, std::true_type());
    else loop3z(K_, std::false_type());
  };
  if (fast) {
    if (ksel == 5) loop3(std::integral_constant<int, 5>());
    else if (ksel == 7) loop3(std::integral_constant<int, 7>());
    else loop3(std::integral_constant<int, BLKSEG_KMAX>());
  } else {
    for (int jj = L - 1; jj >= 0; --jj) {
      if (turns) seg_turn(grp, ngrp, jj);
      sprog.step(L + (L - 1 - jj));
      const int k = kb + jj;
      const bool act = sact && k < ke;
      const double* rk[1] = {rec + 4 * (size_t)(act ? k : 0)};
      const auto gen = gen_at(GREG ? beta : opaque(beta));
      double ar[1][E], ai[1][E], ur[1][E], ui[1][E];
      seg_form<NB, 1>(gen, rk, s0, P, J, ar, ai, ur, ui);
      if constexpr (PEN) {
        // G_{k+1} takes the source of λ_{k+1}, 2 μ D_{k+1} Π; then D_k = U_k^H D_{k+1} U_k
        if (pm && act) pen_step(ur[0], ui[0]);
      }
      // TS: the slice's Re tr(X_k G), in one of two places (the same sum: X_k commutes with U_k).  Blocks of 3 rows at
      // order 1, whose contraction needs no X: here, as Re tr(X_k G_{k+1}) with the source of λ_{k+1} in G and
      // X_k = 2^J Â + μ_k I from the formation's Â, still in registers and dead afterwards (forming X for the trace
      // alone took these kernels from 158 to 256 VGPRs).  Everything else: below, on the X the contraction forms (the
      // early form there keeps Â live across the two products and spills).
      constexpr bool TSE = TS && NB == 3 && ORD == 1;
      if constexpr (TSE) {
        double t_re = 0.0, gtr = 0.0, gti = 0.0;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          gtr += Gr[i * NB + i];
          gti += Gi[i * NB + i];
#pragma unroll
          for (int q = 0; q < NB; ++q)
            t_re = fma(ar[0][i * NB + q], Gr[q * NB + i], fma(-ai[0][i * NB + q], Gi[q * NB + i], t_re));
        }
        const double2 sv = *reinterpret_cast<const double2*>(rk[0] + 2);
        const double v1 = ldexp(sv.x, J), v2 = ldexp(sv.y, J);
        const double nr = fma(v2, sp.mur[2], fma(v1, sp.mur[1], sp.mur[0]));
        const double ni = fma(v2, sp.mui[2], fma(v1, sp.mui[1], sp.mui[0]));
        t_re = fma(nr, gtr, fma(-ni, gti, ldexp(t_re, J)));
        tsr += act ? t_re : 0.0;
      }
      // K_k = U_k^H G_{k+1}, G_k = K_k U_k
      double Kr[E], Ki[E], tr[E], ti[E];
      seg_mm<NB, true, false>(ur[0], ui[0], Gr, Gi, Kr, Ki);
      seg_mm<NB, false, false>(Kr, Ki, ur[0], ui[0], tr, ti);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        Gr[e] = act ? tr[e] : Gr[e];
        Gi[e] = act ? ti[e] : Gi[e];
      }
      // X = A_k = 2^J Â + μ_k I, u_j = 2^J (2^-J u_j) exactly
      const double2 su = *reinterpret_cast<const double2*>(rk[0] + 2);
      const double u1 = ldexp(su.x, J), u2 = ldexp(su.y, J);
      const double mkr = fma(u2, sp.mur[2], fma(u1, sp.mur[1], sp.mur[0]));
      const double mki = fma(u2, sp.mui[2], fma(u1, sp.mui[1], sp.mui[0]));
      // (the exact series takes the shifted Ã_k and e^{μ_k} as a factor: seg_contract_exact)
      const double dgr = ORD == 0 ? 0.0 : mkr, dgi = ORD == 0 ? 0.0 : mki;
      double xr[E], xi[E];
      if constexpr (XA) {  // from the formation's Â
#pragma unroll
        for (int e = 0; e < E; ++e) {
          xr[e] = (J ? ldexp(ar[0][e], J) : ar[0][e]) + (e % (NB + 1) == 0 ? dgr : 0.0);
          xi[e] = (J ? ldexp(ai[0][e], J) : ai[0][e]) + (e % (NB + 1) == 0 ? dgi : 0.0);
        }
      } else {  // re-read (blocks of 3 rows: Â is not kept live across the two products)
        const auto gen2 = gen_at(opaque(beta));
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double2 g0 = gen2(0, e), g1 = gen2(1, e), g2 = gen2(2, e);
          xr[e] = fma(u2, g2.x, fma(u1, g1.x, g0.x)) + (e % (NB + 1) == 0 ? dgr : 0.0);
          xi[e] = fma(u2, g2.y, fma(u1, g1.y, g0.y)) + (e % (NB + 1) == 0 ? dgi : 0.0);
        }
      }
      if constexpr (TS && !TSE) {
        // Re tr(X_k G_k), G_k = K_k U_k just formed (before its own source); the exact series' X is the shifted one,
        // so μ_k tr G_k is added apart.  Taken before G goes to its LDS row (GST) and the contraction needs the registers.
        double t_re = 0.0;
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int q = 0; q < NB; ++q)
            t_re = fma(xr[i * NB + q], Gr[q * NB + i], fma(-xi[i * NB + q], Gi[q * NB + i], t_re));
        if constexpr (ORD == 0) {
          double gtr = 0.0, gti = 0.0;
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            gtr += Gr[i * NB + i];
            gti += Gi[i * NB + i];
          }
          t_re = fma(mkr, gtr, fma(-mki, gti, t_re));
        }
        tsr += act ? t_re : 0.0;
      }
      double acc1, acc2;
      // The exact series on blocks of 3 rows keeps X, L and R live over its loop; with G beside them the kernel spills.
      // G rests in the lane's own row of the segment products' area (free after phase 2; the penalised kernels keep D
      // there) for the length of the contraction, through opaque copies of the segment index so that the row is not
      // promoted back to registers.  Lanes without a segment store nothing and read row 0 (their sums are dropped).
      constexpr bool GST = ORD == 0 && NB == 3 && !PEN;
      if constexpr (GST) {
        double2* const gp = slot + (size_t)opaque(sact ? s : 0) * E * nblk + beta;
        if (sact)
#pragma unroll
          for (int e = 0; e < E; ++e) gp[e * nblk] = make_double2(Gr[e], Gi[e]);
      }
      if constexpr (ORD == 0) {
        seg_contract_exact<NB>([&] { return gen_at(GREG ? beta : opaque(beta)); }, xr, xi, Kr, Ki, nex, rk[0][0],
                               rk[0][1], mu1r, mu1i, mu2r, mu2i, acc1, acc2);
      } else {
        seg_contract<NB, ORD, XA>(gen, xr, xi, Kr, Ki, mu1r, mu1i, mu2r, mu2i, acc1, acc2);
      }
      if constexpr (GST) {
        const double2* const gp = slot + (size_t)opaque(sact ? s : 0) * E * nblk + beta;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double2 v = gp[e * nblk];
          Gr[e] = v.x;
          Gi[e] = v.y;
        }
      }
      reduce(jj, act ? acc1 : 0.0, act ? acc2 : 0.0);
    }
  }
  if (turns || sprog.on) __builtin_amdgcn_s_setprio(0);
  BK_T(t4);
  BK_ADD(3, t4 - t3);
  SEGW_SET(16 + w, t4 - t0);
  if constexpr (TS) {
    // the lanes' sums: z on the phase-free loops' complex trace, a butterfly over the wave (the same order in every
    // launch), then the waves in order below, behind the barrier
    double v = su ? zr * tsr - zi * tsi : tsr;
    v = sact ? v : 0.0;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (l == 0) red[w] = v;
  }
  __syncthreads();
  if constexpr (TS) {
    if (tid == 0) {
      double sum = 0.0;
      for (int q = 0; q < W; ++q) sum += red[q];
      sp.dJdtau[b] = sum / tau;
    }
  }
  double* const og = sp.dJdu + (size_t)b * Nt * nu;
  for (int i = tid; i < Nt * nu; i += nthr) og[i] = dJ[i];
  if (MODE == BLKSEG_FUSED && sp.terms && tid == 0)
    atomicAdd(sp.terms + b % TERM_SLOTS, (unsigned long long)Nt * ((unsigned long long)P << J));
  BK_T(t5);
  BK_ADD(4, t5 - t4);
  BK_ADD(5, t5 - t0);
}

// The weighted sums of an ensemble launch (k_blkseg_eval's ENS instantiations): dJdu[p][i] = Σ_e w_e g[p E + e][i] and
// J[p] = Σ_e w_e Jm[p E + e], the members of pulse p being adjacent rows of g.  One thread per output element (VEC:
// per pair of them, 16-byte loads and stores: n even, 16-byte aligned buffers); the members are added in ascending e
// as acc = fma(w_e, v_e, acc) from 0, without atomics, so the result does not depend on scheduling.  The first B
// threads also sum the costs (J2: the caller's copy, or nullptr).  n = Nt nu; Jm stays as it is (the member costs).
template <bool VEC>
__global__ __launch_bounds__(256) void k_ens_reduce(int B, int E, int n, const double* __restrict__ w,
                                                    const double* __restrict__ g, const double* __restrict__ Jm,
                                                    double* __restrict__ dJdu, double* __restrict__ J,
                                                    double* __restrict__ J2) {
  const int nv = VEC ? n / 2 : n;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < (long long)B * nv) {
    const int p = (int)(idx / nv), i = (int)(idx - (long long)p * nv);
    if constexpr (VEC) {
      const double2* src = reinterpret_cast<const double2*>(g + (size_t)p * E * n) + i;
      double2 acc = make_double2(0.0, 0.0);
      for (int e = 0; e < E; ++e) {
        const double2 v = src[(size_t)e * nv];
        const double we = w[e];
        acc.x = fma(we, v.x, acc.x);
        acc.y = fma(we, v.y, acc.y);
      }
      reinterpret_cast<double2*>(dJdu + (size_t)p * n)[i] = acc;
    } else {
      const double* src = g + (size_t)p * E * n + i;
      double acc = 0.0;
      for (int e = 0; e < E; ++e) acc = fma(w[e], src[(size_t)e * n], acc);
      dJdu[(size_t)p * n + i] = acc;
    }
  }
  if (idx < B) {
    double acc = 0.0;
    for (int e = 0; e < E; ++e) acc = fma(w[e], Jm[(size_t)idx * E + e], acc);
    J[idx] = acc;
    if (J2) J2[idx] = acc;
  }
}

// The risk objectives over an ensemble (include/qoc.h qoc_set_ensemble_objective): from the member costs Jm[B][E] of
// a launch and the weights w[E], the member weights ω[B][E] (Σ_e ω_e = W = Σ_e w_e) and J̄ into J and J2.
//   QOC_ENS_MAX   e* = argmax over w_e > 0 (lowest e on ties), ω_{e*} = W, J̄ = W J_{e*}
//   QOC_ENS_CVAR  before_e = Σ w_f over the f ahead of e (J_f > J_e, or equal and f < e), in ascending f;
//                 ω_e = min(w_e, max(0, α W - before_e)) / α, J̄ = Σ_e ω_e J_e
//   QOC_ENS_LSE   M = max over w_e > 0, d_e = J_e - M, s = Σ_e (w_e / W) expm1(β d_e), J̄ = W (M + log1p(s) / β),
//                 ω_e = w_e exp(β d_e) / (1 + s)
// One wave per pulse (blockIdx.x), lane l owns members l, l + 64, ...; costs and weights are staged in LDS when they
// fit (LDS: 3 E doubles of dynamic LDS), otherwise read where they are, with the pulse's row of om as the scratch of
// the LSE terms: E is not capped.  Ranks are found by counting over all E costs (O(E^2 / 64) per wave).  Every sum
// over the members (W, s, before_e, J̄) is a serial loop in ascending member order (fma from 0 for s and J̄; zero ω
// skipped in J̄), so the result does not depend on the grid.  A non-finite cost among the members with w_e > 0 makes
// every ω of the pulse and J̄ NaN.
enum { ENS_OBJ_MEAN = 0, ENS_OBJ_MAX = 1, ENS_OBJ_CVAR = 2, ENS_OBJ_LSE = 3 };  // (= QOC_ENS_*)
template <bool LDS>
__global__ __launch_bounds__(64) void k_ens_weights(int E, int kind, double param, const double* __restrict__ w,
                                                    const double* __restrict__ Jm, double* __restrict__ om,
                                                    double* __restrict__ J, double* __restrict__ J2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int p = blockIdx.x, l = threadIdx.x;
  const double* Jp = Jm + (size_t)p * E;
  const double* wp = w;
  double* const op = om + (size_t)p * E;
  double* T = op;  // the LSE terms, then ω again for the J̄ sum
  if constexpr (LDS) {
    double* const sJ = reinterpret_cast<double*>(smem);
    double* const sw = sJ + E;
    for (int e = l; e < E; e += 64) {
      sJ[e] = Jp[e];
      sw[e] = w[e];
    }
    Jp = sJ;
    wp = sw;
    T = sw + E;
    __syncthreads();
  }
  // W in ascending order (every lane the same loop), the maximum with its lowest index, the non-finite flag
  double Wt = 0.0;
  for (int e = 0; e < E; ++e) Wt += wp[e];
  double M = -__builtin_inf();
  int im = 0x7fffffff, bad = 0;
  for (int e = l; e < E; e += 64) {
    if (!(wp[e] > 0.0)) continue;
    const double v = Jp[e];
    if (!isfinite(v)) bad = 1;
    if (v > M || im == 0x7fffffff) {  // (ascending e per lane: a tie keeps the lower index)
      M = v;
      im = e;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double oM = __shfl_xor(M, off);
    const int oi = __shfl_xor(im, off);
    bad |= __shfl_xor(bad, off);
    if (oi != 0x7fffffff && (im == 0x7fffffff || oM > M || (oM == M && oi < im))) {
      M = oM;
      im = oi;
    }
  }
  if (bad) {
    const double qn = __builtin_nan("");
    for (int e = l; e < E; e += 64) op[e] = qn;
    if (l == 0) {
      J[p] = qn;
      if (J2) J2[p] = qn;
    }
    return;
  }
  double s = 0.0;
  if (kind == ENS_OBJ_LSE) {
    for (int e = l; e < E; e += 64) T[e] = wp[e] > 0.0 ? expm1(param * (Jp[e] - M)) : 0.0;
    __syncthreads();
    for (int e = 0; e < E; ++e)
      if (wp[e] > 0.0) s = fma(wp[e] / Wt, T[e], s);
    __syncthreads();
  }
  const double aW = param * Wt;
  for (int e = l; e < E; e += 64) {
    const double we = wp[e], Je = Jp[e];
    double o;
    if (kind == ENS_OBJ_MAX) {
      o = e == im ? Wt : 0.0;
    } else if (kind == ENS_OBJ_CVAR) {
      double before = 0.0;
      for (int f = 0; f < E; ++f) {
        const double Jf = Jp[f];
        if (Jf > Je || (Jf == Je && f < e)) before += wp[f];
      }
      o = fmin(we, fmax(0.0, aW - before)) / param;
    } else {
      o = we > 0.0 ? we * exp(param * (Je - M)) / (1.0 + s) : 0.0;
    }
    op[e] = o;
    if constexpr (LDS) T[e] = o;
  }
  __syncthreads();  // (ω of the other lanes: LDS, or the pulse's own row of om in global memory)
  if (l == 0) {
    double Jb;
    if (kind == ENS_OBJ_LSE) {
      Jb = Wt * (M + log1p(s) / param);
    } else {
      Jb = 0.0;
      for (int e = 0; e < E; ++e) {
        const double o = T[e];
        if (o != 0.0) Jb = fma(o, Jp[e], Jb);
      }
    }
    J[p] = Jb;
    if (J2) J2[p] = Jb;
  }
}

// k_ens_reduce with per-pulse weights ω[B][E] (k_ens_weights): dJdu[p][i] = Σ_e ω_pe g[p E + e][i] in ascending e as
// acc = fma(ω_pe, v_e, acc) from 0.  A member whose ω is exactly 0 is skipped, not multiplied: its row may be stale or
// NaN (the member-aware backward leaves it alone), and a worst-case reduction reads one row per pulse, not E.  A NaN ω
// is not skipped.  J̄ is k_ens_weights' and is not touched here.
template <bool VEC>
__global__ __launch_bounds__(256) void k_ens_reduce_w(int B, int E, int n, const double* __restrict__ om,
                                                      const double* __restrict__ g, double* __restrict__ dJdu) {
  const int nv = VEC ? n / 2 : n;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * nv) return;
  const int p = (int)(idx / nv), i = (int)(idx - (long long)p * nv);
  const double* const op = om + (size_t)p * E;
  if constexpr (VEC) {
    const double2* src = reinterpret_cast<const double2*>(g + (size_t)p * E * n) + i;
    double2 acc = make_double2(0.0, 0.0);
    for (int e = 0; e < E; ++e) {
      const double oe = op[e];
      if (oe == 0.0) continue;
      const double2 v = src[(size_t)e * nv];
      acc.x = fma(oe, v.x, acc.x);
      acc.y = fma(oe, v.y, acc.y);
    }
    reinterpret_cast<double2*>(dJdu + (size_t)p * n)[i] = acc;
  } else {
    const double* src = g + (size_t)p * E * n + i;
    double acc = 0.0;
    for (int e = 0; e < E; ++e) {
      const double oe = op[e];
      if (oe == 0.0) continue;
      acc = fma(oe, src[(size_t)e * n], acc);
    }
    dJdu[(size_t)p * n + i] = acc;
  }
}

}  // namespace qoc

