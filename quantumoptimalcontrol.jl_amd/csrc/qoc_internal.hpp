// qoc_internal.hpp — host-side internals of libqoc_mi355x.so shared by its translation units.
//
// The library is compiled as several translation units in parallel (one per kernel family, __graft_entry__.build):
//   qoc_engine.hip        the C ABI (include/qoc.h), context setup, host math, RCCL epilogue
//   qoc_run.hip           run_forward / run_backward: the propagator chains and the per-slice gradient
//   qoc_run_expm.hip      the exponential kernels (k_expm, k_expm_rr*)
//   qoc_run_tchain.hip    the Taylor-action chains (k_tchain_*)
//   qoc_run_grad.hip      the fused order-3 gradient and the exact series gradient (k_grad_rr_*)
//   qoc_run_big.hip       the large-N GEMM pipeline, the GEMM-shaped gradient and the Fréchet gradient
//   qoc_run_ode.hip       the Tsit5 path, the envelope run and its discrete adjoint
//   qoc_run_blk.hip       the block chains and block gradient (generators with small invariant blocks), their router
//   qoc_run_blkp.hip      blocks of 5..16 rows on stored / interpolating propagators
//   qoc_run_blku.hip      blocks of <= 4 rows on block propagators
//   qoc_run_blkseg.hip    the segmented block eval (blocks of <= 3 rows: one launch for J and dJdu)
//   qoc_run_blkseg_ens.hip  its halves per (pulse, member) of a generator ensemble, the risk objectives' weights
// Each kernel template is launched from one translation unit only; the context (qoc_ctx) and the entry points
// between the units are declared here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/qoc.h"
#include "qoc_chain.hpp"
#include "qoc_comm.hpp"
#include "qoc_devbuf.hpp"
#include "qoc_tchain.hpp"

namespace qoc {
struct BlkArgs;  // qoc_blk.hpp
}
using namespace qoc;

// launch shape of the segmented block eval (qoc_run_blkseg.hip blkseg_shape)
struct BlksegShape {
  int W, S, L, UPW, RB;
  size_t lds;
};

// qoc_eval_envelope's launch shape (qoc_run_ode.hip env_grad_plan): checkpoint spacing, checkpoints per column,
// conjugate-transposed generator copies in LDS, column waves, the gradient kernel's dynamic LDS
struct EnvGradPlan {
  int C = 1, nseg = 0, W = 1;
  bool tr = false;
  size_t lds = 0;
};

// The last successful forward (propagate / eval).  Plain: x_k of the u in d_u are in d_X and nothing else is kept.
struct LastFwd {
  // The states (or what rebuilds them) are there.  A setter that changes the system (the model's "cleared") clears this
  // member alone, after blk_materialize: every reader of the others asks for it first, and qoc_get_info goes on
  // reporting the dropped forward's kind, captures and formation until the next forward's reset.
  bool valid = false;
  // what a propagate left for grape_sensitivity (the reference's split call form, examples/ipopt_callbacks_exp.jl:
  // 11-31): 0 states in d_X (every path), 1 the segmented forward's G at every segment end (d_gseg, qoc_blkseg.hpp
  // BLKSEG_FWD), 2 the stored block propagators and states of blocks of 5..16 rows (d_blkU + d_X, qoc_blkp.hpp; or the
  // interpolating chains' states alone, ichain)
  int kind = 0;
  // the segmented block eval (qoc_blkseg.hpp) writes neither x_k nor λ_k: qoc_get_states / a later backward rebuild
  // the states on demand (blku_states) from the u in d_u, with J and the coefficients going to scratch
  bool lazy = false;
  bool captured = false;  // the Taylor-action chain wrote its captures (d_pws)
  // kind 2, blkp_forward's leftovers: it ran the interpolating chains (k_blkp_ichain, no stored propagators:
  // grape_sensitivity's μ recurrence interpolates from the same coefficients); the wave blocks it ran on (the live
  // ones, or all with a co-state source); its propagators were interpolated (the exact backward needs N_i).
  // blkp_backward rewrites the first two when it forms the propagators of another layout.
  bool ichain = false;
  int nwb = 0;
  bool interp = false;
  // The step records in d_steps.  They describe that buffer rather than the forward, and a backward's re-prep
  // (blk_backward) rewrites them; they are here because only a forward makes them stale: every path that reads the
  // records preps in its own forward, except after one on propagators formed without them (blkp), which says so.
  bool steps_old = false;  // not this u's: re-prep first
  bool steps_cheb = false;   // what tchain_prep wrote: Chebyshev coefficients (the backward pass reuses its steps)
  // report only (qoc_get_info), of the last block-propagator formation: the degree it was planned with (blkp_plan; 0:
  // exponentials) and the chains that ran on it (0: stored, 1: interpolating, every entry, 2: the symmetric
  // propagators' upper triangle; blkp_backward writes 0 when it re-forms)
  int formed_D = 0;
  int formed_ichain = 0;
};
// The last successful backward (grape_sensitivity / eval).  Plain: λ_k in d_L.
struct LastBwd {
  bool is_mu = false;  // d_L holds μ_k (qoc_get_costates applies the coefficients d_coef_mu)
  bool lazy = false;   // the fused block backward left d_L unwritten: qoc_get_costates rebuilds it (blku_costates)
                       // from the saved u and λ_N coefficients (d_u_lam, d_coef_lam)
  int route = 0;       // qoc_get_info: 0 other, 1 captured sequential backward, 2 / 3 concurrent μ mode on two streams /
                       // in one dual launch, 4 block chains, 5 fused block gradient, 6 segmented block eval, 7 stored
                       // propagators of blocks of 5..16 rows
};
// The forward whose J is in d_J, for qoc_allgather_best (the setters leave it).  Plain: k_argmin_seed finds the pair.
struct LastJ {
  bool ready = false;   // the eval already wrote this rank's best (J, seed) into the gathered slot
  bool direct = false;  // and the final pair into the result slot and best_out
};

struct qoc_ctx {
  int dev = 0, N = 0, m = 0, nu = 0, Nt = 0, B = 0, prec = QOC_FP64;
  size_t esz = 16;  // bytes per complex element on device
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;        // gradient ranges overlapped with the backward chain
  std::vector<hipEvent_t> sync_ev;      // cross-stream ordering events (no timing)
  int bwd_chunks = 4;                   // slice ranges of the overlapped backward chain (1: not overlapped)
  double bwd_last_frac = 0.5;           // last range's length relative to the others
  int bwd_prio = 0;                     // bit 0: s_setprio in the chain; bit 1: low-priority gradient stream
  int bwd_prestate = 2;                 // P1, P2 of every slice beside the first backward range (k_grad_rr_s): 0 off, 1 on, 2 auto
  // Every device allocation of the context is a DevBuf (qoc_devbuf.hpp) that reports to mem; mem.bytes is info[3] of
  // qoc_get_info.  Whether a buffer is counted is said here, at its declaration, and nowhere else.  kUncounted without
  // a remark: as before (it never was counted; DESIGN.md lists them); d_env_ws has a reason of its own.
  DevLedger mem;
  DevBuf<void> d_A{mem, kCounted};    // (nu+1) x N*N
  DevBuf<void> d_x0{mem, kCounted};   // N*m or B*N*m
  int x0_per_seed = 0;
  DevBuf<void> d_Xt{mem, kCounted};   // N*m target
  int cost_kind = QOC_COST_TRACE;
  double cost_n = 1.0;
  DevBuf<unsigned char> d_pmask{mem, kCounted};
  double mu = 0.0;
  DevBuf<void> d_src{mem, kCounted};   // B x (Nt+1) x N x m caller's dL/dx(x_k) (qoc_set_costate_source), device precision
  bool src_on = false;
  DevBuf<double> d_u{mem, kCounted};     // B*nu*Nt, u of the last propagate
  DevBuf<void> d_U{mem, kCounted};       // B*Nt*N*N
  DevBuf<void> d_X{mem, kCounted};       // B*(Nt+1)*N*m
  DevBuf<void> d_L{mem, kCounted};       // B*(Nt+1)*N*m
  DevBuf<double> d_J{mem, kCounted};     // B
  DevBuf<cx<double>> d_coef{mem, kCounted};  // B*m
  DevBuf<double> d_dJdu{mem, kCounted};  // B*nu*Nt
  DevBuf<int> d_flag{mem, kCounted};
  DevBuf<double> d_sink{mem, kCounted};  // TCHAIN_SINK doubles: the MFMA chains' branch-free stores of lanes without an element
  DevBuf<unsigned long long> d_hist{mem, kCounted};  // 5*64 reference (Padé) selection + 8*64 executed Taylor (r, s) / T12 s
  int chain_cb_fwd = 0, chain_cb_bwd = 0;  // 0: chain_shape's column block; QOC_CHAIN_CB_FWD / _BWD = 1 | 2 (N > 32)
  int expm_alg = 1;  // 1 Taylor: register-resident T12 (default), 2 LDS Paterson-Stockmeyer (QOC_EXPM_LDS=1), 0 Padé (QOC_EXPM_PADE=1)
  int prop_method = 0;                   // QOC_PROP_EXPM / QOC_PROP_TSIT5
  int nsub = 10;                         // Tsit5 steps per slice (reference dt = 0.1 Δt)
  int ode_kernel = 0;                    // 0 register-resident rows when N fits, 1 LDS rows (QOC_ODE_LDS=1)
  DevBuf<double> d_stage{mem, kUncounted};             // host->device staging (fp64 complex), max(B*N*m, (nu+1)*N*N)*2
  std::vector<double> h_u;
  std::vector<double> h_coef;  // spline coefficients of the last qoc_propagate_spline
  // live per-kernel timing (hipEvents recorded on `stream` around each hot-path launch)
  bool profiling = false;
  struct Mark {
    int phase;
    hipEvent_t a, b;
  };
  std::vector<Mark> marks;
  std::vector<hipEvent_t> event_pool;
  double phase_ms[4] = {0, 0, 0, 0};
  long long phase_n[4] = {0, 0, 0, 0};
  // large-N path: every k_bgemm launch bracketed while profiling (algorithmic FLOPs per launch)
  struct GMark {
    hipEvent_t a, b;
    double flops;
  };
  std::vector<GMark> gmarks;
  double gemm_ms = 0, gemm_flops = 0;
  long long gemm_n = 0;
  // large-N path (N beyond the LDS-resident kernels): chunked batched-GEMM pipeline
  bool big = false;
  int chunk = 0;                // slices per chunk
  DevBuf<void> d_ws{mem, kCounted};         // chunk workspace
  DevBuf<double> d_red{mem, kCounted};      // per-item reductions (chunk + 8 doubles)
  long long big_hist[5 * 64] = {};
  long long big_thist[9 * 64] = {};  // executed Taylor (r, s) on the large-N path; row 8: T8
  long long ns_iters = 0;       // Newton-Schulz iterations executed (all chunks)
  // skew-Hermitian generators: ρ_j = ||A_j||_2 (host tridiagonalisation + bisection at qoc_set_generators); the
  // chunk's Taylor degree / squarings then follow the 2-norm bound Σ_j |c_jk| ρ_j instead of the 1-norm
  double big_rho[9] = {};
  bool big_rho_ok = false;
  // spline parameterisation (examples/ipopt_callbacks_exp.jl:13-14, 28)
  DevBuf<double> d_Bs{mem, kUncounted};  // Nt x ns
  int ns = 0;
  DevBuf<double> d_cstage{mem, kUncounted};  // host-pointer variants: B x ns x nu coefficients / gradient
  // GEMM-shaped gradient of the LDS-resident path (order 3, N >= 32: below that the 64-row GEMM tiles
  // are mostly padding and the per-slice k_grad is faster): generator layouts + P/Q/W workspace
  DevBuf<void> d_AH{mem, kCounted};    // (nu+1) x N*N: [A0^H | A1^H | ...]
  DevBuf<void> d_Cst{mem, kCounted};   // nu N x N: [A1; A2; ...]
  DevBuf<void> d_gws{mem, kCounted};   // 6 x N x B(Nt+1)m
  DevBuf<void> d_pws{mem, kCounted};   // 2 x N x B(Nt+1)m: P1, P2 of the state-side gradient pass (bwd_prestate)
  bool grad_gemm = true;
  bool grad_rr = false;  // fused register-resident order-3 gradient (qoc_grad_rr.hpp)
  DevBuf<int> d_ps{mem, kCounted};   // k_expm_rr pass-2 counter + list of Paterson-Stockmeyer units
  double a0norm = 0.0;   // ||A0||_1 of the generators (host-side, at qoc_set_generators)
  // exponential that runs: expm_alg, except that when every slice has a large norm (||A0||_1 > 4 theta_12,
  // tunable bus: ||A_k||_1 ~ 30) the default register-resident Taylor hands over to the reference's own Padé-13
  // + solve (k_expm ALG 0): over 2000 chained slices only the same algorithm holds |ΔJ| <= 1e-12 against the
  // reference (Paterson-Stockmeyer: 1.6e-12).  QOC_EXPM_PS=1 keeps Paterson-Stockmeyer there (1.8x faster).
  int expm_run = 1;
  bool expm_ps = false;
  int ncu = 256;         // compute units of the device (persistent-grid sizing)
  // Taylor-action chains (qoc_tchain.hpp): x_{k+1} = exp(A_k) x_k applied to the state, no U_k formed.
  // chain_mode 1 selects them (QOC_CHAIN=taylor / expm overrides the automatic choice at qoc_set_generators)
  int chain_mode = 0;            // 0: propagators (k_expm + k_chain_*), 1: Taylor action (k_tchain_*)
  int chain_req = QOC_CHAIN_AUTO;  // what qoc_set_chain asked for (kept across qoc_set_generators)
  bool tchain_ok = false;        // the shape fits the Taylor-action kernels
  DevBuf<void> d_At{mem, kCounted};          // (nu+1) N x N shifted generators Ã_j = A_j - μ_j I
  DevBuf<TStep> d_steps{mem, kCounted};      // B x Nt (P, s, e^{μ_k})
  DevBuf<unsigned long long> d_terms{mem, kCounted};  // Σ P s per forward (executed Taylor terms per direction)
  TChainParams tprm{};
  bool cheb_ok = false;          // generators skew-Hermitian with imaginary shifts: Chebyshev applies
  bool cheb = false;             // Chebyshev terms (k_tchain_prep_cheb) instead of Taylor (QOC_TCHAIN_POLY=taylor)
  DevBuf<double> d_tcoef{mem, kCounted};     // B x Nt x TCHEB_STRIDE Chebyshev coefficients (allocated on first use)
  long long props_since_reset = 0;  // forward passes since the last Padé-histogram reset (chain mode 1)
  // Captured products (register-resident MFMA chains, order-3 fused gradient): the chains write their first two
  // products per slice (forward -> d_pws, backward -> d_gws) and the gradient is k_grad_rr_c, contractions only.
  bool cap_ok = false;           // the shape takes it (qoc_set_generators; QOC_CAPTURE=0 turns it off)
  // qoc_eval_dev with a built-in cost and no penalty / co-state source: the backward recurrence runs from X_target
  // (μ_k, λ_k = coef ⊙ μ_k) beside the forward chain: 1 (default) both in one launch (k_tchain_mf_dual), 2 two
  // launches on two streams, 0 off (QOC_CONCURRENT)
  int concurrent = 1;
  // the MFMA chains with the state in registers (TChainRot): 1 (default) for N <= 32 with nu <= 2, 3 also for
  // N <= 48 (generators in LDS), 0 off: TChainMF everywhere (QOC_TCHAIN_ROT)
  int tchain_rot = 1;
  DevBuf<double> d_u_lam{mem, kCounted};     // B x Nt x nu: u of the backward that left λ_k to be rebuilt (bwd.lazy)
  DevBuf<void> d_blkU{mem, kCounted};        // B x Nt x NB^2 x nblk complex: block propagators of the eval's forward (fused backward;
                                             // reallocated when a new block layout needs more)
  // one control: the propagators interpolated in u (qoc_blkp.hpp k_blkp_int): the coefficient matrices of the control
  // range [int_lo, int_hi] for the live-wave layout int_wrow, degree int_D (int_ok: valid for the current generators)
  DevBuf<double2> d_blkp_M{mem, kUncounted};
  bool int_ok = false;
  int int_D = 0;
  std::vector<int> int_Db;           // per live wave block
  double int_lo = 0.0, int_hi = 0.0;
  std::vector<int> int_wrow;
  bool int_sym = false;              // complex-symmetric generators on one live wave block: d_blkp_M also holds its
  int int_nl = 0;                    // packed upper triangle of int_nl live rows, from element int_nfull on
  size_t int_nfull = 0;
  // the exact gradient's coefficients N_i (dU/du on the same curve, k_blkp_grad_exact) beside them, recomputed with
  // them: degree int_E (per block int_Eb), the full layout from element int_noff, the triangle from int_nsoff
  int int_E = 0;
  std::vector<int> int_Eb;
  size_t int_noff = 0, int_nsoff = 0;
  bool int_failed = false;           // [int_fail_lo, int_fail_hi] did not converge (a wider range will not either)
  double int_fail_lo = 0.0, int_fail_hi = 0.0;
  DevBuf<double> d_minmax{mem, kUncounted};        // k_minmax partials (256 blocks x 2)
  DevBuf<double> h_minmax{mem, kUncounted, hipHostMallocDefault};  // pinned host copy
  DevBuf<double2> d_blkp_ph{mem, kUncounted};      // B x Nt: e^{μ(u_k)} for the interpolating chains (k_blkp_phase)
  DevBuf<double> d_blkp_ctab{mem, kUncounted}; // the Chebyshev form's coefficient table (qoc_blkp.hpp blkp_cheb), for ctab_cm / ctab_rmax
  int ctab_cm = 0;
  double ctab_rmax = 0.0;
  DevBuf<double2> d_gseg{mem, kCounted};         // B x NB^2 x S x nblk complex: the segmented forward's G at every segment end (fwd.kind 1)
  // the segmented eval's launch shape, kept between evals: valid while the sizes it was derived from (seg_key: B, Nt,
  // N, m, nu, block rows, blocks, penalised or not, ensemble members) are the context's; the QOC_BLKSEG_W / _S / _RB switches are read
  // when it is derived.  seg_attr[NB - 2][order - 1, exact: 4][mode][penalised]: this context has raised that k_blkseg_eval
  // instance's dynamic-LDS limit (blkseg_lds_attr)
  mutable BlksegShape seg_shape{};
  mutable int seg_key[9] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
  bool seg_attr[2][5][3][2] = {};  // [..][penalised]; order slot 4: the exact instantiation (ORD 0)
  bool seg_attr_ens[2][5][2] = {};  // the same for the ensemble instantiations (fused only)
  // the state penalty as the segmented eval takes it (blkseg_pen): per block row i a bit mask over the blocks
  // (seg_prow[i], bit β: row i of block β is in P) and a bit mask over the columns C; derived from h_pen_rows /
  // h_pen_cols and the block rows h_brow, invalidated by qoc_set_state_penalty and by a new block layout
  mutable bool seg_pen_valid = false;
  mutable unsigned int seg_prow[3] = {0, 0, 0}, seg_pcol = 0;
  std::vector<int> h_brow;           // nblk x blk_nb rows of each block (-1 padding), the host's copy of d_brow
  // A generator ensemble (qoc_set_generator_ensemble): ens_E > 0 sets evaluated for every pulse, one workgroup of the
  // segmented eval per (pulse, member) and k_ens_reduce behind it (qoc_blkseg.hpp).  The block layout stays the
  // nominal set's.  Everything below is allocated by the setter, counted in info[3] and freed when the
  // ensemble is cleared (E = 0, qoc_set_generators) and at qoc_destroy.
  int ens_E = 0;
  DevBuf<double2> d_ens_gtab{mem, kCounted};     // [E][nblk][3][blk_nb^2]: the members' shifted generator blocks (blk_gen_table)
  DevBuf<double> d_ens_prm{mem, kCounted};       // E x 9: rad[3] | mur[3] | mui[3] of each member (gen_shift_bounds)
  DevBuf<double> d_ens_w{mem, kCounted};         // E weights, as given
  DevBuf<double> d_ens_J{mem, kCounted};         // B x E member costs of the last ensemble eval (qoc_member_costs_dev)
  DevBuf<cx<double>> d_ens_coef{mem, kCounted};  // B x E x 2m λ_N coefficients
  DevBuf<double> d_ens_g{mem, kCounted};         // B x E x Nt x nu member gradients
  bool ens_costs = false;            // d_ens_J holds an eval's costs
  // The ensemble's objective (qoc_set_ensemble_objective): a setting of the context that outlives the ensemble.
  // Under a non-mean objective an ensemble eval forms per-pulse member weights ω (k_ens_weights) and takes one of two
  // routes: 1 = the fused launch for every (pulse, member), 2 = the forward half for all, the backward half where ω
  // is not 0.  ens_route is derived by blkseg_ens_plan from the objective, the weights and QOC_ENS_SKIP whenever one of
  // the two setters completes the pair (ensemble + non-mean objective); that setter also allocates ω and, for route 2,
  // G (and D) at the segment ends per (pulse, member).  Counted in info[3], freed with the ensemble.
  int ens_obj = 0;                   // QOC_ENS_MEAN / _MAX / _CVAR / _LSE
  double ens_obj_param = 0.0;        // α (CVaR) or β (LSE), else 0
  int ens_route = 1;                 // the route the next eval under a non-mean objective takes
  int ens_last_route = 0;            // the last ensemble eval's: 0 = none since a setter, 1 = fused, 2 = forward + active backward
  std::vector<double> h_ens_w;       // the weights, host copy
  DevBuf<double> d_ens_om{mem, kCounted};        // B x E member weights ω of the last eval under a non-mean objective
  DevBuf<double2> d_ens_gseg{mem, kCounted};     // B E x NB^2 x S x nblk complex G at the segment ends, and D behind it when penalised
  bool seg_attr_ens_half[2][5][2][2] = {};  // [NB - 2][order slot][forward, backward][penalised]: seg_attr for the ENS halves
  // The gate duration as a per-seed variable (qoc_set_time_scale): while ts_on, qoc_eval_dev runs the segmented
  // eval's TS instantiations (blkseg_eval_ts), which read τ_b from d_ts at launch and leave dJ_b/dτ_b behind it.  A
  // setting of the context: it survives qoc_set_generators, qoc_set_x0 and qoc_set_cost.  Allocated by the setter
  // (counted in info[3]), freed when the scale is cleared and at qoc_destroy.
  bool ts_on = false;
  bool ts_grad = false;              // d_ts + B holds an eval's dJ/dτ
  DevBuf<double> d_ts{mem, kCounted};            // 2 B: τ_b | dJ_b/dτ_b of the last eval under the scale
  bool seg_attr_ts[2][5][3][2] = {};  // seg_attr for the TS instantiations
  DevBuf<int> h_flag{mem, kUncounted, hipHostMallocMapped | hipHostMallocCoherent};  // host-mapped stale-u flag of the queued check (k_compare_u_flags)
  int flag_turn = 0;                 // which of the two device flags d_flag[0 / 1] the next queued check writes
  hipEvent_t flag_ev = nullptr;      // recorded after that copy
  DevBuf<double> d_J_scr{mem, kCounted};         // B
  DevBuf<cx<double>> d_coef_scr{mem, kCounted};  // B x 2m
  // every generator exactly skew-Hermitian (|A + A^H| <= 4 eps max|A|): the slice propagators are unitary, which the
  // segmented eval's backward relies on (λ_{k+1} = U_k λ_k)
  bool skew_exact = false;
  DevBuf<cx<double>> d_coef_lam{mem, kCounted};  // B x 2m: its λ_N coefficients
  DevBuf<cx<double>> d_coef_mu{mem, kCounted};  // B x 2m: the λ_N coefficients of the eval that left μ in d_L
  // generators with small invariant blocks (qoc_blk.hpp, detected at qoc_set_generators; QOC_BLOCKS=0 off): the
  // chains and the gradient run per block
  int blk_nb = 0;                // padded block size 2 / 3 / 4 (VALU lanes), 16 (MFMA block waves), 0: no block path
  int nblk = 0;                  // blocks
  DevBuf<int> d_brow{mem, kCounted};         // nblk x blk_nb rows of each block (-1 padding)
  DevBuf<double2> d_gtab{mem, kCounted};     // blocks of <= 3 rows: [nblk][3][blk_nb^2] shifted generator blocks (blk_detect)
  int blk_jr = 0;                // chain kernels: 0 VALU lanes (k_blk_*), 1 / 4 MFMA block waves (k_blkrot_*<JR>)
  bool blk_real = false;         // MFMA block waves on the real embedding of blocks of <= 2 rows (k_blkrot_*<0>)
  int nwb = 0;                   // MFMA block waves per column pair
  DevBuf<int> d_wrow{mem, kCounted};         // nwb x 16 rows of each wave's state (-1 padding)
  std::vector<int> h_wrow;       // host copy (blocks of 5..16 rows: one wave per block)
  // blocks of 5..16 rows with x_0 and X_target zero on their rows (blk_live): the waves of the others, the dead rows
  std::vector<int> h_wrow_live, h_dead_rows;
  DevBuf<double> d_gc_part{mem, kCounted};   // large-N gradient: per (slice, column block) partial traces (k_gen_contract2)
  // the dead rows known to hold zeros (blk_zero_dead) and the state-shaped buffers, up to six, that hold them there:
  // a backward with an external λ_N or a co-state source (the only writers of nonzero values into rows whose x0 and
  // target are zero) sets dead_dirty, after which no buffer counts
  std::vector<int> h_dead_zeroed;
  const void* dead_bufs[6] = {};
  bool dead_dirty = true;
  DevBuf<int> d_wrow_live{mem, kUncounted};
  DevBuf<int> d_dead_rows{mem, kUncounted};
  DevBuf<double> d_blkrec{mem, kCounted};    // block propagators: B x Ntp x BLKU_REC step records (k_blku_rec, allocated on first use)
  // multi-GPU epilogue (qoc_comm.hpp): RCCL communicator over the ranks' contexts
  ncclComm_t comm = nullptr;
  int world = 1, rank = 0;
  long long seed_offset = 0;   // global id of this context's seed 0
  DevBuf<double> d_best{mem, kUncounted};    // [2 local | 2 x world gathered | 2 result]
  DevBuf<unsigned int> d_done{mem, kUncounted};  // the segmented eval's workgroup counter (its last workgroup finds the best pair)
  double* best_out = nullptr;  // qoc_set_best_output's buffer
  // exact (Fréchet) gradient mode workspace, allocated on first use
  DevBuf<void> d_fws{mem, kUncounted};  // (grown when a call needs more)
  // the exact gradient as a series on dense generators (qoc_grad_rr.hpp k_grad_rr_x*, qoc_run_grad.hip grad_rr_exact);
  // its R(b) workspace is d_fws
  bool exact_series = true;             // QOC_GRAD_EXACT_SERIES=0 at qoc_create: the block exponential everywhere
  DevBuf<unsigned long long> d_xn{mem, kCounted};   // [0] max n_k, [1] Σ n_k of the last call, then B x Nt term counts (first use)
  size_t xws_budget = 0;                // workspace budget: min(2 GiB, free / 8) or QOC_GRAD_EXACT_WS_MB (first use)
  long long xs_stats[4] = {0, 0, 0, 0};  // qoc_exact_series_stats: units, Σ n_k, largest n_k, fallbacks over the cap
  // qoc_eval_envelope (qoc_ode_grad.hpp): the checkpoints (x_n, k1_n) every env C steps, scratch that no later call
  // reads (grown on demand, not counted in info[3]: qoc_get_info reports what qoc_propagate_envelope would leave);
  // the host form's parameters, gradient and caller's λ_N; QOC_ENV_CKPT at qoc_create forces the spacing (0: chosen per
  // call); the checkpoint budget min(1 GiB, free / 4) or QOC_ENV_WS_MB, read at first use
  DevBuf<void> d_env_ws{mem, kUncounted};
  DevBuf<double> d_env_p{mem, kUncounted};   // B x 64 parameters | B x 64 gradient
  DevBuf<void> d_env_lam{mem, kUncounted};   // B x N x m
  int env_ckpt = 0;
  size_t env_budget = 0;
  // packed states (compress_states, src/utils.jl:96-109): two parity sectors share the kernels' columns, so the
  // chains and the gradient run on m = max(n1, n2) columns instead of the caller's m_user = n1 + n2
  int m_user = 0;                       // columns of the caller's states (qoc_create's m)
  bool packed = false;
  std::vector<unsigned char> h_rsec;    // N row sectors (0 / 1)
  std::vector<int> pk_cols[2];          // original columns of sector s: packed column i holds pk_cols[s][i]
  std::vector<int> pk_pos[2];           // m_user: packed column of original column c in sector s, or -1
  int zmap[4] = {0, 1, 2, 3};           // z-calibrated cost: original column c -> s m + i
  DevBuf<unsigned char> d_rsec{mem, kCounted};
  bool grad_rr_any_m = false;           // the fused gradient fits apart from the column count
  // caller-layout copies, re-packed when the packing changes
  std::vector<double> h_gen, h_x0, h_Xt;
  std::vector<int> h_pen_rows, h_pen_cols;
  bool have_gen = false, have_x0 = false, have_cost = false;
  // What the last calls left: the three snapshots of the model in tests/engine_model.py (its table lists, per call, what
  // happens to each).  A forward, an eval and a backward assign the plain record first (c->fwd = {}, c->bwd = {}); a
  // path then writes the members it leaves different, after the launch that makes them so.
  LastFwd fwd;    // the model's fwd
  LastBwd bwd;    // the model's bwd
  LastJ jbest;    // the model's jfwd
  std::string err;
};

namespace qoc_host {

extern thread_local std::string g_err;
int fail(qoc_ctx* ctx, int code, const char* fmt, ...);

#define HIPCHK(ctx, expr)                                                                     \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(ctx, QOC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

constexpr int kChainMaxN = 64;

// The one way to read a switch from the environment (one lookup each: several sit on the per-call path).  env_set: the
// variable exists; env_int / env_dbl: its atoi / atof when it does, else dflt; env_is: it exists and is exactly one of
// the literals.
static inline bool env_set(const char* name) { return getenv(name) != nullptr; }
static inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
static inline double env_dbl(const char* name, double dflt) {
  const char* e = getenv(name);
  return e ? atof(e) : dflt;
}
template <typename... L>
static inline bool env_is(const char* name, L... lits) {
  const char* e = getenv(name);
  return e && (... || !std::strcmp(e, lits));
}

// ---- qoc_engine.hip: staging, packed states, timing marks, dispatch ----
int upload(qoc_ctx* ctx, const double* host, void* dev, size_t nelem);
int download(qoc_ctx* ctx, const void* dev, double* host, size_t nelem);
bool grad_rr_cols(int m);
Sectors sectors(const qoc_ctx* c);
int upload_states(qoc_ctx* c, const double* host, void* dev, size_t count, const char* what);
int download_states(qoc_ctx* c, const void* dev, double* host);
hipEvent_t take_event(qoc_ctx* c);
int mark_begin(qoc_ctx* c, int phase, hipStream_t s = nullptr);
void mark_end(qoc_ctx* c, int idx, hipStream_t s = nullptr);
RcclApi& rccl();

// the shift and bound of one exactly skew-Hermitian generator (N x N, column-major interleaved): μ = -i c with c the
// centre of the spectral interval of H = i A, rad its half-width with the eigenvalue solver's margin
void gen_shift_bounds(const double* G, int N, double& mur, double& mui, double& rad);
// |A + A^H| of one generator against its largest entry: skew (Chebyshev's bar) and exact (the segmented eval's)
void gen_skew_test(const double* G, int N, bool& skew, bool& exact);

// ---- qoc_run_expm.hip ----
bool expm_supported(int N, int prec);
// alg 0: Padé + solve (reference algorithm); alg 1: register-resident Taylor T12; alg 2: LDS Paterson-Stockmeyer.
hipError_t launch_expm(int prec, hipStream_t s, int N, int nu, int nunits, const void* Agen, const double* u,
                       const void* Ain, void* Uout, unsigned long long* hist, int* deg, int* sq, int alg = 0,
                       unsigned long long* thist = nullptr, int* ps = nullptr, bool mix = false);

// ---- qoc_run.hip ----
template <typename T>
int run_forward(qoc_ctx* c);
template <typename T>
int run_backward(qoc_ctx* c, int order, double* d_dJdu);
template <typename T>
int dense_gradient(qoc_ctx* c, int order, double* d_dJdu);

// ---- qoc_run_big.hip ----
size_t big_ws_elems_per_item(int N, int m);
// extreme eigenvalues of the Hermitian H = i A of a skew-Hermitian generator (column-major interleaved N x N):
// Householder tridiagonalisation + Sturm bisection, O(N^3), any N
void herm_extremes(const double* A, int N, double& lmin, double& lmax);
template <typename T>
int big_forward(qoc_ctx* c);
template <typename T>
int big_backward(qoc_ctx* c, int order, double* d_dJdu);
template <typename T>
int grad_gemm_o3(qoc_ctx* c, double* d_dJdu);
template <typename T>
int frechet_grad(qoc_ctx* c, double* d_dJdu);
hipError_t launch_gen_aux(qoc_ctx* c);

// ---- qoc_run_grad.hip ----
template <typename T>
int grad_rr_o3(qoc_ctx* c, double* d_dJdu, hipStream_t st, int k0, int nk, int mode = 0);
// k_grad_rr_c: the order-3 contraction from the chains' captures (mu_mode: L holds μ, λ = coef ⊙ μ)
int grad_rr_cap(qoc_ctx* c, double* d_dJdu, hipStream_t st, int k0, int nk, bool mu_mode);
// QOC_DUKDP_EXACT on dense generators as a series (k_grad_rr_xn / _xq / _xp).  1 (nothing written to d_dJdu): the
// route does not apply, or the largest term count exceeds GRADX_NMAX: the caller runs frechet_grad
template <typename T>
int grad_rr_exact(qoc_ctx* c, double* d_dJdu);

// ---- qoc_run_ode.hip ----
template <typename T>
int ode_forward(qoc_ctx* c);
template <typename T>
int ode_adjoint(qoc_ctx* c);
hipError_t launch_envelope(qoc_ctx* c, int kind, const double* dP, int np, double dt, long long nsteps);
hipError_t launch_terminal_cost(qoc_ctx* c);
int env_grad_plan(qoc_ctx* c, long long nsteps, EnvGradPlan* pl);
hipError_t launch_envelope_ckpt(qoc_ctx* c, int kind, const double* dP, int np, double dt, long long nsteps,
                                const EnvGradPlan& pl);
hipError_t launch_envelope_grad(qoc_ctx* c, int kind, const double* dP, int np, double dt, long long nsteps,
                                const EnvGradPlan& pl, const void* d_lam, double* d_dJdp);

// ---- qoc_run_tchain.hip ----
bool tchain_mf(const qoc_ctx* c);
bool tchain_mf_rot(const qoc_ctx* c);
template <typename T>
int tchain_forward(qoc_ctx* c);
// flags: TB_CAPTURE (write the backward captures), TB_MU (start from X_target: μ mode); st: nullptr = c->stream
enum { TB_CAPTURE = 1, TB_MU = 2 };
template <typename T>
int tchain_backward(qoc_ctx* c, int k_lo = 0, int k_hi = -1, hipStream_t st = nullptr, int flags = 0);
template <typename T>
int tchain_backward_captured(qoc_ctx* c, double* d_dJdu);
template <typename T>
int tchain_eval_concurrent(qoc_ctx* c, double* d_dJdu);
bool tchain_concurrent_ok(const qoc_ctx* c, int order);
bool tchain_cap_ok(const qoc_ctx* c);
int ensure_pws(qoc_ctx* c);
int ensure_stream2(qoc_ctx* c, int nev);
template <typename T>
int tchain_backward_overlapped(qoc_ctx* c, double* d_dJdu);
hipError_t launch_pade_units(qoc_ctx* c, long long units);
TChainArgs tchain_args(qoc_ctx* c);
int tchain_prep(qoc_ctx* c);

// ---- qoc_run_blk.hip ----
int blk_detect(qoc_ctx* c);
// the segmented eval's table of one generator set on the block rows brow (nblk x NB): [nblk][3][NB^2] complex into tab;
// gen: (nu + 1) x N x N column-major interleaved, mur / mui: the shifts taken off the diagonals
void blk_gen_table(const qoc_ctx* c, const std::vector<int>& brow, int NB, int nblk, const double* gen,
                   const double* mur, const double* mui, double* tab);
bool blk_active(const qoc_ctx* c);
bool blk_rot(const qoc_ctx* c);
bool blku_on(const qoc_ctx* c);  // blocks of <= 4 rows on block propagators (qoc_blku.hpp)
bool blkp_on(const qoc_ctx* c);  // blocks of 5..16 rows: the concurrent eval on stored propagators (qoc_blkp.hpp)
int blk_forward(qoc_ctx* c);
int blk_backward(qoc_ctx* c, int order, double* d_dJdu);
bool blk_concurrent_ok(const qoc_ctx* c, int order);
int blk_eval_concurrent(qoc_ctx* c, int order, double* d_dJdu);
int blk_materialize(qoc_ctx* c);  // rebuild every lazily kept x_k / λ_k (before a setter changes what they need)
// blocks of 5..16 rows that carry no state: the live wave blocks' rows and the dead rows (false: every block is live),
// the launch layout of the live blocks (all: every block counts), the dead rows' zeros by k_zero_rows
bool blk_live_rows(const qoc_ctx* c, std::vector<int>& wl, std::vector<int>& dead);
int blk_live(qoc_ctx* c, BlkArgs& bk, bool all = false);
int blk_zero_dead(qoc_ctx* c, std::initializer_list<void*> bufs);
bool blk_dead_pending(const qoc_ctx* c, const void* buf);  // blk_zero_dead would write buf
int wait_stale_check(qoc_ctx* c);                          // qoc_engine.hip: the host's wait for a queued stale-u check

// ---- qoc_run_blkp.hip ----
int blkp_pen_mode(const qoc_ctx* c);  // a penalty / co-state source: 0 none in effect, 1 the PEN chains, 2 Chebyshev
bool blkp_fits_nwb(const qoc_ctx* c, int nwb);
bool blkp_exact_on(const qoc_ctx* c);  // QOC_DUKDP_EXACT may stay on them (one control, the interpolation not switched off)
// 1 (nothing launched): the propagators do not fit in HBM, or exact without a converged interpolation
int blkp_eval_concurrent(qoc_ctx* c, int order, double* d_dJdu, const BlkArgs& bk);
// the reference's split call form for blocks of 5..16 rows on stored propagators: propagate = formation + forward
// chain (1: not applicable), grape_sensitivity = the μ recurrence + the order-3 gradient
int blkp_forward(qoc_ctx* c);
bool blkp_backward_ok(const qoc_ctx* c, int order);
int blkp_backward(qoc_ctx* c, int order, double* d_dJdu, const int* stale);  // 1: exact, see blkp_eval_concurrent

// ---- qoc_run_blku.hip ----
int blku_forward(qoc_ctx* c);
int blku_backward(qoc_ctx* c, int order, double* d_dJdu);
int blku_eval_concurrent(qoc_ctx* c, int order, double* d_dJdu);
int blku_states(qoc_ctx* c);    // rebuild x_k after a segmented eval (no-op unless fwd.lazy)
int blku_costates(qoc_ctx* c);  // qoc_get_costates after the fused block backward

// ---- qoc_run_blkseg.hip ----
// the segmented block eval (qoc_blkseg.hpp): one launch for J and dJdu, x_k / λ_k rebuilt on demand
bool blkseg_ok(const qoc_ctx* c, int order);
int blkseg_eval(qoc_ctx* c, int order, const double* d_u, double* d_J, double* d_dJdu);
// with a generator ensemble set: whether the fused launch takes the eval (blkseg_ok, and not the two-launch penalised
// form of blocks of 3 rows); the eval itself: B E workgroups, then k_ens_reduce into d_J / the caller's J and d_dJdu
bool blkseg_ens_ok(const qoc_ctx* c, int order);
int blkseg_eval_ens(qoc_ctx* c, int order, const double* d_u, double* d_J, double* d_dJdu);
// What an ensemble of E members with weights w needs under the objective (kind, param): the route of its evals (from
// the objective, the weights and QOC_ENS_SKIP alone) and the bytes of ω and of G (and D) at the segment ends; zeros
// under the mean.  Nothing on the context changes.
struct EnsPlan {
  int route = 1;
  size_t om_bytes = 0, gseg_bytes = 0;
};
EnsPlan blkseg_ens_plan(qoc_ctx* c, int E, const double* w, int kind, double param);
// with a time scale set (qoc_ctx::ts_on): whether the segmented eval takes the eval (blkseg_ok; penalised blocks of 3
// rows run as the two halves), and the eval: J, dJdu at fixed τ and dJ/dτ into d_ts + B.  Nothing lazy is kept and
// the last backward's record stands.
bool blkseg_ts_ok(const qoc_ctx* c, int order);
int blkseg_eval_ts(qoc_ctx* c, int order, const double* d_u, double* d_J, double* d_dJdu);
// the reference's split call form on the segmented eval: propagate = phases 0-2 (G at the segment ends to HBM),
// grape_sensitivity = phase 3 (stale: the device flag of a stale-u check queued before it, or nullptr)
bool blkseg_split_ok(const qoc_ctx* c);
int blkseg_forward(qoc_ctx* c, const double* d_u, double* d_J);
int blkseg_backward(qoc_ctx* c, int order, double* d_dJdu, const int* stale);

}  // namespace qoc_host
