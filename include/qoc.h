/*
 * qoc.h — C ABI of the MI355X-native GRAPE propagation/gradient engine (libqoc_mi355x.so).
 *
 * Drop-in boundary for the piecewise-constant Schrödinger hot path of
 * olof3/QuantumOptimalControl.jl.  Every entry point names the reference
 * interface it replaces (file:line in the reference repository).
 *
 * Conventions (identical to Julia's memory layout, so a ccall shim passes
 * arrays without conversion):
 *   - complex matrices are column-major, interleaved (re, im) double pairs
 *     (Julia Matrix{ComplexF64});
 *   - controls u are column-major nu x Nt Float64 per seed (Julia Matrix{Float64}),
 *     seeds contiguous: u[b*nu*Nt + k*nu + j] == u_b[j,k];
 *   - dJdu uses the same layout as u;
 *   - every entry point returns QOC_OK (0) or a negative error code; the
 *     message is available from qoc_last_error(ctx) (ctx may be NULL);
 *   - one caller thread per context (the reference is called from Ipopt's
 *     single callback thread, examples/ipopt_callbacks_exp.jl:11-31).
 * Host-side inputs are always fp64; a QOC_FP32 context converts them once.
 */
#ifndef QOC_MI355X_H
#define QOC_MI355X_H

#ifdef __cplusplus
extern "C" {
#endif

#define QOC_OK 0
#define QOC_ERR_ARG (-1)        /* bad argument / dimension mismatch  (src/gradient_computations.jl:84-87) */
#define QOC_ERR_HIP (-2)        /* HIP runtime failure */
#define QOC_ERR_STALE (-3)      /* u differs from the last propagate  (src/gradient_computations.jl:37-39) */
#define QOC_ERR_STATE (-4)      /* call order violated (e.g. sensitivity before propagate) */
#define QOC_ERR_UNSUPPORTED (-5)/* size outside the compiled kernel envelope */

#define QOC_FP64 0
#define QOC_FP32 1

/* dUkdp_order: 1..4 = truncated Taylor series of expm_jacobian! (src/gradient_computations.jl:177-213,
 * the reference's definition; 3 in the Ipopt path); QOC_DUKDP_EXACT = exact Fréchet derivative of the
 * propagator (opt-in).  Where the segmented eval applies (invariant blocks of <= 3 rows:
 * cavity, zz) it is that kernel's exact contraction, the whole series of the trace form, closed form on blocks of
 * 2 rows.  On invariant blocks of 5-16 rows with one control (the tunable bus) it is the derivative of the
 * interpolating block propagators' own curve, dU/du = e^{mu(u)} sum_i T_i(xi) N_i, on the stored / interpolating
 * propagators (fused and split call forms, penalty and co-state source, TRACE and ZCAL; QOC_BLKP_EXACT=0 off).
 * Elsewhere (two controls on such blocks, a control range the interpolation cannot resolve, QOC_BLKP_INTERP=0,
 * QOC_BLKP=0, QOC_COST_EXTERNAL), or with QOC_BLKSEG_EXACT=0, one 2N x 2N block exponential per slice and control.
 * On dense generators (no block path: none detected, or QOC_BLOCKS=0) that the fused gradient kernels fit (fp64,
 * N <= 48, m in {1, 2, 4, 8, 16}, nu <= 2, QOC_PROP_EXPM) it is the series
 *   Re Σ_{a+b < n_k} <(Ã_k^H)^a λ', A_j Ã_k^b x_k> / (a+b+1)!   (Ã_k = A_k - μ_k I, λ' = conj(e^{μ_k}) λ_{k+1})
 * run on MFMA with no exponential formed, n_k per slice from the chain prep's bound ρ_k (tail below 2^-53).  Its
 * rounding error grows like e^ρ ε, so a call whose largest n_k exceeds 48 (ρ ≈ 8.6) runs the block exponential
 * instead, whole.  That decision needs the largest n_k on the host: every exact gradient on such a context copies 16
 * bytes back and synchronises the stream once, also in qoc_eval_dev (orders 1-4 and the block paths queue as before).
 * QOC_GRAD_EXACT_SERIES=0 at qoc_create keeps the block exponential; QOC_GRAD_EXACT_WS_MB bounds the series'
 * workspace (default min(2 GiB, free / 8)), which only changes how many slices one launch pair covers.
 * qoc_exact_series_stats reports what ran. */
#define QOC_DUKDP_EXACT 0

#define QOC_COST_TRACE 0     /* J = 1-|tr(X'x)|^2/n^2            (src/penalty_fcns.jl:15-24) */
#define QOC_COST_ZCAL 1      /* z-calibrated, 4 columns           (src/penalty_fcns.jl:27-42, src/fidelities.jl:48-137) */
#define QOC_COST_EXTERNAL 2  /* caller supplies lambda_final      (any Julia closure dJfinal_dx) */

typedef struct qoc_ctx qoc_ctx;

/* Workspace for B seeds sharing (A0, A_j, x0, target).
 * Replaces setup_grape_cache (src/gradient_computations.jl:79-96): x, λ (B x (Nt+1) x N x m),
 * propagators Uk_vec (B x Nt x N x N), dJdu and the u copy live in HBM. */
int qoc_create(qoc_ctx** out, int device, int N, int m, int nu, int Nt, int B, int precision);
void qoc_destroy(qoc_ctx* ctx);
const char* qoc_last_error(const qoc_ctx* ctx);
/* sha256 of the sources (csrc/ and include/qoc.h) this library was compiled from ("unknown" when built
 * without the hash); the bindings refuse a library whose hash differs from the sources beside it. */
const char* qoc_source_hash(void);
void* qoc_stream(qoc_ctx* ctx);                 /* hipStream_t the engine launches on */
int qoc_synchronize(qoc_ctx* ctx);

/* Δt-prescaled generators A0Δt and A_jΔt (src/utils.jl:86-91), N x N each. */
int qoc_set_generators(qoc_ctx* ctx, const double* A0, const double* const* Aj);
/* Robust control: every pulse evaluated over an ensemble of E >= 1 generator sets (sampled detunings, couplings,
 * drive-amplitude calibrations), J̄_b = Σ_e w_e J(u_b; member e), in one launch of the segmented eval with one
 * workgroup per (pulse, member) and one reduction launch behind it.  A0s: E x N x N, Ajs[j]: E x N x N (column-major
 * interleaved, members contiguous), each Δt-prescaled like qoc_set_generators' arguments; weights: E values, NULL =
 * 1/E each.  E = 0 clears (A0s, Ajs and weights are then ignored; no effect when none is set).
 * Layout: qoc_set_generators comes first (QOC_ERR_STATE otherwise) and its set, the nominal one, fixes the block
 *   layout: its invariant blocks must have 2 or 3 rows and it must be exactly skew-Hermitian (QOC_ERR_UNSUPPORTED
 *   otherwise, e.g. dense generators or the tunable bus).  Every non-zero off-diagonal entry of every member must lie
 *   inside one of those blocks (QOC_ERR_ARG otherwise); members may lack couplings the nominal set has.  The nominal
 *   set need not be a member: under an ensemble it is not evaluated.
 * Members and weights: every generator of every member must pass qoc_set_generators' exact skew-Hermitian test
 *   (|A + A^H| <= 4 eps max|A|) and be finite, else QOC_ERR_ARG.  Weights must be finite and >= 0 with a positive sum
 *   (QOC_ERR_ARG otherwise) and are used as given, not normalised.  The setter copies everything; a failed call leaves
 *   the context (and an earlier ensemble) as it was.
 * With an ensemble set, qoc_eval_dev returns J̄_b = Σ_e w_e J_{b,e} (the state penalty included) and
 *   dJ̄/du_b = Σ_e w_e dJ_{b,e}/du, the members added in ascending e as acc = fma(w_e, v_e, acc) from 0 (no atomics:
 *   the result does not depend on scheduling).  Everything built on qoc_eval_dev follows with no change of its own:
 *   qoc_eval_spline[_dev], qoc_minimize_spline_dev, and the best (J, seed) of qoc_allgather_best[_dev], which is the
 *   argmin of J̄.  x0 (shared or per seed), the target and the cost are the context's, the same for every member.
 * Supported where the one-launch segmented eval applies: invariant blocks of 2 or 3 rows, QOC_FP64, QOC_COST_TRACE
 *   and QOC_COST_ZCAL, orders 1-4 and QOC_DUKDP_EXACT, and the state penalty on blocks of 2 rows.
 * QOC_ERR_UNSUPPORTED, leaving the context as it was: an eval that kernel does not take (a co-state source,
 *   QOC_COST_EXTERNAL gives its usual QOC_ERR_STATE, qoc_set_compression, QOC_BLKSEG=0, QOC_CONCURRENT=0, Tsit5); the
 *   penalised eval on blocks of 3 rows (its two-launch form keeps G and D per seed in HBM); and, while an ensemble is
 *   set, qoc_propagate[_dev], qoc_grape_sensitivity[_dev], qoc_propagate_spline, qoc_sensitivity_spline,
 *   qoc_propagate_envelope and qoc_eval_envelope[_dev]: state and co-state are per member, and the split call form is
 *   not part of the ensemble eval.
 * What it leaves: the setter (setting or clearing) materialises lazily kept states / co-states and invalidates the
 *   last forward (qoc_get_states: QOC_ERR_STATE); an ensemble eval keeps no state either and nothing lazy.  The
 *   co-states of the last plain backward stay readable (as after a refused call), the context's u holds the B pulses,
 *   and qoc_get_info keeps reporting the last plain backward's route.
 * Clearing: qoc_set_generators drops the ensemble (also one that fails after its argument checks).  After clearing, a
 *   plain eval is bitwise what it was before the ensemble was set.
 * Workspace (allocated by the setter, counted in info[3], freed on clear and qoc_destroy): the members' tables, and
 *   per (pulse, member) J, 2m λ_N coefficients and Nt x nu values of dJdu.
 * qoc_ensemble_size: E, 0 = none.  qoc_get_member_costs: J_{b,e} of the last ensemble eval (B x E, member fastest;
 *   synchronises; QOC_ERR_STATE without an ensemble or before its first eval), for post-processing; the worst-case
 *   objectives themselves are qoc_set_ensemble_objective's.
 * qoc_member_costs_dev: the same buffer on the device (NULL without an ensemble), valid while this ensemble is set and
 *   written by every ensemble eval on qoc_stream. */
int qoc_set_generator_ensemble(qoc_ctx* ctx, int E, const double* A0s, const double* const* Ajs,
                               const double* weights);
int qoc_ensemble_size(qoc_ctx* ctx);
int qoc_get_member_costs(qoc_ctx* ctx, double* Jm);
double* qoc_member_costs_dev(qoc_ctx* ctx);
/* The ensemble's objective: what qoc_eval_dev and everything built on it (qoc_eval_spline, qoc_minimize_spline_dev,
 * the best-(J, seed) pick) minimise over the members.  Let w_e >= 0 be the ensemble's weights as given, W = Σ_e w_e
 * (added in ascending e) and J_e the member costs of one pulse, the state penalty included.  Every objective is a
 * value J̄ and per-pulse member weights ω_e >= 0 with Σ_e ω_e = W, and dJ̄/du = Σ_e ω_e dJ_e/du.  Members with w_e = 0
 * never carry weight and never enter a maximum.
 *   QOC_ENS_MEAN (default)   ω_e = w_e: the weighted mean, on the code path described above, bit for bit.
 *   QOC_ENS_MAX              e* = argmax J_e over w_e > 0, the lowest e on ties; ω_{e*} = W, all others 0;
 *                            J̄ = W J_{e*}.
 *   QOC_ENS_CVAR, param = α in (0, 1]: the mean of the worst α-fraction.  Order the members by J descending, ties by
 *                            ascending e; before_e = Σ w_f over the members ahead of e, added in ascending f;
 *                            ω_e = min(w_e, max(0, α W - before_e)) / α; J̄ = Σ_e ω_e J_e.  α = 1 is the mean, an α no
 *                            larger than the worst member's share the maximum.
 *   QOC_ENS_LSE, param = β > 0, finite: a smooth maximum.  M = max J_e over w_e > 0, d_e = J_e - M,
 *                            s = Σ_e (w_e / W) expm1(β d_e), J̄ = W (M + log1p(s) / β), ω_e = w_e e^{β d_e} / (1 + s)
 *                            (the expm1 / log1p form: the plain log Σ exp loses ε / β to cancellation at small β).
 * Sums: J̄ (MAX, CVaR), s and dJ̄/du are accumulated as acc = fma(ω_e, v_e, acc) from 0 in ascending e, without
 *   atomics.  A member whose ω_e is exactly 0 is skipped, not multiplied by zero: its gradient row may be stale or
 *   NaN.  If any J_e with w_e > 0 is not finite, every ω_e of that pulse is NaN; J̄ and the pulse's gradient are then
 *   NaN and nothing is skipped.
 * qoc_set_ensemble_objective: QOC_ERR_ARG for an unknown kind, an α outside (0, 1] or a β that is not finite and > 0
 *   (param is ignored under MEAN and MAX).  A setting of the context, valid with or without an ensemble set; it
 *   survives qoc_set_generator_ensemble (replace or clear) and qoc_set_generators.  Like the ensemble's setter it
 *   materialises lazily kept states / co-states and invalidates the last forward; the last backward's record and the
 *   best-(J, seed) pick stay.  A failed call (argument or allocation) changes nothing.
 * Routes of an eval under a non-mean objective: 1 = the fused launch for every (pulse, member), the weights, the
 *   ω-weighted sum; 2 = the forward half for every (pulse, member), the weights, the backward half only where ω is not
 *   0, the ω-weighted sum.  LSE takes route 1.  MAX and CVaR take route 2 when n_act / E is at most a measured
 *   threshold and the launch has enough workgroups per compute unit for the skipped ones to make room (both measured,
 *   DESIGN.md §5), n_act = 1 + the largest k for which the k smallest positive weights sum to less than α W (MAX: 1):
 *   decided from the objective, the weights and B E alone, never from data, when one of the two setters completes the
 *   pair (ensemble + non-mean objective); QOC_ENS_SKIP=0|1 in the environment, read then, forces route 1 | 2.
 *   Both routes give the same bits.  What is refused under an ensemble stays refused under every objective.
 * qoc_get_ensemble_objective: the setting, and route = the form of the last ensemble eval (0 = none since a setter,
 *   1 = fused, 2 = forward + active backward); any of the three pointers may be NULL.
 * qoc_get_member_weights: ω of the last ensemble eval, B x E with the member index fastest (synchronises;
 *   QOC_ERR_STATE without an ensemble or before its first eval since a setter); under MEAN w_e for every pulse.
 *   qoc_member_weights_dev: the device buffer the evals under a non-mean objective write (NULL without an ensemble or
 *   under MEAN, where there is no per-pulse buffer).
 * qoc_member_grads_dev: the B E x Nt x nu member gradients dJ_{b,e}/du (row b E + e), for callers with objectives of
 *   their own; NULL without an ensemble.  After an eval that took route 2, the rows of members whose ω was 0 hold
 *   whatever an earlier eval left there (possibly nothing meaningful): read those rows only under route 1 or MEAN.
 * Workspace: ω (B x E doubles) and, for route 2, G (with a penalty on blocks of 2 rows also D) at the segment ends per
 *   (pulse, member); allocated by whichever of the two setters completes the pair, counted in info[3], freed with the
 *   ensemble and at qoc_destroy. */
#define QOC_ENS_MEAN 0
#define QOC_ENS_MAX 1
#define QOC_ENS_CVAR 2
#define QOC_ENS_LSE 3
int qoc_set_ensemble_objective(qoc_ctx* ctx, int kind, double param);
int qoc_get_ensemble_objective(qoc_ctx* ctx, int* kind, double* param, int* route);
int qoc_get_member_weights(qoc_ctx* ctx, double* om);
double* qoc_member_weights_dev(qoc_ctx* ctx);
double* qoc_member_grads_dev(qoc_ctx* ctx);
/* Gate duration as a variable: a per-seed time scale, a setting of the context.  With it set, seed b evolves under
 * tau_b (A0 + Σ_j u_jk A_j) in every slice: its gate duration is tau_b times the nominal one, and seeds of different
 * durations share one launch (a gate-time sweep is one batch).
 * qoc_eval_dev then returns J_b and dJ_b/du_b at fixed tau_b and leaves dJ_b/dtau_b at fixed u_b in the context's
 *   buffer.  J includes the state penalty, which stays Σ_{k=0}^{Nt} L(x_k), not rescaled by tau.  J and dJdu are what
 *   the engine returns for generators scaled by tau_b (orders 1-4: the reference's truncated formula on the scaled
 *   generators).  dJ/dtau = Σ_k Re<lambda_{k+1}, A_k x_{k+1}> with the full co-state (the penalty's sources included)
 *   is the exact derivative of the computed J at every dUkdp_order: exp(tau A_k) commutes with A_k, no series enters.
 *   Everything built on qoc_eval_dev follows with no change of its own: qoc_eval_spline[_dev],
 *   qoc_minimize_spline_dev, and the best (J, seed) of qoc_allgather_best[_dev] / qoc_set_best_output.
 * qoc_set_time_scale: copies B host values; every value must be finite and > 0 (QOC_ERR_ARG otherwise, context
 *   unchanged); NULL clears.  QOC_ERR_UNSUPPORTED on a QOC_FP32 context and while a generator ensemble is set
 *   (qoc_set_generator_ensemble is refused likewise while a time scale is set; both leave the earlier setting in place).
 *   Allocates 2 B doubles on first use, counted in info[3], freed on clear and at qoc_destroy.  Like the ensemble's
 *   setter it materialises lazily kept states / co-states and invalidates the last forward.  The setting survives
 *   qoc_set_generators, qoc_set_x0 and qoc_set_cost.  tau = 1 for every seed is not special-cased: it runs the same
 *   kernels and gives the plain eval's J and dJdu.  After clearing, a plain eval is bitwise what it was before.
 * qoc_time_scale_dev: the context's B values on the device (NULL when none set).  The caller may overwrite them on
 *   qoc_stream between evals (an optimiser of its own, say); every eval reads them at launch.  Values written that
 *   way are not checked: a non-finite or non-positive tau_b gives unspecified results, possibly NaN, for that seed only.
 * qoc_get_time_scale_grad: dJ_b/dtau_b of the last eval under the time scale, B host values (synchronises;
 *   QOC_ERR_STATE without a time scale or before its first eval since the setter).  qoc_time_scale_grad_dev: the same
 *   buffer on the device (NULL when none set), written by every such eval on qoc_stream.  The sum is formed in a fixed
 *   order without atomics: a seed's dJ/dtau has the same bits alone and inside any batch of the same launch shape.
 * Supported where the segmented eval applies: invariant blocks of 2 or 3 rows, exactly skew-Hermitian generators,
 *   QOC_FP64, QOC_COST_TRACE and QOC_COST_ZCAL, orders 1-4 and QOC_DUKDP_EXACT, the state penalty on blocks of 2 rows
 *   in one launch and on blocks of 3 rows as a forward and a backward launch.
 * QOC_ERR_UNSUPPORTED, leaving the context and the caller's output buffers as they were: an eval that kernel does not
 *   take (a co-state source, qoc_set_compression, generators without blocks of 2-3 rows, QOC_BLKSEG=0,
 *   QOC_CONCURRENT=0, Tsit5; QOC_COST_EXTERNAL gives its usual QOC_ERR_STATE); and, while a time scale is set,
 *   qoc_propagate[_dev], qoc_grape_sensitivity[_dev], qoc_propagate_spline, qoc_sensitivity_spline,
 *   qoc_propagate_envelope and qoc_eval_envelope[_dev].
 * What it leaves: an eval under a time scale keeps no states and nothing lazy (qoc_get_states: QOC_ERR_STATE); the
 *   co-states of the last plain backward stay readable, and qoc_get_info keeps reporting the last plain backward's route. */
int qoc_set_time_scale(qoc_ctx* ctx, const double* tau);
double* qoc_time_scale_dev(qoc_ctx* ctx);
int qoc_get_time_scale_grad(qoc_ctx* ctx, double* dJdtau);
double* qoc_time_scale_grad_dev(qoc_ctx* ctx);
/* x0 (N x m) shared by all seeds (per_seed = 0) or B x N x m (per_seed = 1) — propagate :14. */
int qoc_set_x0(qoc_ctx* ctx, const double* x0, int per_seed);
/* Terminal cost: kind QOC_COST_TRACE (X_target N x m, normalisation n),
 * QOC_COST_ZCAL (m must be 4; every propagation path), QOC_COST_EXTERNAL (X_target may be NULL). */
int qoc_set_cost(qoc_ctx* ctx, int kind, const double* X_target, double n);
/* Guard-state penalty L = mu sum |x[P,C]|^2 (src/penalty_fcns.jl:1-11), summed over the Nt + 1 states in J and added
 * as 2 mu x_k[P,C] to every co-state; 0-based indices; mu = 0 (or an empty P or C) disables.  Generators with
 * invariant blocks of 2-3 rows keep the one-launch segmented eval and its split form with the penalty set
 * (QOC_BLKSEG_PEN=0: the block chains instead); a co-state source (qoc_set_costate_source) takes the chains.
 * Generators with invariant blocks of 5-16 rows keep the stored / interpolating block propagators (order 3, TRACE and
 * ZCAL costs, both call forms): the forward chain adds the penalty's sum, the backward chain runs lambda_k with the
 * sources (QOC_BLKP_PEN=0: the Chebyshev block chains instead); rows of a block that carries no state add nothing.  May be
 * called on a live context: lazily kept states / co-states are materialised first, and a propagate made before the
 * call is followed by a grape_sensitivity on rebuilt states. */
int qoc_set_state_penalty(qoc_ctx* ctx, const int* P, int np, const int* C, int nc, double mu);

/* propagate (src/gradient_computations.jl:2-32) for all B seeds, host pointers.
 * u: B x nu x Nt (see layout above).  J_out (B, may be NULL) receives the objective
 * of examples/ipopt_callbacks_exp.jl:18, Jfinal(x[end]) + sum(L, x)
 * (for QOC_COST_EXTERNAL only the penalty part). */
int qoc_propagate(qoc_ctx* ctx, const double* u, double* J_out);
/* grape_sensitivity (src/gradient_computations.jl:35-77), host pointers.
 * Returns QOC_ERR_STALE unless u is bitwise the u of the last propagate.
 * lambda_final (B x N x m) is required for QOC_COST_EXTERNAL and ignored otherwise. */
int qoc_grape_sensitivity(qoc_ctx* ctx, const double* u, int dUkdp_order,
                          const double* lambda_final, double* dJdu_out);

/* A caller's state-penalty gradient that is not a built-in penalty (any Julia closure dL_dx,
 * src/gradient_computations.jl:47-49, 55-57): dLdx holds dL_dx(x_k) for every seed and k = 0..Nt
 * (B x (Nt+1) x N x m, the states' layout), added to λ_k by the following grape_sensitivity calls until cleared
 * with NULL.  The host evaluates the closure on the states (qoc_get_states); J's sum(L, x) stays with the
 * caller.  Not on the Tsit5 path (compute_pwc_gradient has no dL_dx).  On blocks of 5-16 rows the stored block
 * propagators' backward chain adds it (order 3, TRACE and ZCAL costs; QOC_BLKP_PEN=0: the Chebyshev block chains);
 * every block then counts as live, since lambda_k is nonzero on rows that carry no state. */
int qoc_set_costate_source(qoc_ctx* ctx, const double* dLdx);

/* compress_states / decompress_states (src/utils.jl:96-109) inside the engine.  When the generators keep the
 * two row blocks rows1 / rows2 (a partition of the N rows) apart, and the state's columns cols1 live only on
 * rows1 and cols2 only on rows2 (a partition of the m columns), the engine packs both blocks into
 * max(nc1, nc2) columns: the chains and the gradient run on the packed states, and every host-side state
 * argument (x0, X_target, lambda_final, dLdx, penalty columns) and result (qoc_get_states / costates) keeps the
 * caller's N x m layout.  J and dJdu equal the unpacked problem's.  0-based indices; nr1 = nr2 = 0 turns packing
 * off.  Errors: QOC_ERR_ARG when the index lists do not partition rows / columns, the generators couple the blocks,
 * or x0 has an entry outside its block.  Re-packs an x0 / target / penalty already set; a co-state source must be
 * set again.  Co-states come back projected on the blocks (the rest never reaches the gradient). */
int qoc_set_compression(qoc_ctx* ctx, const int* rows1, int nr1, const int* cols1, int nc1, const int* rows2,
                        int nr2, const int* cols2, int nc2);

/* Device-pointer variants (inputs already resident in HBM, asynchronous on qoc_stream). */
int qoc_propagate_dev(qoc_ctx* ctx, const double* d_u, double* d_J);
int qoc_grape_sensitivity_dev(qoc_ctx* ctx, const double* d_u, int dUkdp_order, double* d_dJdu);
/* One GRAPE gradient eval = f + f_grad of examples/ipopt_callbacks_exp.jl:11-31 (no spline map). */
int qoc_eval_dev(qoc_ctx* ctx, const double* d_u, int dUkdp_order, double* d_J, double* d_dJdu);

/* Spline parameterisation of the controls, the optimisation variables of the Ipopt callbacks
 * (examples/ipopt_callbacks_exp.jl:13-14, 28): u_b = transpose(Bs * c_b), dJdc_b = Bs' * transpose(dJdu_b).
 * Bs is Nt x ns column-major (Julia Matrix); c_b is ns x nu column-major (reshape(c, nsplines, nu)),
 * seeds contiguous (B x ns x nu). */
int qoc_set_spline_basis(qoc_ctx* ctx, const double* Bs, int ns);
/* f + f_grad of examples/ipopt_callbacks_exp.jl:11-31 in the coefficients, device pointers. */
int qoc_eval_spline_dev(qoc_ctx* ctx, const double* d_c, int dUkdp_order, double* d_J, double* d_dJdc);
/* Host-pointer variant (J_out: B, dJdc_out: B x ns x nu). */
int qoc_eval_spline(qoc_ctx* ctx, const double* c, int dUkdp_order, double* J_out, double* dJdc_out);
/* f alone (examples/ipopt_callbacks_exp.jl:11-19: spline map, propagate, J; no sensitivity), host pointers; and
 * f_grad's sensitivity (:21-31) for the coefficients last passed to qoc_propagate_spline (QOC_ERR_STALE for any
 * other c, the reference's "Cache data from other control signal u"). */
int qoc_propagate_spline(qoc_ctx* ctx, const double* c, double* J_out);
int qoc_sensitivity_spline(qoc_ctx* ctx, const double* c, int dUkdp_order, double* dJdc_out);
/* Constraints g = [norm(c), norm(diff(c, dims=1))] and their Jacobian (examples/ipopt_callbacks_exp.jl:33-51),
 * device pointers: d_g (B x 2), d_gjac (B x 2 x nc, constraint-major = Ipopt's dense triplet order; may be NULL). */
int qoc_spline_constraints_dev(qoc_ctx* ctx, const double* d_c, double* d_g, double* d_gjac);

/* Lazy readback of cache fields (test/test_gradient_computation.jl:84,86 read cache.x / cache.λ).
 * qoc_get_states: x_k of the last propagate / eval; QOC_ERR_STATE once qoc_set_generators, qoc_set_x0, qoc_set_cost or
 * qoc_set_compression has invalidated it (qoc_set_state_penalty and qoc_set_costate_source keep it).
 * qoc_get_costates: λ_k of the last grape_sensitivity / eval, under the settings of that call: any setter and any later
 * propagate leave them as they are (zeros before the first one).
 * An entry point that returns an error has changed nothing the later calls see: a stale or refused
 * grape_sensitivity leaves the co-states, a refused eval the controls and states of the last propagate. */
int qoc_get_states(qoc_ctx* ctx, int seed, int k, double* x_out);       /* k in [0,Nt], -1 = final */
int qoc_get_costates(qoc_ctx* ctx, int seed, int k, double* lam_out);
int qoc_get_propagator(qoc_ctx* ctx, int seed, int k, double* U_out);   /* Uk_vec[k+1], k in [0,Nt) */
/* Histogram of selected (Padé degree, squarings) since the last reset:
 * hist[di*64 + s], di = index of degree in {3,5,7,9,13}.  Used for the FLOP accounting.  Under
 * QOC_CHAIN_TAYLOR (no exponential is formed) it is evaluated at call time from the last propagated u,
 * counted once per forward pass since the reset. */
int qoc_pade_histogram(qoc_ctx* ctx, long long* hist, int reset);

/* Exponential algorithm actually executed (no linear solve; same result as the reference's Padé to
 * fp rounding; QOC_EXPM_PADE=1 at qoc_create selects the Padé + solve algorithm).  QOC_TAYLOR_HIST_ENTRIES = 9*64 entries:
 *   hist[(r-2)*64 + s], r = 2..8: degree m = 3r+2 Taylor by Paterson-Stockmeyer (2 + r GEMMs) with s
 *     squarings (large-N pipeline; LDS kernel with QOC_EXPM_LDS=1);
 *   hist[7*64 + s]: degree-12 Taylor in 4 GEMMs (Bader-Blanes-Casas form) with s squarings (the
 *     default register-resident kernel);
 *   hist[8*64 + s]: degree-8 Taylor in 3 GEMMs (Bader-Blanes-Casas form) with s squarings (large-N pipeline).
 * The truncation tail is <= 2^-53 in every case.  qoc_pade_histogram keeps reporting the Padé (d, s)
 * the reference would select.  qoc_taylor_histogram_n takes the capacity of hist and fails (QOC_ERR_ARG) when it
 * is below QOC_TAYLOR_HIST_ENTRIES; qoc_taylor_histogram (no capacity) writes QOC_TAYLOR_HIST_ENTRIES entries. */
#define QOC_TAYLOR_HIST_ENTRIES (9 * 64)
int qoc_taylor_histogram(qoc_ctx* ctx, long long* hist /*[QOC_TAYLOR_HIST_ENTRIES]*/, int reset);
int qoc_taylor_histogram_n(qoc_ctx* ctx, long long* hist, int n, int reset);

/* Live per-kernel timing: when enabled, hipEvents are recorded on qoc_stream around each hot-path
 * kernel (phase 0 k_expm, 1 k_chain_fwd, 2 k_chain_bwd, 3 k_grad).  qoc_phase_times synchronises the
 * stream and returns the accumulated milliseconds and launch counts per phase. */
int qoc_set_profiling(qoc_ctx* ctx, int enable);
int qoc_phase_times(qoc_ctx* ctx, double* ms_out /*[4]*/, long long* launches_out /*[4]*/, int reset);

/* Large-N path only: accumulated time, launch count and algorithmic FLOPs (8 M K Ncol per complex
 * GEMM item) of the k_bgemm launches recorded while profiling was enabled. */
int qoc_gemm_stats(qoc_ctx* ctx, double* ms, long long* launches, double* flops, int reset);

/* Propagation method.  QOC_PROP_EXPM (default): U_k = exp(A_k) per slice.
 * QOC_PROP_TSIT5: the reference's ODE path propagate_pwc / compute_pwc_gradient
 * (src/gradient_computations.jl:108-169): nsub fixed Tsit5 steps per slice (the reference's
 * dt = 0.1 Δt is nsub = 10) for the states and, backwards, for the co-states dλ/dτ = -A_k^H λ; the
 * gradient contraction is unchanged.  LDS-resident sizes (N <= 64), trace / external costs. */
#define QOC_PROP_EXPM 0
#define QOC_PROP_TSIT5 1
int qoc_set_propagation(qoc_ctx* ctx, int method, int nsub);

/* Continuous-envelope propagation with fixed-step Tsit5 (wrap_envelope, src/QuantumOptimalControl.jl:43-54;
 * examples/two_qubit_tunable_bus.jl:58-67): dx/dt = (A0 + sum_j c_j(t) A_j) x, t in [0, tgate], step dt,
 * with c(t) from the pulse `kind` and per-seed parameters params[b*np ...] (src/parameterized_pulses.jl).
 * The generators are used as set (not Δt-scaled).  x_out (optional, B x N x m interleaved complex,
 * column-major per seed) receives x(tgate); J_out (optional, B) the trace cost when one is set.  QOC_ENV_TUNABLE_BUS: [t_plateau, t_rise_fall, theta0, omega_Phi, A], nu = 1;
 * QOC_ENV_DRAG (u_drag): [tgate, sigma, A, xi], nu = 2 (Re, Im); QOC_ENV_SINEBASIS: [Tgate, p1x, p1y, ...], nu = 2. */
#define QOC_ENV_TUNABLE_BUS 0
#define QOC_ENV_DRAG 1
#define QOC_ENV_SINEBASIS 2
int qoc_propagate_envelope(qoc_ctx* ctx, int kind, const double* params, int np, double tgate, double dt,
                           double* J_out, double* x_out);
/* J and dJ/dp of qoc_propagate_envelope's run for all B seeds in one call: the discrete adjoint of the fixed-step
 * Tsit5 scheme, i.e. the derivative of the J the engine computes (not the continuous adjoint re-integrated), so a
 * line search sees a consistent (f, g) at any dt.  Convention: dJ = Re<lambda, dx> with lambda_N = dJ/dx(x(tgate))
 * (compute_u_sensitivity, src/gradient_computations.jl:217-223); dJdp_out[b*np + q] = dJ/dp_q of seed b, in the order
 * of params.  Arguments, checks and errors as qoc_propagate_envelope; J is that call's J bit for bit (no state penalty
 * on the envelope path).  QOC_COST_TRACE and QOC_COST_ZCAL in both forms; QOC_COST_EXTERNAL in the host form only,
 * with lambda_final (B x N x m) required and J_out left untouched (the _dev form returns QOC_ERR_ARG there).
 * QOC_ERR_UNSUPPORTED on a QOC_FP32 context and with qoc_set_compression active.
 *   d/dp_0 of QOC_ENV_DRAG (tgate) and QOC_ENV_SINEBASIS (Tgate) is the partial derivative of the pulse formula: the
 *     integration horizon is the argument tgate, held fixed.
 *   QOC_ENV_TUNABLE_BUS: d/dt_plateau and d/dt_rise_fall take the branch of cos_envelope that t lies in (the envelope
 *     is C^1 in both).  sqrt|cos(theta)| has no derivative at cos(theta) = 0: J is not differentiable where the pulse
 *     reaches theta/pi = 1/2 + k at a stage time, and the result there is not guaranteed finite (the reference's
 *     pulse keeps theta/pi within 0.25 +- 0.13).
 *   A parameter the pulse does not read (beyond the kind's list, or the last one of an even np in the sine basis) has
 *     derivative 0.
 * The reverse sweep needs every x_n: the forward stores checkpoints every C steps in a workspace kept on the context
 * (grown when a call needs more; C = 1 while B x nsteps x m x N x 32 bytes fit min(1 GiB, free / 4), else the
 * smallest spacing that fits) and the adjoint re-runs each segment from its checkpoint with the forward's arithmetic,
 * so dJdp does not depend on C in any bit.  QOC_ERR_UNSUPPORTED when the spacing needed exceeds what the LDS holds
 * beside the generators.  QOC_ENV_WS_MB=<MiB> (read at the context's first such call) replaces the budget;
 * QOC_ENV_CKPT=<C> at qoc_create forces the spacing (testing; bounded by the same LDS ring).
 * The call leaves on the context what qoc_propagate_envelope leaves (x(tgate), J) and nothing else: the co-states of
 * the last grape_sensitivity / eval stay readable.  The _dev form is queued on qoc_stream: d_params (B x np), d_J (B,
 * may be NULL) and d_dJdp (B x np) are device pointers, and nothing synchronises once the workspace exists. */
int qoc_eval_envelope(qoc_ctx* ctx, int kind, const double* params, int np, double tgate, double dt,
                      const double* lambda_final, double* J_out, double* dJdp_out, double* x_out);
int qoc_eval_envelope_dev(qoc_ctx* ctx, int kind, const double* d_params, int np, double tgate, double dt,
                          double* d_J, double* d_dJdp);

/* Engine facts: info[0] = path (0 = LDS-resident kernels, 1 = large-N chunked GEMM pipeline),
 * info[1] = slices per chunk (large-N), info[2] = Newton-Schulz iterations executed so far (large-N),
 * info[3] = device bytes allocated by the context, info[4] = chain mode (QOC_CHAIN_PROPAGATORS /
 * QOC_CHAIN_TAYLOR), info[5] = exponential the propagators run (0 the reference's Padé + solve, 1 register-
 * resident Taylor / Paterson-Stockmeyer, 2 LDS Paterson-Stockmeyer), info[6] = 1 when the Taylor-action chains
 * use Chebyshev terms (skew-Hermitian generators, fp64; QOC_TCHAIN_POLY=taylor keeps Taylor), info[7] = state columns the kernels run on (m, or max(nc1, nc2) with qoc_set_compression), info[8] = how the
 * last backward ran (0 generic, 1 from the chains' captured products, 2 concurrent μ recurrence of qoc_eval_dev on
 * a second stream, 3 the same in one launch with the forward chain, 4 the block chains' concurrent eval, 5 the block
 * propagators' fused backward: λ kept on chip, the gradient contracted beside the chain; qoc_get_costates then
 * rebuilds λ on demand, 6 the segmented block eval, 7 the stored / interpolating propagators of blocks of 5..16
 * rows: order 3, and QOC_DUKDP_EXACT where their interpolation in u applies),
 * info[9] = 1 when the last forward chain wrote its captured products, info[10] = the Taylor-action chain kernels
 * (0 none / the fp32 VALU ones, 1 MFMA with the state in LDS, 2 MFMA with the state in registers: N <= 32, nu <= 2,
 * QOC_TCHAIN_ROT=0 keeps 1; 3 block chains: the generators split into invariant blocks of <= 4 rows, one VALU lane
 * per (block, column); 4 block chains with one MFMA wave per (block of 5..16 rows, column pair), or blocks of <= 4 rows
 * packed into MFMA slots (QOC_BLKU=0); 5 block propagators: blocks of <= 4 rows, U_k formed per (slice, block) apart
 * from the serial chain, one block matvec per slice (the default for blocks of <= 4 rows); QOC_BLOCKS=0 at
 * qoc_set_generators keeps the dense kernels).  QOC_FORCE_LARGE_N=1 in the environment at qoc_create selects the
 * large-N path for any size (testing).  qoc_get_info_n takes the capacity of info and fails (QOC_ERR_ARG) when it is
 * below QOC_INFO_ENTRIES; qoc_get_info (no capacity) writes QOC_INFO_ENTRIES entries.  info[11] = what the last
 * propagate left for grape_sensitivity (the reference's split call form, examples/ipopt_callbacks_exp.jl:11-31):
 * 0 the states x_k, 1 the segmented forward (blocks of 2-3 rows: G at every segment's end, x_k rebuilt on demand;
 * grape_sensitivity then runs the segmented backward alone), 2 the stored propagators of blocks of 5..16 rows
 * (grape_sensitivity: the co-state chain and the gradient on them).  info[12] = the degree of the last stored-propagator
 * formation's interpolation in u (one control: U(u) = Σ_i T_i(ξ) M_i over the batch's control range), 0 when the
 * exponentials were formed per slice.  info[13] = 1 when the last eval / propagate on blocks of 5..16 rows ran the
 * interpolating chains (each chain forms its slice propagators from those coefficients in registers: none stored),
 * 2 when they formed the upper triangle alone (complex-symmetric generators), 0 otherwise. */
#define QOC_INFO_ENTRIES 14
int qoc_get_info(qoc_ctx* ctx, long long* info /*[QOC_INFO_ENTRIES]*/);
int qoc_get_info_n(qoc_ctx* ctx, long long* info, int n);

/* How the chains x_{k+1} = U_k x_k (src/gradient_computations.jl:27-29) and λ_k = U_k^H λ_{k+1} (:52-58)
 * apply the slice exponentials:
 *   QOC_CHAIN_PROPAGATORS: form every U_k = exp(A_k) (register-resident Taylor / Padé on MFMA, the
 *     reference's structure), then the serial products;
 *   QOC_CHAIN_TAYLOR: apply exp(A_k) to the N x m state directly (shifted, truncated Taylor series with the
 *     degree chosen per slice for a tail <= 2^-53 / 2^-24) — no U_k is formed (qoc_get_propagator computes
 *     one on demand).  N <= 48 (fp64) / 64 (fp32), nu <= 8;
 *   QOC_CHAIN_AUTO: Taylor when ||A0 - μ I||_1 <= 1 (few terms per slice), else propagators (the default,
 *     chosen at qoc_set_generators; QOC_CHAIN=taylor|expm in the environment overrides it).
 * The states, co-states, J and dJdu agree to rounding either way. */
#define QOC_CHAIN_AUTO (-1)
#define QOC_CHAIN_PROPAGATORS 0
#define QOC_CHAIN_TAYLOR 1
int qoc_set_chain(qoc_ctx* ctx, int mode);
/* Taylor terms executed per direction (Σ over slices of P s) since the last reset (QOC_CHAIN_TAYLOR). */
int qoc_chain_terms(qoc_ctx* ctx, long long* terms, int reset);
/* The exact gradient's series route on dense generators (QOC_DUKDP_EXACT above) since the last reset:
 * stats[0] = (seed, slice) units the series kernels processed, stats[1] = Σ n_k over them (terms per side),
 * stats[2] = the largest n_k among them, stats[3] = calls that fell back to the block exponential because their
 * largest n_k exceeded the cap of 48.  Host counters: no device work, no synchronisation.  QOC_ERR_ARG for a NULL
 * context or buffer. */
int qoc_exact_series_stats(qoc_ctx* ctx, long long* stats /*[4]*/, int reset);

/* Multi-GPU epilogue: seeds are sharded contiguously over ranks, one context per GPU; the
 * only exchange is an all-gather of each rank's best (J, global seed id) over RCCL (xGMI), 16 bytes per rank.
 * qoc_comm_unique_id (one rank) creates the RCCL unique id (QOC_UNIQUE_ID_BYTES opaque bytes) that the caller
 * distributes (MPI / Distributed.jl / torch.distributed); every rank then calls qoc_comm_init with its rank
 * and the global id of its seed 0.  qoc_allgather_best returns the best J of the last propagate over all
 * ranks and its global seed (lowest seed on ties); without qoc_comm_init it covers this context alone.
 * With an id, qoc_comm_init creates a real RCCL communicator for any world size (world = 1 included: a
 * one-rank ncclAllGather on the same path as the multi-GPU run); with id = NULL (world = 1 only) none is made.
 * On any error the context is left without a communicator (world 1, seed offset 0).
 * qoc_comm_ranks returns the communicator's rank count, 0 when the context has none.
 * RCCL is loaded on first use (librccl.so.1); two ranks cannot share one GPU (RCCL rejects duplicate
 * devices).  The _dev variant writes (J_best, seed) as two doubles to device memory on qoc_stream without
 * synchronising. */
#define QOC_UNIQUE_ID_BYTES 128
int qoc_comm_unique_id(void* id_out);
int qoc_comm_init(qoc_ctx* ctx, int world, int rank, const void* id, long long seed_offset);
int qoc_comm_ranks(qoc_ctx* ctx);
int qoc_allgather_best(qoc_ctx* ctx, double* J_best, int* seed_best);
int qoc_allgather_best_dev(qoc_ctx* ctx, double* d_out);
/* Registers a device buffer of two doubles (NULL: none).  With nothing to exchange (no communicator, or one rank) the
 * evals that reduce their own J (the segmented block eval) then also write the best (J, seed) there, and
 * qoc_allgather_best_dev(ctx, that buffer) queues nothing more: the result is the same pair, without the pick kernel
 * after every eval.  The caller keeps the buffer valid while it is registered. */
int qoc_set_best_output(qoc_ctx* ctx, double* d_out);

/* Device-resident multi-start optimiser (the Ipopt multi-start of examples/zz_coupling_ipopt_exp.jl:56-80 as B
 * independent projected L-BFGS runs with an augmented-Lagrangian outer loop).  Every seed is a state
 * machine of its own: at each tick all B trial points are evaluated in one batch and every seed consumes its own
 * (f, grad): it accepts the trial and posts a new one, halves its step, or ends an augmented-Lagrangian round.  No
 * host decision lies between two evals.  All optimiser state is fp64.
 *   n: variables per seed (<= 256); memory: L-BFGS pairs (<= 16); beyond that QOC_ERR_UNSUPPORTED.
 *   ns, nu: 0 = no constraints; otherwise n == ns * nu and the constraints are the two spline norms
 *     g = [norm(c), norm(diff(c, dims=1))] <= g_upper (examples/ipopt_callbacks_exp.jl:33-51).
 *   lower / upper: scalar bounds (+-inf allowed); max_iter: inner iterations per round; outer_iters: augmented-
 *     Lagrangian rounds; max_ls: trials per line search; rho0: first penalty; gtol: projected-gradient bar;
 *   order: dUkdp order of the spline form (qoc_minimize_spline_dev). */
typedef struct qoc_opt qoc_opt;
typedef struct qoc_opt_params {
  int n, ns, nu;
  double lower, upper;
  double g_upper[2];
  int max_iter, memory, outer_iters, max_ls;
  double rho0, gtol;
  int order;
} qoc_opt_params;
/* The object is independent of any engine context: ask (qoc_opt_trial_dev) / tell with any objective.  stream: the
 * hipStream_t the kernels are queued on (NULL: the default stream); nothing synchronises. */
int qoc_opt_create(qoc_opt** out, int device, int B, const qoc_opt_params* params);
void qoc_opt_destroy(qoc_opt* opt);
/* Starts at clamp(c0) (B x n, device); the first trial is that point. */
int qoc_opt_start_dev(qoc_opt* opt, void* stream, const double* d_c0);
/* Device pointer of the B x n trial points (fixed for the object's life). */
double* qoc_opt_trial_dev(qoc_opt* opt);
/* f (B) and grad (B x n) at the current trials, device pointers: every seed advances by one tick and the next
 * trials are written.  A finished seed keeps its iterate as its trial; its state no longer changes. */
int qoc_opt_tell_dev(qoc_opt* opt, void* stream, const double* d_f, const double* d_grad);
/* The whole multi-start run on the engine's stream: ticks of (eval, one fused step kernel: dJdc = Bs' dJdu', the
 * seed's state machine, u = transpose(Bs c) of its next trial written into the context's controls) are queued in
 * groups of poll_every (<= 0: 16); after each group the host waits on one event and reads the mirrored count of
 * finished seeds.  Stops when all seeds are done or after max_ticks ticks, QOC_OK either way (qoc_opt_result tells
 * which).  Then one closing eval at the final iterates: the context's u, J, lazy states and best-(J, seed) epilogue
 * (qoc_allgather_best) belong to the result; with max_ticks = 0 no seed takes an eval and the result's f is the
 * closing eval's, at the clamped starts.  d_c (B x ns x nu, device): the starts in, the final iterates out.
 * ticks_out: the ticks the slowest seed used.  QOC_ERR_STATE without a spline basis, QOC_ERR_ARG when B or n differ. */
int qoc_minimize_spline_dev(qoc_ctx* ctx, qoc_opt* opt, double* d_c, long long max_ticks, int poll_every,
                            long long* ticks_out);
/* The duration form: every seed's variables are z_b = [c_b (ns * nu values, index s + ns * j), tau_b], the gate
 * duration of qoc_set_time_scale as the last of n = ns * nu + 1 <= 256 variables, for time-optimal control
 * (minimise f = J + time_weight * tau).  lower / upper of params bound c; tau has tau_lower / tau_upper of its own; the
 * two spline norms and their Jacobians run over c only; the L-BFGS recursion, the line search and the gtol test run
 * over all n variables.
 * qoc_opt_create_duration: params->n == ns * nu + 1 when ns, nu > 0; with ns = nu = 0 the last of the n variables is the
 *   one with its own bounds and there are no constraints.  tau_lower finite and > 0, tau_lower <= tau_upper (+inf
 *   allowed), time_weight finite: QOC_ERR_ARG otherwise; QOC_ERR_UNSUPPORTED for n > 256 or memory > 16; all checked
 *   before the GPU is touched.  qoc_opt_start_dev, qoc_opt_tell_dev, qoc_opt_trial_dev, qoc_opt_field_dev and
 *   qoc_opt_result work on the object as on a plain one.  In ask / tell the caller's f and grad are complete:
 *   time_weight is used by qoc_minimize_spline_duration_dev only.
 * qoc_minimize_spline_duration_dev: qoc_minimize_spline_dev for such an object, with the same grouping, polling,
 *   max_ticks = 0 behaviour and closing eval.  Per tick one eval under the time scale and one fused step kernel:
 *   grad = [Bs' dJdu', dJ/dtau + time_weight], f = J + time_weight * tau (a product, then a sum), the seed's state
 *   machine, then u = transpose(Bs c) and tau of its next trial written into the context's controls and time-scale
 *   buffer.  d_z (B x (ns * nu + 1), device): the starts in, the final iterates out.  QOC_OPT_F and the result's f are
 *   J + time_weight * tau at the iterate.  The context's best (J, seed) (qoc_allgather_best) is the closing eval's own:
 *   the minimum of J, not of f.  What the call leaves on the context is what qoc_minimize_spline_dev leaves under a
 *   time scale.
 *   Requires qoc_set_time_scale to have been made (any values: the call overwrites all B; on return the buffer holds
 *   the final tau).  QOC_ERR_STATE: no spline basis, no time scale, QOC_COST_EXTERNAL.  QOC_ERR_ARG: an object made by
 *   qoc_opt_create (and a duration object passed to qoc_minimize_spline_dev); B, device or n differ.  Everything an
 *   eval under a time scale refuses (QOC_ERR_UNSUPPORTED, see qoc_set_time_scale) is refused before anything changes:
 *   d_z, the time-scale buffer, the context's controls and J are as they were. */
typedef struct qoc_opt_duration {
  double tau_lower, tau_upper, time_weight;
} qoc_opt_duration;
int qoc_opt_create_duration(qoc_opt** out, int device, int B, const qoc_opt_params* params, const qoc_opt_duration* dur);
int qoc_minimize_spline_duration_dev(qoc_ctx* ctx, qoc_opt* opt, double* d_z, long long max_ticks, int poll_every,
                                     long long* ticks_out);
/* Device pointers of the per-seed results (valid for the object's life; read them after the stream has drained). */
#define QOC_OPT_X 0          /* B x n doubles: iterates */
#define QOC_OPT_F 1          /* B doubles: objective at the iterate (without constraint terms) */
#define QOC_OPT_G 2          /* B x 2 doubles: constraint values */
#define QOC_OPT_LAM 3        /* B x 2 doubles: multipliers */
#define QOC_OPT_RHO 4        /* B doubles: penalty */
#define QOC_OPT_EVALS 5      /* B ints: evals consumed */
#define QOC_OPT_ITERS 6      /* B ints: accepted iterations */
#define QOC_OPT_ROUNDS 7     /* B ints: augmented-Lagrangian rounds ended */
#define QOC_OPT_CONVERGED 8  /* B ints */
#define QOC_OPT_DONE 9       /* B ints */
#define QOC_OPT_LSFAILS 10   /* B ints: failed line searches */
void* qoc_opt_field_dev(qoc_opt* opt, int field);
/* Host copies (any pointer may be NULL), after synchronising stream: x (B x n), f (B), g and lam (B x 2), rho (B),
 * evals / iters / rounds / converged / done / lsfails (B ints each), not_done: seeds that have not finished. */
int qoc_opt_result(qoc_opt* opt, void* stream, double* x, double* f, double* g, double* lam, double* rho, int* evals,
                   int* iters, int* rounds, int* converged, int* done, int* lsfails, int* not_done);

/* Standalone ops on the same kernels. */
/* exponential!(A, ExpMethodHigham2005()) for `count` independent N x N matrices
 * (src/gradient_computations.jl:24, third-party ExponentialUtilities). */
int qoc_expm_batched(int device, int N, int count, int precision, const double* A, double* X,
                     int* degree_out, int* squarings_out);
/* expm_jacobian! (src/gradient_computations.jl:177-213): dFdp_j for F = exp(dt(A0 + sum p_j A_j)),
 * truncated Taylor order 1..4; dFdp_out is nu x (N x N). */
int qoc_expm_jacobian(int device, int N, int nu, const double* A0, const double* const* Aj,
                      const double* p, int order, double dt, double* dFdp_out);

#ifdef __cplusplus
}
#endif
#endif /* QOC_MI355X_H */
