// qoc_blkseg_host.hpp — what the translation units that launch the segmented eval share (qoc_run_blkseg.hip: the
// plain and the fused ensemble launches; qoc_run_blkseg_ens.hip: the ensemble's forward and backward halves;
// qoc_run_blkseg_ts.hip: the launches under a time scale).
#pragma once
#include "qoc_blk_host.hpp"
#include "qoc_blkseg.hpp"
#include "qoc_internal.hpp"

namespace qoc_host {

// (the exact tag has its own dispatch: blk_order_dispatch and BLK_ORDMAX stay the Taylor orders' alone, so the
// k_blku_*, k_blkp_* and dense kernels keep refusing or routing QOC_DUKDP_EXACT as before)
template <typename F>
static hipError_t blkseg_dispatch(int NB, int order, F&& f) {
  if (order == QOC_DUKDP_EXACT) {
    const std::integral_constant<int, 0> ex;
    if (NB == 2) return f(std::integral_constant<int, 2>(), ex);
    return f(std::integral_constant<int, 3>(), ex);
  }
  return blk_order_dispatch(order, [&](auto ORD_) {
    if (NB == 2) return f(std::integral_constant<int, 2>(), ORD_);
    return f(std::integral_constant<int, 3>(), ORD_);
  });
}

// One half of the segmented eval on B E (pulse, member) workgroups (mode BLKSEG_FWD or BLKSEG_BWD; the forward half
// ignores the order).  sp is complete (the member tables, E, gseg / dseg, and for the backward half omega); J and the
// coefficients go to the ensemble's workspace.
hipError_t blkseg_launch_ens_half(qoc_ctx* c, int mode, int order, const BlksegShape& s, const BlksegParams& sp);

// The segmented eval under a per-seed time scale on B workgroups (qoc_run_blkseg_ts.hip; mode BLKSEG_FUSED, or
// BLKSEG_FWD / BLKSEG_BWD for penalised blocks of 3 rows).  sp is complete, with tau and dJdtau.
hipError_t blkseg_launch_ts(qoc_ctx* c, int mode, int order, const BlksegShape& s, const BlksegParams& sp);

// ω and J̄ from the member costs of the launch before it (k_ens_weights), and the ω-weighted sum of the member
// gradients (k_ens_reduce_w), on the context's stream
hipError_t ens_weights_launch(qoc_ctx* c, double* d_J);
hipError_t ens_reduce_w_launch(qoc_ctx* c, double* d_dJdu);

}  // namespace qoc_host
