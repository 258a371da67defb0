// qoc_blk_host.hpp — host helpers shared by the translation units that launch block kernels (qoc_run_blk.hip,
// qoc_run_blkseg.hip).
#pragma once
#include "qoc_blk.hpp"
#include "qoc_internal.hpp"

namespace qoc_host {

static inline BlkArgs blk_args(const qoc_ctx* c) {
  BlkArgs bk{};
  bk.brow = c->d_brow;
  bk.A = c->d_A;
  bk.nblk = c->nblk;
  bk.wrow = c->d_wrow;
  bk.nwb = c->nwb;
  return bk;
}

// the gradient order 1..4 as a compile-time constant
template <typename F>
static hipError_t blk_order_dispatch(int order, F&& f) {
  using std::integral_constant;
  switch (order) {
    case 1: return f(integral_constant<int, 1>());
    case 2: return f(integral_constant<int, 2>());
    case 3: return f(integral_constant<int, 3>());
    default: return f(integral_constant<int, 4>());
  }
}

}  // namespace qoc_host
