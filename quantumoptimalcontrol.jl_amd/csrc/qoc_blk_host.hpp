// qoc_blk_host.hpp — host helpers shared by the translation units that launch block kernels (qoc_run_blk.hip,
// qoc_run_blkp.hip, qoc_run_blku.hip, qoc_run_blkseg.hip).
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

static inline bool blk_big(const qoc_ctx* c) { return c->blk_nb == 16; }  // blocks of 5..16 rows: one MFMA wave each

// dynamic LDS above the 64 KiB default (up to 16 MFMA block waves of staging)
template <typename K>
static inline hipError_t blk_lds_attr(K kern, size_t lds) {
  return lds > 65536 ? hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                     : hipSuccess;
}

// d_coef_mu (allocated on first use): the λ_N coefficients of an eval or backward that leaves μ_k in d_L
static inline int blk_coef_mu(qoc_ctx* c) {
  if (c->d_coef_mu) return QOC_OK;
  HIPCHK(c, c->d_coef_mu.alloc((size_t)c->B * 2 * c->m_user * sizeof(cx<double>)));
  return QOC_OK;
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
