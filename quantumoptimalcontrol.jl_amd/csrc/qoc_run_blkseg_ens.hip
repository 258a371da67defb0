// qoc_run_blkseg_ens.hip — the risk objectives over a generator ensemble (qoc_set_ensemble_objective): the ENS
// instantiations of the segmented eval's forward and backward halves (a translation unit of their own: 18 kernels),
// k_ens_weights and k_ens_reduce_w.  The eval that strings them together is blkseg_eval_ens (qoc_run_blkseg.hip).
#include "qoc_blkseg_host.hpp"

namespace qoc_host {

hipError_t blkseg_launch_ens_half(qoc_ctx* c, int mode, int order, const BlksegShape& s, const BlksegParams& sp) {
  TChainArgs g = tchain_args(c);
  g.J = c->d_ens_J;
  g.coef = c->d_ens_coef;
  const BlkArgs bk = blk_args(c);
  const bool fwd = mode == BLKSEG_FWD;
  return blkseg_dispatch(c->blk_nb, fwd ? 1 : order, [&](auto NB_, auto ORD_) {
    constexpr int NB = decltype(NB_)::value, ORD = decltype(ORD_)::value;
    auto launch = [&](auto PEN_, auto MODE_) {
      constexpr bool PEN = decltype(PEN_)::value;
      constexpr int MODE = decltype(MODE_)::value;
      // built: blocks of 2 rows with and without the penalty, blocks of 3 rows without; the forward half at ORD 1 only
      if constexpr ((PEN && NB == 3) || (MODE == BLKSEG_FWD && ORD != 1)) {
        return hipErrorInvalidValue;
      } else {
        auto kern = k_blkseg_eval<NB, ORD, 8, MODE, PEN, true>;
        bool& set = c->seg_attr_ens_half[NB - 2][ORD == 0 ? BLK_ORDMAX : ORD - 1][MODE - 1][PEN ? 1 : 0];
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
    auto with_pen = [&](auto MODE_) {
      if (sp.pen_mu != 0.0) return launch(std::true_type(), MODE_);
      return launch(std::false_type(), MODE_);
    };
    if (fwd) return with_pen(std::integral_constant<int, BLKSEG_FWD>());
    return with_pen(std::integral_constant<int, BLKSEG_BWD>());
  });
}

hipError_t ens_weights_launch(qoc_ctx* c, double* d_J) {
  const int E = c->ens_E;
  double* const J2 = d_J && d_J != c->d_J ? d_J : nullptr;
  // costs, weights and a scratch row in LDS while they fit the default limit; a larger ensemble reads them in place
  const bool lds_ok = (size_t)E * 3 * sizeof(double) <= 48 * 1024;
  if (lds_ok)
    hipLaunchKernelGGL(k_ens_weights<true>, dim3((unsigned)c->B), dim3(64), (size_t)E * 3 * sizeof(double), c->stream, E,
                       c->ens_obj, c->ens_obj_param, c->d_ens_w, c->d_ens_J, c->d_ens_om, c->d_J, J2);
  else
    hipLaunchKernelGGL(k_ens_weights<false>, dim3((unsigned)c->B), dim3(64), 0, c->stream, E, c->ens_obj,
                       c->ens_obj_param, c->d_ens_w, c->d_ens_J, c->d_ens_om, c->d_J, J2);
  return hipGetLastError();
}

hipError_t ens_reduce_w_launch(qoc_ctx* c, double* d_dJdu) {
  const int n = c->Nt * c->nu;
  const bool vec = c->nu == 2 && (reinterpret_cast<size_t>(d_dJdu) & 15) == 0;
  const long long thr = std::max<long long>((long long)c->B * (vec ? n / 2 : n), 1);
  const unsigned grid = (unsigned)((thr + 255) / 256);
  if (vec)
    hipLaunchKernelGGL(k_ens_reduce_w<true>, dim3(grid), dim3(256), 0, c->stream, c->B, c->ens_E, n, c->d_ens_om,
                       c->d_ens_g, d_dJdu);
  else
    hipLaunchKernelGGL(k_ens_reduce_w<false>, dim3(grid), dim3(256), 0, c->stream, c->B, c->ens_E, n, c->d_ens_om,
                       c->d_ens_g, d_dJdu);
  return hipGetLastError();
}

}  // namespace qoc_host
