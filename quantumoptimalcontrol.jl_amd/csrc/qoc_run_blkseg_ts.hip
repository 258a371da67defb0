// qoc_run_blkseg_ts.hip — the gate duration as a per-seed variable (qoc_set_time_scale): the TS instantiations of the
// segmented eval, fused and as forward and backward halves (a translation unit of their own: 21 kernels, all at 8
// waves).  The eval that launches them is blkseg_eval_ts (qoc_run_blkseg.hip).
#include "qoc_blkseg_host.hpp"

namespace qoc_host {

hipError_t blkseg_launch_ts(qoc_ctx* c, int mode, int order, const BlksegShape& s, const BlksegParams& sp) {
  const TChainArgs g = tchain_args(c);
  const BlkArgs bk = blk_args(c);
  const bool fwd = mode == BLKSEG_FWD;
  return blkseg_dispatch(c->blk_nb, fwd ? 1 : order, [&](auto NB_, auto ORD_) {
    constexpr int NB = decltype(NB_)::value, ORD = decltype(ORD_)::value;
    auto launch = [&](auto PEN_, auto MODE_) {
      constexpr bool PEN = decltype(PEN_)::value;
      constexpr int MODE = decltype(MODE_)::value;
      // built: the fused eval on blocks of 2 rows with and without the penalty and on blocks of 3 rows without; the
      // halves for penalised blocks of 3 rows alone (blkseg_eval_ts), the forward half at ORD 1 only
      if constexpr (MODE == BLKSEG_FUSED ? (PEN && NB == 3) : (!PEN || NB != 3 || (MODE == BLKSEG_FWD && ORD != 1))) {
        return hipErrorInvalidValue;
      } else {
        auto kern = k_blkseg_eval<NB, ORD, 8, MODE, PEN, false, true>;
        bool& set = c->seg_attr_ts[NB - 2][ORD == 0 ? BLK_ORDMAX : ORD - 1][MODE][PEN ? 1 : 0];
        if (s.lds > 65536 && !set) {
          hipFuncAttributes fa{};
          hipError_t e = hipFuncGetAttributes(&fa, (const void*)kern);
          if (e != hipSuccess) return e;
          e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(BLKSEG_LDS_MAX - fa.sharedSizeBytes));
          if (e != hipSuccess) return e;
          set = true;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)c->B), dim3(64 * s.W), s.lds, c->stream, g, bk, sp);
        return hipGetLastError();
      }
    };
    auto with_pen = [&](auto MODE_) {
      if (sp.pen_mu != 0.0) return launch(std::true_type(), MODE_);
      return launch(std::false_type(), MODE_);
    };
    if (fwd) return with_pen(std::integral_constant<int, BLKSEG_FWD>());
    if (mode == BLKSEG_BWD) return with_pen(std::integral_constant<int, BLKSEG_BWD>());
    return with_pen(std::integral_constant<int, BLKSEG_FUSED>());
  });
}

}  // namespace qoc_host
