// Exact-f32 sampler instantiations: SAMPLER_POSTERIOR, the stochastic table-driven multistep sampler
// (SOLVER_TABLE_SDE: SDE-DPM-Solver++(2M), ancestral / eta-DDIM; dmip_f32.h, dmip_device.h MultistepStep), at the
// shapes of the deterministic unit dmip_f32_post_ms.hip: no width 512. Every kernel is free of scratch.
#include "dmip_f32.h"

namespace dmip {

hipError_t launch_f32_sampler_post_ms_sde(const F32SamplerParams& p, int width, int xdim, int n_y, hipStream_t st,
                                        bool* ok) {
  *ok = true;
#define X(Wv, Dv)                \
  if (width == Wv && xdim == Dv) \
    return launch_f32_sampler_t<SAMPLER_POSTERIOR, Wv, Dv, 0, false, 0, SOLVER_TABLE_SDE>(p, n_y, st);
  X(64, 2) X(128, 2) X(256, 2) X(64, 3) X(128, 3) X(256, 3)
#undef X
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
