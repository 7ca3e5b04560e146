// fp32-accurate split-fp16 sampler instantiations: SAMPLER_CDE, the stochastic table-driven multistep sampler
// (SOLVER_TABLE_SDE: SDE-DPM-Solver++(2M), ancestral / eta-DDIM; the one-tile engine of dmip_x3.h, dmip_device.h
// MultistepStep), at the shapes of the deterministic unit dmip_x3_cde_ms.hip. Every kernel is free of scratch.
#include "dmip_x3.h"

namespace dmip {

hipError_t launch_x3_sampler_cde_ms_sde(const X3SamplerParams& p, int width, int xdim, int n_y, hipStream_t st,
                                           bool* ok) {
  *ok = true;
#define X(Wv, Dv)                \
  if (width == Wv && xdim == Dv) \
    return launch_x3_sampler_t<SAMPLER_CDE, Wv, Dv, 0, false, 0, SOLVER_TABLE_SDE>(p, n_y, st);
  X(64, 2) X(128, 2) X(256, 2) X(512, 2) X(64, 3) X(128, 3) X(256, 3) X(512, 3)
#undef X
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
