// Exact-f32 sampler instantiations: SAMPLER_CDE, Heun's trapezoid on the probability-flow ODE (dmip_f32.h,
// dmip_device.h HeunStep). Width 512 has the SiLU chain only: with the tanh chain the kernel needs scratch (as its
// Euler kernel does), and a Heun instantiation that spills is left out (f32_heun_supported).
#include "dmip_f32.h"

namespace dmip {

hipError_t launch_f32_sampler_cde_heun(const F32SamplerParams& p, int width, int xdim, int n_y, hipStream_t st,
                                       bool* ok) {
  *ok = true;
#define X(Wv, Dv)                                                                                   \
  if (width == Wv && xdim == Dv)                                                                    \
    return p.act ? launch_f32_sampler_t<SAMPLER_CDE, Wv, Dv, 0, false, 1, SOLVER_HEUN>(p, n_y, st)  \
                 : launch_f32_sampler_t<SAMPLER_CDE, Wv, Dv, 0, false, 0, SOLVER_HEUN>(p, n_y, st);
#define XS(Wv, Dv)                         \
  if (width == Wv && xdim == Dv && p.act) \
    return launch_f32_sampler_t<SAMPLER_CDE, Wv, Dv, 0, false, 1, SOLVER_HEUN>(p, n_y, st);
  X(64, 2) X(128, 2) X(256, 2) XS(512, 2) X(64, 3) X(128, 3) X(256, 3) XS(512, 3)
#undef X
#undef XS
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
