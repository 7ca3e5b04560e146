// fp32-accurate split-fp16 flow kernel instantiations: log p(x | y) (x3_flow_kernel), SAMPLER_CDE
// (dmip_x3_flow.h). Every shape is free of scratch, width 512 included.
#include "dmip_x3_flow.h"

namespace dmip {

hipError_t launch_x3_flow_cde(const X3FlowParams& p, int width, int xdim, int n_y, hipStream_t st, bool* ok) {
  *ok = true;
#define X(Wv, Dv) \
  if (width == Wv && xdim == Dv) return launch_x3_flow_t<SAMPLER_CDE, Wv, Dv>(p, n_y, st);
  X(64, 2) X(128, 2) X(256, 2) X(512, 2) X(64, 3) X(128, 3) X(256, 3) X(512, 3)
#undef X
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
