// fp32-accurate split-fp16 flow kernel instantiations: log p(x | y) (x3_flow_kernel), SAMPLER_CDE
// (dmip_x3_flow.h). Every shape is free of scratch, width 512 included.
#include "dmip_x3_flow.h"

namespace dmip {

hipError_t launch_x3_flow_cde(const X3FlowParams& p, int width, int xdim, int n_y, hipStream_t st, bool* ok) {
  *ok = true;
#define X(Wv, Dv) \
  if (width == Wv && xdim == Dv) \
    return flow_launch(x3::x3_flow_kernel<SAMPLER_CDE, Wv, Dv>, x3::Shape<Wv>::NW, p, p.rows.n, n_y, st);
  DMIP_FLOW_SHAPES(X)
#undef X
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
