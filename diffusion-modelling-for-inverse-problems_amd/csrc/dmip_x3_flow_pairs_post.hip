// fp32-accurate split-fp16 paired flow kernel instantiations (one observation per row): log p(x_i | y_i),
// x3_flow_pairs_kernel, SAMPLER_POSTERIOR (dmip_x3_flow_pairs.h). Every shape is free of scratch.
#include "dmip_x3_flow_pairs.h"

namespace dmip {

hipError_t launch_x3_flow_pairs_post(const X3FlowPairsParams& p, int width, int xdim, hipStream_t st,
                                     bool* ok) {
  *ok = true;
#define X(Wv, Dv)                \
  if (width == Wv && xdim == Dv) \
    return flow_launch(x3::x3_flow_pairs_kernel<SAMPLER_POSTERIOR, Wv, Dv>, x3::Shape<Wv>::NW, p, p.x.rows.n, 1, st);
  DMIP_FLOW_SHAPES(X)
#undef X
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
