// fp32x3 flow kernel instantiations: samples with their log-density (x3_flow_sample_kernel), SAMPLER_POSTERIOR
// (dmip_x3_flow.h). Every shape is free of scratch, width 512 included.
#include "dmip_x3_flow.h"

namespace dmip {

hipError_t launch_x3_flow_sample_post(const X3FlowSampleParams& p, int width, int xdim, int n_y, hipStream_t st,
                                      bool* ok) {
  *ok = true;
#define X(Wv, Dv) \
  if (width == Wv && xdim == Dv) return launch_x3_flow_sample_t<SAMPLER_POSTERIOR, Wv, Dv>(p, n_y, st);
  X(64, 2) X(128, 2) X(256, 2) X(512, 2) X(64, 3) X(128, 3) X(256, 3) X(512, 3)
#undef X
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
