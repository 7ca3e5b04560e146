// The paired probability-flow kernels on the fp32x3 engine: dispatch. Device code: dmip_x3_flow_pairs.h; the
// instantiations are spread over dmip_x3_flow_pairs_{cde,post}.hip (log p(x_i | y_i)) and
// dmip_x3_flow_sample_pairs_{cde,post}.hip (samples with their log-density) so they compile in parallel.
#include "dmip_pairs.h"

namespace dmip {

hipError_t launch_x3_flow_pairs(const X3FlowPairsParams& p, int mode, int width, int n_hidden, int xdim, int ydim,
                                hipStream_t st, bool* supported) {
  *supported = false;
  if (!x3_flow_supported(mode, width, n_hidden, xdim, ydim)) return hipSuccess;
  if (mode == SAMPLER_CDE) return launch_x3_flow_pairs_cde(p, width, xdim, st, supported);
  return launch_x3_flow_pairs_post(p, width, xdim, st, supported);
}

hipError_t launch_x3_flow_sample_pairs(const X3FlowSamplePairsParams& p, int mode, int width, int n_hidden, int xdim,
                                       int ydim, hipStream_t st, bool* supported) {
  *supported = false;
  if (!x3_flow_supported(mode, width, n_hidden, xdim, ydim)) return hipSuccess;
  if (mode == SAMPLER_CDE) return launch_x3_flow_sample_pairs_cde(p, width, xdim, st, supported);
  return launch_x3_flow_sample_pairs_post(p, width, xdim, st, supported);
}

}  // namespace dmip
