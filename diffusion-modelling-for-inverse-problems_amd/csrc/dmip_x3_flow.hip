// The probability-flow kernels on the fp32x3 engine (DMIP_PREC_F32X3): dispatch and the shapes compiled. Device code:
// dmip_x3_flow.h; the instantiations are spread over dmip_x3_flow_{cde,post}.hip (log p(x | y)) and
// dmip_x3_flow_sample_{cde,post}.hip (samples with their log-density) so they compile in parallel.
#include "dmip_x3_flow.h"

namespace dmip {

// Compiled: CDE and Posterior, xdim 2 or 3 (any ydim: y is folded into layer 1's bias), 1 to 3 hidden layers (a
// runtime count), widths 64 / 128 / 256 / 512 -- every one free of scratch
bool x3_flow_supported(int mode, int width, int n_hidden, int xdim, int ydim) {
  if (mode != SAMPLER_CDE && mode != SAMPLER_POSTERIOR) return false;
  return x3_sampler_supported(mode, width, n_hidden, xdim, ydim);
}

hipError_t launch_x3_flow(const X3FlowParams& p, int mode, int width, int n_hidden, int xdim, int ydim, int n_y,
                          hipStream_t st, bool* supported) {
  *supported = false;
  if (!x3_flow_supported(mode, width, n_hidden, xdim, ydim)) return hipSuccess;
  if (mode == SAMPLER_CDE) return launch_x3_flow_cde(p, width, xdim, n_y, st, supported);
  return launch_x3_flow_post(p, width, xdim, n_y, st, supported);
}

hipError_t launch_x3_flow_sample(const X3FlowSampleParams& p, int mode, int width, int n_hidden, int xdim, int ydim,
                                 int n_y, hipStream_t st, bool* supported) {
  *supported = false;
  if (!x3_flow_supported(mode, width, n_hidden, xdim, ydim)) return hipSuccess;
  if (mode == SAMPLER_CDE) return launch_x3_flow_sample_cde(p, width, xdim, n_y, st, supported);
  return launch_x3_flow_sample_post(p, width, xdim, n_y, st, supported);
}

}  // namespace dmip
