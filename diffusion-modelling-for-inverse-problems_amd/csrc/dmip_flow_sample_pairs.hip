// Paired samples with their log-density, one observation per row, in exact f32: x_i ~ q(. | y_i) and log q(x_i | y_i)
// by dmip_flow_rows.h's sample_rows at y index 0 over a (g, 1) grid, the network with the rows' own layer-1 bias
// (dmip_flow_pairs.h). Row i draws its start from stream (seed, chain_offset + i, 0): the start of the per-y sampler's
// chain `chain_offset + i` of y index 0.
#include "dmip_flow_pairs.h"

namespace dmip {
namespace f32 {

template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, 1) f32_flow_sample_pairs_kernel(F32FlowSamplePairsParams pp) {
  using C = SamplerCfg<MODE, W, D, 0, 0>;
  using L = typename C::L;
  using E = typename C::E;
  static_assert(L::TOTAL <= kLdsBudget, "LDS budget");
  static_assert(D <= 3, "a quad holds the primal and at most 3 tangents");
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const F32FlowSampleParams& p = pp.f;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15, m = lane & 3;

  E eng{lds, {p.net[0].stream, p.net[1].stream}, {L::BIAS, L::BIAS + L::BIAS_BYTES}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<Shape<W>::NW> rows(p.chains.n, w, g, j, m);
  flow_setup<C, W>(eng, lds, p.net, p.l1y, p.n_hidden, 0);  // the one shared image

  bool nonfinite = false;  // exact f32 has no range to leave: not reported
  flow::sample_rows<D>(p.chains, rows, 0, nonfinite,
                       [&](const float (&xt)[D], const StepCoef& c, float (&a)[D], float& dv)
                           __attribute__((always_inline)) {
        // the row's bias address (dmip_flow_pairs.h) is formed here, at each evaluation, from the row index the
        // driver keeps anyway: a pointer held across the layers cost the W >= 256 kernels more scratch
        unsigned r = (unsigned)rows.row;
        asm volatile("" : "+v"(r));
        const float* cb = pp.row_bias + ((rows.valid ? r : 0u) * (unsigned)W + 4u * (unsigned)g);
        flow_score_pairs<C, MODE, D>(eng, g, j, m, xt, c, cb, a, dv);
      });
  eng.finish();
}

}  // namespace f32

hipError_t launch_f32_flow_sample_pairs(const F32FlowSamplePairsParams& p, int mode, int width, int n_hidden, int xdim,
                                        int ydim, hipStream_t st, bool* supported) {
  *supported = false;
  if (!f32_flow_sample_supported(mode, width, n_hidden, xdim, ydim)) return hipSuccess;
  *supported = true;
#define X(Wv, Dv)                                                                                           \
  if (width == Wv && xdim == Dv)                                                                            \
    return flow_launch(mode == SAMPLER_CDE ? f32::f32_flow_sample_pairs_kernel<SAMPLER_CDE, Wv, Dv>         \
                                           : f32::f32_flow_sample_pairs_kernel<SAMPLER_POSTERIOR, Wv, Dv>,  \
                       f32::Shape<Wv>::NW, p, p.f.chains.n, 1, st);
  DMIP_FLOW_SHAPES(X)
#undef X
  *supported = false;
  return hipSuccess;
}

}  // namespace dmip
