// Guided posterior sampling for a linear-Gaussian problem with the Tweedie-covariance guidance
// (dmip_dps_tweedie_sample): the fp32x3 kernel. dmip_x3_dps_linear.hip's kernel with DpsTweedieChains: the scheme, and
// the D x D solve it adds per row and step (plain f32 beside the split network), are stated at dmip_flow_rows.h's
// dps_linear_rows. A layer-1 input of a kept row beyond the split's range, or a kept row whose final state is not finite
// (a zero determinant ends there), is reported through the device status word (kErrRange).
#include "dmip_x3_flow.h"

namespace dmip {
namespace x3 {

template <int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, Shape<W>::NW / 4) x3_dps_tweedie_kernel(X3DpsTweedieParams p) {
  using C = SamplerCfg<SAMPLER_CDE, W, D, 0, 0>;
  using L = typename C::L;
  using E = typename C::E;
  constexpr int NW = Shape<W>::NW;
  static_assert(L::TOTAL <= kLdsBudget, "LDS budget");
  static_assert(D <= 3, "a quad holds the primal and at most 3 tangents");
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15, m = lane & 3;
  const int yi = blockIdx.y;

  E eng{lds, {p.net.stream, p.net.stream}, {L::L1, L::L1}, {L::BIAS, L::BIAS}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<NW> rows(p.chains.lin.n, w, g, j, m);
  // set-up (flow_setup's, one network, the network's own layer-1 bias): layer-1 image and biases into LDS, ring started
  if constexpr (C::L1H) {  // lanes 0-31 of each tile's 1 KiB ([tile][64 lanes][16 B] -> [tile][32][16 B])
    const uint4* s1 = (const uint4*)p.net.l1;
    uint4* d1 = (uint4*)(lds + L::L1);
    for (int e = threadIdx.x; e < L::L1_BYTES / 16; e += NW * 64) d1[e] = s1[(e >> 5) * 64 + (e & 31)];
  } else {
    eng.stage(lds + L::L1, p.net.l1, L::L1_BYTES);
  }
  const int bf = p.n_hidden * W + 16;
  float* bl = (float*)(lds + L::BIAS);
  for (int i = threadIdx.x; i < bf; i += NW * 64) bl[i] = p.net.bias[i];
  eng.start();

  bool oor = false;
  flow::dps_linear_rows<D>(p.chains, rows, yi, oor,
                           [&](const float (&xt)[D], const StepCoef& c, float (&s)[D], float (&J)[D][D])
                               __attribute__((always_inline)) {
                                 const f32x4 out = flow_out<C, D>(eng, g, m, xt, c, rows.valid, oor);
                                 flow::gather_jac<D>(out, j, s, J);
                               });
  eng.finish();
  report_range(oor, p.err, lane);
}

}  // namespace x3

hipError_t launch_x3_dps_tweedie(const X3DpsTweedieParams& p, int width, int xdim, int n_y, hipStream_t st, bool* ok) {
  *ok = true;
#define X(Wv, Dv) \
  if (width == Wv && xdim == Dv) \
    return flow_launch(x3::x3_dps_tweedie_kernel<Wv, Dv>, x3::Shape<Wv>::NW, p, p.chains.lin.n, n_y, st);
  DMIP_FLOW_SHAPES(X)
#undef X
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
