// Guided posterior sampling for a linear-Gaussian problem with the Tweedie-covariance guidance
// (dmip_dps_tweedie_sample): the exact-f32 kernel. dmip_dps_linear.hip's kernel with DpsTweedieChains: the scheme, and the
// D x D solve it adds per row and step, are stated at dmip_flow_rows.h's dps_linear_rows. Network, columns, static grid
// and LDS layout are the dps_linear kernel's.
#include "dmip_flow.h"

namespace dmip {
namespace f32 {

template <int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, 1) f32_dps_tweedie_kernel(F32DpsTweedieParams p) {
  using C = SamplerCfg<SAMPLER_CDE, W, D, 0, 0>;
  using L = typename C::L;
  using E = typename C::E;
  constexpr int NW = Shape<W>::NW, ST = Shape<W>::ST;
  static_assert(L::TOTAL <= kLdsBudget, "LDS budget");
  static_assert(D <= 3, "a quad holds the primal and at most 3 tangents");
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15, m = lane & 3;
  const int yi = blockIdx.y;

  E eng{lds, {p.net.stream, p.net.stream}, {L::BIAS, L::BIAS}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<NW> rows(p.chains.lin.n, w, g, j, m);
  // set-up: the prior's layer-1 image and biases into LDS, ring started
  const int bf = (p.n_hidden - 1) * W + 16;
  eng.stage(lds + L::L1_0, (const char*)p.net.l1, ST * C::K1Q0 * 256);
  float* bl = (float*)(lds + L::BIAS);
  for (int i = threadIdx.x; i < bf; i += NW * 64) bl[i] = p.net.bias[i];
  eng.start();

  bool nonfinite = false;  // (the exact-f32 engine has no range to report)
  flow::dps_linear_rows<D>(p.chains, rows, yi, nonfinite,
                           [&](const float (&xt)[D], const StepCoef& c, float (&s)[D], float (&J)[D][D])
                               __attribute__((always_inline)) {
                                 const f32x4 out = flow_out<C, D>(eng, g, m, xt, c);
                                 flow::gather_jac<D>(out, j, s, J);
                               });
  eng.finish();
}

}  // namespace f32

// Compiled: the shapes of dps_linear_supported
hipError_t launch_f32_dps_tweedie(const F32DpsTweedieParams& p, int width, int xdim, int n_y, hipStream_t st, bool* ok) {
  *ok = true;
#define X(Wv, Dv) \
  if (width == Wv && xdim == Dv) \
    return flow_launch(f32::f32_dps_tweedie_kernel<Wv, Dv>, f32::Shape<Wv>::NW, p, p.chains.lin.n, n_y, st);
  DMIP_FLOW_SHAPES(X)
#undef X
  *ok = false;
  return hipSuccess;
}

}  // namespace dmip
