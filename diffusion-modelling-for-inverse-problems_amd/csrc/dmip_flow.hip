// Model log-density log p(x | y) of the CDE and Posterior estimators by the instantaneous change of variables along
// the probability-flow ODE (sdes.py:77-87 at lmbd = 1; Song et al. 2021, section 4.3), in exact f32 on the f32 MFMA.
// The integrator (forward grid, Heun, an f64 sum of 2S divergence terms) is dmip_flow_rows.h's logp_rows.
// a is the network output (CDE), or g(tau) (prior(x, tau) + likelihood(x, y, tau)) (Posterior, nets.py:155-157).
//
// The networks run on dmip_f32.h's FEngine: the samplers' weight images, LDS-DMA ring and per-y layer-1 image (y
// folded into the bias column), over 4 rows x (primal + 3 tangents) per wave (dmip_flow.h). Rows are spread over a
// static grid: the rows of a call share a step count, so the samplers' balanced hand-over is not needed.
#include "dmip_flow.h"

namespace dmip {
namespace f32 {

template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, 1) f32_flow_kernel(F32FlowParams p) {
  using C = SamplerCfg<MODE, W, D, 0, 0>;
  using L = typename C::L;
  using E = typename C::E;
  static_assert(L::TOTAL <= kLdsBudget, "LDS budget");
  static_assert(D <= 3, "a quad holds the primal and at most 3 tangents");
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15, m = lane & 3;
  const int yi = blockIdx.y;

  E eng{lds, {p.net[0].stream, p.net[1].stream}, {L::BIAS, L::BIAS + L::BIAS_BYTES}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<Shape<W>::NW> rows(p.rows.n, w, g, j, m);
  flow_setup<C, W>(eng, lds, p.net, p.l1y, p.n_hidden, yi);

  bool nonfinite = false;  // exact f32 has no range to leave: not reported
  flow::logp_rows<D>(p.rows, rows, yi, nonfinite,
                     [&](const float (&xt)[D], const flow::FlowCoef& cf, float (&a)[D], float& dv)
                         __attribute__((always_inline)) { flow_score<C, MODE, D>(eng, g, j, m, xt, cf, a, dv); });
  eng.finish();
}

}  // namespace f32

// Compiled: what the exact-f32 CDE and Posterior samplers support (widths 64 / 128 / 256 / 512, 1 to 3 hidden
// layers, xdim 2 or 3, any ydim), the tanh chain only (the caller refuses a SiLU network)
bool f32_flow_supported(int mode, int width, int n_hidden, int xdim, int ydim) {
  if (mode != SAMPLER_CDE && mode != SAMPLER_POSTERIOR) return false;
  return f32_sampler_supported(mode, width, n_hidden, xdim, ydim);
}

hipError_t launch_f32_flow(const F32FlowParams& p, int mode, int width, int n_hidden, int xdim, int ydim, int n_y,
                           hipStream_t st, bool* supported) {
  *supported = false;
  if (!f32_flow_supported(mode, width, n_hidden, xdim, ydim)) return hipSuccess;
  *supported = true;
#define X(Wv, Dv)                                                                                        \
  if (width == Wv && xdim == Dv)                                                                         \
    return flow_launch(mode == SAMPLER_CDE ? f32::f32_flow_kernel<SAMPLER_CDE, Wv, Dv>                   \
                                           : f32::f32_flow_kernel<SAMPLER_POSTERIOR, Wv, Dv>,            \
                       f32::Shape<Wv>::NW, p, p.rows.n, n_y, st);
  DMIP_FLOW_SHAPES(X)
#undef X
  *supported = false;
  return hipSuccess;
}

}  // namespace dmip
