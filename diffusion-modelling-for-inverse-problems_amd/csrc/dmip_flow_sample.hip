// Samples of the CDE and Posterior estimators together with their model log-density: x ~ q(. | y) by the Heun sampler
// of the probability-flow ODE (dmip_device.h HeunStep) and log q(x | y) by the instantaneous change of variables along
// the same trajectory, in exact f32 on the f32 MFMA, one launch. The scheme (the samplers' reverse grid, the x0 or RNG
// start, the base density folded into the f64 accumulator) is stated at dmip_flow_rows.h's sample_rows; a is the
// network output (CDE) or g_i (prior + likelihood) (Posterior, whose divergence carries g_i too).
//
// Networks, columns (4 rows x (primal + 3 tangents) per wave) and the static grid are dmip_flow.hip's (dmip_flow.h).
#include "dmip_flow.h"

namespace dmip {
namespace f32 {

// This kernel keeps its set-up and its loop written out: the text of f32::flow_setup and of flow::sample_rows (keep
// the three in step). Through the shared functions the W 512 instantiations, which spill 728 to 1,416 B per lane,
// were allocated differently: the CDE xdim-3 kernel grew by 189 instructions and measured 0.5 % slower at 30,000 rows
// x 200 steps (profiles/flow_rows/README.md). Written out, every instantiation compiles to the code it had.
template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, 1) f32_flow_sample_kernel(F32FlowSampleParams p) {
  using C = SamplerCfg<MODE, W, D, 0, 0>;
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
  const FlowChains& q = p.chains;

  E eng{lds, {p.net[0].stream, p.net[1].stream}, {L::BIAS, L::BIAS + L::BIAS_BYTES}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  const int bf = (p.n_hidden - 1) * W + 16;
  eng.stage(lds + L::L1_0, (const char*)(p.l1y + (size_t)yi * ST * C::K1Q0 * 64), ST * C::K1Q0 * 256);
  if constexpr (C::NNET > 1) eng.stage(lds + L::L1_1, (const char*)p.net[1].l1, ST * C::K1Q1 * 256);
  for (int ni = 0; ni < C::NNET; ++ni) {
    float* bl = (float*)(lds + L::BIAS + ni * L::BIAS_BYTES);
    for (int i = threadIdx.x; i < bf; i += NW * 64) bl[i] = p.net[ni].bias[i];
  }
  eng.start();

  const int S = q.num_steps;
  const long long tiles = (q.n + 3) / 4;  // 4 rows per wave pass
  const long long per_round = (long long)gridDim.x * NW;
  const long long rounds = (tiles + per_round - 1) / per_round;
  const float hd = __fmul_rn(0.5f, q.delta);

  for (long long rd = 0; rd < rounds; ++rd) {
    const long long row = ((rd * gridDim.x + blockIdx.x) * NW + w) * 4 + (j >> 2);
    const bool valid = row < q.n;
    const long long rr = valid ? row : 0;
    float x[D];
    if (q.x0) {
      const float* src = q.x0 + ((size_t)yi * q.n + rr) * D;
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = src[k];
    } else {
      Rng rng = rng_init(q.seed, (uint64_t)(q.chain_offset + rr), (uint64_t)yi);
      float n0[D];
      rng_normals<D>(rng, n0);
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = __fadd_rn(__fmul_rn(n0[k], q.stdv), q.mean);
    }
    // acc = log N(x_0; mean, std^2 I) - J, from the f32 x_0 whichever way it came
    double acc = q.base;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double z = ((double)x[k] - (double)q.mean) / (double)q.stdv;
      acc -= 0.5 * z * z;
      x[k] = valid ? x[k] : 0.0f;  // idle columns compute on zeros and are not stored
    }
    for (int i = 0; i < S; ++i) {
      float k1[D], xt[D], d1 = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) xt[k] = x[k];
      // stage 0: k1 and dm at (x_i, i); stage 1: k2 and dm at (x~, i + 1) -- one copy of the network code
#pragma unroll 1
      for (int stage = 0; stage < 2; ++stage) {
        const StepCoef c = step_coef(i + stage, S, q.T, q.bmin, q.bdiff, 0.5f, 0.0f);  // lmbd = 1: g_mu = fl(0.5 g)
        float a[D], dv;
        flow_score<C, MODE, D>(eng, g, j, m, xt, c, a, dv);
        const float dd = 0.5f * c.g * dv + 0.5f * c.beta * (float)D;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float mk = HeunStep::slope(xt[k], a[k], c);
          if (stage == 0) {
            k1[k] = mk;
            xt[k] = HeunStep::predict(x[k], mk, q.delta);
          } else {
            x[k] = HeunStep::correct(x[k], k1[k], mk, q.delta);
          }
        }
        if (stage == 0) d1 = dd;
        else acc -= (double)hd * ((double)d1 + (double)dd);
      }
    }
    if (valid && g == 0 && m == 0) {
      const size_t o = (size_t)yi * q.n + row;
      q.logq[o] = (float)acc;
#pragma unroll
      for (int k = 0; k < D; ++k) q.x_out[o * D + k] = x[k];
    }
  }
  eng.finish();
}

}  // namespace f32

// Compiled: the shapes of the log-likelihood kernel (f32_flow_supported), the tanh chain only
bool f32_flow_sample_supported(int mode, int width, int n_hidden, int xdim, int ydim) {
  return f32_flow_supported(mode, width, n_hidden, xdim, ydim);
}

hipError_t launch_f32_flow_sample(const F32FlowSampleParams& p, int mode, int width, int n_hidden, int xdim, int ydim,
                                  int n_y, hipStream_t st, bool* supported) {
  *supported = false;
  if (!f32_flow_sample_supported(mode, width, n_hidden, xdim, ydim)) return hipSuccess;
  *supported = true;
#define X(Wv, Dv)                                                                                        \
  if (width == Wv && xdim == Dv)                                                                         \
    return flow_launch(mode == SAMPLER_CDE ? f32::f32_flow_sample_kernel<SAMPLER_CDE, Wv, Dv>            \
                                           : f32::f32_flow_sample_kernel<SAMPLER_POSTERIOR, Wv, Dv>,     \
                       f32::Shape<Wv>::NW, p, p.chains.n, n_y, st);
  DMIP_FLOW_SHAPES(X)
#undef X
  *supported = false;
  return hipSuccess;
}

}  // namespace dmip
