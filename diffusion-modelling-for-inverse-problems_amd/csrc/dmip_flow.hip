// Model log-density log p(x | y) of the CDE and Posterior estimators by the instantaneous change of variables along
// the probability-flow ODE (sdes.py:77-87 at lmbd = 1; Song et al. 2021, section 4.3), in exact f32 on the f32 MFMA.
//
// Forward time grid tau_k = linspace_at(k, S) T (the sampler's schedule, reversed), h = T / S, and for a row x_0 = x
//   v(x, tau)    = -1/2 beta(tau) x - 1/2 g(tau) a(x, y, tau)                 (= -mu(T - tau, x, y, lmbd = 1))
//   divv(x, tau) = -1/2 beta(tau) d - 1/2 g(tau) sum_i da_i/dx_i
// integrated with Heun's explicit trapezoid, k = 0..S-1:
//   k1 = v(x_k, tau_k), x~ = x_k + h k1, k2 = v(x~, tau_{k+1}), x_{k+1} = x_k + (h/2)(k1 + k2)
//   I += (h/2)(divv(x_k, tau_k) + divv(x~, tau_{k+1}))                        (f64: 2S terms)
//   log p(x | y) = -(d/2) log 2 pi - 1/2 |x_S|^2 + I
// a is the network output (CDE), or g(tau) (prior(x, tau) + likelihood(x, y, tau)) (Posterior, nets.py:155-157).
//
// The networks run on dmip_f32.h's FEngine: the samplers' weight images, LDS-DMA ring and per-y layer-1 image (y
// folded into the bias column), over 4 rows x (primal + 3 tangents) per wave (dmip_flow.h). Rows are spread over a
// static grid: the rows of a call share a step count, so the samplers' balanced hand-over is not needed.
#include "dmip_flow.h"

namespace dmip {
namespace f32 {

struct FlowCoef {
  float tau, beta, g;
};
__device__ __forceinline__ FlowCoef flow_coef(int k, int S, float T, float bmin, float bdiff) {
  FlowCoef c;
  c.tau = __fmul_rn(linspace_at(k, S), T);
  c.beta = __fadd_rn(bmin, __fmul_rn(bdiff, c.tau));
  c.g = (float)__dsqrt_rn((double)c.beta);
  return c;
}

template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, 1) f32_flow_kernel(F32FlowParams p) {
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

  const int S = p.num_steps;
  const long long tiles = (p.n + 3) / 4;  // 4 rows per wave pass
  const long long per_round = (long long)gridDim.x * NW;
  const long long rounds = (tiles + per_round - 1) / per_round;
  const float hh = __fmul_rn(0.5f, p.h);

  for (long long rd = 0; rd < rounds; ++rd) {
    const long long row = ((rd * gridDim.x + blockIdx.x) * NW + w) * 4 + (j >> 2);
    const bool valid = row < p.n;
    const long long rr = valid ? row : 0;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const float xv = p.x[((size_t)yi * p.n + rr) * D + k];
      x[k] = valid ? xv : 0.0f;  // idle columns compute on zeros and are not stored
    }
    double I = 0.0;
    for (int k = 0; k < S; ++k) {
      float k1[D], xt[D], d1 = 0.0f;
#pragma unroll
      for (int i = 0; i < D; ++i) xt[i] = x[i];
      // stage 0: k1 and divv at (x_k, tau_k); stage 1: k2 and divv at (x~, tau_{k+1}) -- one copy of the network code
#pragma unroll 1
      for (int stage = 0; stage < 2; ++stage) {
        const FlowCoef cf = flow_coef(k + stage, S, p.T, p.bmin, p.bdiff);
        float a[D], dv;
        flow_score<C, MODE, D>(eng, g, j, m, xt, cf, a, dv);
        const float dd = -(0.5f * cf.beta * (float)D + 0.5f * cf.g * dv);
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const float kv = -(0.5f * cf.g * a[i] + 0.5f * cf.beta * xt[i]);
          if (stage == 0) {
            k1[i] = kv;
            xt[i] = x[i] + p.h * kv;
          } else {
            x[i] = x[i] + hh * (k1[i] + kv);
          }
        }
        if (stage == 0) d1 = dd;
        else I += (double)hh * ((double)d1 + (double)dd);
      }
    }
    if (valid && g == 0 && m == 0) {
      double r2 = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) r2 += (double)x[i] * (double)x[i];
      const size_t o = (size_t)yi * p.n + row;
      p.logp[o] = (float)(-0.5 * (double)D * 1.8378770664093453 - 0.5 * r2 + I);  // log 2 pi
      if (p.latent) {
#pragma unroll
        for (int i = 0; i < D; ++i) p.latent[o * D + i] = x[i];
      }
    }
  }
  eng.finish();
}

}  // namespace f32

template <int MODE, int W, int D>
static hipError_t launch_f32_flow_t(const F32FlowParams& p, int n_y, hipStream_t st) {
  constexpr int NW = f32::Shape<W>::NW;
  auto kern = f32::f32_flow_kernel<MODE, W, D>;
  const unsigned g = f32::flow_grid_x(kern, NW, p.n, n_y, st);
  hipLaunchKernelGGL(kern, dim3(g, (unsigned)n_y), dim3(NW * 64), 0, st, p);
  return hipGetLastError();
}

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
#define X(Wv, Dv)                                                                              \
  if (width == Wv && xdim == Dv)                                                               \
    return mode == SAMPLER_CDE ? launch_f32_flow_t<SAMPLER_CDE, Wv, Dv>(p, n_y, st)            \
                               : launch_f32_flow_t<SAMPLER_POSTERIOR, Wv, Dv>(p, n_y, st);
  X(64, 2) X(128, 2) X(256, 2) X(512, 2) X(64, 3) X(128, 3) X(256, 3) X(512, 3)
#undef X
  *supported = false;
  return hipSuccess;
}

}  // namespace dmip
