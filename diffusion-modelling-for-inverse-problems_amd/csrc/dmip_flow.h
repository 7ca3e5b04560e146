// What the probability-flow kernels with an exact divergence share (dmip_flow.hip: log p(x | y) of given rows;
// dmip_flow_sample.hip: samples with their log-density): the score network over primal + tangent columns on
// dmip_f32.h's FEngine.
//
// Columns follow the DPS kernel's scheme (dmip_surrogate.hip): the 16-column B operand of a wave holds 4 rows x
// (primal + 3 tangents), column j = 4 c + m with m = 0 the primal of row c and m = 1..3 the tangent along x_{m-1}.
// A tangent column enters layer 1 as the unit vector e_{m-1} in the x slots (0 in the t and bias slots), takes no
// bias in any layer, and its activation is act'(z_primal) z with the primal read from its quad by DPP. For xdim = 2
// the fourth column of a quad computes on zeros.
#pragma once
#include "dmip_f32.h"
#include "dmip_flow_rows.h"

namespace dmip {
namespace f32 {

using flow::quad_primal;

// activation of one tile: primal columns tanh (twice on layer 1, nets.py:21-26), tangent columns act'(z_primal) z
template <bool TWICE>
__device__ __forceinline__ void flow_act(const f32x4& z, int m, float (&H)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float zp = quad_primal(z[r]);
    const float t1 = tanhf(zp);
    float val, d;
    if constexpr (TWICE) {
      const float t2 = tanhf(t1);
      val = t2;
      d = (1.0f - t2 * t2) * (1.0f - t1 * t1);
    } else {
      val = t1;
      d = 1.0f - t1 * t1;
    }
    H[r] = m == 0 ? val : d * z[r];
  }
}

// one network over the 16 columns: the output tile (rows 4 g + r; a_i of the primal columns, da_i/dx_{m-1} of the
// tangent columns, at g = 0). The chunk stream is FEngine::eval's: (nl - 1) ST hidden tiles, then the output tile.
template <typename E, int K1Q>
__device__ __forceinline__ f32x4 flow_eval(E& eng, int ni, int l1_off, const float (&b)[K1Q], int m) {
  constexpr int ST = E::ST;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  float Ha[ST][4], Hb[ST][4];
  asm volatile("" ::: "memory");
  const float* l1 = (const float*)(eng.lds + l1_off);
#pragma unroll
  for (int o = 0; o < ST; ++o) {
    f32x4 z = zero;
#pragma unroll
    for (int s = 0; s < K1Q; ++s) z = mfma4(l1[(o * K1Q + s) * 64 + eng.lane], b[s], z);
    flow_act<true>(z, m, Ha[o]);
  }
  auto hidden = [&](int li, const float (&Hin)[ST][4], float (&Hout)[ST][4]) __attribute__((always_inline)) {
#pragma unroll
    for (int o = 0; o < ST; ++o) {
      const char* ch = eng.chunk_sync();
      const f32x4 bias = eng.bias4(ni, li, o);
      flow_act<false>(eng.tile_product(ch, Hin, m == 0 ? bias : zero), m, Hout[o]);
    }
  };
  const int nl = eng.nl;
  for (int li = 0; li + 1 < nl; li += 2) {
    hidden(li, Ha, Hb);
    if (li + 2 < nl) hidden(li + 1, Hb, Ha);
  }
  const char* ch = eng.chunk_sync();
  const f32x4 bias = eng.bias4(ni, nl - 1, 0);
  if ((nl & 1) != 0) return eng.tile_product(ch, Ha, m == 0 ? bias : zero);  // nl - 1 even: the last output is in Ha
  return eng.tile_product(ch, Hb, m == 0 ? bias : zero);
}

// a(x, y, tau) of the row on all its lanes, and sum_i da_i/dx_i (the tangent column 1 + i carries row i's derivative).
// C: the SamplerCfg of the kernel (its layer-1 images at L::L1_0 / L::L1_1); lane = 16 g + j, m = lane & 3; cf: the
// stage's coefficients (.tau, and .g: the Posterior estimator's factor on a and on its divergence, nets.py:155-157).
// Always inlined: an outlined call would put the activation arrays on the scratch stack. (Every argument by reference,
// as the lambda this was captured them: by value, the log-likelihood kernels compiled to other code)
template <typename C, int MODE, int D, typename Coef>
__device__ __forceinline__ void flow_score(typename C::E& eng, const int& g, const int& j, const int& m,
                                           const float (&xin)[D], const Coef& cf, float (&a)[D], float& dv) {
  using L = typename C::L;
  using E = typename C::E;
  float v[D + 1];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = xin[k];
  v[D] = cf.tau;
  float b0[C::K1Q0];
  l1_operand<D + 1, C::K1Q0>(v, g, b0);
#pragma unroll
  for (int s = 0; s < C::K1Q0; ++s) {
    const float e = (4 * s + g == m - 1 && m - 1 < D) ? 1.0f : 0.0f;
    b0[s] = m == 0 ? b0[s] : e;
  }
  f32x4 out = flow_eval<E, C::K1Q0>(eng, 0, L::L1_0, b0, m);
  if constexpr (C::NNET > 1) {
    static_assert(C::K1Q1 == C::K1Q0, "the prior's (x, t, bias) columns are the likelihood's");
    out = out + flow_eval<E, C::K1Q1>(eng, 1, L::L1_1, b0, m);  // prior + likelihood
  }
  flow::gather_score<MODE, D>(out, j, cf, a, dv);
}

// flow_score's network half for a one-network configuration, the output tile itself: rows 4 g + r of net 0 over the
// 16 columns (s_k of the primal columns, ds_k/dx_{m-1} of the tangent columns, at g = 0), for a caller that keeps every
// tangent entry (flow::gather_jac; dmip_dps_linear.hip)
template <typename C, int D, typename Coef>
__device__ __forceinline__ f32x4 flow_out(typename C::E& eng, const int& g, const int& m, const float (&xin)[D],
                                          const Coef& cf) {
  using L = typename C::L;
  using E = typename C::E;
  static_assert(C::NNET == 1, "one network");
  float v[D + 1];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = xin[k];
  v[D] = cf.tau;
  float b0[C::K1Q0];
  l1_operand<D + 1, C::K1Q0>(v, g, b0);
#pragma unroll
  for (int s = 0; s < C::K1Q0; ++s) {
    const float e = (4 * s + g == m - 1 && m - 1 < D) ? 1.0f : 0.0f;
    b0[s] = m == 0 ? b0[s] : e;
  }
  return flow_eval<E, C::K1Q0>(eng, 0, L::L1_0, b0, m);
}

// the flow kernels' set-up: layer-1 images (net 0's is the per-y one) and biases into LDS, ring started
// (f32_flow_kernel calls it; f32_flow_sample_kernel carries the same text, dmip_flow_sample.hip says why)
template <typename C, int W>
__device__ __forceinline__ void flow_setup(typename C::E& eng, char* lds, const F32Net (&net)[2], const float* l1y,
                                           int n_hidden, int yi) {
  using L = typename C::L;
  constexpr int NW = Shape<W>::NW, ST = Shape<W>::ST;
  const int bf = (n_hidden - 1) * W + 16;
  eng.stage(lds + L::L1_0, (const char*)(l1y + (size_t)yi * ST * C::K1Q0 * 64), ST * C::K1Q0 * 256);
  if constexpr (C::NNET > 1) eng.stage(lds + L::L1_1, (const char*)net[1].l1, ST * C::K1Q1 * 256);
  for (int ni = 0; ni < C::NNET; ++ni) {
    float* bl = (float*)(lds + L::BIAS + ni * L::BIAS_BYTES);
    for (int i = threadIdx.x; i < bf; i += NW * 64) bl[i] = net[ni].bias[i];
  }
  eng.start();
}

}  // namespace f32
}  // namespace dmip
