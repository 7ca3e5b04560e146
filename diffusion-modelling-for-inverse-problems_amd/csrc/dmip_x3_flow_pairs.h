// The paired probability-flow kernels on the fp32x3 engine (dmip_pairs.h says what "paired" is): dmip_x3_flow.h's
// network over primal + tangent columns with layer 1's bias taken per row. Siblings of flow_layer1 / flow_eval /
// flow_score and of the two kernels beside them: dmip_x3_flow.h is unchanged.
//
// y never enters the split: row c's bias 2 log2(e) (b1 + W1_y y_c), the f32 value the per-y kernels stage in LDS, is
// the initial value of layer 1's accumulators on the row's primal column -- lane (g, j) holds units 16 o + 4 g + r of
// column j, so one 16-byte load per output tile and lane from cb = row_bias + row W + 4 g, straight into the
// accumulators that are live there anyway. Tangent columns start at zero. Layer 0's LDS bias of net 0 is staged (the
// set-up is flow_setup's, with row 0's bias) and not read. Range handling is the per-y kernels': only (x, tau) is
// checked, a tangent beyond the split shows as a non-finite accumulator.
#pragma once
#include "dmip_pairs.h"
#include "dmip_x3_flow.h"

namespace dmip {
namespace x3 {

// flow_layer1 of net 0 with the accumulators started at the row's bias
template <typename C>
__device__ __forceinline__ void flow_layer1_pairs(typename C::E& eng, int m, const u32x4 (&b1)[C::K1Q],
                                                  u32x4 (&Oh)[C::E::KQ], u32x4 (&Ol)[C::E::KQ], const float* cb) {
  using E = typename C::E;
  constexpr int ST = E::ST, K1Q = C::K1Q;
  asm volatile("" ::: "memory");
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 acc[ST];
#pragma unroll
  for (int o = 0; o < ST; ++o) {
    const f32x4 c4 = *(const f32x4*)(cb + 16 * o);
    acc[o] = m == 0 ? c4 : zero;
  }
  lgkm_drain();
  constexpr int STR = C::L1H ? 512 : 1024;
  const lds_cptr base = (lds_cptr)(eng.lds + eng.l1_off[0] + (C::L1H ? (eng.lane & 31) : eng.lane) * 16);
  constexpr int NU = ST * K1Q;
  u32x4 fa[4];
  fa[0] = lds_rd<0>(base);
  if constexpr (NU > 1) fa[1] = lds_rd<STR>(base);
  if constexpr (NU > 2) fa[2] = lds_rd<2 * STR>(base);
  l1_chain<K1Q, NU, 3, 0, STR>(base, b1, acc, fa);
#pragma unroll
  for (int o = 0; o < ST; ++o) flow_act_store<true, E::KQ>(acc[o], m, o, Oh, Ol);
}

// flow_eval of net 0 through flow_layer1_pairs: the engine's chunk stream, in its order
template <typename C>
__device__ __forceinline__ f32x4 flow_eval_pairs(typename C::E& eng, int m, const u32x4 (&b1)[C::K1Q],
                                                 const float* cb) {
  constexpr int KQ = C::E::KQ;
  static_assert(!C::L1R, "the flow kernels keep layer 1 resident");
  u32x4 Ah[KQ], Al[KQ], Bh[KQ], Bl[KQ];
  flow_layer1_pairs<C>(eng, m, b1, Ah, Al, cb);
  for (int li = 1; li < eng.nl; li += 2) {
    flow_hidden(eng, m, 0, li, Ah, Al, Bh, Bl);
    if (li + 1 < eng.nl) flow_hidden(eng, m, 0, li + 1, Bh, Bl, Ah, Al);
  }
  if (((eng.nl - 1) & 1) != 0) return flow_output(eng, m, 0, Bh, Bl);
  return flow_output(eng, m, 0, Ah, Al);
}

// flow_score with net 0 (the CDE network or the Posterior likelihood) through flow_eval_pairs; the Posterior prior
// takes no y and runs flow_eval as it is. cb: this lane's row bias (row_bias + row W + 4 g)
template <typename C, int MODE, int D, typename Coef>
__device__ __forceinline__ void flow_score_pairs(typename C::E& eng, const int& g, const int& j, const int& m,
                                                 const float (&xin)[D], const Coef& cf, const bool& kept, bool& oor,
                                                 const float* cb, float (&a)[D], float& dv) {
  static_assert(C::K1Q == 1 && C::NV == D + 1, "layer 1 over (x, tau): one k-step");
  float v[D + 1];
#pragma unroll
  for (int k = 0; k < D; ++k) v[k] = xin[k];
  v[D] = cf.tau;
  oor |= kept && out_of_range(v);
  u32x4 b1[1];
  l1_operand<D + 1, 1>(v, g, b1);
  {
    // the tangent column of input n = m - 1: fp16 1.0 at k-slots 3n and 3n + 2 (this lane supplies slots 8 g + e)
    const int n = m - 1;
    f16x8 u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int s = 8 * g + e;
      u[e] = (n < D && (s == 3 * n || s == 3 * n + 2)) ? (_Float16)1.0f : (_Float16)0.0f;
    }
    const u32x4 ub = __builtin_bit_cast(u32x4, u);
#pragma unroll
    for (int e = 0; e < 4; ++e) b1[0][e] = m == 0 ? b1[0][e] : ub[e];
  }
  f32x4 out = flow_eval_pairs<C>(eng, m, b1, cb);
  if constexpr (C::NNET > 1) out = out + flow_eval<C>(eng, m, 1, b1);  // likelihood + prior
  flow::gather_score<MODE, D>(out, j, cf, a, dv);
}

// paired log p(x_i | y_i): x3_flow_kernel over a (g, 1) grid at y index 0
template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, Shape<W>::NW / 4) x3_flow_pairs_kernel(X3FlowPairsParams pp) {
  using C = SamplerCfg<MODE, W, D, 0, 0>;
  using L = typename C::L;
  using E = typename C::E;
  static_assert(L::TOTAL <= kLdsBudget, "LDS budget");
  static_assert(D <= 3, "a quad holds the primal and at most 3 tangents");
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const X3FlowParams& p = pp.x;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15, m = lane & 3;

  E eng{lds, {p.net[0].stream, p.net[1].stream}, {L::L1, L::L1 + L::L1_BYTES}, {L::BIAS, L::BIAS + L::BIAS_BYTES}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<Shape<W>::NW> rows(p.rows.n, w, g, j, m);
  flow_setup<C, W>(eng, lds, p.net, p.bias_y, p.n_hidden, 0);

  bool oor = false;
  flow::logp_rows<D>(p.rows, rows, 0, oor,
                     [&](const float (&xt)[D], const flow::FlowCoef& cf, float (&a)[D], float& dv)
                         __attribute__((always_inline)) {
                           flow_score_pairs<C, MODE, D>(eng, g, j, m, xt, cf, rows.valid, oor,
                                                        pp.row_bias + rows.rr * W + 4 * g, a, dv);
                         });
  eng.finish();
  report_range(oor, p.err, lane);
}

// paired samples with their log-density: x3_flow_sample_kernel over a (g, 1) grid at y index 0 (row i's stream is
// (seed, chain_offset + i, 0))
template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, Shape<W>::NW / 4)
    x3_flow_sample_pairs_kernel(X3FlowSamplePairsParams pp) {
  using C = SamplerCfg<MODE, W, D, 0, 0>;
  using L = typename C::L;
  using E = typename C::E;
  static_assert(L::TOTAL <= kLdsBudget, "LDS budget");
  static_assert(D <= 3, "a quad holds the primal and at most 3 tangents");
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const X3FlowSampleParams& p = pp.x;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15, m = lane & 3;

  E eng{lds, {p.net[0].stream, p.net[1].stream}, {L::L1, L::L1 + L::L1_BYTES}, {L::BIAS, L::BIAS + L::BIAS_BYTES}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<Shape<W>::NW> rows(p.chains.n, w, g, j, m);
  flow_setup<C, W>(eng, lds, p.net, p.bias_y, p.n_hidden, 0);

  bool oor = false;
  flow::sample_rows<D>(p.chains, rows, 0, oor,
                       [&](const float (&xt)[D], const StepCoef& c, float (&a)[D], float& dv)
                           __attribute__((always_inline)) {
                             flow_score_pairs<C, MODE, D>(eng, g, j, m, xt, c, rows.valid, oor,
                                                          pp.row_bias + rows.rr * W + 4 * g, a, dv);
                           });
  eng.finish();
  report_range(oor, p.err, lane);
}

}  // namespace x3
}  // namespace dmip
