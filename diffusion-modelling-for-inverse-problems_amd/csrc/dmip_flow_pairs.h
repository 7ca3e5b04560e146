// The paired probability-flow kernels on the exact-f32 engine (dmip_pairs.h says what "paired" is): dmip_flow.h's
// network over primal + tangent columns with layer 1's bias taken per row. Siblings of flow_eval / flow_score beside
// them: dmip_flow.h is unchanged.
//
// The shared layer-1 image carries (x, t) and a zero bias column, so the bias slot of the B operand (1.0 on a primal
// column) contributes an exact zero. Row c's bias enters as the accumulator's initial value on its primal column:
// lane (g, j) holds units 16 o + 4 g + r of column j, so one 16-byte load per output tile and lane, from
// cb = row_bias + row W + 4 g. Tangent columns start at zero, as in dmip_flow.h. The loads go through the vector memory
// counter beside the ring's LDS-DMA pieces; memory operations return in order, so a load among them can only make the
// ring's counted waits wait for more, never for less.
#pragma once
#include "dmip_flow.h"
#include "dmip_pairs.h"

namespace dmip {
namespace f32 {

// flow_eval with layer 1's accumulators started at the row's bias (primal columns) instead of zero
template <typename E, int K1Q>
__device__ __forceinline__ f32x4 flow_eval_pairs(E& eng, int ni, int l1_off, const float (&b)[K1Q], int m,
                                                 const float* cb) {
  constexpr int ST = E::ST;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  float Ha[ST][4], Hb[ST][4];
  asm volatile("" ::: "memory");
  const float* l1 = (const float*)(eng.lds + l1_off);
#pragma unroll
  for (int o = 0; o < ST; ++o) {
    const f32x4 c4 = *(const f32x4*)(cb + 16 * o);
    f32x4 z = m == 0 ? c4 : zero;
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

// flow_score with net 0 (the CDE network or the Posterior likelihood) through flow_eval_pairs; the Posterior prior
// takes no y and runs flow_eval as it is. cb: this lane's row bias (row_bias + row W + 4 g)
template <typename C, int MODE, int D, typename Coef>
__device__ __forceinline__ void flow_score_pairs(typename C::E& eng, const int& g, const int& j, const int& m,
                                                 const float (&xin)[D], const Coef& cf, const float* cb,
                                                 float (&a)[D], float& dv) {
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
  f32x4 out = flow_eval_pairs<E, C::K1Q0>(eng, 0, L::L1_0, b0, m, cb);
  if constexpr (C::NNET > 1) {
    static_assert(C::K1Q1 == C::K1Q0, "the prior's (x, t, bias) columns are the likelihood's");
    out = out + flow_eval<E, C::K1Q1>(eng, 1, L::L1_1, b0, m);  // prior + likelihood
  }
  flow::gather_score<MODE, D>(out, j, cf, a, dv);
}

}  // namespace f32
}  // namespace dmip
