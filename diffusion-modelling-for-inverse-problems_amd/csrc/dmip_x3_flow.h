// The probability-flow kernels with an exact divergence on the fp32x3 engine (dmip_x3.h XEngine): log p(x | y) of given
// rows (x3_flow_kernel, the scheme of dmip_flow.hip) and samples with their log-density (x3_flow_sample_kernel, the
// scheme of dmip_flow_sample.hip). Free functions beside the engine: dmip_x3.h is unchanged.
//
// Columns are dmip_flow.h's: the 16-column B operand of a wave holds 4 rows x (primal + 3 tangents), column
// j = 4 c + m with m = 0 the primal of row c and m = 1..3 the tangent along x_{m-1}; for xdim = 2 the fourth column of
// a quad computes on zeros. An MFMA column does not depend on its neighbours, so a primal column is the sampler's
// chain bit for bit.
//
// Tangents in r-form. The engine carries r = 1 / (1 + 2^zs) = (1 - tanh z) / 2 with zs = c z, c = 2 log2(e), and the
// host folds h = 1 - 2 r into the next layer (pack_x3_net: A = s (-2 W), init = s b - 1/2 sum A, with s = c for a
// hidden layer and s = 1 for the output rows). Every layer after the first is therefore affine in r, and a tangent
// column carries dr through the same images with a zero accumulator init:
//   layer 1   the B operand of input n = m - 1 is the unit vector: k-slots 3n and 3n + 2 hold fp16 1.0, slot 3n + 1
//             holds 0; against A = [W_hi, W_hi, W_lo] of c W1 that is dzs = c W1[:, n] (hi + lo)
//             dr1 = -ln2 r1 (1 - r1) dzs, u = c (1 - 2 r1), dr2 = -ln2 r2 (1 - r2) (-2 c dr1)
//   hidden    dzs = A dr (no init), dr = -ln2 r (1 - r) dzs
//   output    A = -2 Wo at scale 1: A dr = Wo dh = da_i/dx_n, with no further factor
// r of the primal is re-activated from the quad's primal pre-activation (one DPP move), as dmip_flow.h's flow_act; dr
// is split into (hi, lo) fp16 like any activation.
#pragma once
#include "dmip_flow_rows.h"
#include "dmip_x3.h"

namespace dmip {
namespace x3 {

constexpr float kLn2 = 0.69314718055994531f;

using flow::quad_primal;

// activate tile o into the (hi, lo) B operands of the next layer: primal columns r (XEngine::act_store's values),
// tangent columns dr
template <bool L1, int KQ>
__device__ __forceinline__ void flow_act_store(const f32x4& z, int m, int o, u32x4 (&Oh)[KQ], u32x4 (&Ol)[KQ]) {
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float r1 = x3_act_r(quad_primal(z[k]));
    float val = r1, d = -kLn2 * (r1 * (1.0f - r1));
    if constexpr (L1) {
      const float r2 = x3_act_r(__builtin_fmaf(-2.0f * kTanhScale, r1, kTanhScale));  // x3_act_r2
      val = r2;
      d = (-kLn2 * (r2 * (1.0f - r2))) * ((-2.0f * kTanhScale) * d);
    }
    r[k] = m == 0 ? val : d * z[k];
  }
  uint32_t h0, l0, h1, l1;
  split_pair(r[0], r[1], h0, l0);
  split_pair(r[2], r[3], h1, l1);
  const int q = o >> 1, e = (o & 1) * 2;
  Oh[q][e] = h0, Oh[q][e + 1] = h1;
  Ol[q][e] = l0, Ol[q][e + 1] = l1;
}

// accumulator init of a tile: the engine's bias on primal columns, zero on tangent columns
template <typename E>
__device__ __forceinline__ f32x4 flow_bias4(const E& eng, int m, int ni, int li, int tile) {
  const f32x4 b = eng.bias4(ni, li, tile);
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  return m == 0 ? b : zero;
}

// XEngine::layer1 over the flow columns (C: the SamplerCfg; its layer 1 is resident)
template <typename C>
__device__ __forceinline__ void flow_layer1(typename C::E& eng, int m, int ni, const u32x4 (&b1)[C::K1Q],
                                            u32x4 (&Oh)[C::E::KQ], u32x4 (&Ol)[C::E::KQ]) {
  using E = typename C::E;
  constexpr int ST = E::ST, K1Q = C::K1Q;
  asm volatile("" ::: "memory");
  f32x4 acc[ST];
#pragma unroll
  for (int o = 0; o < ST; ++o) acc[o] = flow_bias4(eng, m, ni, 0, o);
  lgkm_drain();
  constexpr int STR = C::L1H ? 512 : 1024;
  const lds_cptr base = (lds_cptr)(eng.lds + eng.l1_off[ni] + (C::L1H ? (eng.lane & 31) : eng.lane) * 16);
  constexpr int NU = ST * K1Q;
  u32x4 fa[4];
  fa[0] = lds_rd<0>(base);
  if constexpr (NU > 1) fa[1] = lds_rd<STR>(base);
  if constexpr (NU > 2) fa[2] = lds_rd<2 * STR>(base);
  l1_chain<K1Q, NU, 3, 0, STR>(base, b1, acc, fa);
#pragma unroll
  for (int o = 0; o < ST; ++o) flow_act_store<true, E::KQ>(acc[o], m, o, Oh, Ol);
}

// XEngine::hidden over the flow columns
template <typename E>
__device__ __forceinline__ void flow_hidden(E& eng, int m, int ni, int li, const u32x4 (&Hh)[E::KQ],
                                            const u32x4 (&Hl)[E::KQ], u32x4 (&Oh)[E::KQ], u32x4 (&Ol)[E::KQ]) {
  constexpr int CT = E::CT, NCH = E::NCH, KQ = E::KQ;
  f32x4 pend[CT];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    f32x4 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = flow_bias4(eng, m, ni, li, c * CT + t);
    lgkm_drain();
    if constexpr (E::SPREAD) {
      const char* ch = eng.chunk_sync_deferred();
      split_product_h<KQ, CT * KQ, 2>((lds_cptr)(ch + eng.lane * 16), Hh, Hl, acc, typename E::SpreadPieces{&eng});
    } else {
      const char* ch = eng.chunk_sync();
      split_product<KQ, CT * KQ, 2>((lds_cptr)(ch + eng.lane * 16), Hh, Hl, acc);
    }
    // the previous chunk's tiles are activated beside this chunk's MFMAs
    if (c > 0) {
#pragma unroll
      for (int t = 0; t < CT; ++t) flow_act_store<false, KQ>(pend[t], m, (c - 1) * CT + t, Oh, Ol);
    }
#pragma unroll
    for (int t = 0; t < CT; ++t) pend[t] = acc[t];
  }
#pragma unroll
  for (int t = 0; t < CT; ++t) flow_act_store<false, KQ>(pend[t], m, (NCH - 1) * CT + t, Oh, Ol);
}

// XEngine::output over the flow columns: rows 0..15; a_i on the primal columns, da_i/dx_{m-1} on the tangent columns
template <typename E>
__device__ __forceinline__ f32x4 flow_output(E& eng, int m, int ni, const u32x4 (&Hh)[E::KQ],
                                             const u32x4 (&Hl)[E::KQ]) {
  constexpr int KQ = E::KQ;
  f32x4 acc[1] = {flow_bias4(eng, m, ni, eng.nl, 0)};
  lgkm_drain();
  if constexpr (E::SPREAD) {
    const char* ch = eng.chunk_sync_deferred();
    split_product_h<KQ, KQ, 2>((lds_cptr)(ch + eng.lane * 16), Hh, Hl, acc, typename E::SpreadPieces{&eng});
  } else {
    const char* ch = eng.chunk_sync();
    split_product<KQ, KQ, 2>((lds_cptr)(ch + eng.lane * 16), Hh, Hl, acc);
  }
  return acc[0];
}

// XEngine::eval over the flow columns: the engine's chunk stream, in its order
template <typename C>
__device__ __forceinline__ f32x4 flow_eval(typename C::E& eng, int m, int ni, const u32x4 (&b1)[C::K1Q]) {
  constexpr int KQ = C::E::KQ;
  static_assert(!C::L1R, "the flow kernels keep layer 1 resident");
  u32x4 Ah[KQ], Al[KQ], Bh[KQ], Bl[KQ];
  flow_layer1<C>(eng, m, ni, b1, Ah, Al);
  for (int li = 1; li < eng.nl; li += 2) {
    flow_hidden(eng, m, ni, li, Ah, Al, Bh, Bl);
    if (li + 1 < eng.nl) flow_hidden(eng, m, ni, li + 1, Bh, Bl, Ah, Al);
  }
  if (((eng.nl - 1) & 1) != 0) return flow_output(eng, m, ni, Bh, Bl);
  return flow_output(eng, m, ni, Ah, Al);
}

// a(x, y, tau) of the row on all its lanes, and sum_i da_i/dx_i (the tangent column 1 + i carries row i's
// derivative): dmip_flow.h's flow_score on this engine. lane = 16 g + j, m = lane & 3; cf: the stage's coefficients
// (.tau, and .g: the Posterior estimator's factor on a and on its divergence, nets.py:155-157). `oor`: a layer-1
// input of a kept row outside the split's range (x3::out_of_range). Always inlined, every argument by reference.
template <typename C, int MODE, int D, typename Coef>
__device__ __forceinline__ void flow_score(typename C::E& eng, const int& g, const int& j, const int& m,
                                           const float (&xin)[D], const Coef& cf, const bool& kept, bool& oor,
                                           float (&a)[D], float& dv) {
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
  f32x4 out = flow_eval<C>(eng, m, 0, b1);
  if constexpr (C::NNET > 1) out = out + flow_eval<C>(eng, m, 1, b1);  // likelihood + prior
  flow::gather_score<MODE, D>(out, j, cf, a, dv);
}

// flow_score's network half for a one-network configuration, the output tile itself: rows 0..15 of net 0 over the 16
// columns (s_k of the primal columns, ds_k/dx_{m-1} of the tangent columns), for a caller that keeps every tangent
// entry (flow::gather_jac; dmip_x3_dps_linear.hip). `kept`, `oor` as flow_score's
template <typename C, int D, typename Coef>
__device__ __forceinline__ f32x4 flow_out(typename C::E& eng, const int& g, const int& m, const float (&xin)[D],
                                          const Coef& cf, const bool& kept, bool& oor) {
  static_assert(C::K1Q == 1 && C::NV == D + 1 && C::NNET == 1, "one network, layer 1 over (x, tau): one k-step");
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
  return flow_eval<C>(eng, m, 0, b1);
}

// the sampler kernel's set-up: layer-1 images and biases into LDS (net 0's layer-1 bias is the per-y one), ring started
template <typename C, int W>
__device__ __forceinline__ void flow_setup(typename C::E& eng, char* lds, const X3Net (&net)[2], const float* bias_y,
                                           int n_hidden, int yi) {
  using L = typename C::L;
  constexpr int NW = Shape<W>::NW;
  const int bf = n_hidden * W + 16;
  for (int ni = 0; ni < C::NNET; ++ni) {
    if constexpr (C::L1H) {  // lanes 0-31 of each tile's 1 KiB ([tile][64 lanes][16 B] -> [tile][32][16 B])
      const uint4* s1 = (const uint4*)net[ni].l1;
      uint4* d1 = (uint4*)(lds + L::L1 + ni * L::L1_BYTES);
      for (int e = threadIdx.x; e < L::L1_BYTES / 16; e += NW * 64) d1[e] = s1[(e >> 5) * 64 + (e & 31)];
    } else {
      eng.stage(lds + L::L1 + ni * L::L1_BYTES, net[ni].l1, L::L1_BYTES);
    }
    float* bl = (float*)(lds + L::BIAS + ni * L::BIAS_BYTES);
    for (int i = threadIdx.x; i < bf; i += NW * 64)
      bl[i] = (ni == 0 && i < W) ? bias_y[(size_t)yi * W + i] : net[ni].bias[i];
  }
  eng.start();
}

// log p(x | y): dmip_flow_rows.h's logp_rows (dmip_flow.hip's scheme) over this engine's flow_score. `oor` collects a
// kept row's layer-1 input outside the split's range and a tangent beyond it (a non-finite accumulator)
template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, Shape<W>::NW / 4) x3_flow_kernel(X3FlowParams p) {
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

  E eng{lds, {p.net[0].stream, p.net[1].stream}, {L::L1, L::L1 + L::L1_BYTES}, {L::BIAS, L::BIAS + L::BIAS_BYTES}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<Shape<W>::NW> rows(p.rows.n, w, g, j, m);
  flow_setup<C, W>(eng, lds, p.net, p.bias_y, p.n_hidden, yi);

  bool oor = false;
  flow::logp_rows<D>(p.rows, rows, yi, oor,
                     [&](const float (&xt)[D], const flow::FlowCoef& cf, float (&a)[D], float& dv)
                         __attribute__((always_inline)) {
                           flow_score<C, MODE, D>(eng, g, j, m, xt, cf, rows.valid, oor, a, dv);
                         });
  eng.finish();
  report_range(oor, p.err, lane);
}

// samples with their log-density: dmip_flow_rows.h's sample_rows (dmip_flow_sample.hip's scheme); `oor` as above
template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, Shape<W>::NW / 4) x3_flow_sample_kernel(X3FlowSampleParams p) {
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

  E eng{lds, {p.net[0].stream, p.net[1].stream}, {L::L1, L::L1 + L::L1_BYTES}, {L::BIAS, L::BIAS + L::BIAS_BYTES}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<Shape<W>::NW> rows(p.chains.n, w, g, j, m);
  flow_setup<C, W>(eng, lds, p.net, p.bias_y, p.n_hidden, yi);

  bool oor = false;
  flow::sample_rows<D>(p.chains, rows, yi, oor,
                       [&](const float (&xt)[D], const StepCoef& c, float (&a)[D], float& dv)
                           __attribute__((always_inline)) {
                             flow_score<C, MODE, D>(eng, g, j, m, xt, c, rows.valid, oor, a, dv);
                           });
  eng.finish();
  report_range(oor, p.err, lane);
}

}  // namespace x3

// per-mode instantiations (dmip_x3_flow_{cde,post}.hip, dmip_x3_flow_sample_{cde,post}.hip)
hipError_t launch_x3_flow_cde(const X3FlowParams& p, int width, int xdim, int n_y, hipStream_t st, bool* ok);
hipError_t launch_x3_flow_post(const X3FlowParams& p, int width, int xdim, int n_y, hipStream_t st, bool* ok);
hipError_t launch_x3_flow_sample_cde(const X3FlowSampleParams& p, int width, int xdim, int n_y, hipStream_t st,
                                     bool* ok);
hipError_t launch_x3_flow_sample_post(const X3FlowSampleParams& p, int width, int xdim, int n_y, hipStream_t st,
                                      bool* ok);

}  // namespace dmip
