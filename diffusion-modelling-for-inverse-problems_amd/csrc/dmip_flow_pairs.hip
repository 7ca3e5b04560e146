// Paired log p(x_i | y_i), one observation per row, in exact f32: dmip_flow.hip's kernel over a (g, 1) grid with the
// rows' own layer-1 bias (dmip_flow_pairs.h). The integrator is dmip_flow_rows.h's logp_rows at y index 0, so the rows
// of flow::Rows run over all pairs. Also here: the prep kernel both engines' paired launches share.
#include "dmip_flow_pairs.h"

namespace dmip {
static_assert(kPairsTanhScale == kTanhScale, "the host layer's name of kTanhScale");

// c_i for a slab of rows, and (l1 non-null) the exact-f32 engine's shared layer-1 image: f32_l1_prep_kernel's with
// the bias column zero. One thread per (row, hidden unit); the image is written by the threads of row 0
__global__ void pairs_prep_kernel(PairsPrepParams p) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.n * p.width) return;
  const long long row = e / p.width;
  const int u = (int)(e - row * p.width);
  const float* wrow = p.w1 + (size_t)u * p.in_dim;
  double c = p.b1[u];
  for (int m = 0; m < p.ydim; ++m) c += (double)wrow[p.xdim + m] * (double)p.y[(size_t)row * p.ydim + m];
  p.out[(size_t)row * p.width + u] = (float)(p.scale * c);
  if (p.l1 && row == 0) {
    const int o = u / 16, i = u % 16;
    for (int s = 0; s < p.k1q; ++s)
      for (int gg = 0; gg < 4; ++gg) {
        const int col = 4 * s + gg;
        float val = 0.0f;
        if (col < p.xdim) val = wrow[col];
        else if (col == p.xdim) val = wrow[p.in_dim - 1];  // t
        p.l1[((size_t)o * p.k1q + s) * 64 + i + 16 * gg] = val;
      }
  }
}

hipError_t launch_pairs_prep(const PairsPrepParams& p, hipStream_t st) {
  const long long blocks = (p.n * p.width + 255) / 256;
  hipLaunchKernelGGL(pairs_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p);
  return hipGetLastError();
}

namespace f32 {

template <int MODE, int W, int D>
__global__ void __launch_bounds__(Shape<W>::NW * 64, 1) f32_flow_pairs_kernel(F32FlowPairsParams pp) {
  using C = SamplerCfg<MODE, W, D, 0, 0>;
  using L = typename C::L;
  using E = typename C::E;
  static_assert(L::TOTAL <= kLdsBudget, "LDS budget");
  static_assert(D <= 3, "a quad holds the primal and at most 3 tangents");
  __shared__ __attribute__((aligned(16))) char lds[L::TOTAL];
  const F32FlowParams& p = pp.f;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15, m = lane & 3;

  E eng{lds, {p.net[0].stream, p.net[1].stream}, {L::BIAS, L::BIAS + L::BIAS_BYTES}};
  eng.w = w, eng.lane = lane, eng.g = g;
  eng.init(p.n_hidden);
  flow::Rows<Shape<W>::NW> rows(p.rows.n, w, g, j, m);
  flow_setup<C, W>(eng, lds, p.net, p.l1y, p.n_hidden, 0);  // the one shared image

  bool nonfinite = false;  // exact f32 has no range to leave: not reported
  flow::logp_rows<D>(p.rows, rows, 0, nonfinite,
                     [&](const float (&xt)[D], const flow::FlowCoef& cf, float (&a)[D], float& dv)
                         __attribute__((always_inline)) {
        // the row's bias address (dmip_flow_pairs.h) is formed here, at each evaluation, from the row index the
        // driver keeps anyway: a pointer held across the layers cost the W >= 256 kernels more scratch
        unsigned r = (unsigned)rows.row;
        asm volatile("" : "+v"(r));
        const float* cb = pp.row_bias + ((rows.valid ? r : 0u) * (unsigned)W + 4u * (unsigned)g);
        flow_score_pairs<C, MODE, D>(eng, g, j, m, xt, cf, cb, a, dv);
      });
  eng.finish();
}

}  // namespace f32

hipError_t launch_f32_flow_pairs(const F32FlowPairsParams& p, int mode, int width, int n_hidden, int xdim, int ydim,
                                 hipStream_t st, bool* supported) {
  *supported = false;
  if (!f32_flow_supported(mode, width, n_hidden, xdim, ydim)) return hipSuccess;
  *supported = true;
#define X(Wv, Dv)                                                                                        \
  if (width == Wv && xdim == Dv)                                                                         \
    return flow_launch(mode == SAMPLER_CDE ? f32::f32_flow_pairs_kernel<SAMPLER_CDE, Wv, Dv>             \
                                           : f32::f32_flow_pairs_kernel<SAMPLER_POSTERIOR, Wv, Dv>,      \
                       f32::Shape<Wv>::NW, p, p.f.rows.n, 1, st);
  DMIP_FLOW_SHAPES(X)
#undef X
  *supported = false;
  return hipSuccess;
}

}  // namespace dmip
