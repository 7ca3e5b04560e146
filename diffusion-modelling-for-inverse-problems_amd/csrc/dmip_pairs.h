// The paired probability-flow kernels: one observation per row. Row i of a call has its own y_i, which enters the
// network only through layer 1's c_i = b1 + W1_y y_i (W floats, constant over the steps). The host forms c for a slab
// of rows once (f64 accumulation, one rounding; the fp32x3 engine's scaled by 2 log2 e as its per-y bias is) into a
// stream-ordered scratch [rows][W]; the kernels run the per-y kernels' row drivers (dmip_flow_rows.h) over a (g, 1)
// grid with y index 0 and take c_i as the initial value of layer 1's accumulator on row i's primal column.
// What the host layer and the kernels share; device code: dmip_flow_pairs.h (exact f32), dmip_x3_flow_pairs.h (fp32x3).
#pragma once
#include "dmip_internal.h"

namespace dmip {

// 2 log2(e): dmip_device.h's kTanhScale for the host layer, which does not include device headers (dmip_flow_pairs.hip
// asserts the two equal)
constexpr float kPairsTanhScale = 2.8853900817779268f;

// the per-y kernels' parameters with n_y = 1, plus the rows' layer-1 bias. f.l1y: ONE layer-1 image over (x, t) with
// the bias column zero (pairs_prep_kernel); x.bias_y: any [W] floats (layer 0's LDS bias of net 0 is not read)
struct F32FlowPairsParams {
  F32FlowParams f;
  const float* row_bias;  // [rows.n][W] c_i
};
struct F32FlowSamplePairsParams {
  F32FlowSampleParams f;
  const float* row_bias;  // [chains.n][W] c_i
};
struct X3FlowPairsParams {
  X3FlowParams x;
  const float* row_bias;  // [rows.n][W] 2 log2(e) c_i
};
struct X3FlowSamplePairsParams {
  X3FlowSampleParams x;
  const float* row_bias;
};

// c for rows [0, n): out[i][u] = (float)(scale (b1_u + W1_{u,y} . y_i)) in f64 (x3_bias_prep_kernel's expression; a
// flat grid, so n is not bound by a grid dimension). l1: the exact-f32 engine's shared image, or null
struct PairsPrepParams {
  const float* w1;  // [width][in_dim] (nn.Linear layout)
  const float* b1;
  const float* y;   // [n][ydim]
  float* out;       // [n][width]
  float* l1;        // out: [width/16][k1q][64] over (x, t), bias column zero; or null
  long long n;
  int width, in_dim, xdim, ydim, k1q;
  double scale;
};
hipError_t launch_pairs_prep(const PairsPrepParams& p, hipStream_t st);

// compiled: every shape of the per-y kernels (f32_flow_supported / x3_flow_supported)
hipError_t launch_f32_flow_pairs(const F32FlowPairsParams& p, int mode, int width, int n_hidden, int xdim, int ydim,
                                 hipStream_t st, bool* supported);
hipError_t launch_f32_flow_sample_pairs(const F32FlowSamplePairsParams& p, int mode, int width, int n_hidden, int xdim,
                                        int ydim, hipStream_t st, bool* supported);
hipError_t launch_x3_flow_pairs(const X3FlowPairsParams& p, int mode, int width, int n_hidden, int xdim, int ydim,
                                hipStream_t st, bool* supported);
hipError_t launch_x3_flow_sample_pairs(const X3FlowSamplePairsParams& p, int mode, int width, int n_hidden, int xdim,
                                       int ydim, hipStream_t st, bool* supported);
// per-mode instantiations (dmip_x3_flow_pairs_{cde,post}.hip, dmip_x3_flow_sample_pairs_{cde,post}.hip)
hipError_t launch_x3_flow_pairs_cde(const X3FlowPairsParams& p, int width, int xdim, hipStream_t st, bool* ok);
hipError_t launch_x3_flow_pairs_post(const X3FlowPairsParams& p, int width, int xdim, hipStream_t st, bool* ok);
hipError_t launch_x3_flow_sample_pairs_cde(const X3FlowSamplePairsParams& p, int width, int xdim, hipStream_t st,
                                           bool* ok);
hipError_t launch_x3_flow_sample_pairs_post(const X3FlowSamplePairsParams& p, int width, int xdim, hipStream_t st,
                                            bool* ok);

}  // namespace dmip
