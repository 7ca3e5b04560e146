// Shared by the C-ABI sources (dmip_capi_pack.cpp, dmip_capi_sample.cpp, dmip_capi_flow.cpp, dmip_capi_dps_linear.cpp,
// dmip_capi_train.cpp): error reporting, the handle structs behind include/dmip.h's opaque types, and the helpers more
// than one of them uses (the schedule, the networks' check, the per-y layer-1 preps, the fp32x3 range refusal, the
// device status word). Host code only; no kernel includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dmip.h"
#include "dmip_internal.h"
#include "dmip_pack.h"

// A device buffer a handle owns: freed with the handle, read as a plain pointer
struct DevMem {
  void* ptr = nullptr;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() {
    if (ptr) (void)hipFree(ptr);
  }
};
template <typename T>
struct DevBuf : DevMem {
  operator T*() const { return (T*)ptr; }
};

// Every device buffer is the upload of the image of the same name in dmip_pack.h (dmip_mlp_create)
struct dmip_mlp {
  int in_dim = 0, out_dim = 0, n_hidden = 0, width = 0, act_mode = 0, layout = 0, xdim = 0;
  int k1s_full = 0;
  DevBuf<char> hidden;          // [(L-1)][W/32][W/16] KiB | ao_samp
  DevBuf<char> ao_samp;         // [W/16] KiB, output rows duplicated into lanes 32-63
  DevBuf<char> ao_full;         // [W/16] KiB, natural output rows
  DevBuf<float> bias_hidden;    // [(L-1)][W/32][2][16]
  DevBuf<float> bias_out_samp;  // [2][16]
  DevBuf<float> bias_out_full;  // [2][16]
  DevBuf<char> a1_full;         // [W/32][k1s_full] KiB (every input column varying)
  DevBuf<char> ring_l1;         // width 512: [layer-1 chunks (split image) | hidden | output] (CDiffE sampler)
  DevBuf<float> w1, b1;         // layer-1 fp32 [W][in_dim], [W] (per-y prep of the sampler's A1)
  // exact-f32 images of a DPS prior (MLP2 (x, t), x 3, widths [256]*3): dmip_dps_sample
  DevBuf<float> dps_l1;         // [16 tiles][2 k-steps][64]
  DevBuf<char> dps_w2, dps_w3;  // [16][16][64][4]
  DevBuf<char> dps_w4;          // [1][16][64][4], rows >= 3 zero
  DevBuf<float> dps_bias;       // b2 | b3 | b4[16]
  // fp32x3 images of a DPS prior (dmip_dps_x3.hip): the chunk stream, layer 1, the biases; none when a weight is
  // beyond fp16's range (dps_x3_range: that magnitude)
  DevBuf<char> dps_x3_img;      // [kDpsX3PriorChunks][32 KiB]
  DevBuf<char> dps_x3_l1;       // [16 tiles][64][8] fp16, scaled by 2 log2 e
  DevBuf<float> dps_x3_bias;    // c b1 | init2 | init3 [256] | out init [16]
  double dps_x3_range = 0.0;
  // exact-f32 images (DMIP_PREC_F32, dmip_f32.h): every input column + bias as layer 1
  DevBuf<float> f32_l1;         // [W/16][k1q][64]
  DevBuf<char> f32_stream;      // [(L-1) W/16 + f32_ot chunks][W/16][64][4]
  DevBuf<float> f32_bias;       // [(L-1)][W] | [16 f32_ot]
  int f32_k1q = 0, f32_ot = 0;
  // fp32-accurate split-fp16 images (DMIP_PREC_F32X3, dmip_x3.h); none when a scaled weight or folded bias
  // is outside fp16's range (x3_range: that magnitude, reported by em_sample_x3)
  double x3_range = 0.0;
  DevBuf<char> x3_l1;           // [W/16][K1Q][64][8] fp16 over (x, t)
  DevBuf<char> x3_l1_full;      // the same over every input column (X_Y_T networks: CDiffE)
  DevBuf<char> x3_stream;       // hidden chunks | output chunk
  DevBuf<char> x3_stream_l1r;   // CDiffE at width 512: layer-1 chunks ([K1Q][W/16 tiles][64][8]) | x3_stream
  DevBuf<float> x3_bias;        // [L W + 16]
  // the k-major engine's images (dmip_x3k.h; width 256, 3 hidden layers, xdim <= 4)
  DevBuf<char> x3k_stream;      // [2 layers][8 k-steps][16 tiles][hi, lo][64][8] fp16
  DevBuf<char> x3k_out;         // [8 k-steps][64][8]: rows 0..xdim-1 W_hi, rows 4..4+xdim-1 W_lo
  // the paired-tile 32x32 engine's images (dmip_x3p.h; same shapes)
  DevBuf<char> x3p_stream;      // [16 chunks][32 KiB]
  DevBuf<char> x3p_l1;          // [8 layer-1 tiles][64][8] | [2 hidden layers][8 bias tiles][64][8] fp16
  DevBuf<float> x3p_ow;         // f32 output rows [8][2][4][4][4] | init[16]
};

// the scatterometry surrogate
struct dmip_surrogate {
  DevBuf<float> l1, bias;
  DevBuf<char> img[7];  // w2, w3, w4, w3t, w2t, w4t, w1t
  // fp32x3 images (dmip_dps_x3.hip): chunks S2 | S3 | Sout | S4^T | S3^T | S2^T | S1^T, layer 1, biases; none when
  // a weight is beyond fp16's range (x3_range)
  DevBuf<char> x3_img, x3_l1;
  DevBuf<float> x3_bias;  // b1 | b2 | b3 [256] | b4 [32]
  double x3_range = 0.0;
};

namespace dmip_capi {

// dmip_last_error's text and the per-device status words: defined in dmip_capi_pack.cpp
extern thread_local std::string g_err;
unsigned* status_word(int dev);

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

inline int hip_fail(hipError_t e, const char* what) {
  return fail(DMIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

using dmip_pack::k1s_for;

// Scratch of one launch sequence, allocated on its stream and freed on it when the owner leaves scope: the free is
// enqueued behind whatever the entry point launched, on every return path.
struct StreamScratch {
  void* ptr = nullptr;
  hipStream_t st = nullptr;
  StreamScratch() = default;
  StreamScratch(const StreamScratch&) = delete;
  StreamScratch& operator=(const StreamScratch&) = delete;
  ~StreamScratch() {
    if (ptr) (void)hipFreeAsync(ptr, st);
  }
  int alloc(size_t bytes, hipStream_t stream) {
    st = stream;
    const hipError_t e = hipMallocAsync(&ptr, bytes, st);
    if (e == hipSuccess) return DMIP_OK;
    ptr = nullptr;
    return fail(DMIP_ERR_ALLOC, std::string("hipMallocAsync: ") + hipGetErrorString(e));
  }
};

inline dmip::F32Net f32_net(const dmip_mlp* n) { return dmip::F32Net{n->f32_l1, n->f32_stream, n->f32_bias}; }
// the fp32x3 images over (x, t) (a CDiffE launch swaps in the full layer-1 image: em_sample_x3)
inline dmip::X3Net x3_net(const dmip_mlp* n) { return dmip::X3Net{n->x3_l1, n->x3_stream, n->x3_bias}; }

// the device status word of the stream's device into a kernel's `err` field
inline int status_word_or_fail(unsigned*& err, hipStream_t st) {
  err = status_word(dmip::stream_device(st));
  return err ? DMIP_OK : fail(DMIP_ERR_ALLOC, "device status word");
}

// the activation chain's code in the exact-f32 kernels (dmip_f32.h act_f32): 0 tanh, 1 SiLU. Only the exact-f32
// forward and the exact-f32 CDE sampler compile the SiLU chain; every other kernel computes tanh.
inline int f32_act(const dmip_mlp* n) { return n->act_mode == DMIP_ACT_SILU_TWICE_FIRST ? 1 : 0; }

inline int act_refused(const char* what) {
  return fail(DMIP_ERR_UNSUPPORTED, std::string(what) +
                                        ": the SiLU chain is compiled for the exact-f32 forward and the exact-f32 "
                                        "CDE sampler only (DMIP_PREC_F32)");
}

// the VP-SDE schedule of a launch: each value evaluated in double and rounded once to the kernels' f32.
// `step` is T / num_steps (the samplers' delta, the flow's h); `sqrt_step` where the kernel takes it
inline void fill_schedule(const dmip_vpsde& sde, int num_steps, float& T, float& bmin, float& bdiff, float& step,
                          float* sqrt_step = nullptr) {
  T = (float)sde.T;
  bmin = (float)sde.beta_min;
  bdiff = (float)(sde.beta_max - sde.beta_min);
  step = (float)(sde.T / (double)num_steps);
  if (sqrt_step) *sqrt_step = (float)std::sqrt(sde.T / (double)num_steps);
}

// "no compiled <kind> (mode m[, precision p]) for width w, layers l, xdim x[, ydim y]"
inline int no_kernel(const char* kind, int mode, const dmip_mlp* net, int xdim, int ydim = -1, int precision = -1) {
  return fail(DMIP_ERR_UNSUPPORTED,
              std::string("no compiled ") + kind + " (mode " + std::to_string(mode) +
                  (precision >= 0 ? ", precision " + std::to_string(precision) : "") + ") for width " +
                  std::to_string(net->width) + ", layers " + std::to_string(net->n_hidden) + ", xdim " +
                  std::to_string(xdim) + (ydim >= 0 ? ", ydim " + std::to_string(ydim) : ""));
}

// the networks and sizes of a sampler (`who` "sampler") or flow ("flow_logp", "flow_sample", ...) launch. net0: the
// CDE / CDiffE network or the Posterior likelihood; net1: the Posterior prior (else null). `rows`: `count` is a
// log-density call's row count, else the chain count (checked with `offset`)
inline int check_nets(const char* who, const dmip_mlp* net0, const dmip_mlp* net1, int out_expected, int xdim, int ydim,
                      int n_y, bool rows, int64_t count, int64_t offset, int num_steps, const dmip_vpsde* sde) {
  if (net0->layout != DMIP_INPUT_X_Y_T) return fail(DMIP_ERR_INVALID, std::string(who) + " needs an x,y,t network");
  if (xdim != net0->xdim || net0->out_dim != out_expected)
    return fail(DMIP_ERR_INVALID, "xdim does not match the network");
  if (ydim != net0->in_dim - xdim - 1) return fail(DMIP_ERR_INVALID, "ydim does not match the network");
  if (net1) {
    if (net1->layout != DMIP_INPUT_X_T || net1->xdim != xdim || net1->out_dim != xdim)
      return fail(DMIP_ERR_INVALID, "prior must be an x,t network with out_dim == xdim");
    if (net1->width != net0->width || net1->n_hidden != net0->n_hidden)
      return fail(DMIP_ERR_UNSUPPORTED, "prior and likelihood networks must have the same hidden layers");
  }
  if (n_y < 1 || n_y > 65535) return fail(DMIP_ERR_INVALID, "n_y must be in [1, 65535]");
  if (rows && count < 0) return fail(DMIP_ERR_INVALID, "negative row count");
  if (!rows && (count < 0 || offset < 0)) return fail(DMIP_ERR_INVALID, "negative chain count/offset");
  if (num_steps < 1) return fail(DMIP_ERR_INVALID, "num_steps must be >= 1");
  if (!(sde->T > 0.0)) return fail(DMIP_ERR_INVALID, "T must be > 0");
  return DMIP_OK;
}

// the exact-f32 engine's per-y layer-1 images (the samplers and the flow): y is constant per y index, so layer 1 runs
// over (x, t) with W1_y y + b1 folded into the bias column
inline int f32_l1_prep(StreamScratch& l1y, const dmip_mlp* net, const float* y_dev, int n_y, int xdim, int ydim,
                       hipStream_t st) {
  const int k1q = (xdim + 2 + 3) / 4;
  if (int rc = l1y.alloc((size_t)n_y * (net->width / 16) * k1q * 64 * sizeof(float), st)) return rc;
  dmip::F32L1PrepParams lp{net->w1, net->b1, y_dev, (float*)l1y.ptr, net->width, net->in_dim, xdim, ydim, k1q};
  const hipError_t e = dmip::launch_f32_l1_prep(lp, n_y, st);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "f32 layer-1 prep launch");
}

// the refusal of every fp32x3 entry point whose split images could not be packed (`what`: "|w|" or "scaled |w|")
inline int x3_range_refused(const std::string& who, const char* what, double range) {
  return fail(DMIP_ERR_UNSUPPORTED, who + ": a weight is outside the fp16 range of the split engine (largest " + what +
                                        " " + std::to_string(range) + " > 65504); use DMIP_PREC_F32");
}
inline int x3_check_range(const dmip_mlp* net0, const dmip_mlp* net1) {  // the samplers' and the flow's networks
  for (const dmip_mlp* n : {net0, net1})
    if (n && n->x3_range > 0.0) return x3_range_refused("fp32x3", "scaled |w|", n->x3_range);
  return DMIP_OK;
}

// the fp32x3 engine's per-y layer-1 bias (the samplers and the flow): y is constant per y index, so c (b1 + W1_y y)
// becomes layer 1's bias (f64 prep)
inline int x3_bias_prep(StreamScratch& bias_y, const dmip_mlp* net, const float* y_dev, int n_y, int xdim, int ydim,
                        hipStream_t st) {
  if (int rc = bias_y.alloc((size_t)n_y * net->width * sizeof(float), st)) return rc;
  dmip::X3BiasPrepParams bp{net->w1, net->b1, y_dev, (float*)bias_y.ptr, net->width, net->in_dim, xdim, ydim};
  const hipError_t e = dmip::launch_x3_bias_prep(bp, n_y, st);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "x3 bias prep launch");
}

inline int surrogate_n_wg(int64_t rows, hipStream_t st) {
  int n_cu = 256;
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dmip::stream_device(st));
  if (n_cu < 1) n_cu = 256;
  const int64_t per = dmip::surrogate_rows_per_wg();
  return (int)std::max<int64_t>(1, std::min<int64_t>(n_cu, (rows + per - 1) / per));
}

inline void surrogate_params(const dmip_surrogate* s, dmip::SurrogateParams& p) {
  p.l1 = s->l1;
  p.bias = s->bias;
  p.w2 = s->img[0];
  p.w3 = s->img[1];
  p.w4 = s->img[2];
  p.w3t = s->img[3];
  p.w2t = s->img[4];
  p.w4t = s->img[5];
  p.w1t = s->img[6];
}

}  // namespace dmip_capi
