// Shared by the C-ABI sources (dmip_capi_pack.cpp, dmip_capi_sample.cpp, dmip_capi_train.cpp): error reporting, the
// handle structs behind include/dmip.h's opaque types, and the small helpers more than one of them uses. Host code
// only; no kernel includes this header.
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

struct dmip_mlp {
  int in_dim = 0, out_dim = 0, n_hidden = 0, width = 0, act_mode = 0, layout = 0, xdim = 0;
  int k1s_full = 0;
  char* hidden = nullptr;         // [(L-1)][W/32][W/16] KiB
  char* ao_samp = nullptr;        // [W/16] KiB, output rows duplicated into lanes 32-63
  char* ao_full = nullptr;        // [W/16] KiB, natural output rows
  float* bias_hidden = nullptr;   // [(L-1)][W/32][2][16]
  float* bias_out_samp = nullptr; // [2][16]
  float* bias_out_full = nullptr; // [2][16]
  char* a1_full = nullptr;        // [W/32][k1s_full] KiB (every input column varying)
  char* ring_l1 = nullptr;        // width 512: [layer-1 chunks (split image) | hidden | output] (CDiffE sampler)
  float* w1 = nullptr;            // layer-1 fp32 [W][in_dim] (per-y prep of the sampler's A1)
  float* b1 = nullptr;
  // exact-f32 images of a DPS prior (MLP2 (x, t), x 3, widths [256]*3): dmip_dps_sample
  float* dps_l1 = nullptr;        // [16 tiles][2 k-steps][64]
  char* dps_w2 = nullptr;         // [16][16][64][4]
  char* dps_w3 = nullptr;
  char* dps_w4 = nullptr;         // [1][16][64][4], rows >= 3 zero
  float* dps_bias = nullptr;      // b2 | b3 | b4[16]
  // fp32x3 images of a DPS prior (dmip_dps_x3.hip): the chunk stream, layer 1, the biases; none when a weight is
  // beyond fp16's range (dps_x3_range: that magnitude)
  char* dps_x3_img = nullptr;     // [kDpsX3PriorChunks][32 KiB]
  char* dps_x3_l1 = nullptr;      // [16 tiles][64][8] fp16, scaled by 2 log2 e
  float* dps_x3_bias = nullptr;   // c b1 | init2 | init3 [256] | out init [16]
  double dps_x3_range = 0.0;
  // exact-f32 images (DMIP_PREC_F32, dmip_f32.h): every input column + bias as layer 1
  float* f32_l1 = nullptr;        // [W/16][k1q][64]
  char* f32_stream = nullptr;     // [(L-1) W/16 + f32_ot chunks][W/16][64][4]
  float* f32_bias = nullptr;      // [(L-1)][W] | [16 f32_ot]
  int f32_k1q = 0, f32_ot = 0;
  // fp32-accurate split-fp16 images (DMIP_PREC_F32X3, dmip_x3.h); none when a scaled weight or folded bias
  // is outside fp16's range (x3_range: that magnitude, reported by em_sample_x3)
  double x3_range = 0.0;
  char* x3_l1 = nullptr;          // [W/16][K1Q][64][8] fp16 over (x, t)
  char* x3_l1_full = nullptr;     // the same over every input column (X_Y_T networks: CDiffE)
  char* x3_stream = nullptr;      // hidden chunks | output chunk
  char* x3_stream_l1r = nullptr;  // CDiffE at width 512: layer-1 chunks ([K1Q][W/16 tiles][64][8]) | x3_stream
  float* x3_bias = nullptr;       // [L W + 16]
  // the k-major engine's images (dmip_x3k.h; width 256, 3 hidden layers, xdim <= 4)
  char* x3k_stream = nullptr;     // [2 layers][8 k-steps][16 tiles][hi, lo][64][8] fp16
  char* x3k_out = nullptr;        // [8 k-steps][64][8]: rows 0..xdim-1 W_hi, rows 4..4+xdim-1 W_lo
  // the paired-tile 32x32 engine's images (dmip_x3p.h; same shapes)
  char* x3p_stream = nullptr;     // [16 chunks][32 KiB]
  char* x3p_l1 = nullptr;         // [8 layer-1 tiles][64][8] | [2 hidden layers][8 bias tiles][64][8] fp16
  float* x3p_ow = nullptr;        // f32 output rows [8][2][4][4][4] | init[16]
  ~dmip_mlp() {
    for (void* p : {(void*)ring_l1, (void*)hidden, (void*)ao_samp, (void*)ao_full, (void*)bias_hidden, (void*)bias_out_samp,
                    (void*)bias_out_full, (void*)a1_full, (void*)w1, (void*)b1, (void*)dps_l1, (void*)dps_w2,
                    (void*)dps_w3, (void*)dps_w4, (void*)dps_bias, (void*)f32_l1, (void*)f32_stream,
                    (void*)f32_bias, (void*)x3_l1, (void*)x3_l1_full, (void*)x3_stream, (void*)x3_stream_l1r,
                    (void*)x3_bias,
                    (void*)x3k_stream, (void*)x3k_out, (void*)x3p_stream, (void*)x3p_l1, (void*)x3p_ow,
                    (void*)dps_x3_img, (void*)dps_x3_l1, (void*)dps_x3_bias})
      if (p) (void)hipFree(p);
  }
};

// the scatterometry surrogate
struct dmip_surrogate {
  float* l1 = nullptr;
  float* bias = nullptr;
  char* img[7] = {};  // w2, w3, w4, w3t, w2t, w4t, w1t
  // fp32x3 images (dmip_dps_x3.hip): chunks S2 | S3 | Sout | S4^T | S3^T | S2^T | S1^T, layer 1, biases; none when
  // a weight is beyond fp16's range (x3_range)
  char* x3_img = nullptr;
  char* x3_l1 = nullptr;
  float* x3_bias = nullptr;  // b1 | b2 | b3 [256] | b4 [32]
  double x3_range = 0.0;
  ~dmip_surrogate() {
    if (l1) (void)hipFree(l1);
    if (bias) (void)hipFree(bias);
    for (char* p : img)
      if (p) (void)hipFree(p);
    for (void* p : {(void*)x3_img, (void*)x3_l1, (void*)x3_bias})
      if (p) (void)hipFree(p);
  }
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

inline int k1s_for(int n_slots) { return (n_slots + 15) / 16; }

template <typename T>
int upload(T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  if (src.empty()) return DMIP_OK;
  hipError_t e = hipMalloc((void**)dst, src.size() * sizeof(T));
  if (e != hipSuccess) return fail(DMIP_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
  e = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
  return DMIP_OK;
}

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

// the activation chain's code in the exact-f32 kernels (dmip_f32.h act_f32): 0 tanh, 1 SiLU. Only the exact-f32
// forward and the exact-f32 CDE sampler compile the SiLU chain; every other kernel computes tanh.
inline int f32_act(const dmip_mlp* n) { return n->act_mode == DMIP_ACT_SILU_TWICE_FIRST ? 1 : 0; }

inline int act_refused(const char* what) {
  return fail(DMIP_ERR_UNSUPPORTED, std::string(what) +
                                        ": the SiLU chain is compiled for the exact-f32 forward and the exact-f32 "
                                        "CDE sampler only (DMIP_PREC_F32)");
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
