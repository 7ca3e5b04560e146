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
