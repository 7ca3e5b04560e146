// Host-side weight packing: a torch MLP's weights as the MFMA fragment images the kernels read. Pure host code (no
// HIP runtime call), so every packer runs, and is tested, without a GPU (tests/pack/pack_images.cpp). The C-ABI
// layer (dmip_capi_pack.cpp) uploads what these return.
#pragma once
#include <cstdint>
#include <vector>

namespace dmip_pack {

using Img16 = std::vector<uint16_t>;  // bf16 / fp16 fragment images
using ImgF = std::vector<float>;

inline int k1s_for(int n_slots) { return (n_slots + 15) / 16; }

// the validated arguments of dmip_mlp_create that the images depend on (the activation chain is not one of them)
struct MlpDesc {
  int in_dim, out_dim, n_hidden, width, layout, xdim;
};

// One host image per device buffer of dmip_mlp, under the same name (dmip_capi_common.h has each one's layout), and
// the scalars the handle keeps. An empty image is not uploaded: the engine it serves is absent for this network.
struct MlpImages {
  int k1s_full = 0, f32_k1q = 0, f32_ot = 0;
  double x3_range = 0.0, dps_x3_range = 0.0;
  Img16 hidden, ao_samp, ao_full, a1_full, ring_l1;
  ImgF bias_hidden, bias_out_samp, bias_out_full, w1, b1;
  ImgF dps_l1, dps_w2, dps_w3, dps_w4, dps_bias, dps_x3_bias;
  Img16 dps_x3_img, dps_x3_l1;
  ImgF f32_l1, f32_stream, f32_bias, x3_bias;
  Img16 x3_l1, x3_l1_full, x3_stream, x3_stream_l1r, x3k_stream, x3k_out;
  Img16 x3p_stream, x3p_l1;  // packed under DMIP_WITH_X3P only
  ImgF x3p_ow;
};

struct SurrogateImages {
  ImgF l1, bias, img[7], x3_bias;
  Img16 x3_img, x3_l1;
  double x3_range = 0.0;
};

MlpImages pack_mlp(const MlpDesc& d, const float* const* weights, const float* const* biases);
SurrogateImages pack_surrogate(const float* const* weights, const float* const* biases);

}  // namespace dmip_pack
