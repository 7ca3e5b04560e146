// Pins every weight image of the packing layer (csrc/dmip_pack.h) without a GPU: for a few small networks, the
// smallest that reach each branch of the packers, prints one line per image (case, name, bytes, 64-bit FNV-1a of the
// bytes) and one per scalar. tests/test_pack_images.py compares the lines with tests/golden/pack_images.json
// (recorded from the packers as they were before the split, tests/golden/pack_images.md); `make asan` runs the same
// program under AddressSanitizer. Weights come from a fixed integer LCG: no input files, no libm.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../diffusion-modelling-for-inverse-problems_amd/csrc/dmip_pack.h"
#include "../../include/dmip.h"

using dmip_pack::MlpImages;
using dmip_pack::SurrogateImages;

// weights in [-1/4, 1/4): 24 bits of a 64-bit LCG (Knuth's MMIX constants), exact in f32
struct Lcg {
  uint64_t s;
  float next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((int32_t)(s >> 40) - (1 << 23)) * (1.0f / (float)(1 << 25));
  }
};

struct Net {
  std::vector<std::vector<float>> w, b;
  std::vector<const float*> wp, bp;
  // layer li is [n[li + 1]][n[li]]
  Net(const std::vector<int>& n, uint64_t seed) {
    Lcg g{seed};
    for (size_t li = 0; li + 1 < n.size(); ++li) {
      w.emplace_back((size_t)n[li + 1] * n[li]);
      b.emplace_back((size_t)n[li + 1]);
      for (float& v : w.back()) v = g.next();
      for (float& v : b.back()) v = g.next();
    }
    for (size_t li = 0; li < w.size(); ++li) wp.push_back(w[li].data()), bp.push_back(b[li].data());
  }
};

template <typename T>
static void image(const char* c, const char* name, const std::vector<T>& v) {
  uint64_t h = 14695981039346656037ull;
  const unsigned char* p = (const unsigned char*)v.data();
  for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
  std::printf("img %s %s %zu %016llx\n", c, name, v.size() * sizeof(T), (unsigned long long)h);
}

struct MlpCase {
  const char* name;
  int layout, width, n_hidden, xdim, in_dim, out_dim;
  int poke_layer;  // one weight of this layer replaced by `poke` (-1: none)
  float poke;
};

static void mlp_case(const MlpCase& c) {
  std::vector<int> n{c.in_dim};
  n.insert(n.end(), c.n_hidden, c.width);
  n.push_back(c.out_dim);
  Net net(n, 0x5eed0000u + (unsigned)c.width + 7u * c.in_dim);
  if (c.poke_layer >= 0) net.w[c.poke_layer][net.w[c.poke_layer].size() / 3] = c.poke;
  const auto t0 = std::chrono::steady_clock::now();
  const MlpImages im = dmip_pack::pack_mlp({c.in_dim, c.out_dim, c.n_hidden, c.width, c.layout, c.xdim},
                                           net.wp.data(), net.bp.data());
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::printf("# time %s pack_mlp %.3f ms\n", c.name, ms);
#define IMG(f) image(c.name, #f, im.f)
  IMG(hidden), IMG(ao_samp), IMG(ao_full), IMG(a1_full), IMG(ring_l1), IMG(bias_hidden), IMG(bias_out_samp);
  IMG(bias_out_full), IMG(w1), IMG(b1), IMG(dps_l1), IMG(dps_w2), IMG(dps_w3), IMG(dps_w4), IMG(dps_bias);
  IMG(dps_x3_img), IMG(dps_x3_l1), IMG(dps_x3_bias), IMG(f32_l1), IMG(f32_stream), IMG(f32_bias), IMG(x3_l1);
  IMG(x3_l1_full), IMG(x3_stream), IMG(x3_stream_l1r), IMG(x3_bias), IMG(x3k_stream), IMG(x3k_out), IMG(x3p_stream);
  IMG(x3p_l1), IMG(x3p_ow);
  std::printf("val %s k1s_full %d\nval %s f32_k1q %d\nval %s f32_ot %d\n", c.name, im.k1s_full, c.name, im.f32_k1q,
              c.name, im.f32_ot);
  std::printf("val %s x3_range %.17g\nval %s dps_x3_range %.17g\n", c.name, im.x3_range, c.name, im.dps_x3_range);
}

static void surrogate_case(const char* name, float poke) {
  Net net({3, 256, 256, 256, 23}, 0x5eed5005u);
  if (poke != 0.0f) net.w[1][net.w[1].size() / 3] = poke;
  const SurrogateImages im = dmip_pack::pack_surrogate(net.wp.data(), net.bp.data());
  const char* img[7] = {"img0", "img1", "img2", "img3", "img4", "img5", "img6"};
  image(name, "l1", im.l1), image(name, "bias", im.bias);
  for (int i = 0; i < 7; ++i) image(name, img[i], im.img[i]);
  image(name, "x3_img", im.x3_img), image(name, "x3_l1", im.x3_l1), image(name, "x3_bias", im.x3_bias);
  std::printf("val %s x3_range %.17g\n", name, im.x3_range);
}

int main() {
  const int XYT = DMIP_INPUT_X_Y_T, XT = DMIP_INPUT_X_T;
  const MlpCase cases[] = {
      {"a", XT, 32, 1, 2, 3, 2, -1, 0.f},      // t-form output layer; no fp32x3 kernels at width 32
      {"b", XYT, 64, 3, 2, 5, 2, -1, 0.f},     // the base 16-bit / f32 / fp32x3 images, x3_l1_full, split layer 1
      {"c", XYT, 64, 3, 2, 5, 2, -1, 0.f},     // b with the SiLU chain: the activation is no packing input
      {"d", XYT, 256, 3, 2, 5, 2, -1, 0.f},    // k-major and paired-tile images
      {"e", XT, 256, 3, 3, 4, 3, -1, 0.f},     // a DPS prior; k-major at xdim 3
      {"f", XYT, 512, 3, 3, 27, 26, -1, 0.f},  // ring_l1, x3_stream_l1r, unsplit forward layer 1, two f32 output tiles
      {"g", XYT, 512, 3, 2, 5, 2, -1, 0.f},    // split forward layer 1 at 512, several row tiles per ring chunk
      {"h", XYT, 64, 3, 2, 5, 2, 1, 3e4f},     // a hidden weight beyond the fp16 split: x3_range, no fp32x3 images
      {"i", XT, 256, 3, 3, 4, 3, 0, 5e4f},     // a layer-1 weight beyond it: dps_x3_range, no dps_x3 images
  };
  for (const MlpCase& c : cases) mlp_case(c);
  surrogate_case("j", 0.0f);
  surrogate_case("k", 7e4f);  // x3_range, no fp32x3 images
  return 0;
}
