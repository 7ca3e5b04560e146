// libdmip.so C-ABI (include/dmip.h), handles and library state: host-side weight packing into the kernels' MFMA
// fragment layouts (dmip_mlp_create, dmip_surrogate_create), the network forward, the error text and the device
// status words. The sampling entry points are in dmip_capi_sample.cpp, the training ones in dmip_capi_train.cpp.
//
// Packing conventions (shared with dmip_kernels.hip):
//   * One 1 KiB fragment block = 64 lanes x 8 bf16, the A operand of one
//     v_mfma_f32_32x32x16_bf16: lane l = i + 32h holds A[row i][k = 8h + j], j = 0..7.
//   * Hidden layer k-order: the B operand is the previous layer's accumulator registers, so
//     element j of lane half h in k-step s is hidden unit kperm(s, h, j) (see below).
//   * r-form activations: kernels carry r = 1/(1+exp(2z)) = (1 - tanh z)/2 after a single tanh,
//     so the next layer uses weights -2W and bias b + sum_k W; after layer 1's double tanh they
//     carry the value itself (t-form: weights W, bias b). Pre-activations of tanh layers are
//     scaled by c = 2 log2(e) (exp2 instead of exp).
#include <map>
#include <mutex>
#include <new>
#include <tuple>

#include "dmip_capi_common.h"

using namespace dmip_capi;

namespace {

constexpr double kC = 2.8853900817779268;  // 2 log2(e)

uint16_t f2bf(float f) {  // round to nearest even (inputs are finite)
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

float bf2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// fp16 images of the hidden and output layers (the engine's v_mfma_f32_32x32x16_f16 operands):
// round to nearest even, subnormals kept, |v| <= 65504 (trained and random-init weights are far inside)
uint16_t f2h(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t u;
  std::memcpy(&u, &h, 2);
  return u;
}

float h2f(uint16_t u) {
  _Float16 h;
  std::memcpy(&h, &u, 2);
  return (float)h;
}

// f32 A-fragment images for v_mfma_f32_16x16x4_f32 (dmip_surrogate.hip): k-step (q, r) of output
// tile o, lane l = i + 16 g, holds M[16 o + i][16 q + 4 g + r]; stored [o][q][lane][r] (one float4
// per lane per q). M(row, col) returns 0 outside the matrix.
template <typename F>
std::vector<char> pack_f32_tiles(int n_tiles, int n_q, F M) {
  std::vector<float> v((size_t)n_tiles * n_q * 64 * 4);
  for (int o = 0; o < n_tiles; ++o)
    for (int q = 0; q < n_q; ++q)
      for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r)
          v[(((size_t)o * n_q + q) * 64 + l) * 4 + r] = M(16 * o + (l & 15), 16 * q + 4 * (l >> 4) + r);
  std::vector<char> b(v.size() * 4);
  std::memcpy(b.data(), v.data(), b.size());
  return b;
}

inline int kperm(int s, int h, int j) { return 32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }
inline int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// One device status word per device (kernels report asynchronous failures into it; read and
// cleared by dmip_device_status). Allocated on first use, never freed (4 bytes per device).
std::mutex g_status_mu;
unsigned* g_status[dmip::kMaxDevices] = {};

// a pinned host mirror of the status word: dmip_device_status copies the word into it on the stream and synchronises
// once (round 6; before, a stream synchronise and then a blocking 4-byte hipMemcpy: two round trips per read)
unsigned* g_status_host[dmip::kMaxDevices] = {};
unsigned* status_host(int dev) {
  if (dev < 0 || dev >= dmip::kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lk(g_status_mu);
  if (!g_status_host[dev]) {
    unsigned* h = nullptr;
    if (hipHostMalloc((void**)&h, sizeof(unsigned), hipHostMallocDefault) == hipSuccess) g_status_host[dev] = h;
  }
  return g_status_host[dev];
}

}  // namespace

thread_local std::string dmip_capi::g_err;

unsigned* dmip_capi::status_word(int dev) {
  if (dev < 0 || dev >= dmip::kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lk(g_status_mu);
  if (!g_status[dev]) {
    int cur = dev;
    (void)hipGetDevice(&cur);
    if (cur != dev) (void)hipSetDevice(dev);
    unsigned* w = nullptr;
    if (hipMalloc((void**)&w, sizeof(unsigned)) == hipSuccess && hipMemset(w, 0, sizeof(unsigned)) == hipSuccess)
      g_status[dev] = w;
    if (cur != dev) (void)hipSetDevice(cur);
  }
  return g_status[dev];
}

namespace dmip {

int resident_slots_impl(const void* fn, int nthreads, hipStream_t st) {
  static std::mutex mu;
  static std::map<std::tuple<const void*, int, int>, int> cache;
  const int dev = stream_device(st);
  const auto key = std::make_tuple(fn, nthreads, dev);
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
  }
  int n_cu = 256, per_cu = 1, cur = dev;
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
  (void)hipGetDevice(&cur);
  if (cur != dev) (void)hipSetDevice(dev);  // the occupancy query is for the current device
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, nthreads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  if (cur != dev) (void)hipSetDevice(cur);
  const int slots = (n_cu > 0 ? n_cu : 256) * per_cu;
  std::lock_guard<std::mutex> lk(mu);
  cache[key] = slots;
  return slots;
}

}  // namespace dmip

namespace {

// exact-f32 images of a network (dmip_f32.h FEngine): layer 1 over every input column then the bias
// column; the W x W layers and the output layer as 16-row chunks in stream order; the biases.
int pack_f32_net(dmip_mlp* net, const float* const* weights, const float* const* biases) {
  const int W = net->width, L = net->n_hidden, IN = net->in_dim, OUT = net->out_dim, ST = W / 16;
  const int K1Q = (IN + 1 + 3) / 4, OT = (OUT + 15) / 16;
  net->f32_k1q = K1Q;
  net->f32_ot = OT;
  std::vector<float> l1((size_t)ST * K1Q * 64);
  for (int o = 0; o < ST; ++o)
    for (int s = 0; s < K1Q; ++s)
      for (int l = 0; l < 64; ++l) {
        const int u = 16 * o + (l & 15), c = 4 * s + (l >> 4);
        l1[((size_t)o * K1Q + s) * 64 + l] = c < IN ? weights[0][(size_t)u * IN + c] : (c == IN ? biases[0][u] : 0.0f);
      }
  std::vector<char> stream;
  for (int li = 1; li < L; ++li) {
    const float* Wl = weights[li];
    std::vector<char> img = pack_f32_tiles(ST, ST, [Wl, W](int r, int c) { return Wl[(size_t)r * W + c]; });
    stream.insert(stream.end(), img.begin(), img.end());
  }
  const float* Wo = weights[L];
  std::vector<char> oimg =
      pack_f32_tiles(OT, ST, [Wo, W, OUT](int r, int c) { return r < OUT ? Wo[(size_t)r * W + c] : 0.0f; });
  stream.insert(stream.end(), oimg.begin(), oimg.end());
  std::vector<float> bias((size_t)(L - 1) * W + 16 * OT, 0.0f);
  for (int li = 1; li < L; ++li)
    for (int k = 0; k < W; ++k) bias[(size_t)(li - 1) * W + k] = biases[li][k];
  for (int k = 0; k < OUT; ++k) bias[(size_t)(L - 1) * W + k] = biases[L][k];
  int rc = DMIP_OK;
  if ((rc = upload(&net->f32_l1, l1)) || (rc = upload(&net->f32_stream, stream)) || (rc = upload(&net->f32_bias, bias)))
    return rc;
  return DMIP_OK;
}

// ---- fp32-accurate split-fp16 images (DMIP_PREC_F32X3, dmip_x3.h). A 16x16x32 f16 fragment block:
// lane l = i + 16 g holds A[row i][k-slot 8 g + m], m = 0..7. Hidden-layer k-slots follow the previous
// layer's accumulator tiles: slot (q, g, m) is unit kperm16(q, g, m).
inline int kperm16(int q, int g, int m) { return 32 * q + 16 * (m >> 2) + 4 * g + (m & 3); }
inline int x3_k1q(int nv) { return (3 * nv + 31) / 32; }

// v = hi + lo in fp16 (hi = fp16(v), lo = fp16(v - hi))
void split_h(double v, uint16_t& hi, uint16_t& lo) {
  hi = f2h((float)v);
  lo = f2h((float)(v - (double)h2f(hi)));
}

#ifdef DMIP_WITH_X3P
// 32x32x16 fragments (dmip_x3p.h): lane l = i + 32 h holds A[row i][k-slot 8 h + j]; k-step s of a hidden layer
// covers the previous layer's accumulator registers 8 (s & 1) .. + 7 of its output tile s >> 1
inline int kperm32(int s, int h, int j) { return 32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }

// the paired-tile engine's images of a [256]*3 CDE (dmip_x3p.h): the same hi / lo split and folded scales as
// pack_x3_layer / pack_x3_l1 in the 32x32x16 fragment layout; hidden layer 1's bias (`init1`, already folded)
// and hidden layer 2's (`init1`, `init2`: the folded inits of pack_x3_layer) as three-part fp16 A fragments per
// output tile; the output layer in f32 (r-form fold: A = -2 W, init = b + sum_k W, in double)
int pack_x3p(dmip_mlp* net, const float* const* weights, const float* const* biases, const float* init1,
             const float* init2) {
  const int W = net->width, IN = net->in_dim, D = net->xdim, OT = W / 32, KS = W / 16;
  std::vector<uint16_t> l1((size_t)3 * OT * 512, 0);
  std::vector<int> cols;
  for (int k = 0; k < D; ++k) cols.push_back(k);
  cols.push_back(IN - 1);
  const int NV = (int)cols.size();
  for (int o = 0; o < OT; ++o)
    for (int l = 0; l < 64; ++l) {
      const int i = l & 31, h = l >> 5;
      for (int j = 0; j < 8; ++j) {
        const int sl = 8 * h + j, n = sl / 3, pt = sl % 3;
        if (n >= NV) continue;
        uint16_t hi, lo;
        split_h(kC * (double)weights[0][(size_t)(32 * o + i) * IN + cols[n]], hi, lo);
        l1[((size_t)o * 64 + l) * 8 + j] = pt < 2 ? hi : lo;
      }
      for (int li = 1; li <= 2 && h == 0; ++li) {  // bias = hi + mid + lo in k-slots 0..2 (against ones)
        const double v = (double)(li == 1 ? init1 : init2)[32 * o + i];
        const uint16_t a = f2h((float)v);
        const double r1 = v - (double)h2f(a);
        const uint16_t b = f2h((float)r1);
        const uint16_t c = f2h((float)(r1 - (double)h2f(b)));
        uint16_t* dst = &l1[((size_t)(li * OT + o) * 64 + l) * 8];
        dst[0] = a, dst[1] = b, dst[2] = c;
      }
    }
  std::vector<char> stream;
  std::vector<uint16_t> hi((size_t)W * W), lo((size_t)W * W), img((size_t)OT * KS * 1024);
  for (int li = 1; li <= 2; ++li) {
    for (int r = 0; r < W; ++r)
      for (int k = 0; k < W; ++k)
        split_h(-2.0 * kC * (double)weights[li][(size_t)r * W + k], hi[(size_t)r * W + k], lo[(size_t)r * W + k]);
    size_t at = 0;
    // hidden layer 1 k-major: chunk q, output tile o, k-step half e; hidden layer 2 output-major: chunk c, k-step s
    for (int a = 0; a < OT; ++a)
      for (int b = 0; b < KS; ++b)
        for (int pt = 0; pt < 2; ++pt)
          for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
              const int row = li == 1 ? 32 * (b >> 1) + (l & 31) : 32 * a + (l & 31);
              const int s = li == 1 ? 2 * a + (b & 1) : b;
              const size_t src = (size_t)row * W + kperm32(s, l >> 5, j);
              img[at++] = pt == 0 ? hi[src] : lo[src];
            }
    const char* p = (const char*)img.data();
    stream.insert(stream.end(), p, p + img.size() * 2);
  }
  std::vector<float> ow((size_t)OT * 2 * 64 + 16, 0.0f);
  for (int c = 0; c < OT; ++c)
    for (int h = 0; h < 2; ++h)
      for (int k = 0; k < D && k < 4; ++k)
        for (int part = 0; part < 4; ++part)
          for (int m = 0; m < 4; ++m)
            ow[(((size_t)c * 2 + h) * 4 + k) * 16 + part * 4 + m] =
                (float)(-2.0 * (double)weights[3][(size_t)k * W + 32 * c + 8 * part + 4 * h + m]);
  for (int k = 0; k < D && k < 4; ++k) {
    double acc = (double)biases[3][k];
    for (int u = 0; u < W; ++u) acc += (double)weights[3][(size_t)k * W + u];
    ow[(size_t)OT * 2 * 64 + k] = (float)acc;
  }
  std::vector<char> l1b(l1.size() * 2);
  std::memcpy(l1b.data(), l1.data(), l1b.size());
  int rc = DMIP_OK;
  if ((rc = upload(&net->x3p_stream, stream)) || (rc = upload(&net->x3p_l1, l1b)) || (rc = upload(&net->x3p_ow, ow)))
    return rc;
  return DMIP_OK;
}

#endif  // DMIP_WITH_X3P

// [n_tiles][KQ][hi, lo][64][8] fp16 split of A[r][c] = get(r, c): lane i + 16 g of tile o holds A[16 o + i][kperm16(q,
// g, m)], m = 0..7 -- pack_x3_layer's layout without its r-form fold (the DPS engine's plain and transposed layers).
// *maxabs: the largest |A| (the split needs it inside fp16's range)
template <typename Get>
std::vector<uint16_t> pack_x3_plain(int n_tiles, int KQ, Get get, double* maxabs) {
  std::vector<uint16_t> img((size_t)n_tiles * KQ * 2 * 512, 0);
  for (int o = 0; o < n_tiles; ++o)
    for (int q = 0; q < KQ; ++q)
      for (int l = 0; l < 64; ++l)
        for (int m = 0; m < 8; ++m) {
          const double v = (double)get(16 * o + (l & 15), kperm16(q, l >> 4, m));
          *maxabs = std::max(*maxabs, std::fabs(v));
          uint16_t hi, lo;
          split_h(v, hi, lo);
          img[((((size_t)o * KQ + q) * 2 + 0) * 64 + l) * 8 + m] = hi;
          img[((((size_t)o * KQ + q) * 2 + 1) * 64 + l) * 8 + m] = lo;
        }
  return img;
}

// append an image to a chunk stream, zero-padded to whole 32 KiB chunks
void append_chunks(std::vector<char>& out, const std::vector<uint16_t>& img) {
  const size_t bytes = img.size() * 2, padded = (bytes + dmip::kDpsX3Chunk - 1) / dmip::kDpsX3Chunk * dmip::kDpsX3Chunk;
  const size_t at = out.size();
  out.resize(at + padded, 0);
  std::memcpy(out.data() + at, img.data(), bytes);
}

// layer-1 image over the input columns `cols` (scaled by c): input n at k-slots 3n, 3n+1, 3n+2 with
// A = [W_hi, W_hi, W_lo] (the kernel's B = [v_hi, v_lo, v_hi])
std::vector<uint16_t> pack_x3_l1(const float* W1, int W, int in_dim, const std::vector<int>& cols, double scale = kC) {
  const int NV = (int)cols.size(), K1Q = x3_k1q(NV), ST = W / 16;
  std::vector<uint16_t> img((size_t)ST * K1Q * 512, 0);
  for (int o = 0; o < ST; ++o)
    for (int q = 0; q < K1Q; ++q)
      for (int l = 0; l < 64; ++l)
        for (int m = 0; m < 8; ++m) {
          const int i = l & 15, g = l >> 4, s = 32 * q + 8 * g + m, n = s / 3, p = s % 3;
          if (n >= NV) continue;
          uint16_t hi, lo;
          split_h(scale * (double)W1[(size_t)(16 * o + i) * in_dim + cols[n]], hi, lo);
          img[(((size_t)o * K1Q + q) * 64 + l) * 8 + m] = p < 2 ? hi : lo;
        }
  return img;
}

// [n_tiles][KQ][2][64][8] image of an r-form-input layer: A = scale * (-2 W), init = scale b - 0.5 sum_k A
// (with A = hi + lo as the kernel applies it); rows >= n_rows zero
void pack_x3_layer(const float* Wl, const float* bl, int n_rows, int W, int n_tiles, double scale,
                   std::vector<uint16_t>& img, float* init) {
  const int KQ = W / 32;
  img.assign((size_t)n_tiles * KQ * 2 * 512, 0);
  std::vector<uint16_t> hi((size_t)n_rows * W), lo((size_t)n_rows * W);
  for (int r = 0; r < n_rows; ++r) {
    double acc = 0.0;
    for (int k = 0; k < W; ++k) {
      split_h(-2.0 * scale * (double)Wl[(size_t)r * W + k], hi[(size_t)r * W + k], lo[(size_t)r * W + k]);
      acc += (double)h2f(hi[(size_t)r * W + k]) + (double)h2f(lo[(size_t)r * W + k]);
    }
    init[r] = (float)(scale * (double)bl[r] - 0.5 * acc);
  }
  for (int o = 0; o < n_tiles; ++o)
    for (int q = 0; q < KQ; ++q)
      for (int p = 0; p < 2; ++p)
        for (int l = 0; l < 64; ++l)
          for (int m = 0; m < 8; ++m) {
            const int row = 16 * o + (l & 15);
            if (row >= n_rows) continue;
            const size_t src = (size_t)row * W + kperm16(q, l >> 4, m);
            img[((((size_t)o * KQ + q) * 2 + p) * 64 + l) * 8 + m] = p == 0 ? hi[src] : lo[src];
          }
}

// the fp32x3 DPS engine's prior images (dmip_dps_x3.hip): layer 1 over (x, t) scaled by 2 log2 e; the forward chunks
// P2 | P3 (pack_x3_layer: r-form folds) | Pout (folded, scale 1); the reverse chunks P4^T (one k-step: the 3 output
// rows) | P3^T | P2^T (plain transposes) | P1^T (W1's x columns); biases c b1 | init2 | init3 | out init
int pack_dps_x3_prior(dmip_mlp* net, const float* const* weights, const float* const* biases) {
  const int W = 256;
  const float *W1 = weights[0], *W2 = weights[1], *W3 = weights[2], *W4 = weights[3];
  double mx = 0.0;
  std::vector<float> bias((size_t)3 * W + 16, 0.0f);
  for (int u = 0; u < W; ++u) bias[u] = (float)(kC * (double)biases[0][u]);
  std::vector<char> chunks;
  std::vector<uint16_t> img;
  pack_x3_layer(W2, biases[1], W, W, 16, kC, img, bias.data() + W);
  for (uint16_t h : img) mx = std::max(mx, std::fabs((double)h2f(h)));
  append_chunks(chunks, img);
  pack_x3_layer(W3, biases[2], W, W, 16, kC, img, bias.data() + 2 * W);
  for (uint16_t h : img) mx = std::max(mx, std::fabs((double)h2f(h)));
  append_chunks(chunks, img);
  pack_x3_layer(W4, biases[3], 3, W, 1, 1.0, img, bias.data() + 3 * W);
  for (uint16_t h : img) mx = std::max(mx, std::fabs((double)h2f(h)));
  append_chunks(chunks, img);
  append_chunks(chunks, pack_x3_plain(16, 1, [&](int r, int c) { return c < 3 ? W4[(size_t)c * W + r] : 0.0f; }, &mx));
  append_chunks(chunks, pack_x3_plain(16, 8, [&](int r, int c) { return W3[(size_t)c * W + r]; }, &mx));
  append_chunks(chunks, pack_x3_plain(16, 8, [&](int r, int c) { return W2[(size_t)c * W + r]; }, &mx));
  append_chunks(chunks, pack_x3_plain(1, 8, [&](int r, int c) { return r < 3 ? W1[(size_t)c * 4 + r] : 0.0f; }, &mx));
  for (size_t i = 0; i < (size_t)W * 4; ++i) mx = std::max(mx, kC * std::fabs((double)W1[i]));
  if (!(mx <= 65504.0) || chunks.size() != (size_t)dmip::kDpsX3PriorChunks * dmip::kDpsX3Chunk) {
    net->dps_x3_range = std::isfinite(mx) ? mx : 1e300;
    return DMIP_OK;  // no fp32x3 DPS for this prior (fp16 range)
  }
  const std::vector<uint16_t> l1 = pack_x3_l1(W1, W, 4, {0, 1, 2, 3});
  std::vector<char> l1b(l1.size() * 2);
  std::memcpy(l1b.data(), l1.data(), l1b.size());
  int rc = DMIP_OK;
  if ((rc = upload(&net->dps_x3_img, chunks)) || (rc = upload(&net->dps_x3_l1, l1b)) ||
      (rc = upload(&net->dps_x3_bias, bias)))
    return rc;
  return DMIP_OK;
}

// largest magnitude the fp32x3 images would hold in fp16: layer 1 scaled by 2 log2(e), the hidden layers by
// -2 * 2 log2(e), the output rows by -2 (r-form folds). The folded hidden biases stay f32 (x3_bias) in the
// product engines, so they do not limit them (only the A/B paired engine stores them in fp16: x3p_bias_range)
double x3_max_scaled(const dmip_mlp* net, const float* const* weights) {
  const int W = net->width, L = net->n_hidden, IN = net->in_dim, OUT = net->out_dim;
  double m = 0.0;
  for (size_t i = 0; i < (size_t)W * IN; ++i) m = std::max(m, kC * std::fabs((double)weights[0][i]));
  for (int li = 1; li < L; ++li)
    for (size_t i = 0; i < (size_t)W * W; ++i) m = std::max(m, 2.0 * kC * std::fabs((double)weights[li][i]));
  for (size_t i = 0; i < (size_t)std::min(OUT, 16) * W; ++i) m = std::max(m, 2.0 * std::fabs((double)weights[L][i]));
  return m;
}

#ifdef DMIP_WITH_X3P
// the paired engine's fp16 folded hidden biases kC (b + sum_k W) (pack_x3p): their largest magnitude
double x3p_bias_range(const dmip_mlp* net, const float* const* weights, const float* const* biases) {
  const int W = net->width, L = net->n_hidden;
  double m = 0.0;
  for (int li = 1; li < L; ++li)
    for (int r = 0; r < W; ++r) {
      double acc = (double)biases[li][r];
      for (int k = 0; k < W; ++k) acc += (double)weights[li][(size_t)r * W + k];
      m = std::max(m, kC * std::fabs(acc));
    }
  return m;
}
#endif

int pack_x3_net(dmip_mlp* net, const float* const* weights, const float* const* biases) {
  const int W = net->width, L = net->n_hidden, IN = net->in_dim, OUT = net->out_dim, ST = W / 16;
  const int chunk = dmip::x3_chunk_bytes(W);
  if (chunk == 0) return DMIP_OK;  // no x3 kernels at this width
  const double mx = x3_max_scaled(net, weights);
  if (!(mx <= 65504.0)) {  // beyond fp16 (or not finite): no split images; fp32x3 requests are refused
    net->x3_range = std::isfinite(mx) ? mx : 1e300;
    return DMIP_OK;
  }
  std::vector<int> xt;
  for (int k = 0; k < net->xdim; ++k) xt.push_back(k);
  xt.push_back(IN - 1);
  std::vector<int> full;
  for (int k = 0; k < IN; ++k) full.push_back(k);
  const std::vector<uint16_t> l1 = pack_x3_l1(weights[0], W, IN, xt);
  std::vector<uint16_t> l1f;
  if (net->layout == DMIP_INPUT_X_Y_T) l1f = pack_x3_l1(weights[0], W, IN, full);
  std::vector<float> bias((size_t)L * W + 16, 0.0f);
  for (int u = 0; u < W; ++u) bias[u] = (float)(kC * (double)biases[0][u]);
  std::vector<char> stream;
  std::vector<uint16_t> img;
  // k-major engine (dmip_x3k.h): the same hi / lo fragments, a layer's chunk q = k-step q of all its
  // tiles ([o][q][p] -> [q][o][p])
  const bool kmajor = W == 256 && L == 3 && net->xdim >= 1 && net->xdim <= 4;
  const int KQ = W / 32;
  std::vector<char> kstream;
  for (int li = 1; li < L; ++li) {
    pack_x3_layer(weights[li], biases[li], W, W, ST, kC, img, bias.data() + (size_t)li * W);
    const char* b = (const char*)img.data();
    stream.insert(stream.end(), b, b + img.size() * 2);
    if (kmajor && li == 1)
      for (int q = 0; q < KQ; ++q)
        for (int o = 0; o < ST; ++o) {
          const char* f = b + (((size_t)o * KQ + q) * 2) * 1024;
          kstream.insert(kstream.end(), f, f + 2048);
        }
    if (kmajor && li == 2)  // two output halves, each k-major: chunk (h, q2) = k-steps 2 q2, 2 q2 + 1 of tiles 8h..8h+7
      for (int h = 0; h < 2; ++h)
        for (int q2 = 0; q2 < KQ / 2; ++q2)
          for (int kk = 0; kk < 2; ++kk)
            for (int o = 8 * h; o < 8 * h + 8; ++o) {
              const char* f = b + (((size_t)o * KQ + 2 * q2 + kk) * 2) * 1024;
              kstream.insert(kstream.end(), f, f + 2048);
            }
  }
  const int orows = OUT < 16 ? OUT : 16;  // the samplers read output rows 0..15 (the x rows)
  pack_x3_layer(weights[L], biases[L], orows, W, 1, 1.0, img, bias.data() + (size_t)L * W);
  std::vector<uint16_t> kout;
  if (kmajor) {  // one fragment per k-step: rows 0..D-1 the hi parts, rows 4..4+D-1 the lo parts
    const int D = net->xdim;
    kout.assign((size_t)KQ * 512, 0);
    for (int q = 0; q < KQ; ++q)
      for (int l = 0; l < 64; ++l) {
        const int i = l & 15, gg = l >> 4;
        int row = -1, part = 0;
        if (i < D) row = i, part = 0;
        else if (i >= 4 && i < 4 + D) row = i - 4, part = 1;
        if (row < 0) continue;
        for (int m = 0; m < 8; ++m)
          kout[((size_t)q * 64 + l) * 8 + m] = img[(((size_t)q * 2 + part) * 64 + row + 16 * gg) * 8 + m];
      }
  }
  std::vector<char> ochunk((size_t)chunk, 0);
  std::memcpy(ochunk.data(), img.data(), img.size() * 2);
  stream.insert(stream.end(), ochunk.begin(), ochunk.end());
  std::vector<char> l1b(l1.size() * 2), l1fb(l1f.size() * 2);
  std::memcpy(l1b.data(), l1.data(), l1b.size());
  if (!l1f.empty()) std::memcpy(l1fb.data(), l1f.data(), l1fb.size());
  int rc = DMIP_OK;
  if ((rc = upload(&net->x3_l1, l1b)) || (rc = upload(&net->x3_l1_full, l1fb)) || (rc = upload(&net->x3_stream, stream)) ||
      (rc = upload(&net->x3_bias, bias)))
    return rc;
  const int k1q_full = x3_k1q(IN);
  if (!l1f.empty() && ST * 1024 == chunk && ST * k1q_full * 1024 > 48 * 1024) {
    // the sampler streams this layer 1 through the ring (dmip_x3.h L1R): chunk q = k-step q of every tile
    std::vector<char> s1((size_t)k1q_full * chunk);
    for (int q = 0; q < k1q_full; ++q)
      for (int o = 0; o < ST; ++o)
        std::memcpy(s1.data() + ((size_t)q * ST + o) * 1024, l1fb.data() + ((size_t)o * k1q_full + q) * 1024, 1024);
    s1.insert(s1.end(), stream.begin(), stream.end());
    if ((rc = upload(&net->x3_stream_l1r, s1))) return rc;
  }
  if (kmajor) {
    std::vector<char> koutb(kout.size() * 2);
    std::memcpy(koutb.data(), kout.data(), koutb.size());
    if ((rc = upload(&net->x3k_stream, kstream)) || (rc = upload(&net->x3k_out, koutb))) return rc;
#ifdef DMIP_WITH_X3P
    if (net->xdim <= 4 && x3p_bias_range(net, weights, biases) <= 65504.0 &&
        (rc = pack_x3p(net, weights, biases, bias.data() + W, bias.data() + 2 * W)))
      return rc;
#endif
  }
  return DMIP_OK;
}

}  // namespace

extern "C" {

const char* dmip_last_error(void) { return g_err.c_str(); }

int dmip_device_status(void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int dev = dmip::stream_device(st);
  unsigned* w = status_word(dev);
  if (!w) return fail(DMIP_ERR_ALLOC, "device status word");
  unsigned* h = status_host(dev);
  hipError_t e = hipSuccess;
  unsigned v = 0;
  if (h) {  // the word's copy ordered after the stream's work, then one synchronise
    if ((e = hipMemcpyAsync(h, w, sizeof(unsigned), hipMemcpyDeviceToHost, st)) != hipSuccess)
      return hip_fail(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    v = *(volatile unsigned*)h;
  } else {
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    if ((e = hipMemcpy(&v, w, sizeof(unsigned), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "hipMemcpy");
  }
  if (v == 0) return DMIP_OK;
  (void)hipMemset(w, 0, sizeof(unsigned));
  if (v == dmip::kErrHandover)
    return fail(DMIP_ERR_HIP, "sampler: a split tile's hand-over never arrived (workgroups of the balanced schedule "
                              "were not co-resident); the affected chains were written as NaN");
  if (v == dmip::kErrRange)
    return fail(DMIP_ERR_HIP, "fp32x3 sampler: a chain's layer-1 input left the fp16 range of the split arithmetic "
                              "(|x| > 65504); those chains are not fp32-accurate (use DMIP_PREC_F32)");
  return fail(DMIP_ERR_HIP, "device status " + std::to_string(v));
}

int dmip_abi_version(void) { return DMIP_ABI_VERSION; }

#ifdef DMIP_WITH_X3P
// not ABI: present only in the A/B library (make diag), which also holds the paired-tile engine (DMIP_X3P=1)
int dmip_x3p_available(void) { return 1; }
#endif

int dmip_mlp_create(int in_dim, int out_dim, int n_hidden, const int* widths, int act_mode, int input_layout,
                    int xdim, const float* const* weights, const float* const* biases, dmip_mlp** out) {
  if (!out || !widths || !weights || !biases) return fail(DMIP_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_hidden < 1) return fail(DMIP_ERR_INVALID, "n_hidden must be >= 1");
  const int W = widths[0];
  for (int i = 1; i < n_hidden; ++i)
    if (widths[i] != W) return fail(DMIP_ERR_UNSUPPORTED, "hidden widths must all be equal");
  if (W % 32 != 0 || W < 32) return fail(DMIP_ERR_UNSUPPORTED, "hidden width must be a multiple of 32");
  if (out_dim < 1 || out_dim > 32) return fail(DMIP_ERR_UNSUPPORTED, "out_dim must be in [1, 32]");
  if (act_mode != DMIP_ACT_TANH_TWICE_FIRST && act_mode != DMIP_ACT_SILU_TWICE_FIRST)
    return fail(DMIP_ERR_UNSUPPORTED, "compiled activation chains: DMIP_ACT_TANH_TWICE_FIRST, DMIP_ACT_SILU_TWICE_FIRST");
  if (input_layout != DMIP_INPUT_X_Y_T && input_layout != DMIP_INPUT_X_T)
    return fail(DMIP_ERR_INVALID, "unknown input layout");
  if (xdim < 1 || xdim + 1 > in_dim) return fail(DMIP_ERR_INVALID, "xdim inconsistent with in_dim");
  if (input_layout == DMIP_INPUT_X_T && in_dim != xdim + 1)
    return fail(DMIP_ERR_INVALID, "X_T layout needs in_dim == xdim + 1");
  for (int i = 0; i <= n_hidden; ++i)
    if (!weights[i] || !biases[i]) return fail(DMIP_ERR_INVALID, "null layer pointer");

  dmip_mlp* net = new (std::nothrow) dmip_mlp;
  if (!net) return fail(DMIP_ERR_ALLOC, "host allocation");
  net->in_dim = in_dim;
  net->out_dim = out_dim;
  net->n_hidden = n_hidden;
  net->width = W;
  net->act_mode = act_mode;
  net->layout = input_layout;
  net->xdim = xdim;
  const int T = W / 32, KS = W / 16, L = n_hidden;

  // ---- hidden W x W layers (fp16 images). Input in r-form (after a single tanh): A = fp16(-2c W),
  // init = c b - 0.5 sum_k A. Input in t-form (the first W x W layer: layer 1's double tanh is
  // emitted as the value itself, dmip_device.h act_t_twice_pk_f16): A = fp16(c W), init = c b.
  std::vector<uint16_t> hid((size_t)(L - 1) * T * KS * 512);
  std::vector<float> bh((size_t)(L - 1) * T * 32);
  for (int li = 0; li < L - 1; ++li) {
    const float* Wl = weights[li + 1];
    const float* bl = biases[li + 1];
    const bool t_form = li == 0;
    std::vector<uint16_t> A((size_t)W * W);
    std::vector<float> init(W);
    for (int r = 0; r < W; ++r) {
      double acc = 0.0;
      for (int k = 0; k < W; ++k) {
        const float v = (float)((t_form ? 1.0 : -2.0) * kC * (double)Wl[(size_t)r * W + k]);
        const uint16_t a = f2h(v);
        A[(size_t)r * W + k] = a;
        acc += (double)h2f(a);
      }
      init[r] = (float)(kC * (double)bl[r] - (t_form ? 0.0 : 0.5 * acc));
    }
    for (int rt = 0; rt < T; ++rt)
      for (int s = 0; s < KS; ++s)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j) {
            const int i = l & 31, h = l >> 5;
            hid[(((size_t)(li * T + rt) * KS + s) * 64 + l) * 8 + j] = A[(size_t)(rt * 32 + i) * W + kperm(s, h, j)];
          }
    for (int rt = 0; rt < T; ++rt)
      for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) bh[((size_t)(li * T + rt) * 2 + h) * 16 + r] = init[rt * 32 + acc_row(r, h)];
  }

  // ---- output layer (fp16 image): A = fp16(-2 W), init = b - 0.5 sum_k A (no tanh scale: raw
  // drift a); t-form input (L == 1: directly after layer 1's double tanh): A = fp16(W), init = b
  const float* Wo = weights[L];
  const float* bo = biases[L];
  const bool out_t_form = L == 1;
  std::vector<uint16_t> Ao((size_t)out_dim * W);
  std::vector<float> init_o(out_dim);
  for (int d = 0; d < out_dim; ++d) {
    double acc = 0.0;
    for (int k = 0; k < W; ++k) {
      const float v = (float)((out_t_form ? 1.0 : -2.0) * (double)Wo[(size_t)d * W + k]);
      const uint16_t a = f2h(v);
      Ao[(size_t)d * W + k] = a;
      acc += (double)h2f(a);
    }
    init_o[d] = (float)((double)bo[d] - (out_t_form ? 0.0 : 0.5 * acc));
  }
  std::vector<uint16_t> ao_s((size_t)KS * 512, 0), ao_f((size_t)KS * 512, 0);
  std::vector<float> bo_s(32, 0.0f), bo_f(32, 0.0f);
  for (int s = 0; s < KS; ++s)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j) {
        const int i = l & 31, h = l >> 5;
        const int ds = i < 4 ? i : (i < 8 ? i - 4 : -1);  // sampler: rows 0-3 duplicated at 4-7
        if (ds >= 0 && ds < out_dim) ao_s[((size_t)s * 64 + l) * 8 + j] = Ao[(size_t)ds * W + kperm(s, h, j)];
        if (i < out_dim) ao_f[((size_t)s * 64 + l) * 8 + j] = Ao[(size_t)i * W + kperm(s, h, j)];
      }
  for (int h = 0; h < 2; ++h)
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, h);
      const int ds = row < 4 ? row : (row < 8 ? row - 4 : -1);
      if (ds >= 0 && ds < out_dim) bo_s[h * 16 + r] = init_o[ds];
      if (row < out_dim) bo_f[h * 16 + r] = init_o[row];
    }

  // ---- layer 1, forward variant: every column varying, split bf16 [hi | hi | lo | b_hi | b_lo]
  const float* W1 = weights[0];
  const float* b1 = biases[0];
  const int IN = in_dim;
  const bool split = dmip::forward_split(W, IN);
  net->k1s_full = split ? k1s_for(3 * IN + 2) : k1s_for(IN + 2);
  auto pack_a1 = [&](bool split, int K1S) {
  std::vector<uint16_t> a1f((size_t)T * K1S * 512, 0);
  for (int jr = 0; jr < W; ++jr) {
    const int rt = jr / 32, i = jr % 32;
    for (int k = 0; k < K1S * 16; ++k) {
      float val = 0.0f;
      auto hilo = [&](double v, bool lo) {
        const float f = (float)v;
        const uint16_t hi = f2bf(f);
        return lo ? bf2f(f2bf(f - bf2f(hi))) : bf2f(hi);
      };
      if (split) {
        if (k < IN) val = hilo(kC * W1[(size_t)jr * IN + k], false);
        else if (k < 2 * IN) val = hilo(kC * W1[(size_t)jr * IN + k - IN], false);
        else if (k < 3 * IN) val = hilo(kC * W1[(size_t)jr * IN + k - 2 * IN], true);
        else if (k == 3 * IN) val = hilo(kC * b1[jr], false);
        else if (k == 3 * IN + 1) val = hilo(kC * b1[jr], true);
      } else {  // [v | 1 | 1] x [W | b_hi | b_lo]
        if (k < IN) val = hilo(kC * W1[(size_t)jr * IN + k], false);
        else if (k == IN) val = hilo(kC * b1[jr], false);
        else if (k == IN + 1) val = hilo(kC * b1[jr], true);
      }
      const int s = k / 16, hh = (k % 16) / 8, jj = k % 8;
      a1f[(((size_t)(rt * K1S + s)) * 64 + i + 32 * hh) * 8 + jj] = f2bf(val);
    }
  }
  return a1f;
  };
  const std::vector<uint16_t> a1f = pack_a1(split, net->k1s_full);

  int rc = DMIP_OK;
  if (input_layout == DMIP_INPUT_X_T && xdim == 3 && in_dim == 4 && out_dim == 3 && L == 3 && W == dmip::kDpsPriorW) {
    // exact-f32 images for the DPS sampler's prior (dmip_surrogate.hip dps_kernel)
    const float *P1 = weights[0], *P2 = weights[1], *P3 = weights[2], *P4 = weights[3];
    std::vector<float> l1((size_t)16 * 2 * 64), pb((size_t)2 * W + 16, 0.0f);
    for (int o = 0; o < 16; ++o)
      for (int l = 0; l < 64; ++l) {
        const int row = 16 * o + (l & 15), g = l >> 4;
        l1[((size_t)o * 2 + 0) * 64 + l] = P1[(size_t)row * 4 + g];
        l1[((size_t)o * 2 + 1) * 64 + l] = g == 0 ? biases[0][row] : 0.0f;
      }
    for (int k = 0; k < W; ++k) pb[k] = biases[1][k], pb[W + k] = biases[2][k];
    for (int k = 0; k < 3; ++k) pb[2 * W + k] = biases[3][k];
    const auto sqm = [W](const float* Wm) { return [Wm, W](int r, int c) { return Wm[(size_t)r * W + c]; }; };
    if ((rc = upload(&net->dps_l1, l1)) || (rc = upload(&net->dps_bias, pb)) ||
        (rc = upload(&net->dps_w2, pack_f32_tiles(16, 16, sqm(P2)))) ||
        (rc = upload(&net->dps_w3, pack_f32_tiles(16, 16, sqm(P3)))) ||
        (rc = upload(&net->dps_w4, pack_f32_tiles(1, 16, [&](int r, int c) { return r < 3 ? P4[(size_t)r * W + c] : 0.0f; }))) ||
        (rc = pack_dps_x3_prior(net, weights, biases))) {
      delete net;
      return rc;
    }
  }
  std::vector<char> hid_b(hid.size() * 2), ao_sb(ao_s.size() * 2), ao_fb(ao_f.size() * 2), a1f_b(a1f.size() * 2);
  std::memcpy(hid_b.data(), hid.data(), hid_b.size());
  std::memcpy(ao_sb.data(), ao_s.data(), ao_sb.size());
  std::memcpy(ao_fb.data(), ao_f.data(), ao_fb.size());
  std::memcpy(a1f_b.data(), a1f.data(), a1f_b.size());
  // the output image also follows the hidden chunks in one buffer: the two-network sampler at width 512
  // streams it through the weight ring as the network's last chunk (dmip_kernels.hip Lay<AOR>)
  hid_b.insert(hid_b.end(), ao_sb.begin(), ao_sb.end());
  // the CDiffE sampler at width 512 streams its split layer 1 (3 in + 2 slots, 6 KiB per row tile at
  // in_dim 27) through the ring as well: [ceil(T / TPC) layer-1 chunks of TPC row tiles | hidden | output]
  // (dmip_kernels.hip Lay<L1R>)
  std::vector<char> ring_b;
  if (W == 512 && input_layout == DMIP_INPUT_X_Y_T) {
    const int k1s = k1s_for(3 * IN + 2), chunk = (W / 16) * 1024, tpc = chunk / (k1s * 1024);
    if (tpc >= 1) {
      const std::vector<uint16_t> a1s = pack_a1(true, k1s);
      const int l1c = (T + tpc - 1) / tpc;
      ring_b.assign((size_t)l1c * chunk, 0);
      for (int rt = 0; rt < T; ++rt)
        std::memcpy(ring_b.data() + (size_t)(rt / tpc) * chunk + (size_t)(rt % tpc) * k1s * 1024,
                    (const char*)a1s.data() + (size_t)rt * k1s * 1024, (size_t)k1s * 1024);
      ring_b.insert(ring_b.end(), hid_b.begin(), hid_b.end());
    }
  }
  std::vector<float> w1v(W1, W1 + (size_t)W * IN), b1v(b1, b1 + W);
  if (!ring_b.empty() && (rc = upload(&net->ring_l1, ring_b))) {
    delete net;
    return rc;
  }
  if ((rc = upload(&net->hidden, hid_b)) || (rc = upload(&net->ao_samp, ao_sb)) || (rc = upload(&net->ao_full, ao_fb)) ||
      (rc = upload(&net->bias_hidden, bh)) || (rc = upload(&net->bias_out_samp, bo_s)) ||
      (rc = upload(&net->bias_out_full, bo_f)) || (rc = upload(&net->a1_full, a1f_b)) ||
      (rc = upload(&net->w1, w1v)) || (rc = upload(&net->b1, b1v)) || (rc = pack_f32_net(net, weights, biases)) ||
      (rc = pack_x3_net(net, weights, biases))) {
    delete net;
    return rc;
  }
  *out = net;
  return DMIP_OK;
}

int dmip_mlp_destroy(dmip_mlp* net) {
  delete net;
  return DMIP_OK;
}

int dmip_mlp_forward(const dmip_mlp* net, const float* x_dev, const float* y_dev, int64_t y_stride,
                     const float* t_dev, int t_stride, int64_t n, float* out_dev, int precision, void* stream) {
  if (!net || !x_dev || !t_dev || !out_dev) return fail(DMIP_ERR_INVALID, "null argument");
  if (precision != DMIP_PREC_FP16 && precision != DMIP_PREC_F32 && precision != DMIP_PREC_F32X3)
    return fail(DMIP_ERR_INVALID, "unknown precision");
  if (n < 0) return fail(DMIP_ERR_INVALID, "n < 0");
  if (n == 0) return DMIP_OK;
  const int ydim = net->layout == DMIP_INPUT_X_Y_T ? net->in_dim - net->xdim - 1 : 0;
  if (ydim > 0 && !y_dev) return fail(DMIP_ERR_INVALID, "y required for an X_Y_T network");
  if (ydim > 0 && y_stride != 0 && y_stride != ydim) return fail(DMIP_ERR_INVALID, "y_stride must be 0 or ydim");
  if (t_stride != 0 && t_stride != 1) return fail(DMIP_ERR_INVALID, "t_stride must be 0 or 1");
  if (precision == DMIP_PREC_F32 || precision == DMIP_PREC_F32X3) {  // F32X3: the exact-f32 forward (fp32 either way)
    dmip::F32ForwardParams q{};
    q.net = f32_net(net);
    q.n_hidden = net->n_hidden;
    q.x = x_dev;
    q.y = y_dev;
    q.t = t_dev;
    q.out = out_dev;
    q.n = n;
    q.y_stride = y_stride;
    q.t_stride = t_stride;
    q.xdim = net->xdim;
    q.ydim = ydim;
    q.out_dim = net->out_dim;
    q.k1q = net->f32_k1q;
    q.act = f32_act(net);
    bool ok = false;
    hipError_t e = dmip::launch_f32_forward(q, net->width, net->f32_ot, (hipStream_t)stream, &ok);
    if (!ok)
      return fail(DMIP_ERR_UNSUPPORTED, "no compiled f32 forward kernel for width " + std::to_string(net->width) +
                                            ", layers " + std::to_string(net->n_hidden) + ", in_dim " +
                                            std::to_string(net->in_dim) + ", out_dim " + std::to_string(net->out_dim));
    if (e != hipSuccess) return hip_fail(e, "mlp_forward (f32) launch");
    return DMIP_OK;
  }
  if (f32_act(net)) return act_refused("mlp_forward at DMIP_PREC_FP16");
  dmip::ForwardParams p{};
  p.hidden = net->hidden;
  p.a1 = net->a1_full;
  p.ao = net->ao_full;
  p.bias_hidden = net->bias_hidden;
  p.bias_out = net->bias_out_full;
  p.x = x_dev;
  p.y = y_dev;
  p.t = t_dev;
  p.out = out_dev;
  p.n = n;
  p.y_stride = y_stride;
  p.t_stride = t_stride;
  p.xdim = net->xdim;
  p.ydim = ydim;
  p.out_dim = net->out_dim;
  bool ok = false;
  hipError_t e = dmip::launch_forward(p, net->width, net->n_hidden, net->in_dim, (hipStream_t)stream, &ok);
  if (!ok) return fail(DMIP_ERR_UNSUPPORTED, "no compiled forward kernel for width " + std::to_string(net->width) +
                                                 ", layers " + std::to_string(net->n_hidden) + ", in_dim " +
                                                 std::to_string(net->in_dim));
  if (e != hipSuccess) return hip_fail(e, "mlp_forward launch");
  return DMIP_OK;
}

int dmip_surrogate_create(int in_dim, int out_dim, int n_hidden, const int* widths, const float* const* weights,
                          const float* const* biases, dmip_surrogate** out) {
  using dmip::kSurW;
  if (!out || !widths || !weights || !biases) return fail(DMIP_ERR_INVALID, "null argument");
  *out = nullptr;
  if (in_dim != dmip::kSurXdim || out_dim != dmip::kSurYdim || n_hidden != 3)
    return fail(DMIP_ERR_UNSUPPORTED, "surrogate compiled for in 3, out 23, 3 hidden layers");
  for (int i = 0; i < 3; ++i)
    if (widths[i] != kSurW) return fail(DMIP_ERR_UNSUPPORTED, "surrogate compiled for hidden widths [256]*3");
  for (int i = 0; i < 4; ++i)
    if (!weights[i] || !biases[i]) return fail(DMIP_ERR_INVALID, "null layer pointer");
  const float *W1 = weights[0], *W2 = weights[1], *W3 = weights[2], *W4 = weights[3];
  const int XD = dmip::kSurXdim, YD = dmip::kSurYdim;
  auto sq = [](const float* Wm) {
    return [Wm](int r, int c) { return Wm[(size_t)r * kSurW + c]; };
  };
  auto tr = [](const float* Wm) {
    return [Wm](int r, int c) { return Wm[(size_t)c * kSurW + r]; };
  };
  std::vector<char> imgs[7] = {
      pack_f32_tiles(16, 16, sq(W2)),
      pack_f32_tiles(16, 16, sq(W3)),
      pack_f32_tiles(2, 16, [&](int r, int c) { return r < YD ? W4[(size_t)r * kSurW + c] : 0.0f; }),
      pack_f32_tiles(16, 16, tr(W3)),
      pack_f32_tiles(16, 16, tr(W2)),
      pack_f32_tiles(16, 2, [&](int r, int c) { return c < YD ? W4[(size_t)c * kSurW + r] : 0.0f; }),
      pack_f32_tiles(1, 16, [&](int r, int c) { return r < XD ? W1[(size_t)c * XD + r] : 0.0f; }),
  };
  std::vector<float> l1((size_t)16 * 64), bias((size_t)3 * kSurW + 32, 0.0f);
  for (int o = 0; o < 16; ++o)
    for (int l = 0; l < 64; ++l) {
      const int row = 16 * o + (l & 15), g = l >> 4;
      l1[(size_t)o * 64 + l] = g < XD ? W1[(size_t)row * XD + g] : biases[0][row];
    }
  for (int li = 0; li < 3; ++li)
    for (int k = 0; k < kSurW; ++k) bias[(size_t)li * kSurW + k] = biases[li][k];
  for (int k = 0; k < YD; ++k) bias[(size_t)3 * kSurW + k] = biases[3][k];

  dmip_surrogate* s = new (std::nothrow) dmip_surrogate;
  if (!s) return fail(DMIP_ERR_ALLOC, "host allocation");
  int rc = DMIP_OK;
  if ((rc = upload(&s->l1, l1)) || (rc = upload(&s->bias, bias))) {
    delete s;
    return rc;
  }
  for (int i = 0; i < 7; ++i)
    if ((rc = upload(&s->img[i], imgs[i]))) {
      delete s;
      return rc;
    }
  {  // the fp32x3 DPS engine's images (plain splits; the surrogate is ReLU, no folds)
    double mx = 0.0;
    std::vector<char> chunks;
    append_chunks(chunks, pack_x3_plain(16, 8, [&](int r, int c) { return W2[(size_t)r * kSurW + c]; }, &mx));
    append_chunks(chunks, pack_x3_plain(16, 8, [&](int r, int c) { return W3[(size_t)r * kSurW + c]; }, &mx));
    append_chunks(chunks, pack_x3_plain(2, 8, [&](int r, int c) { return r < YD ? W4[(size_t)r * kSurW + c] : 0.0f; }, &mx));
    append_chunks(chunks, pack_x3_plain(16, 1, [&](int r, int c) { return c < YD ? W4[(size_t)c * kSurW + r] : 0.0f; }, &mx));
    append_chunks(chunks, pack_x3_plain(16, 8, [&](int r, int c) { return W3[(size_t)c * kSurW + r]; }, &mx));
    append_chunks(chunks, pack_x3_plain(16, 8, [&](int r, int c) { return W2[(size_t)c * kSurW + r]; }, &mx));
    append_chunks(chunks, pack_x3_plain(1, 8, [&](int r, int c) { return r < XD ? W1[(size_t)c * XD + r] : 0.0f; }, &mx));
    for (size_t i = 0; i < (size_t)kSurW * XD; ++i) mx = std::max(mx, std::fabs((double)W1[i]));
    if (!(mx <= 65504.0) || chunks.size() != (size_t)dmip::kDpsX3SurChunks * dmip::kDpsX3Chunk) {
      s->x3_range = std::isfinite(mx) ? mx : 1e300;
    } else {
      const std::vector<uint16_t> l1x = pack_x3_l1(W1, kSurW, XD, {0, 1, 2}, 1.0);
      std::vector<char> l1b(l1x.size() * 2);
      std::memcpy(l1b.data(), l1x.data(), l1b.size());
      if ((rc = upload(&s->x3_img, chunks)) || (rc = upload(&s->x3_l1, l1b)) || (rc = upload(&s->x3_bias, bias))) {
        delete s;
        return rc;
      }
    }
  }
  *out = s;
  return DMIP_OK;
}

int dmip_surrogate_destroy(dmip_surrogate* s) {
  delete s;
  return DMIP_OK;
}

}  // extern "C"
