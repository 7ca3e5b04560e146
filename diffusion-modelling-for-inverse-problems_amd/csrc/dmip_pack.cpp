// Host-side weight packing (dmip_pack.h): one packer per engine, each stated once.
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
#include "dmip_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/dmip.h"
#include "dmip_internal.h"

namespace dmip_pack {
namespace {

constexpr double kC = 2.8853900817779268;  // 2 log2(e)
constexpr double kHalfMax = 65504.0;       // the largest finite fp16

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

// v = hi + lo in fp16 (hi = fp16(v), lo = fp16(v - hi))
void split_h(double v, uint16_t& hi, uint16_t& lo) {
  hi = f2h((float)v);
  lo = f2h((float)(v - (double)h2f(hi)));
}

template <typename T>
void append(std::vector<T>& out, const std::vector<T>& img) {
  out.insert(out.end(), img.begin(), img.end());
}

// append an fp16 image to a chunk stream, zero-padded to whole 32 KiB chunks
void append_chunks(Img16& out, const Img16& img) {
  const size_t chunk = dmip::kDpsX3Chunk / 2;
  append(out, img);
  out.resize(out.size() + (chunk - img.size() % chunk) % chunk, 0);
}

// the largest |fp16| of an image, or mx if that is larger
double max_abs_h(const Img16& img, double mx) {
  for (uint16_t h : img) mx = std::max(mx, std::fabs((double)h2f(h)));
  return mx;
}

// the magnitude a refused fp16 split reports (x3_range, dps_x3_range)
double range_of(double mx) { return std::isfinite(mx) ? mx : 1e300; }

// hidden unit of element j, lane half h, k-step s of a 32x32x16 fragment: k-step s covers the previous layer's
// accumulator registers 8 (s & 1) .. + 7 of its output tile s >> 1 (the 16-bit engine and the paired fp32x3 engine)
inline int kperm(int s, int h, int j) { return 32 * (s >> 1) + 16 * (s & 1) + 8 * (j >> 2) + 4 * h + (j & 3); }
inline int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- the 16-bit engine (dmip_kernels.hip)

// One layer's fold. Input in r-form (after a single tanh): A = fp16(-2 scale W), init = scale b - 0.5 sum_k A.
// Input in t-form (directly after layer 1's double tanh, emitted as the value itself, dmip_device.h
// act_t_twice_pk_f16): A = fp16(scale W), init = scale b. scale = c for a tanh layer, 1 for the output (raw drift).
void fold_16bit(const float* Wl, const float* bl, int n_rows, int W, double scale, bool t_form, Img16& A, ImgF& init) {
  A.resize((size_t)n_rows * W);
  init.resize(n_rows);
  for (int r = 0; r < n_rows; ++r) {
    double acc = 0.0;
    for (int k = 0; k < W; ++k) {
      const uint16_t a = f2h((float)((t_form ? 1.0 : -2.0) * scale * (double)Wl[(size_t)r * W + k]));
      A[(size_t)r * W + k] = a;
      acc += (double)h2f(a);
    }
    init[r] = (float)(scale * (double)bl[r] - (t_form ? 0.0 : 0.5 * acc));
  }
}

// layer 1 as [W/32][K1S] fragment blocks in split bf16: slots [hi | hi | lo | b_hi | b_lo] over the columns when
// `split` (the kernel's B = [v_hi | v_lo | v_hi | 1 | 1]), else [W | b_hi | b_lo] against [v | 1 | 1]
Img16 pack_a1(const float* W1, const float* b1, int W, int IN, bool split, int K1S) {
  Img16 a1((size_t)(W / 32) * K1S * 512, 0);
  const int NW = split ? 3 * IN : IN;  // the weight slots
  const auto hilo = [](double v, bool lo) {
    const float f = (float)v;
    const uint16_t hi = f2bf(f);
    return lo ? bf2f(f2bf(f - bf2f(hi))) : bf2f(hi);
  };
  for (int jr = 0; jr < W; ++jr) {
    const int rt = jr / 32, i = jr % 32;
    for (int k = 0; k < K1S * 16; ++k) {
      float val = 0.0f;
      if (k < NW) val = hilo(kC * W1[(size_t)jr * IN + k % IN], k >= 2 * IN);
      else if (k <= NW + 1) val = hilo(kC * b1[jr], k == NW + 1);
      const int s = k / 16, hh = (k % 16) / 8, jj = k % 8;
      a1[(((size_t)(rt * K1S + s)) * 64 + i + 32 * hh) * 8 + jj] = f2bf(val);
    }
  }
  return a1;
}

void pack_16bit(const MlpDesc& d, const float* const* weights, const float* const* biases, MlpImages& im) {
  const int W = d.width, L = d.n_hidden, IN = d.in_dim, OUT = d.out_dim, T = W / 32, KS = W / 16;
  Img16 A;
  ImgF init;
  im.hidden.resize((size_t)(L - 1) * T * KS * 512);
  im.bias_hidden.resize((size_t)(L - 1) * T * 32);
  for (int li = 0; li < L - 1; ++li) {  // the W x W layers; the first one reads layer 1's t-form
    fold_16bit(weights[li + 1], biases[li + 1], W, W, kC, li == 0, A, init);
    for (int rt = 0; rt < T; ++rt)
      for (int s = 0; s < KS; ++s)
        for (int l = 0; l < 64; ++l)
          for (int j = 0; j < 8; ++j)
            im.hidden[(((size_t)(li * T + rt) * KS + s) * 64 + l) * 8 + j] =
                A[(size_t)(rt * 32 + (l & 31)) * W + kperm(s, l >> 5, j)];
    for (int rt = 0; rt < T; ++rt)
      for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r)
          im.bias_hidden[((size_t)(li * T + rt) * 2 + h) * 16 + r] = init[rt * 32 + acc_row(r, h)];
  }
  fold_16bit(weights[L], biases[L], OUT, W, 1.0, L == 1, A, init);
  im.ao_samp.assign((size_t)KS * 512, 0);
  im.ao_full.assign((size_t)KS * 512, 0);
  im.bias_out_samp.assign(32, 0.0f);
  im.bias_out_full.assign(32, 0.0f);
  const auto samp_row = [](int i) { return i < 4 ? i : (i < 8 ? i - 4 : -1); };  // sampler: rows 0-3 duplicated at 4-7
  for (int s = 0; s < KS; ++s)
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < 8; ++j) {
        const int i = l & 31, ds = samp_row(i), k = kperm(s, l >> 5, j);
        if (ds >= 0 && ds < OUT) im.ao_samp[((size_t)s * 64 + l) * 8 + j] = A[(size_t)ds * W + k];
        if (i < OUT) im.ao_full[((size_t)s * 64 + l) * 8 + j] = A[(size_t)i * W + k];
      }
  for (int h = 0; h < 2; ++h)
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, h), ds = samp_row(row);
      if (ds >= 0 && ds < OUT) im.bias_out_samp[h * 16 + r] = init[ds];
      if (row < OUT) im.bias_out_full[h * 16 + r] = init[row];
    }
  // the output image also follows the hidden chunks in one buffer: the two-network sampler at width 512
  // streams it through the weight ring as the network's last chunk (dmip_kernels.hip Lay<AOR>)
  append(im.hidden, im.ao_samp);

  // layer 1, forward variant: every column varying
  const bool split = dmip::forward_split(W, IN);
  im.k1s_full = split ? k1s_for(3 * IN + 2) : k1s_for(IN + 2);
  im.a1_full = pack_a1(weights[0], biases[0], W, IN, split, im.k1s_full);
  // the CDiffE sampler at width 512 streams its split layer 1 (3 in + 2 slots, 6 KiB per row tile at
  // in_dim 27) through the ring as well: [ceil(T / TPC) layer-1 chunks of TPC row tiles | hidden | output]
  // (dmip_kernels.hip Lay<L1R>)
  const int k1s = k1s_for(3 * IN + 2), chunk = KS * 512, tpc = chunk / (k1s * 512);
  if (W == 512 && d.layout == DMIP_INPUT_X_Y_T && tpc >= 1) {
    const Img16 a1s = pack_a1(weights[0], biases[0], W, IN, true, k1s);
    im.ring_l1.assign((size_t)((T + tpc - 1) / tpc) * chunk, 0);
    for (int rt = 0; rt < T; ++rt)
      std::copy_n(a1s.begin() + (size_t)rt * k1s * 512, (size_t)k1s * 512,
                  im.ring_l1.begin() + (size_t)(rt / tpc) * chunk + (size_t)(rt % tpc) * k1s * 512);
    append(im.ring_l1, im.hidden);
  }
  im.w1.assign(weights[0], weights[0] + (size_t)W * IN);
  im.b1.assign(biases[0], biases[0] + W);
}

// ---- exact-f32 images (dmip_f32.h FEngine, dmip_surrogate.hip)

// f32 A-fragment images for v_mfma_f32_16x16x4_f32: k-step (q, r) of output tile o, lane l = i + 16 g, holds
// M[16 o + i][16 q + 4 g + r]; stored [o][q][lane][r] (one float4 per lane per q). M(row, col) returns 0 outside
// the matrix.
template <typename F>
ImgF pack_f32_tiles(int n_tiles, int n_q, F M) {
  ImgF v((size_t)n_tiles * n_q * 64 * 4);
  for (int o = 0; o < n_tiles; ++o)
    for (int q = 0; q < n_q; ++q)
      for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r)
          v[(((size_t)o * n_q + q) * 64 + l) * 4 + r] = M(16 * o + (l & 15), 16 * q + 4 * (l >> 4) + r);
  return v;
}

// rows < n_rows of a [.][W] matrix, and its transpose
auto rows_of(const float* M, int W, int n_rows) {
  return [=](int r, int c) { return r < n_rows ? M[(size_t)r * W + c] : 0.0f; };
}
auto cols_of(const float* M, int W, int n_rows) {
  return [=](int r, int c) { return c < n_rows ? M[(size_t)c * W + r] : 0.0f; };
}

// a network's exact-f32 images: layer 1 over every input column then the bias column; the W x W layers and the
// output layer as 16-row chunks in stream order; the biases
void pack_f32_net(const MlpDesc& d, const float* const* weights, const float* const* biases, MlpImages& im) {
  const int W = d.width, L = d.n_hidden, IN = d.in_dim, OUT = d.out_dim, ST = W / 16;
  const int K1Q = im.f32_k1q = (IN + 1 + 3) / 4, OT = im.f32_ot = (OUT + 15) / 16;
  im.f32_l1.resize((size_t)ST * K1Q * 64);
  for (int o = 0; o < ST; ++o)
    for (int s = 0; s < K1Q; ++s)
      for (int l = 0; l < 64; ++l) {
        const int u = 16 * o + (l & 15), c = 4 * s + (l >> 4);
        im.f32_l1[((size_t)o * K1Q + s) * 64 + l] =
            c < IN ? weights[0][(size_t)u * IN + c] : (c == IN ? biases[0][u] : 0.0f);
      }
  for (int li = 1; li < L; ++li) append(im.f32_stream, pack_f32_tiles(ST, ST, rows_of(weights[li], W, W)));
  append(im.f32_stream, pack_f32_tiles(OT, ST, rows_of(weights[L], W, OUT)));
  im.f32_bias.assign((size_t)(L - 1) * W + 16 * OT, 0.0f);
  for (int li = 1; li < L; ++li) std::copy_n(biases[li], W, im.f32_bias.begin() + (size_t)(li - 1) * W);
  std::copy_n(biases[L], OUT, im.f32_bias.begin() + (size_t)(L - 1) * W);
}

// ---- fp32-accurate split-fp16 images (DMIP_PREC_F32X3, dmip_x3.h). A 16x16x32 f16 fragment block:
// lane l = i + 16 g holds A[row i][k-slot 8 g + m], m = 0..7. Hidden-layer k-slots follow the previous
// layer's accumulator tiles: slot (q, g, m) is unit kperm16(q, g, m).
inline int kperm16(int q, int g, int m) { return 32 * q + 16 * (m >> 2) + 4 * g + (m & 3); }
inline int x3_k1q(int nv) { return (3 * nv + 31) / 32; }

// [n_tiles][KQ][hi, lo][64][8] fp16 split of A[r][c] = get(r, c): lane i + 16 g of tile o holds A[16 o + i][kperm16(q,
// g, m)], m = 0..7 -- pack_x3_layer's layout without its r-form fold (the DPS engine's plain and transposed layers).
// *maxabs: the largest |A| (the split needs it inside fp16's range)
template <typename Get>
Img16 pack_x3_plain(int n_tiles, int KQ, Get get, double* maxabs) {
  Img16 img((size_t)n_tiles * KQ * 2 * 512, 0);
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

// layer-1 image over the first n_cols input columns, then column `last` when it is >= 0 (scaled by `scale`): input n
// at k-slots 3n, 3n+1, 3n+2 with A = [W_hi, W_hi, W_lo] (the kernel's B = [v_hi, v_lo, v_hi])
Img16 pack_x3_l1(const float* W1, int W, int in_dim, int n_cols, int last = -1, double scale = kC) {
  const int NV = n_cols + (last >= 0), K1Q = x3_k1q(NV), ST = W / 16;
  Img16 img((size_t)ST * K1Q * 512, 0);
  for (int o = 0; o < ST; ++o)
    for (int q = 0; q < K1Q; ++q)
      for (int l = 0; l < 64; ++l)
        for (int m = 0; m < 8; ++m) {
          const int i = l & 15, g = l >> 4, s = 32 * q + 8 * g + m, n = s / 3, p = s % 3;
          if (n >= NV) continue;
          uint16_t hi, lo;
          split_h(scale * (double)W1[(size_t)(16 * o + i) * in_dim + (n < n_cols ? n : last)], hi, lo);
          img[(((size_t)o * K1Q + q) * 64 + l) * 8 + m] = p < 2 ? hi : lo;
        }
  return img;
}

// [n_tiles][KQ][2][64][8] image of an r-form-input layer: A = scale * (-2 W), init = scale b - 0.5 sum_k A
// (with A = hi + lo as the kernel applies it); rows >= n_rows zero
void pack_x3_layer(const float* Wl, const float* bl, int n_rows, int W, int n_tiles, double scale, Img16& img,
                   float* init) {
  const int KQ = W / 32;
  img.assign((size_t)n_tiles * KQ * 2 * 512, 0);
  Img16 hi((size_t)n_rows * W), lo((size_t)n_rows * W);
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

// largest magnitude the fp32x3 images would hold in fp16: layer 1 scaled by 2 log2(e), the hidden layers by
// -2 * 2 log2(e), the output rows by -2 (r-form folds). The folded hidden biases stay f32 (x3_bias) in the
// product engines, so they do not limit them (only the A/B paired engine stores them in fp16: x3p_bias_range)
double x3_max_scaled(const MlpDesc& d, const float* const* weights) {
  const int W = d.width, L = d.n_hidden;
  double m = 0.0;
  for (size_t i = 0; i < (size_t)W * d.in_dim; ++i) m = std::max(m, kC * std::fabs((double)weights[0][i]));
  for (int li = 1; li < L; ++li)
    for (size_t i = 0; i < (size_t)W * W; ++i) m = std::max(m, 2.0 * kC * std::fabs((double)weights[li][i]));
  for (size_t i = 0; i < (size_t)std::min(d.out_dim, 16) * W; ++i) m = std::max(m, 2.0 * std::fabs((double)weights[L][i]));
  return m;
}

#ifdef DMIP_WITH_X3P
// the paired engine's fp16 folded hidden biases kC (b + sum_k W) (pack_x3p): their largest magnitude
double x3p_bias_range(const MlpDesc& d, const float* const* weights, const float* const* biases) {
  const int W = d.width;
  double m = 0.0;
  for (int li = 1; li < d.n_hidden; ++li)
    for (int r = 0; r < W; ++r) {
      double acc = (double)biases[li][r];
      for (int k = 0; k < W; ++k) acc += (double)weights[li][(size_t)r * W + k];
      m = std::max(m, kC * std::fabs(acc));
    }
  return m;
}

// the paired-tile engine's images of a [256]*3 CDE (dmip_x3p.h): the same hi / lo split and folded scales as
// pack_x3_layer / pack_x3_l1 in the 32x32x16 fragment layout (lane l = i + 32 h holds A[row i][k-slot 8 h + j], hidden
// k-slots by kperm); hidden layer 1's bias (`init1`, already folded) and hidden layer 2's (`init2`: the folded inits
// of pack_x3_layer) as three-part fp16 A fragments per output tile; the output layer in f32 (r-form fold: A = -2 W,
// init = b + sum_k W, in double)
void pack_x3p(const MlpDesc& d, const float* const* weights, const float* const* biases, const float* init1,
              const float* init2, MlpImages& im) {
  const int W = d.width, IN = d.in_dim, D = d.xdim, OT = W / 32, KS = W / 16, NV = D + 1;
  Img16& l1 = im.x3p_l1;
  l1.assign((size_t)3 * OT * 512, 0);
  for (int o = 0; o < OT; ++o)
    for (int l = 0; l < 64; ++l) {
      const int i = l & 31, h = l >> 5;
      for (int j = 0; j < 8; ++j) {
        const int sl = 8 * h + j, n = sl / 3, pt = sl % 3;
        if (n >= NV) continue;
        uint16_t hi, lo;
        split_h(kC * (double)weights[0][(size_t)(32 * o + i) * IN + (n < D ? n : IN - 1)], hi, lo);
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
  Img16 hi((size_t)W * W), lo((size_t)W * W);
  for (int li = 1; li <= 2; ++li) {
    for (size_t i = 0; i < (size_t)W * W; ++i) split_h(-2.0 * kC * (double)weights[li][i], hi[i], lo[i]);
    // hidden layer 1 k-major: chunk q, output tile o, k-step half e; hidden layer 2 output-major: chunk c, k-step s
    for (int a = 0; a < OT; ++a)
      for (int b = 0; b < KS; ++b)
        for (int pt = 0; pt < 2; ++pt)
          for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j) {
              const int row = li == 1 ? 32 * (b >> 1) + (l & 31) : 32 * a + (l & 31);
              const int s = li == 1 ? 2 * a + (b & 1) : b;
              const size_t src = (size_t)row * W + kperm(s, l >> 5, j);
              im.x3p_stream.push_back(pt == 0 ? hi[src] : lo[src]);
            }
  }
  ImgF& ow = im.x3p_ow;
  ow.assign((size_t)OT * 2 * 64 + 16, 0.0f);
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
}
#endif  // DMIP_WITH_X3P

// the fp32x3 images of a network: none at a width without x3 kernels, or beyond fp16's range (x3_range; fp32x3
// requests are then refused)
void pack_x3_net(const MlpDesc& d, const float* const* weights, const float* const* biases, MlpImages& im) {
  const int W = d.width, L = d.n_hidden, IN = d.in_dim, ST = W / 16, KQ = W / 32;
  const int chunk = dmip::x3_chunk_bytes(W) / 2;  // in fp16 elements, like every offset below (a fragment is 512)
  if (chunk == 0) return;
  const double mx = x3_max_scaled(d, weights);
  if (!(mx <= kHalfMax)) {
    im.x3_range = range_of(mx);
    return;
  }
  im.x3_l1 = pack_x3_l1(weights[0], W, IN, d.xdim, IN - 1);  // over (x, t)
  if (d.layout == DMIP_INPUT_X_Y_T) im.x3_l1_full = pack_x3_l1(weights[0], W, IN, IN);
  im.x3_bias.assign((size_t)L * W + 16, 0.0f);
  for (int u = 0; u < W; ++u) im.x3_bias[u] = (float)(kC * (double)biases[0][u]);
  // k-major engine (dmip_x3k.h): the same hi / lo fragments, a layer's chunk q = k-step q of all its
  // tiles ([o][q][p] -> [q][o][p])
  const bool kmajor = W == 256 && L == 3 && d.xdim >= 1 && d.xdim <= 4;
  Img16 img;
  const auto frag = [&](int o, int q) { return img.begin() + ((size_t)o * KQ + q) * 1024; };  // hi and lo: 1024
  for (int li = 1; li < L; ++li) {
    pack_x3_layer(weights[li], biases[li], W, W, ST, kC, img, im.x3_bias.data() + (size_t)li * W);
    append(im.x3_stream, img);
    if (kmajor && li == 1)
      for (int q = 0; q < KQ; ++q)
        for (int o = 0; o < ST; ++o) im.x3k_stream.insert(im.x3k_stream.end(), frag(o, q), frag(o, q) + 1024);
    if (kmajor && li == 2)  // two output halves, each k-major: chunk (h, q2) = k-steps 2 q2, 2 q2 + 1 of tiles 8h..8h+7
      for (int h = 0; h < 2; ++h)
        for (int q = 0; q < KQ; ++q)
          for (int o = 8 * h; o < 8 * h + 8; ++o) im.x3k_stream.insert(im.x3k_stream.end(), frag(o, q), frag(o, q) + 1024);
  }
  // the samplers read output rows 0..15 (the x rows); the layer is one zero-padded chunk
  pack_x3_layer(weights[L], biases[L], std::min(d.out_dim, 16), W, 1, 1.0, img, im.x3_bias.data() + (size_t)L * W);
  append(im.x3_stream, img);
  im.x3_stream.resize(im.x3_stream.size() + chunk - img.size(), 0);
  const int k1q_full = x3_k1q(IN);
  if (!im.x3_l1_full.empty() && ST * 512 == chunk && ST * k1q_full * 1024 > 48 * 1024) {
    // the sampler streams this layer 1 through the ring (dmip_x3.h L1R): chunk q = k-step q of every tile
    im.x3_stream_l1r.resize((size_t)k1q_full * chunk);
    for (int q = 0; q < k1q_full; ++q)
      for (int o = 0; o < ST; ++o)
        std::copy_n(im.x3_l1_full.begin() + ((size_t)o * k1q_full + q) * 512, 512,
                    im.x3_stream_l1r.begin() + ((size_t)q * ST + o) * 512);
    append(im.x3_stream_l1r, im.x3_stream);
  }
  if (!kmajor) return;
  // one output fragment per k-step: rows 0..D-1 the hi parts, rows 4..4+D-1 the lo parts
  const int D = d.xdim;
  im.x3k_out.assign((size_t)KQ * 512, 0);
  for (int q = 0; q < KQ; ++q)
    for (int l = 0; l < 64; ++l) {
      const int i = l & 15, part = i >= 4, row = i - 4 * part;
      if (i >= 8 || row >= D) continue;
      std::copy_n(img.begin() + (((size_t)q * 2 + part) * 64 + row + 16 * (l >> 4)) * 8, 8,
                  im.x3k_out.begin() + ((size_t)q * 64 + l) * 8);
    }
#ifdef DMIP_WITH_X3P
  if (x3p_bias_range(d, weights, biases) <= kHalfMax)
    pack_x3p(d, weights, biases, im.x3_bias.data() + W, im.x3_bias.data() + 2 * W, im);
#endif
}

// ---- DPS (dmip_surrogate.hip dps_kernel, dmip_dps_x3.hip): the prior is an MLP over (x, t), x 3, widths [256]*3

// exact-f32 images of the prior
void pack_dps_f32_prior(const float* const* weights, const float* const* biases, MlpImages& im) {
  const int W = dmip::kDpsPriorW;
  im.dps_l1.resize((size_t)16 * 2 * 64);
  for (int o = 0; o < 16; ++o)
    for (int l = 0; l < 64; ++l) {
      const int row = 16 * o + (l & 15), g = l >> 4;
      im.dps_l1[((size_t)o * 2 + 0) * 64 + l] = weights[0][(size_t)row * 4 + g];
      im.dps_l1[((size_t)o * 2 + 1) * 64 + l] = g == 0 ? biases[0][row] : 0.0f;
    }
  im.dps_bias.assign((size_t)2 * W + 16, 0.0f);
  std::copy_n(biases[1], W, im.dps_bias.begin());
  std::copy_n(biases[2], W, im.dps_bias.begin() + W);
  std::copy_n(biases[3], 3, im.dps_bias.begin() + 2 * W);
  im.dps_w2 = pack_f32_tiles(16, 16, rows_of(weights[1], W, W));
  im.dps_w3 = pack_f32_tiles(16, 16, rows_of(weights[2], W, W));
  im.dps_w4 = pack_f32_tiles(1, 16, rows_of(weights[3], W, 3));
}

// the fp32x3 DPS engine's prior images: layer 1 over (x, t) scaled by 2 log2 e; the forward chunks P2 | P3
// (pack_x3_layer: r-form folds) | Pout (folded, scale 1); the reverse chunks P4^T (one k-step: the 3 output rows) |
// P3^T | P2^T (plain transposes) | P1^T (W1's x columns); biases c b1 | init2 | init3 | out init. None beyond fp16's
// range (dps_x3_range).
void pack_dps_x3_prior(const float* const* weights, const float* const* biases, MlpImages& im) {
  const int W = dmip::kDpsPriorW;
  const float *W1 = weights[0], *W2 = weights[1], *W3 = weights[2], *W4 = weights[3];
  double mx = 0.0;
  ImgF bias((size_t)3 * W + 16, 0.0f);
  for (int u = 0; u < W; ++u) bias[u] = (float)(kC * (double)biases[0][u]);
  Img16 chunks, img;
  const auto folded = [&](int li, int n_rows, int n_tiles, double scale) {
    pack_x3_layer(weights[li], biases[li], n_rows, W, n_tiles, scale, img, bias.data() + (size_t)li * W);
    mx = max_abs_h(img, mx);
    append_chunks(chunks, img);
  };
  folded(1, W, 16, kC);
  folded(2, W, 16, kC);
  folded(3, 3, 1, 1.0);
  append_chunks(chunks, pack_x3_plain(16, 1, cols_of(W4, W, 3), &mx));
  append_chunks(chunks, pack_x3_plain(16, 8, cols_of(W3, W, W), &mx));
  append_chunks(chunks, pack_x3_plain(16, 8, cols_of(W2, W, W), &mx));
  append_chunks(chunks, pack_x3_plain(1, 8, [&](int r, int c) { return r < 3 ? W1[(size_t)c * 4 + r] : 0.0f; }, &mx));
  for (size_t i = 0; i < (size_t)W * 4; ++i) mx = std::max(mx, kC * std::fabs((double)W1[i]));
  if (!(mx <= kHalfMax) || chunks.size() * 2 != (size_t)dmip::kDpsX3PriorChunks * dmip::kDpsX3Chunk) {
    im.dps_x3_range = range_of(mx);
    return;
  }
  im.dps_x3_img = std::move(chunks);
  im.dps_x3_l1 = pack_x3_l1(W1, W, 4, 4);
  im.dps_x3_bias = std::move(bias);
}

}  // namespace

MlpImages pack_mlp(const MlpDesc& d, const float* const* weights, const float* const* biases) {
  MlpImages im;
  pack_16bit(d, weights, biases, im);
  if (d.layout == DMIP_INPUT_X_T && d.xdim == 3 && d.in_dim == 4 && d.out_dim == 3 && d.n_hidden == 3 &&
      d.width == dmip::kDpsPriorW) {
    pack_dps_f32_prior(weights, biases, im);
    pack_dps_x3_prior(weights, biases, im);
  }
  pack_f32_net(d, weights, biases, im);
  pack_x3_net(d, weights, biases, im);
  return im;
}

// the scatterometry surrogate ([256]*3, ReLU: no folds): f32 images w2, w3, w4, w3t, w2t, w4t, w1t (dmip_surrogate.hip)
// and the fp32x3 DPS engine's plain splits (dmip_dps_x3.hip), none beyond fp16's range (x3_range)
SurrogateImages pack_surrogate(const float* const* weights, const float* const* biases) {
  const int W = dmip::kSurW, XD = dmip::kSurXdim, YD = dmip::kSurYdim;
  const float *W1 = weights[0], *W2 = weights[1], *W3 = weights[2], *W4 = weights[3];
  const auto w1t = [&](int r, int c) { return r < XD ? W1[(size_t)c * XD + r] : 0.0f; };
  SurrogateImages im;
  im.img[0] = pack_f32_tiles(16, 16, rows_of(W2, W, W));
  im.img[1] = pack_f32_tiles(16, 16, rows_of(W3, W, W));
  im.img[2] = pack_f32_tiles(2, 16, rows_of(W4, W, YD));
  im.img[3] = pack_f32_tiles(16, 16, cols_of(W3, W, W));
  im.img[4] = pack_f32_tiles(16, 16, cols_of(W2, W, W));
  im.img[5] = pack_f32_tiles(16, 2, cols_of(W4, W, YD));
  im.img[6] = pack_f32_tiles(1, 16, w1t);
  im.l1.resize((size_t)16 * 64);
  for (int o = 0; o < 16; ++o)
    for (int l = 0; l < 64; ++l) {
      const int row = 16 * o + (l & 15), g = l >> 4;
      im.l1[(size_t)o * 64 + l] = g < XD ? W1[(size_t)row * XD + g] : biases[0][row];
    }
  im.bias.assign((size_t)3 * W + 32, 0.0f);
  for (int li = 0; li < 3; ++li) std::copy_n(biases[li], W, im.bias.begin() + (size_t)li * W);
  std::copy_n(biases[3], YD, im.bias.begin() + (size_t)3 * W);

  double mx = 0.0;
  Img16 chunks;
  append_chunks(chunks, pack_x3_plain(16, 8, rows_of(W2, W, W), &mx));
  append_chunks(chunks, pack_x3_plain(16, 8, rows_of(W3, W, W), &mx));
  append_chunks(chunks, pack_x3_plain(2, 8, rows_of(W4, W, YD), &mx));
  append_chunks(chunks, pack_x3_plain(16, 1, cols_of(W4, W, YD), &mx));
  append_chunks(chunks, pack_x3_plain(16, 8, cols_of(W3, W, W), &mx));
  append_chunks(chunks, pack_x3_plain(16, 8, cols_of(W2, W, W), &mx));
  append_chunks(chunks, pack_x3_plain(1, 8, w1t, &mx));
  for (size_t i = 0; i < (size_t)W * XD; ++i) mx = std::max(mx, std::fabs((double)W1[i]));
  if (!(mx <= kHalfMax) || chunks.size() * 2 != (size_t)dmip::kDpsX3SurChunks * dmip::kDpsX3Chunk) {
    im.x3_range = range_of(mx);
    return im;
  }
  im.x3_img = std::move(chunks);
  im.x3_l1 = pack_x3_l1(W1, W, XD, XD, -1, 1.0);
  im.x3_bias = im.bias;
  return im;
}

}  // namespace dmip_pack
