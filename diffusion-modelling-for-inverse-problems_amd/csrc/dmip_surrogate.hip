// The scatterometry forward model on gfx950: the frozen surrogate 3 -> 256 -> 256 -> 256 -> 23 ReLU
// (utils_scatterometry.py:8-25), the negative log posterior built on it (get_log_posterior,
// utils_scatterometry.py:30-38), its input gradient (energy_grad, models/SNF.py:234-237), and the
// random-walk Metropolis-Hastings ground-truth sampler that anneals to it (anneal_to_energy,
// models/SNF.py:250-275, driven by generate_scatterometry_ground_truth.py:26-39).
//
// Arithmetic: exact f32 on the matrix cores (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, no
// reduced-precision operands). The MH acceptance exp(E_cur - E_prop) and the heteroscedastic
// likelihood (prefactor (a f)^2 + b^2 with b = 0.01) turn bf16-level errors of f into O(0.1)
// energy errors for small outputs, so this path keeps the reference's f32.
//
// Layout (one wave = 16 chains; 8 waves = 128 chains per workgroup):
//   * a layer's output tile is 16 units x 16 chains: lane (g = l>>4, j = l&15) holds units 4g + r
//     (r = 0..3) of chain j. That tile IS the B operand of 4 k-steps of the next layer (k-step r
//     takes register r: B[k = g][j]), so activations stay in registers between layers, in f32.
//   * weights are packed on the host so the A fragment of k-step (q, r) of output tile o is
//     lane (i, g): W[16o + i][16q + 4g + r] -- a float4 per lane per q (one ds_read_b128 for
//     4 MFMAs).
//   * the 256 x 256 layers (forward W2, W3; backward W3^T, W2^T) and the output layer W4 stream
//     from L2 through a 4-slot LDS ring in 16 KiB chunks (one output tile each) by LDS-DMA;
//     layer 1, W4^T, W1^T and the biases are LDS-resident.
//   * the gradient is a reverse pass (vector-Jacobian product) with the ReLU masks of the forward
//     pass kept as bits (2 VGPRs per layer).
#include "dmip_device.h"
#include "dmip_internal.h"
#include "dmip_mh_chains.h"

#include <type_traits>

namespace dmip {
namespace sg {

constexpr int W = kSurW;           // 256
constexpr int ST = W / 16;         // 16 output tiles per 256-wide layer
constexpr int KG = W / 16;         // 16 k-groups (of 4 k-steps) over 256 inputs
constexpr int XD = kSurXdim, YD = kSurYdim;
constexpr int NW = 8;              // waves per workgroup (two per SIMD)
constexpr int R = 4;               // ring slots
constexpr int CHUNK = KG * 64 * 16;      // 16 KiB
constexpr int PPW = CHUNK / 1024 / NW;   // LDS-DMA pieces per wave per chunk
constexpr int NCF = 2 * ST + 2;          // forward chunks per evaluation: W2, W3 tiles, W4 tiles
constexpr int NCB = 2 * ST;              // backward chunks: W3^T, W2^T tiles

// LDS layout
constexpr int L1_OFF = 0, L1_BYTES = ST * 64 * 4;
constexpr int BIAS_OFF = L1_OFF + L1_BYTES;  // b1 | b2 | b3 [256] | b4 [32]
constexpr int BIAS_FLOATS = 3 * W + 32;
constexpr int Y_OFF = BIAS_OFF + BIAS_FLOATS * 4;  // the workgroup's observation y [32]
constexpr int W4T_OFF = Y_OFF + 32 * 4;
constexpr int W4T_BYTES = ST * 2 * 64 * 16;
constexpr int W1T_OFF = W4T_OFF + W4T_BYTES;
constexpr int W1T_BYTES = KG * 64 * 16;
// chunk streams (cycled once per evaluation / step): a Plan maps a chunk index of the cycle to the
// global address of that 16 KiB chunk (wave-uniform; the pointers are kernel arguments in SGPRs)
struct PlanFwd {  // W2 (16 tiles), W3 (16), W4 (2)
  const char *w2, *w3, *w4;
  static constexpr int N = NCF;
  __device__ __forceinline__ const char* src(int c) const {
    return c < ST ? w2 + (size_t)c * CHUNK : (c < 2 * ST ? w3 + (size_t)(c - ST) * CHUNK : w4 + (size_t)(c - 2 * ST) * CHUNK);
  }
};
struct PlanGrad {  // + W3^T (16), W2^T (16)
  PlanFwd f;
  const char *w3t, *w2t;
  static constexpr int N = NCF + NCB;
  __device__ __forceinline__ const char* src(int c) const {
    if (c < NCF) return f.src(c);
    return c < NCF + ST ? w3t + (size_t)(c - NCF) * CHUNK : w2t + (size_t)(c - NCF - ST) * CHUNK;
  }
};
constexpr int RING_OFF_FWD = W4T_OFF;
constexpr int RING_OFF_GRAD = W1T_OFF + W1T_BYTES;
static_assert(RING_OFF_GRAD + R * CHUNK <= 160 * 1024, "LDS budget");
static_assert(W4T_OFF % 16 == 0 && L1_BYTES % 16 == 0, "LDS-DMA alignment");

__device__ __forceinline__ f32x4 mfma4(float a, float b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float shfl_xor(float v, int m) { return __shfl_xor(v, m, 64); }

template <bool GRAD, int RING_OFF, typename Plan>
struct Engine {
  char* lds;
  Plan plan;
  long long gc;
  int w, lane, g;

  __device__ __forceinline__ void ring_issue(long long gi) {
    const char* base = plan.src((int)(gi % Plan::N));
    char* dst = lds + RING_OFF + (int)(gi % R) * CHUNK;
#pragma unroll
    for (int q = 0; q < PPW; ++q) {
      const int piece = w * PPW + q;
      const char* gp = base + piece * 1024;
      asm volatile("" : "+s"(gp));  // keep the per-chunk address out of the loop-invariant hoist
      glds16(gp, dst + piece * 1024, lane);
    }
  }

  // the next chunk of the stream: landed (own pieces counted, others' by the barrier), and the
  // slot it replaces is refilled R-1 chunks ahead. Other VMEM ops only make the wait stricter.
  __device__ __forceinline__ const char* chunk_sync() {
    wait_vmcnt<(R - 2) * PPW>();
    lds_barrier();
    ring_issue(gc + R - 1);
    const char* slot = lds + RING_OFF + (int)(gc % R) * CHUNK;
    ++gc;
    return slot;
  }

  // stage the resident parts (plus `extra` (dst, src, bytes) blocks of the caller), then start the ring
  __device__ __forceinline__ void prologue(const SurrogateParams& p, int n_extra = 0, char* const* xdst = nullptr,
                                           const char* const* xsrc = nullptr, const int* xbytes = nullptr) {
    const int tid = threadIdx.x;
    stage_lds(lds + L1_OFF, (const char*)p.l1, L1_BYTES);
    if constexpr (GRAD) {
      stage_lds(lds + W4T_OFF, p.w4t, W4T_BYTES);
      stage_lds(lds + W1T_OFF, p.w1t, W1T_BYTES);
    }
    for (int k = 0; k < n_extra; ++k) stage_lds(xdst[k], xsrc[k], xbytes[k]);
    float* bl = (float*)(lds + BIAS_OFF);
    for (int i = tid; i < BIAS_FLOATS; i += NW * 64) bl[i] = p.bias[i];
    wait_vmcnt<0>();
    __syncthreads();
    for (int q = 0; q < R - 1; ++q) ring_issue(q);
  }

  __device__ __forceinline__ void stage_lds(char* dst, const char* src, int bytes) {
    for (int blk = w; blk < bytes / 1024; blk += NW) glds16(src + blk * 1024, dst + blk * 1024, lane);
  }

  __device__ __forceinline__ void epilogue() { wait_vmcnt<0>(); }

  __device__ __forceinline__ f32x4 bias4(int layer, int tile) const {
    return *(const f32x4*)((const float*)(lds + BIAS_OFF) + layer * W + 16 * tile + 4 * g);
  }

  // layer 1 (3 -> 256, bias as the 4th k): exact f32, then ReLU (+ mask bits)
  __device__ __forceinline__ void layer1(const float (&x)[XD], float (&H)[ST][4], uint32_t (&m)[2]) {
    const float bsel = g == 0 ? x[0] : (g == 1 ? x[1] : (g == 2 ? x[2] : 1.0f));
    m[0] = m[1] = 0u;
#pragma unroll
    for (int o = 0; o < ST; ++o) {
      const float a = ((const float*)(lds + L1_OFF))[o * 64 + lane];
      const f32x4 z = mfma4(a, bsel, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
      relu_tile(z, o, H, m);
    }
  }

  __device__ __forceinline__ static void relu_tile(const f32x4& z, int o, float (&H)[ST][4], uint32_t (&m)[2]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool pos = z[r] > 0.0f;
      H[o][r] = pos ? z[r] : 0.0f;
      if constexpr (GRAD) m[o >> 3] |= (pos ? 1u : 0u) << ((o & 7) * 4 + r);
    }
  }

  // acc(tile) = sum over the 64 k-steps of a streamed 256-k chunk; two accumulation chains
  // (even / odd k-groups) so the 40-cycle MFMA dependency does not pace one wave
  __device__ __forceinline__ static f32x4 tile_product(const char* ch, int lane, const float (&H)[ST][4],
                                                        f32x4 acc0) {
    f32x4 acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < KG; ++q) {
      const f32x4 a = *(const f32x4*)(ch + (q * 64 + lane) * 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (q & 1) acc1 = mfma4(a[r], H[q][r], acc1);
        else acc0 = mfma4(a[r], H[q][r], acc0);
      }
    }
    return acc0 + acc1;
  }

  // a 256 -> 256 ReLU layer from the ring (layer index li = 1, 2 for the biases)
  __device__ __forceinline__ void hidden(int li, const float (&Hin)[ST][4], float (&Hout)[ST][4], uint32_t (&m)[2]) {
    m[0] = m[1] = 0u;
#pragma unroll
    for (int o = 0; o < ST; ++o) {
      const char* ch = chunk_sync();
      const f32x4 z = tile_product(ch, lane, Hin, bias4(li, o));
      relu_tile(z, o, Hout, m);
    }
  }

  // output layer (256 -> 23, two 16-row tiles): f rows 16t + 4g + r
  __device__ __forceinline__ void output(const float (&Hin)[ST][4], f32x4 (&f)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const char* ch = chunk_sync();
      f[t] = tile_product(ch, lane, Hin, bias4(3, t));
    }
  }

  // full forward; masks only in GRAD mode
  __device__ __forceinline__ void forward(const float (&x)[XD], f32x4 (&f)[2], uint32_t (&m)[3][2]) {
    float Ha[ST][4], Hb[ST][4];
    layer1(x, Ha, m[0]);
    hidden(1, Ha, Hb, m[1]);
    hidden(2, Hb, Ha, m[2]);
    output(Ha, f);
  }

  // reverse pass: v = dE/df (rows as f) -> dE/dx (every lane of the chain gets it)
  __device__ __forceinline__ void backward(const f32x4 (&v)[2], const uint32_t (&m)[3][2], float (&gx)[XD]) {
    float Ga[ST][4], Gb[ST][4];
    // W4^T (LDS-resident, k = 32 padded output rows): unit tiles of layer 3, masked by m3
#pragma unroll
    for (int o = 0; o < ST; ++o) {
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4 a = *(const f32x4*)(lds + W4T_OFF + ((o * 2 + q) * 64 + lane) * 16);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = mfma4(a[r], v[q][r], acc);
      }
      mask_tile(acc, o, m[2], Ga);
    }
    // W3^T then W2^T from the ring
#pragma unroll
    for (int o = 0; o < ST; ++o) {
      const char* ch = chunk_sync();
      mask_tile(tile_product(ch, lane, Ga, f32x4{0.0f, 0.0f, 0.0f, 0.0f}), o, m[1], Gb);
    }
#pragma unroll
    for (int o = 0; o < ST; ++o) {
      const char* ch = chunk_sync();
      mask_tile(tile_product(ch, lane, Gb, f32x4{0.0f, 0.0f, 0.0f, 0.0f}), o, m[0], Ga);
    }
    // W1^T (LDS-resident): rows 0..2 = dE/dx at lane group 0
    asm volatile("" ::: "memory");
    const f32x4 gxa = tile_product(lds + W1T_OFF, lane, Ga, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
    const int src = lane & 15;
#pragma unroll
    for (int d = 0; d < XD; ++d) gx[d] = __shfl(gxa[d], src, 64);
  }

  __device__ __forceinline__ static void mask_tile(const f32x4& z, int o, const uint32_t (&m)[2], float (&G)[ST][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) G[o][r] = ((m[o >> 3] >> ((o & 7) * 4 + r)) & 1u) ? z[r] : 0.0f;
  }
};

// Negative log posterior of the scatterometry problem (utils_scatterometry.py:30-38):
//   E = 0.5 sum_k log((a f_k)^2 + b^2) + 0.5 sum_k (y_k - f_k)^2 / ((a f_k)^2 + b^2)
//       + lambda sum_d relu(x_d - 1) + relu(-1 - x_d)
// The 23 output rows are spread over the 4 lane groups of a chain: partial sums, then two xor
// shuffles. v = dE/df_k for the reverse pass (rows >= 23 zero).
// KEEP IN STEP with scat_energy (dmip_mh_chains.h), its value-only form for the Metropolis kernels: the same operations
// in the same order. Shared forms tried (this function calling scat_energy's row loop as a template on want_v, or with
// want_v at run time, from the header or through a wrapper here): surrogate_eval_kernel<1>, <2> changed their code in
// each; with the shuffles behind a forceinline wrapper they kept it, but the fp32x3 two-tile MH kernel then ran 1.2 %
// slower than before in two sessions (profiles/mh_chains/README.md).
__device__ __forceinline__ float energy(const f32x4 (&f)[2], const float* y, const float (&x)[XD], float a,
                                        float b2, float lam, int g, f32x4 (&v)[2], bool want_v) {
  float slog = 0.0f, ssq = 0.0f;
  const float a2 = a * a;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + 4 * g + r;
      float vk = 0.0f;
      if (row < YD) {
        const float fk = f[t][r];
        const float af = a * fk;
        const float pref = af * af + b2;
        const float res = y[row] - fk;
        slog += logf(pref);
        const float q = res * res / pref;
        ssq += q;
        if (want_v) {
          // d/df [0.5 log pref + 0.5 res^2 / pref] = a^2 f / pref - res / pref - a^2 f res^2 / pref^2
          vk = (a2 * fk * (1.0f - q) - res) / pref;
        }
      }
      v[t][r] = vk;
    }
  }
  slog += shfl_xor(slog, 16);
  slog += shfl_xor(slog, 32);
  ssq += shfl_xor(ssq, 16);
  ssq += shfl_xor(ssq, 32);
  float bd = 0.0f;
#pragma unroll
  for (int d = 0; d < XD; ++d) bd += fmaxf(x[d] - 1.0f, 0.0f) + fmaxf(-1.0f - x[d], 0.0f);
  return 0.5f * slog + 0.5f * ssq + lam * bd;
}

// v = v2 + a^2 (v3 - v1) with v1 = f / pref, v2 = (y - f) / pref, v3 = (y - f)^2 f / pref: the
// combination of PosteriorLoss.likelihood_target's three VJP vectors (losses.py:353-356,366) -- the
// target is linear in them, so one reverse pass through the surrogate gives their weighted sum.
__device__ __forceinline__ void posterior_target_v(const f32x4 (&f)[2], const float* y, float a, float b2, int g,
                                                   f32x4 (&v)[2]) {
  const float a2 = a * a;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + 4 * g + r;
      float vk = 0.0f;
      if (row < YD) {
        const float fk = f[t][r];
        const float af = a * fk;
        const float pref = af * af + b2;
        const float res = y[row] - fk;
        const float v1 = fk / pref, v2 = res / pref, v3 = res * res * fk / pref;
        vk = v2 + a2 * (v3 - v1);
      }
      v[t][r] = vk;
    }
  }
}

__device__ __forceinline__ float boundary_grad(float xd, float lam) {
  return (xd > 1.0f ? lam : 0.0f) - (xd < -1.0f ? lam : 0.0f);
}

template <typename Plan>
__device__ __forceinline__ Plan make_plan(const SurrogateParams& p) {
  if constexpr (std::is_same<Plan, PlanFwd>::value) return PlanFwd{p.w2, p.w3, p.w4};
  else return PlanGrad{PlanFwd{p.w2, p.w3, p.w4}, p.w3t, p.w2t};
}

// ------------------------------------------------------------------------- evaluation kernel
// MODE 0: f = F(x); 1: E(x, y); 2: E and dE/dx; 3: J_F^T v with PosteriorLoss's target vector v
// (posterior_target_v, into g_out). Rows strided over the grid, 16 per wave.
template <int MODE>
__global__ void __launch_bounds__(NW * 64, 1) surrogate_eval_kernel(SurrogateParams p) {
  constexpr bool GRAD = MODE >= 2;
  constexpr int RING_OFF = GRAD ? RING_OFF_GRAD : RING_OFF_FWD;
  __shared__ __attribute__((aligned(16))) char lds[RING_OFF + R * CHUNK];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4;
  using Plan = typename std::conditional<GRAD, PlanGrad, PlanFwd>::type;
  Engine<GRAD, RING_OFF, Plan> eng{lds, make_plan<Plan>(p), 0, w, lane, g};
  eng.prologue(p);
  const long long n_tiles = (p.n + 15) / 16;
  const long long per_round = (long long)gridDim.x * NW;
  const long long rounds = (n_tiles + per_round - 1) / per_round;
  for (long long rd = 0; rd < rounds; ++rd) {
    const long long row = ((rd * gridDim.x + blockIdx.x) * NW + w) * 16 + (lane & 15);
    const bool valid = row < p.n;
    const long long rr = valid ? row : 0;
    float x[XD];
#pragma unroll
    for (int d = 0; d < XD; ++d) x[d] = p.x[rr * XD + d];
    f32x4 f[2];
    uint32_t m[3][2];
    eng.forward(x, f, m);
    if constexpr (MODE == 0) {
      if (valid) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 16 * t + 4 * g + r;
            if (k < YD) p.f_out[row * YD + k] = f[t][r];
          }
      }
    } else if constexpr (MODE == 3) {
      const float* y = p.y + (p.y_stride ? rr * p.y_stride : 0);
      f32x4 v[2];
      posterior_target_v(f, y, p.a, p.b2, g, v);
      float gx[XD];
      eng.backward(v, m, gx);
      if (valid && g == 0) {
#pragma unroll
        for (int d = 0; d < XD; ++d) p.g_out[row * XD + d] = gx[d];
      }
    } else {
      const float* y = p.y + (p.y_stride ? rr * p.y_stride : 0);
      f32x4 v[2];
      const float e = energy(f, y, x, p.a, p.b2, p.lam, g, v, GRAD);
      if (valid && g == 0) p.e_out[row] = e;
      if constexpr (GRAD) {
        float gx[XD];
        eng.backward(v, m, gx);
        if (valid && g == 0) {
#pragma unroll
          for (int d = 0; d < XD; ++d) p.g_out[row * XD + d] = gx[d] + boundary_grad(x[d], p.lam);
        }
      }
    }
  }
  eng.epilogue();
}

// ------------------------------------------------------------------- Metropolis-Hastings kernel
// anneal_to_energy (models/SNF.py:250-275) without Langevin proposals, with E the negative log posterior for this
// workgroup's y: the chain life cycle and the step loop of dmip_mh_chains.h on the exact-f32 forward pass.
// Outputs x and E(x_final) - E(x_0). INJECT: captured draws replace the RNG (random_walk).
template <bool INJECT>
__global__ void __launch_bounds__(NW * 64, 1) mh_kernel(SurrogateParams p) {
  __shared__ __attribute__((aligned(16))) char lds[RING_OFF_FWD + R * CHUNK];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4;
  const int yi = blockIdx.y;
  const ChainLane ln[1] = {chain_lane<NW>(w, lane, p.ch.n_chains, yi)};
  Engine<false, RING_OFF_FWD, PlanFwd> eng{lds, make_plan<PlanFwd>(p), 0, w, lane, g};
  float* ylds = (float*)(lds + Y_OFF);
  stage_y<NW>(ylds, p.y, yi);
  eng.prologue(p);

  float x[1][XD], de[1];
  Rng rng[1] = {chain_start(p.ch, ln[0], x[0])};
  // (always inlined, as every eval of random_walk: an outlined call would put the forward pass's arrays on the stack)
  const auto eval = [&](const float (&xs)[1][XD], float (&es)[1]) __attribute__((always_inline)) {
    f32x4 f[2];
    uint32_t m[3][2];
    eng.forward(xs[0], f, m);
    es[0] = scat_energy(f, ylds, xs[0], p.a, p.b2, p.lam, g);
  };
  random_walk<1, INJECT>(p.ch, ln, rng, x, de, eval);
  eng.epilogue();
  chain_store(p.ch, ln[0], g, x[0], p.e_out, de[0]);
}

// ------------------------------------------------------- Metropolis-adjusted Langevin kernel
// anneal_to_energy with langevin_prop=True (models/SNF.py:250-300) on the interpolated energy of
// get_interpolated_energy_fun (models/SNF.py:220-231):
//   E_l(x) = l E(x) + (1 - l) |x|^2 / 2,   grad E_l(x) = l grad E(x) + (1 - l) x
// with E the negative log posterior above; l = 1 is E itself and l = 0 the Gaussian alone (the reference's
// branches, taken by select so that a non-finite other term cannot leak in through a zero weight).
// One evaluation = one forward and one reverse pass = one cycle of the ring (NCF + NCB chunks).
template <typename E>
__device__ __forceinline__ float interp_energy_grad(E& eng, const float* ylds, const MalaParams& q,
                                                    const float (&x)[XD], float (&gr)[XD]) {
  const SurrogateParams& p = q.s;
  f32x4 f[2], v[2];
  uint32_t m[3][2];
  eng.forward(x, f, m);
  const float e = energy(f, ylds, x, p.a, p.b2, p.lam, eng.g, v, true);
  float gx[XD];
  eng.backward(v, m, gx);
  const float sq = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  const bool one = q.lam_e == 1.0f, zero = q.lam_e == 0.0f;
#pragma unroll
  for (int d = 0; d < XD; ++d) {
    const float ge = gx[d] + boundary_grad(x[d], p.lam);
    gr[d] = one ? ge : (zero ? x[d] : q.lam_e * ge + (2.0f * q.lam_q) * x[d]);
  }
  return one ? e : (zero ? q.lam_q * sq : q.lam_e * e + q.lam_q * sq);
}

// Per Metropolis step: L Langevin sub-steps from (xx, gg) = (x, grad E_l(x)) with h = stepsize, c = sqrt(2 h):
//   yy = xx - h gg + c eta;  eta' = (xx - yy + h grad E_l(yy)) / c;  ld += sum_d (eta_d^2 - eta'_d^2) / 2
// then accept iff u < exp(-E_l(yy) + E_l(x) + ld). The chain state (x, E_l(x), grad E_l(x), RNG, accept count)
// stays in registers for all steps; E_l and its gradient at the current point are carried (the reference
// recomputes them: the same values), so a sub-step costs one evaluation. The state is chosen by select: a
// non-finite proposal fails the comparison and is dropped, where the reference's blend rej * x + acc * x_prop
// would turn 0 * inf into NaN. Outputs x, E_l(x_S) - E_l(x_0) and the number of accepted steps.
// Product RNG per step: L x rng_normals<3>, then one word for u. INJECT: eta [S][L][n_y][n][3] and
// u [S][n_y][n] replace it (replaying the reference's captured draws).
// Of dmip_mh_chains.h's life cycle this kernel takes chain_lane and uniform01; y's staging, the start and the store
// stay written out. It sits at 256 VGPRs with 104 / 108 B of scratch (product RNG / injected draws), and every other
// helper moved that: all of them 112 / 116 B, stage_y alone 108 / 108, chain_lane + chain_start 108 / 108,
// chain_lane + chain_store 116 / 116.
template <bool INJECT>
__global__ void __launch_bounds__(NW * 64, 1) mala_kernel(MalaParams q) {
  const SurrogateParams& p = q.s;
  __shared__ __attribute__((aligned(16))) char lds[RING_OFF_GRAD + R * CHUNK];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4;
  const int yi = blockIdx.y;
  const ChainLane ln = chain_lane<NW>(w, lane, p.ch.n_chains, yi);
  Engine<true, RING_OFF_GRAD, PlanGrad> eng{lds, make_plan<PlanGrad>(p), 0, w, lane, g};
  float* ylds = (float*)(lds + Y_OFF);
  for (int i = threadIdx.x; i < 32; i += NW * 64) ylds[i] = i < YD ? p.y[(size_t)yi * YD + i] : 0.0f;
  eng.prologue(p);

  Rng rng = rng_init(p.ch.seed, (uint64_t)(p.ch.chain_offset + ln.c), (uint64_t)yi);
  float x[XD];
  if (p.ch.x_init) {
#pragma unroll
    for (int d = 0; d < XD; ++d) x[d] = p.ch.x_init[ln.at(p.ch.n_chains) * XD + d];
  } else {
#pragma unroll
    for (int d = 0; d < XD; ++d) x[d] = uniform01(rng) * 2.0f - 1.0f;
  }
  float g_cur[XD];
  const float e0 = interp_energy_grad(eng, ylds, q, x, g_cur);
  float e_cur = e0;
  int n_acc = 0;
  const size_t plane = (size_t)gridDim.y * p.ch.n_chains, at = ln.at(p.ch.n_chains);
  for (int s = 0; s < p.ch.num_steps; ++s) {
    float xx[XD], gg[XD], ld = 0.0f, e_y = e_cur;
#pragma unroll
    for (int d = 0; d < XD; ++d) xx[d] = x[d], gg[d] = g_cur[d];
#pragma unroll 1
    for (int l = 0; l < q.lang_steps; ++l) {
      float eta[XD];
      if constexpr (INJECT) {
        const float* src = p.ch.noise + (((size_t)s * q.lang_steps + l) * plane + at) * XD;
#pragma unroll
        for (int d = 0; d < XD; ++d) eta[d] = src[d];
      } else {
        rng_normals<XD>(rng, eta);
      }
      float yy[XD], g_y[XD];
#pragma unroll
      for (int d = 0; d < XD; ++d) yy[d] = xx[d] - q.h * gg[d] + q.c * eta[d];
      e_y = interp_energy_grad(eng, ylds, q, yy, g_y);
      float dsum = 0.0f;
#pragma unroll
      for (int d = 0; d < XD; ++d) {
        const float eb = (xx[d] - yy[d] + q.h * g_y[d]) / q.c;
        dsum += eta[d] * eta[d] - eb * eb;
        xx[d] = yy[d];
        gg[d] = g_y[d];
      }
      ld += 0.5f * dsum;
      // the carried sums stay one dependent chain per sub-step
      asm volatile("" : "+v"(ld), "+v"(e_y));
    }
    float u;
    if constexpr (INJECT) u = p.ch.unif[(size_t)s * plane + at];
    else u = uniform01(rng);
    const bool acc = u < expf(-e_y + e_cur + ld);
#pragma unroll
    for (int d = 0; d < XD; ++d) {
      x[d] = acc ? xx[d] : x[d];
      g_cur[d] = acc ? gg[d] : g_cur[d];
    }
    e_cur = acc ? e_y : e_cur;
    n_acc += acc ? 1 : 0;
  }
  eng.epilogue();
  if (ln.valid && g == 0) {
    float* dst = p.ch.x_out + at * XD;
#pragma unroll
    for (int d = 0; d < XD; ++d) dst[d] = x[d];
    if (p.e_out) p.e_out[at] = e_cur - e0;
    if (q.acc_out) q.acc_out[at] = n_acc;
  }
}


// ---------------------------------------------------------------------------- DPS sampler
// BASELINE config 4 (no reference code for sampling-time guidance): diffusion
// posterior sampling (Chung et al. 2023) on the reference's EM predictor, with the Posterior
// estimator's prior score network MLP2(x, t) (nets.py:37-57) and the scatterometry surrogate F as the
// measurement operator. Per step (tau = T - t_i):
//   s, J = prior(x, tau), ds/dx            (forward-mode Jacobian, 3 tangents)
//   x0 = (x + var(tau) s) / mean_weight(tau)                      (Tweedie)
//   G  = dL/dx = (I + var J^T) (dL/dx0) / mean_weight             (chain rule through x0(x))
//   x <- EM(x, a = g s) - lambda G
// with, by `mode`,
//   NLL:  L = 0.5 sum log pref + 0.5 sum (y - F)^2 / pref (get_log_posterior's likelihood part,
//         utils_scatterometry.py:33-35), lambda = zeta delta g^2 -- i.e. the score s + zeta grad log
//         p(y | x0(x)), the target the reference's PosteriorLoss.likelihood_target (losses.py:349-371)
//         trains its likelihood network on;
//   NORM: L = ||y - F(x0)||^2, lambda = zeta / ||y - F(x0)|| (Chung et al. Alg. 1 step-size rule).
// Everything runs in exact f32 on the f32 MFMA. The prior network's primal and its three tangents
// share one 16-column B operand: column j = 4c + m is chain c of the pass (4 chains per pass, 4
// passes per 16-chain wave) with m = 0 the primal and m = 1..3 the tangent along x_{m-1}; the
// activation derivative of a tangent column is taken from its quad's primal lane (DPP broadcast).
constexpr int PL1_OFF = RING_OFF_GRAD;                 // prior layer 1: [16][2][64] floats
constexpr int PL1_BYTES = ST * 2 * 64 * 4;
constexpr int PW4_OFF = PL1_OFF + PL1_BYTES;           // prior output tile, resident
constexpr int PW4_BYTES = KG * 64 * 16;
constexpr int PB_OFF = PW4_OFF + PW4_BYTES;            // prior b2 | b3 | b4[16]
constexpr int PB_FLOATS = 2 * W + 16;
constexpr int SJ_OFF = PB_OFF + PB_FLOATS * 4;         // per-wave s / J exchange [NW][16 chains][4][4]
constexpr int SJ_BYTES = NW * 16 * 16 * 4;
constexpr int RING_OFF_DPS = SJ_OFF + SJ_BYTES;
static_assert(RING_OFF_DPS + R * CHUNK <= 160 * 1024, "DPS LDS budget");
static_assert(PL1_OFF % 16 == 0 && PW4_OFF % 16 == 0 && SJ_OFF % 16 == 0 && RING_OFF_DPS % 16 == 0, "align");

struct PlanDps {  // 4 prior passes x (W2p, W3p), then the surrogate forward + reverse stream
  const char *pw2, *pw3;
  PlanGrad s;
  static constexpr int NP = 4 * 2 * ST;
  static constexpr int N = NP + PlanGrad::N;
  __device__ __forceinline__ const char* src(int c) const {
    if (c < NP) {
      const int k = c % (2 * ST);
      return k < ST ? pw2 + (size_t)k * CHUNK : pw3 + (size_t)(k - ST) * CHUNK;
    }
    return s.src(c - NP);
  }
};

__device__ __forceinline__ float quad_primal(float v) {  // value of lane 4*(l/4) (DPP quad_perm 0,0,0,0)
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x00, 0xF, 0xF, true));
}

__device__ __forceinline__ float tanh_f32(float z) {  // 1 - 2 / (e^{2z} + 1): a few ulp, saturates cleanly
  return 1.0f - __fdividef(2.0f, __expf(2.0f * z) + 1.0f);
}

// activation of one prior tile: primal columns tanh (twice on layer 1, nets.py:21-26), tangent
// columns act'(z_primal) * z
template <bool TWICE>
__device__ __forceinline__ void prior_act(const f32x4& z, int m, float (&H)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float zp = quad_primal(z[r]);
    const float t1 = tanh_f32(zp);
    float val, d;
    if constexpr (TWICE) {
      const float t2 = tanh_f32(t1);
      val = t2;
      d = (1.0f - t2 * t2) * (1.0f - t1 * t1);
    } else {
      val = t1;
      d = 1.0f - t1 * t1;
    }
    H[r] = m == 0 ? val : d * z[r];
  }
}

template <typename E>
__device__ __forceinline__ f32x4 prior_bias4(const E& eng, int layer, int tile, int m) {
  if (m != 0) return f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  return *(const f32x4*)((const float*)(eng.lds + PB_OFF) + layer * W + 16 * tile + 4 * eng.g);
}

// one prior pass: rows 4g + r of the output tile (s_i for m = 0, ds_i/dx_{m-1} otherwise) at g = 0
template <typename E>
__device__ __forceinline__ f32x4 prior_pass(E& eng, const float (&xin)[XD], float tau, int m) {
  const int g = eng.g, lane = eng.lane;
  float Ha[ST][4], Hb[ST][4];
  const float b0 = m == 0 ? (g == 0 ? xin[0] : (g == 1 ? xin[1] : (g == 2 ? xin[2] : tau)))
                          : (g == m - 1 ? 1.0f : 0.0f);
  const float b1 = (m == 0 && g == 0) ? 1.0f : 0.0f;
#pragma unroll
  for (int o = 0; o < ST; ++o) {
    const float a0 = ((const float*)(eng.lds + PL1_OFF))[(o * 2 + 0) * 64 + lane];
    const float a1 = ((const float*)(eng.lds + PL1_OFF))[(o * 2 + 1) * 64 + lane];
    const f32x4 z = mfma4(a1, b1, mfma4(a0, b0, f32x4{0.0f, 0.0f, 0.0f, 0.0f}));
    prior_act<true>(z, m, Ha[o]);
  }
#pragma unroll
  for (int o = 0; o < ST; ++o) {
    const char* ch = eng.chunk_sync();
    prior_act<false>(E::tile_product(ch, lane, Ha, prior_bias4(eng, 0, o, m)), m, Hb[o]);
  }
#pragma unroll
  for (int o = 0; o < ST; ++o) {
    const char* ch = eng.chunk_sync();
    prior_act<false>(E::tile_product(ch, lane, Hb, prior_bias4(eng, 1, o, m)), m, Ha[o]);
  }
  asm volatile("" ::: "memory");
  return E::tile_product(eng.lds + PW4_OFF, lane, Ha, prior_bias4(eng, 2, 0, m));
}

__global__ void __launch_bounds__(NW * 64, 1) dps_kernel(DpsParams p) {
  __shared__ __attribute__((aligned(16))) char lds[RING_OFF_DPS + R * CHUNK];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, j = lane & 15;
  const int yi = blockIdx.y;
  const long long c_local = (long long)blockIdx.x * (NW * 16) + w * 16 + j;
  const bool valid = c_local < p.s.ch.n_chains;
  Engine<true, RING_OFF_DPS, PlanDps> eng{
      lds, PlanDps{p.pw2, p.pw3, make_plan<PlanGrad>(p.s)}, 0, w, lane, g};
  float* ylds = (float*)(lds + Y_OFF);
  for (int i = threadIdx.x; i < 32; i += NW * 64) ylds[i] = i < YD ? p.s.y[(size_t)yi * YD + i] : 0.0f;
  float* pb = (float*)(lds + PB_OFF);
  for (int i = threadIdx.x; i < PB_FLOATS; i += NW * 64) pb[i] = p.pbias[i];
  {
    char* const xd[2] = {lds + PL1_OFF, lds + PW4_OFF};
    const char* const xs[2] = {(const char*)p.pl1, p.pw4};
    const int xb[2] = {PL1_BYTES, PW4_BYTES};
    eng.prologue(p.s, 2, xd, xs, xb);
  }
  float* sj = (float*)(lds + SJ_OFF) + w * 256;  // [16 chains][m][r]

  Rng rng = rng_init(p.s.ch.seed, (uint64_t)(p.s.ch.chain_offset + c_local), (uint64_t)yi);
  float x[XD];
  {
    float n0[XD];
    rng_normals<XD>(rng, n0);
#pragma unroll
    for (int d = 0; d < XD; ++d) x[d] = __fadd_rn(__fmul_rn(n0[d], p.stdv), p.mean);
  }
  for (int i = 0; i < p.s.ch.num_steps; ++i) {
    const StepCoef cf = step_coef(i, p.s.ch.num_steps, p.T, p.bmin, p.bdiff);
    // prior score and Jacobian, 4 chains per pass
    const int m = lane & 3;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
      const int src = 4 * pass + (j >> 2);
      float xin[XD];
#pragma unroll
      for (int d = 0; d < XD; ++d) xin[d] = __shfl(x[d], src, 64);
      const f32x4 o = prior_pass(eng, xin, cf.tau, m);
      if (g == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) sj[(src * 4 + m) * 4 + r] = o[r];
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float sc[XD], J[XD][XD];
#pragma unroll
    for (int r = 0; r < XD; ++r) {
      sc[r] = sj[(j * 4 + 0) * 4 + r];
#pragma unroll
      for (int k = 0; k < XD; ++k) J[r][k] = sj[(j * 4 + 1 + k) * 4 + r];
    }
    // Tweedie estimate and the residual gradient through the surrogate
    const float mw = vp_mean_weight(cf.tau, p.bmin, p.bdiff);
    const float sd = vp_std(cf.tau, p.bmin, p.bdiff);
    const float var = sd * sd;
    float x0h[XD];
#pragma unroll
    for (int d = 0; d < XD; ++d) x0h[d] = (x[d] + var * sc[d]) / mw;
    f32x4 f[2], v[2];
    uint32_t mk[3][2];
    eng.forward(x0h, f, mk);
    float scale;
    if (p.mode == 0) {  // NLL: v = dNLL/df (the likelihood terms of get_log_posterior, no boundary prior)
      (void)energy(f, ylds, x0h, p.s.a, p.s.b2, 0.0f, g, v, true);
      scale = p.zeta * p.delta * cf.beta;  // zeta delta g^2
    } else {            // NORM: v = d||r||^2/df = -2 r, step zeta / ||r||
      float rr = 0.0f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * t + 4 * g + r;
          const float res = row < YD ? ylds[row] - f[t][r] : 0.0f;
          rr += res * res;
          v[t][r] = -2.0f * res;
        }
      rr += shfl_xor(rr, 16);
      rr += shfl_xor(rr, 32);
      scale = p.zeta * __frsqrt_rn(fmaxf(rr, 1e-30f));
    }
    float gx[XD];
    eng.backward(v, mk, gx);
    float xi[XD];
    rng_normals<XD>(rng, xi);
#pragma unroll
    for (int k = 0; k < XD; ++k) {
      float jt = gx[k];
#pragma unroll
      for (int r = 0; r < XD; ++r) jt += var * J[r][k] * gx[r];
      const float gt = jt / mw;
      const float xe = em_update(x[k], __fmul_rn(cf.g, sc[k]), xi[k], cf, p.delta, p.sqrt_delta);
      x[k] = xe - scale * gt;
    }
  }
  eng.epilogue();
  if (valid && g == 0) {
    float* dst = p.s.ch.x_out + ((size_t)yi * p.s.ch.n_chains + c_local) * XD;
#pragma unroll
    for (int d = 0; d < XD; ++d) dst[d] = x[d];
  }
}
}  // namespace sg

hipError_t launch_surrogate_eval(const SurrogateParams& p, int mode, int n_wg, hipStream_t st) {
  const dim3 grid((unsigned)n_wg), block(sg::NW * 64);
  switch (mode) {
    case 0: hipLaunchKernelGGL(sg::surrogate_eval_kernel<0>, grid, block, 0, st, p); break;
    case 1: hipLaunchKernelGGL(sg::surrogate_eval_kernel<1>, grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL(sg::surrogate_eval_kernel<3>, grid, block, 0, st, p); break;
    default: hipLaunchKernelGGL(sg::surrogate_eval_kernel<2>, grid, block, 0, st, p); break;
  }
  return hipGetLastError();
}

int surrogate_rows_per_wg() { return sg::NW * 16; }

hipError_t launch_dps(const DpsParams& p, int n_y, hipStream_t st) {
  hipLaunchKernelGGL(sg::dps_kernel, chain_grid(p.s.ch.n_chains, sg::NW * 16, n_y), dim3(sg::NW * 64), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_mh(const SurrogateParams& p, int n_y, hipStream_t st) {
  const dim3 grid = chain_grid(p.ch.n_chains, sg::NW * 16, n_y), block(sg::NW * 64);
  if (p.ch.noise)
    hipLaunchKernelGGL(sg::mh_kernel<true>, grid, block, 0, st, p);
  else
    hipLaunchKernelGGL(sg::mh_kernel<false>, grid, block, 0, st, p);
  return hipGetLastError();
}

hipError_t launch_mala(const MalaParams& q, int n_y, hipStream_t st) {
  const dim3 grid = chain_grid(q.s.ch.n_chains, sg::NW * 16, n_y), block(sg::NW * 64);
  if (q.s.ch.noise)
    hipLaunchKernelGGL(sg::mala_kernel<true>, grid, block, 0, st, q);
  else
    hipLaunchKernelGGL(sg::mala_kernel<false>, grid, block, 0, st, q);
  return hipGetLastError();
}

}  // namespace dmip
