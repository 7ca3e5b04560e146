// The chain life cycle of the surrogate's Metropolis kernels (dmip_surrogate.hip mh_kernel, mala_kernel;
// dmip_dps_x3.hip mh_x3_kernel, mh_x3_mt_kernel), written once: which chain a lane runs, the workgroup's observation in
// LDS, the chain's RNG stream and start state, the energy (get_log_posterior), the random-walk step loop and the final
// store. The RNG consumption per chain defined here is what makes shards and tile variants bit-identical:
//   rng_init(seed, chain_offset + c, yi);  x0 given, or 3 uniforms;  then per step 3 normals and 1 uniform
// (MALA, which keeps its own step loop: L x 3 normals and 1 uniform). A kernel supplies how an energy is evaluated.
#pragma once
#include "dmip_device.h"
#include "dmip_internal.h"

#include <utility>

namespace dmip {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// compile-time loops over a wave's tiles (the index is a constant in every body)
template <typename F, int... I>
__device__ __forceinline__ void sfor_impl(const F& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void sfor(const F& f) {
  sfor_impl(f, std::make_integer_sequence<int, N>{});
}

// Tile m of wave w (MT tiles of 16 chains per wave, NW waves per workgroup): lane (g, j) runs chain
// c = 16 NW MT block + 16 (MT w + m) + j of observation yi. at(): its place in the [n_y][n_chains] tensors, the index
// clamped to chain 0 for the lanes past the end (they compute, and are never stored)
struct ChainLane {
  long long c;
  bool valid;
  int yi;
  __device__ __forceinline__ size_t at(long long n_chains) const { return (size_t)yi * n_chains + (valid ? c : 0); }
};
template <int NW>
__device__ __forceinline__ ChainLane chain_lane(int w, int lane, long long n_chains, int yi, int MT = 1, int m = 0) {
  const long long c = (long long)blockIdx.x * (NW * 16 * MT) + (MT * w + m) * 16 + (lane & 15);
  return ChainLane{c, c < n_chains, yi};
}

// the workgroup's observation y[yi] as 32 floats in LDS (rows >= 23 zero); the caller's barrier publishes it
template <int NW>
__device__ __forceinline__ void stage_y(float* ylds, const float* y, int yi) {
  for (int i = threadIdx.x; i < 32; i += NW * 64) ylds[i] = i < kSurYdim ? y[(size_t)yi * kSurYdim + i] : 0.0f;
}

// one RNG word as a uniform on [0, 1): torch.rand's 24 bits
__device__ __forceinline__ float uniform01(Rng& rng) { return (float)(rng_next(rng) >> 8) * 0x1p-24f; }

// the chain's RNG stream, and its start state: x_init, or torch.rand(n, 3) * 2 - 1
// (generate_scatterometry_ground_truth.py:27)
__device__ __forceinline__ Rng chain_start(const MhChains& ch, const ChainLane& ln, float (&x)[kSurXdim]) {
  Rng rng = rng_init(ch.seed, (uint64_t)(ch.chain_offset + ln.c), (uint64_t)ln.yi);
  if (ch.x_init) {
#pragma unroll
    for (int d = 0; d < kSurXdim; ++d) x[d] = ch.x_init[ln.at(ch.n_chains) * kSurXdim + d];
  } else {
#pragma unroll
    for (int d = 0; d < kSurXdim; ++d) x[d] = uniform01(rng) * 2.0f - 1.0f;
  }
  return rng;
}

// x and, when asked for, de = E(x_S) - E(x_0) (the reference's second return value), by lane group 0 of a real chain
__device__ __forceinline__ void chain_store(const MhChains& ch, const ChainLane& ln, int g, const float (&x)[kSurXdim],
                                            float* e_out, float de) {
  if (ln.valid && g == 0) {
    const size_t at = ln.at(ch.n_chains);
#pragma unroll
    for (int d = 0; d < kSurXdim; ++d) ch.x_out[at * kSurXdim + d] = x[d];
    if (e_out) e_out[at] = de;
  }
}

// Negative log posterior of the scatterometry problem for one chain (get_log_posterior, utils_scatterometry.py:30-38):
//   E = 0.5 sum_k log((a f_k)^2 + b^2) + 0.5 sum_k (y_k - f_k)^2 / ((a f_k)^2 + b^2)
//       + lambda sum_d relu(x_d - 1) + relu(-1 - x_d)
// f: the surrogate's output tiles in accumulator form, so the 23 rows are spread over the 4 lane groups of a chain:
// partial sums, then two xor shuffles. KEEP IN STEP with dmip_surrogate.hip's energy, which also gives dE/df for the
// reverse pass and says why the two are not one function.
__device__ __forceinline__ float scat_energy(const f32x4 (&f)[2], const float* y, const float (&x)[kSurXdim], float a,
                                             float b2, float lam, int g) {
  float slog = 0.0f, ssq = 0.0f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + 4 * g + r;
      if (row < kSurYdim) {
        const float fk = f[t][r];
        const float af = a * fk;
        const float pref = af * af + b2;
        const float res = y[row] - fk;
        slog += logf(pref);
        ssq += res * res / pref;
      }
    }
  slog += __shfl_xor(slog, 16, 64);
  slog += __shfl_xor(slog, 32, 64);
  ssq += __shfl_xor(ssq, 16, 64);
  ssq += __shfl_xor(ssq, 32, 64);
  float bd = 0.0f;
#pragma unroll
  for (int d = 0; d < kSurXdim; ++d) bd += fmaxf(x[d] - 1.0f, 0.0f) + fmaxf(-1.0f - x[d], 0.0f);
  return 0.5f * slog + 0.5f * ssq + lam * bd;
}

// anneal_to_energy (models/SNF.py:250-275) without Langevin proposals, for the MT tiles of a wave: per step and chain
//   x_prop = x + noise_std * xi;  accept iff u < exp(-E(x_prop) + E(x))
// eval(xs, es) gives the energies of all MT tiles' states at once. The chain state (x, E(x), RNG) stays in registers
// for all steps (every lane of a chain carries an identical copy); E(x) is carried instead of being recomputed (the
// reference's energy(x_curr) is the same value). Leaves x = x_S and de = E(x_S) - E(x_0).
// INJECT: ch.noise [S][n_y][n][3] and ch.unif [S][n_y][n] replace the RNG (replaying captured draws).
template <int MT, bool INJECT, typename Eval>
__device__ __forceinline__ void random_walk(const MhChains& ch, const ChainLane (&ln)[MT], Rng (&rng)[MT],
                                            float (&x)[MT][kSurXdim], float (&de)[MT], const Eval& eval) {
  float e0[MT], e_cur[MT];
  eval(x, e0);
  sfor<MT>([&](auto m) { e_cur[m] = e0[m]; });
  const size_t plane = (size_t)gridDim.y * ch.n_chains;
  for (int s = 0; s < ch.num_steps; ++s) {
    float xp[MT][kSurXdim], u[MT], e_prop[MT];
    sfor<MT>([&](auto m) {
      float xi[kSurXdim];
      if constexpr (INJECT) {
        const size_t at = (size_t)s * plane + ln[m].at(ch.n_chains);
#pragma unroll
        for (int d = 0; d < kSurXdim; ++d) xi[d] = ch.noise[at * kSurXdim + d];
        u[m] = ch.unif[at];
      } else {
        rng_normals<kSurXdim>(rng[m], xi);
        u[m] = uniform01(rng[m]);
      }
#pragma unroll
      for (int d = 0; d < kSurXdim; ++d) xp[m][d] = x[m][d] + ch.noise_std * xi[d];
    });
    eval(xp, e_prop);
    sfor<MT>([&](auto m) {
      const bool acc = u[m] < expf(-e_prop[m] + e_cur[m]);
#pragma unroll
      for (int d = 0; d < kSurXdim; ++d) x[m][d] = acc ? xp[m][d] : x[m][d];
      e_cur[m] = acc ? e_prop[m] : e_cur[m];
    });
  }
  sfor<MT>([&](auto m) { de[m] = e_cur[m] - e0[m]; });
}

}  // namespace dmip
