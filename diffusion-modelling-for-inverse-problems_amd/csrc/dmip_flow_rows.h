// What the four probability-flow kernels with an exact divergence share whatever engine runs the network
// (f32_flow_kernel / f32_flow_sample_kernel: dmip_flow.hip, dmip_flow_sample.hip on dmip_flow.h; x3_flow_kernel /
// x3_flow_sample_kernel: dmip_x3_flow.h): the rows of a wave pass, the two integrators over them, and the launch.
//
// A wave pass holds 4 rows x (primal + 3 tangents) in the 16 columns of its B operand, column j = 4 c + m (m = 0 the
// primal of row c, m = 1..3 the tangent along x_{m-1}); lane = 16 g + j. The kernel supplies the network as a functor
// score(xt, coef, a, dv) over its engine's flow_score; the drivers own the rounds, the steps and the stores.
// Everything is always inlined and the functor takes the driver's state by reference: by value, or behind a call, the
// kernels compiled to other code. The library is built with -ffp-contract=off: the source order of
// every expression below is its result. One kernel does not go through sample_rows: f32_flow_sample_kernel keeps the
// same text written out, because its spilling W 512 instantiations measured slower through it (dmip_flow_sample.hip).
#pragma once
#include <type_traits>

#include "dmip_device.h"
#include "dmip_internal.h"

namespace dmip {
namespace flow {

__device__ __forceinline__ float quad_primal(float v) {  // value of lane 4 (l / 4) (DPP quad_perm 0,0,0,0)
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x00, 0xF, 0xF, true));
}

// the forward grid of log p(x | y): tau_k = linspace_at(k, S) T (the sampler's schedule, reversed)
struct FlowCoef {
  float tau, beta, g;
};
__device__ __forceinline__ FlowCoef flow_coef(int k, int S, float T, float bmin, float bdiff) {
  FlowCoef c;
  c.tau = __fmul_rn(linspace_at(k, S), T);
  c.beta = __fadd_rn(bmin, __fmul_rn(bdiff, c.tau));
  c.g = (float)__dsqrt_rn((double)c.beta);
  return c;
}

// The rows of a wave over a static grid: 4 rows per wave pass, NW waves per workgroup, gridDim.x workgroups per y.
// `rounds` is the same for every wave (one barrier sequence). An idle column (`valid` false: the ragged last pass)
// reads row 0, computes on zeros and is not stored; stores(): the lane that stores a kept row (its primal column, at
// g = 0). It reads only the arguments and the grid; the kernels build it before their set-up.
template <int NW>
struct Rows {
  long long n, rounds, row = 0, rr = 0;
  int w, g, j, m;
  bool valid = false;
  __device__ __forceinline__ Rows(long long n_, int w_, int g_, int j_, int m_) : n(n_), w(w_), g(g_), j(j_), m(m_) {
    const long long tiles = (n + 3) / 4;
    const long long per_round = (long long)gridDim.x * NW;
    rounds = (tiles + per_round - 1) / per_round;
  }
  __device__ __forceinline__ void seek(long long rd) {
    row = ((rd * gridDim.x + blockIdx.x) * NW + w) * 4 + (j >> 2);
    valid = row < n;
    rr = valid ? row : 0;
  }
  __device__ __forceinline__ bool stores() const { return valid && g == 0 && m == 0; }
};

// a(x, y, tau) of the row on all its lanes, and sum_i da_i/dx_i, from the output tile (rows 4 g + r; the tangent
// column 1 + i carries row i's derivative); cf.g: the Posterior estimator's factor on a and on its divergence
// (nets.py:155-157). The scaling of a keeps the fp32x3 kernels' form, __fmul_rn(cf.g, a[k]); the exact-f32 flow_score
// wrote cf.g * a[k], the same single rounded multiply (HIP's __fmul_rn is the plain operator, and nothing is
// contracted).
template <int MODE, int D, typename V, typename Coef>
__device__ __forceinline__ void gather_score(const V& out, const int& j, const Coef& cf, float (&a)[D], float& dv) {
  const int q0 = j & 12;  // the row's primal column, at g = 0
  dv = 0.0f;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    a[k] = __shfl(out[k], q0, 64);
    dv = dv + __shfl(out[k], q0 + 1 + k, 64);
  }
  if constexpr (MODE == SAMPLER_POSTERIOR) {
#pragma unroll
    for (int k = 0; k < D; ++k) a[k] = __fmul_rn(cf.g, a[k]);
    dv = cf.g * dv;
  }
}

// ---------------------------------------------------------------------------- log p(x | y)
// Forward grid, h = T / S, and for a row x_0 = x
//   v(x, tau)    = -1/2 beta(tau) x - 1/2 g(tau) a(x, y, tau)                 (= -mu(T - tau, x, y, lmbd = 1))
//   divv(x, tau) = -1/2 beta(tau) d - 1/2 g(tau) sum_i da_i/dx_i
// integrated with Heun's explicit trapezoid, k = 0..S-1:
//   k1 = v(x_k, tau_k), x~ = x_k + h k1, k2 = v(x~, tau_{k+1}), x_{k+1} = x_k + (h/2)(k1 + k2)
//   I += (h/2)(divv(x_k, tau_k) + divv(x~, tau_{k+1}))                        (f64: 2S terms)
//   log p(x | y) = -(d/2) log 2 pi - 1/2 |x_S|^2 + I
// `nonfinite` is ORed with "a kept row's I is not finite" (the fp32x3 engine: a tangent beyond the split's range).
template <int D, int NW, typename Score>
__device__ __forceinline__ void logp_rows(const FlowRows& p, Rows<NW>& rows, int yi, bool& nonfinite, Score&& score) {
  const int S = p.num_steps;
  const float hh = __fmul_rn(0.5f, p.h);
  for (long long rd = 0; rd < rows.rounds; ++rd) {
    rows.seek(rd);
    float x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const float xv = p.x[((size_t)yi * p.n + rows.rr) * D + k];
      x[k] = rows.valid ? xv : 0.0f;  // idle columns compute on zeros and are not stored
    }
    double I = 0.0;
    for (int k = 0; k < S; ++k) {
      float k1[D], xt[D], d1 = 0.0f;
#pragma unroll
      for (int i = 0; i < D; ++i) xt[i] = x[i];
      // stage 0: k1 and divv at (x_k, tau_k); stage 1: k2 and divv at (x~, tau_{k+1}) -- one copy of the network code
#pragma unroll 1
      for (int stage = 0; stage < 2; ++stage) {
        const FlowCoef cf = flow_coef(k + stage, S, p.T, p.bmin, p.bdiff);
        float a[D], dv;
        score(xt, cf, a, dv);
        const float dd = -(0.5f * cf.beta * (float)D + 0.5f * cf.g * dv);
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const float kv = -(0.5f * cf.g * a[i] + 0.5f * cf.beta * xt[i]);
          if (stage == 0) {
            k1[i] = kv;
            xt[i] = x[i] + p.h * kv;
          } else {
            x[i] = x[i] + hh * (k1[i] + kv);
          }
        }
        if (stage == 0) d1 = dd;
        else I += (double)hh * ((double)d1 + (double)dd);
      }
    }
    nonfinite |= rows.valid && !__builtin_isfinite(I);
    if (rows.stores()) {
      double r2 = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) r2 += (double)x[i] * (double)x[i];
      const size_t o = (size_t)yi * p.n + rows.row;
      p.logp[o] = (float)(-0.5 * (double)D * 1.8378770664093453 - 0.5 * r2 + I);  // log 2 pi
      if (p.latent) {
#pragma unroll
        for (int i = 0; i < D; ++i) p.latent[o * D + i] = x[i];
      }
    }
  }
}

// ---------------------------------------------------------------------------- samples with their log-density
// Reverse grid of the samplers: tau_i, beta_i, g_i = step_coef(i, S, ...) at lmbd = 1 for i = 0..S, delta = T / S. A
// chain starts at x_0 = mean + std n (the first normals of its stream (seed, chain_offset + row, y index), as every
// sampler) or at row [y][row] of the caller's x0, and for i = 0..S-1
//   k1 = m(x_i, i), x~ = fl(x_i + fl(delta k1)), k2 = m(x~, i + 1), x_{i+1} = fl(x_i + fl(fl(delta/2) fl(k1 + k2)))
//   dm(x, i) = 1/2 g_i sum_j da_j/dx_j (x, y, tau_i) + 1/2 beta_i d           (the divergence of m(., i))
//   J += (delta/2) (dm(x_i, i) + dm(x~, i + 1))                                (f64: 2S terms)
//   log q(x_S | y) = -(d/2) log 2 pi - d log std - 1/2 |(x_0 - mean) / std|^2 - J
// m is HeunStep::slope, so x_S is the Heun sampler's x_S. The base term is folded into the f64 accumulator before the
// step loop: only x and the accumulator live across it. `nonfinite` as logp_rows'.
template <int D, int NW, typename Score>
__device__ __forceinline__ void sample_rows(const FlowChains& p, Rows<NW>& rows, int yi, bool& nonfinite,
                                            Score&& score) {
  const int S = p.num_steps;
  const float hd = __fmul_rn(0.5f, p.delta);
  for (long long rd = 0; rd < rows.rounds; ++rd) {
    rows.seek(rd);
    float x[D];
    if (p.x0) {
      const float* src = p.x0 + ((size_t)yi * p.n + rows.rr) * D;
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = src[k];
    } else {
      Rng rng = rng_init(p.seed, (uint64_t)(p.chain_offset + rows.rr), (uint64_t)yi);
      float n0[D];
      rng_normals<D>(rng, n0);
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = __fadd_rn(__fmul_rn(n0[k], p.stdv), p.mean);
    }
    // acc = log N(x_0; mean, std^2 I) - J, from the f32 x_0 whichever way it came
    double acc = p.base;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double z = ((double)x[k] - (double)p.mean) / (double)p.stdv;
      acc -= 0.5 * z * z;
      x[k] = rows.valid ? x[k] : 0.0f;  // idle columns compute on zeros and are not stored
    }
    for (int i = 0; i < S; ++i) {
      float k1[D], xt[D], d1 = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) xt[k] = x[k];
      // stage 0: k1 and dm at (x_i, i); stage 1: k2 and dm at (x~, i + 1) -- one copy of the network code
#pragma unroll 1
      for (int stage = 0; stage < 2; ++stage) {
        const StepCoef c = step_coef(i + stage, S, p.T, p.bmin, p.bdiff, 0.5f, 0.0f);  // lmbd = 1: g_mu = fl(0.5 g)
        float a[D], dv;
        score(xt, c, a, dv);
        const float dd = 0.5f * c.g * dv + 0.5f * c.beta * (float)D;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float mk = HeunStep::slope(xt[k], a[k], c);
          if (stage == 0) {
            k1[k] = mk;
            xt[k] = HeunStep::predict(x[k], mk, p.delta);
          } else {
            x[k] = HeunStep::correct(x[k], k1[k], mk, p.delta);
          }
        }
        if (stage == 0) d1 = dd;
        else acc -= (double)hd * ((double)d1 + (double)dd);
      }
    }
    nonfinite |= rows.valid && !__builtin_isfinite(acc);
    if (rows.stores()) {
      const size_t o = (size_t)yi * p.n + rows.row;
      p.logq[o] = (float)acc;
#pragma unroll
      for (int k = 0; k < D; ++k) p.x_out[o * D + k] = x[k];
    }
  }
}

// ---------------------------------------------------------------------------- guided sampling, linear problems
// gather_score's sibling that keeps every tangent entry: s_k of the row on all its lanes and J[k][n] = ds_k/dx_n (the
// tangent column 1 + n carries d/dx_n of every output row k)
template <int D, typename V>
__device__ __forceinline__ void gather_jac(const V& out, const int& j, float (&s)[D], float (&J)[D][D]) {
  const int q0 = j & 12;  // the row's primal column, at g = 0
#pragma unroll
  for (int k = 0; k < D; ++k) {
    s[k] = __shfl(out[k], q0, 64);
#pragma unroll
    for (int n = 0; n < D; ++n) J[k][n] = __shfl(out[k], q0 + 1 + n, 64);
  }
}

// var(t) = 1 - exp(-0.5 t^2 (bmax - bmin) - t bmin) in the reference's evaluation order (sdes.py:27-28), beside
// dmip_device.h's vp_mean_weight
__device__ __forceinline__ float vp_var(float t, float bmin, float bdiff) {
  const float a = __fmul_rn(__fmul_rn(-0.5f, __fmul_rn(t, t)), bdiff);
  return __fsub_rn(1.0f, expf(__fsub_rn(a, __fmul_rn(t, bmin))));
}

// Posterior samples of y = A x + b + eta, eta ~ N(0, Sigma), from a prior score network s(x, tau) alone. Reverse grid
// of the samplers at lmbd = 0: tau_i, beta_i, g_i = step_coef(i, S, ...), alpha_i = vp_mean_weight(tau_i), v_i =
// vp_var(tau_i), delta = T / S. A chain starts at x = mean + std n (the first normals of its stream (seed,
// chain_offset + row, y index), as every sampler), draws one rng_normals<D> per step, and for i = 0..S-1
//   s, J = score(x, tau_i)                  J[k][n] = ds_k/dx_n
//   x0h  = (x + v_i s) / alpha_i            (Tweedie)
//   r    = y' - A x0h                       y' = y - b: p.yres
//   u    = B_i^T r                          B_i: row min(i, n_B - 1) of the host's table
//   G    = -(u + v_i J^T u) / alpha_i
//   lam  = zeta delta beta_i (step_rule 0)  or  zeta / sqrt(max(|r|^2, 1e-30)) (step_rule 1)
//   x   <- em_update(x, fl(g_i s), xi) - fl(lam G)
// Sums run over the measurement index first to last, each product rounded (nothing is contracted). A, B_i and y' are
// wave-uniform: plain loads the compiler may issue as scalar ones. Every lane of a row holds its state and does the
// same arithmetic; the only stores are the final x. `nonfinite` is ORed with "a kept row's final state is not finite".
//
// Chains = DpsTweedieChains (a compile-time rule: the DpsLinearChains instantiations hold none of it) puts the
// conditional covariance of Tweedie's second-order formula, Cov[x0 | x_tau] = C = (v / alpha^2) K, K = I + v J, into the
// likelihood of y' given x_tau. With w = B^T r, B = Sigma^-1 A (n_B = 1), and H = A^T Sigma^-1 A (p.H, [D][D]) the push-
// through identity A^T (Sigma + A C A^T)^-1 = (I + H C)^-1 A^T Sigma^-1 leaves one D x D system per row and step:
//   K[k][n]  = [k == n] + v J[k][n]              cs = v / (alpha alpha)
//   Mx[k][n] = [k == n] + sum_r H[k][r] (cs K[r][n])      (r first to last)
//   u        = adj(Mx) w / det(Mx)               (tweedie_solve: cofactors, no pivoting, no guard on det)
// and G, lam (the beta rule) and the update are the ones above with this u. J enters as computed, not symmetrised.
__device__ __forceinline__ void tweedie_solve(const float (&m)[2][2], const float (&w)[2], float (&u)[2]) {
  const float det = m[0][0] * m[1][1] - m[0][1] * m[1][0];
  u[0] = (m[1][1] * w[0] - m[0][1] * w[1]) / det;
  u[1] = (m[0][0] * w[1] - m[1][0] * w[0]) / det;
}
// cof[i][j] = m[i+1][j+1] m[i+2][j+2] - m[i+1][j+2] m[i+2][j+1] (indices mod 3: the signed cofactor), det along row 0,
// u_k = (cof[0][k] w_0 + cof[1][k] w_1 + cof[2][k] w_2) / det
__device__ __forceinline__ void tweedie_solve(const float (&m)[3][3], const float (&w)[3], float (&u)[3]) {
  float cof[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      cof[i][j] = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
    }
  }
  const float det = m[0][0] * cof[0][0] + m[0][1] * cof[0][1] + m[0][2] * cof[0][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = (cof[0][k] * w[0] + cof[1][k] * w[1] + cof[2][k] * w[2]) / det;
}

__device__ __forceinline__ const DpsLinearChains& dps_lin(const DpsLinearChains& p) { return p; }
__device__ __forceinline__ const DpsLinearChains& dps_lin(const DpsTweedieChains& p) { return p.lin; }

template <int D, int NW, typename Chains, typename Score>
__device__ __forceinline__ void dps_linear_rows(const Chains& pc, Rows<NW>& rows, int yi, bool& nonfinite,
                                                Score&& score) {
  constexpr bool kTweedie = std::is_same<Chains, DpsTweedieChains>::value;
  static_assert(!kTweedie || D == 2 || D == 3, "the closed-form solve is written for D = 2 and D = 3");
  const DpsLinearChains& p = dps_lin(pc);
  const int S = p.num_steps, M = p.ydim;
  const float* yr = p.yres + (size_t)yi * M;
  for (long long rd = 0; rd < rows.rounds; ++rd) {
    rows.seek(rd);
    Rng rng = rng_init(p.seed, (uint64_t)(p.chain_offset + rows.rr), (uint64_t)yi);
    float x[D];
    {
      float n0[D];
      rng_normals<D>(rng, n0);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const float xv = __fadd_rn(__fmul_rn(n0[k], p.stdv), p.mean);
        x[k] = rows.valid ? xv : 0.0f;  // idle columns compute on zeros and are not stored
      }
    }
    for (int i = 0; i < S; ++i) {
      const StepCoef c = step_coef(i, S, p.T, p.bmin, p.bdiff);
      float s[D], J[D][D];
      score(x, c, s, J);
      const float mw = vp_mean_weight(c.tau, p.bmin, p.bdiff);
      const float var = vp_var(c.tau, p.bmin, p.bdiff);
      float x0h[D];
#pragma unroll
      for (int k = 0; k < D; ++k) x0h[k] = (x[k] + var * s[k]) / mw;
      const float* Bi = p.B + (size_t)(p.n_B == 1 ? 0 : i) * M * D;
      float u[D], rr = 0.0f;
#pragma unroll
      for (int k = 0; k < D; ++k) u[k] = 0.0f;
#pragma unroll 4
      for (int q = 0; q < M; ++q) {
        float ax = p.A[q * D] * x0h[0];
#pragma unroll
        for (int k = 1; k < D; ++k) ax = ax + p.A[q * D + k] * x0h[k];
        const float r = yr[q] - ax;
        rr = rr + r * r;
#pragma unroll
        for (int k = 0; k < D; ++k) u[k] = u[k] + Bi[q * D + k] * r;
      }
      if constexpr (kTweedie) {
        const float cs = var / (mw * mw);
        float Kc[D][D], Mx[D][D], wv[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
          wv[k] = u[k];
#pragma unroll
          for (int n = 0; n < D; ++n) Kc[k][n] = cs * ((k == n ? 1.0f : 0.0f) + var * J[k][n]);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
#pragma unroll
          for (int n = 0; n < D; ++n) {
            float a = k == n ? 1.0f : 0.0f;
#pragma unroll
            for (int r = 0; r < D; ++r) a = a + pc.H[k * D + r] * Kc[r][n];
            Mx[k][n] = a;
          }
        }
        tweedie_solve(Mx, wv, u);
      }
      const float lam = p.step_rule == 0 ? p.zeta * p.delta * c.beta : p.zeta / sqrtf(fmaxf(rr, 1e-30f));
      float xi[D];
      rng_normals<D>(rng, xi);
      float xn[D];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        float jt = u[k];
#pragma unroll
        for (int r = 0; r < D; ++r) jt = jt + var * J[r][k] * u[r];
        const float G = -(jt / mw);
        const float xe = em_update(x[k], __fmul_rn(c.g, s[k]), xi[k], c, p.delta, p.sqrt_delta);
        xn[k] = xe - lam * G;
      }
#pragma unroll
      for (int k = 0; k < D; ++k) x[k] = xn[k];
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < D; ++k) finite &= __builtin_isfinite(x[k]);
    nonfinite |= rows.valid && !finite;
    if (rows.stores()) {
      const size_t o = (size_t)yi * p.n + rows.row;
#pragma unroll
      for (int k = 0; k < D; ++k) p.x_out[o * D + k] = x[k];
    }
  }
}

}  // namespace flow

// ----------------------------------------------------------------- launch helpers (per TU)
// the static grid of the four kernels: at most one resident wave set per y, no more workgroups than 4-row passes
template <typename K>
inline unsigned flow_grid_x(K kern, int nw, long long n, int n_y, hipStream_t st) {
  const long long tiles = (n + 3) / 4;
  long long g = resident_slots(kern, nw * 64, st) / (n_y > 0 ? n_y : 1);
  const long long cap = (tiles + nw - 1) / nw;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// n: the rows (chains) per y of p
template <typename K, typename P>
inline hipError_t flow_launch(K kern, int nw, const P& p, long long n, int n_y, hipStream_t st) {
  const unsigned g = flow_grid_x(kern, nw, n, n_y, st);
  hipLaunchKernelGGL(kern, dim3(g, (unsigned)n_y), dim3(nw * 64), 0, st, p);
  return hipGetLastError();
}

// the (width, xdim) pairs every dispatcher compiles: X(width, xdim) per shape
#define DMIP_FLOW_SHAPES(X) X(64, 2) X(128, 2) X(256, 2) X(512, 2) X(64, 3) X(128, 3) X(256, 3) X(512, 3)

}  // namespace dmip
