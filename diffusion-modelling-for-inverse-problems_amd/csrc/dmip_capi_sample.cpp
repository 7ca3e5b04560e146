// libdmip.so C-ABI, sampling entry points: the fused samplers of the three engines (16-bit, exact f32, fp32x3), the
// surrogate's forward / log-posterior, MH and DPS, the RNG and schedule probes, and the samplers' *_supported queries
// (the probability-flow entry points: dmip_capi_flow.cpp). Argument validation first, then stream-ordered launches.
#include "dmip_capi_common.h"

using namespace dmip_capi;

namespace {

// test hook (not ABI): DMIP_DEBUG_NO_HANDOVER=1 makes the balanced sampler's producers never publish
// their hand-over, with a short spin bound, so the consumer's timeout path runs
int debug_no_handover() {
  const char* e = getenv("DMIP_DEBUG_NO_HANDOVER");
  return e && e[0] == '1' ? 1 : 0;
}

// What every sampler entry point takes (the C-ABI's argument order), then what only some of them set.
struct SampleArgs {
  const dmip_vpsde* sde;
  const float* y_dev;
  int n_y, ydim, xdim;
  int64_t n_chains, chain_offset;
  int num_steps;
  float mean, stdv;
  uint64_t seed;
  int precision;
  float* x_out_dev;
  void* stream;
  SampleArgs(const dmip_vpsde* sde, const float* y_dev, int n_y, int ydim, int xdim, int64_t n_chains,
             int64_t chain_offset, int num_steps, float mean, float stdv, uint64_t seed, int precision,
             float* x_out_dev, void* stream)
      : sde(sde), y_dev(y_dev), n_y(n_y), ydim(ydim), xdim(xdim), n_chains(n_chains), chain_offset(chain_offset),
        num_steps(num_steps), mean(mean), stdv(stdv), seed(seed), precision(precision), x_out_dev(x_out_dev),
        stream(stream) {}
  const float* noise_dev = nullptr;
  uint64_t* stamps = nullptr;
  int n_corr = 0;
  float snr = 0.16f;
  int snap_every = 0;
  float* snap_out_dev = nullptr;
  double lmbd = 0.0;  // sdes.py:77-87: 0 the reverse SDE, 1 the probability-flow ODE (CDE and Posterior)
  int solver = DMIP_SOLVER_EULER;   // DMIP_SOLVER_HEUN: dmip_ode_sample's second-order ODE steps (lmbd = 1)
  const float* x0_dev = nullptr;    // Heun: start states [n_y][n_chains][xdim] in place of randn stdv + mean
  // dmip_multistep_sample: the step table [num_steps][kMultistepCols]; its launch is SOLVER_TABLE whatever `solver`
  const float* table_dev = nullptr;
  bool table_sde = false;           // dmip_multistep_sde_sample: SOLVER_TABLE_SDE (the table's column 7 is read)
};

// the fields SamplerParams, F32SamplerParams and X3SamplerParams share. c_mu / c_sig are step_coef's lambda factors:
// the Python scalars (1 - 0.5 lmbd) and (1 - lmbd) ** 0.5, evaluated in double and rounded once to the f32 torch
// multiplies the tensor g by (exactly 1, 1 at lmbd = 0)
template <typename P>
int fill_common(P& p, const SampleArgs& a, hipStream_t st) {
  p.y_obs = a.y_dev;
  p.n_corr = a.n_corr;
  p.snr = a.snr;
  p.noise = a.noise_dev;
  p.x_out = a.x_out_dev;
  p.snap_out = a.snap_out_dev;
  p.snap_every = a.snap_every;
  p.n_chains = a.n_chains;
  p.chain_offset = a.chain_offset;
  p.num_steps = a.num_steps;
  fill_schedule(*a.sde, a.num_steps, p.T, p.bmin, p.bdiff, p.delta, &p.sqrt_delta);
  p.c_mu = (float)(1.0 - 0.5 * a.lmbd);
  p.c_sig = (float)std::sqrt(1.0 - a.lmbd);
  p.mean = a.mean;
  p.stdv = a.stdv;
  p.seed = a.seed;
  if (int rc = status_word_or_fail(p.err, st)) return rc;
  p.debug_flags = debug_no_handover();
  p.spin_limit = p.debug_flags ? (1u << 10) : (1u << 22);
  return DMIP_OK;
}

// exact-f32 samplers (dmip_f32.h): same loop, RNG and sharding as the 16-bit kernels; arguments
// already validated by em_sample_impl
int em_sample_f32(int mode, const dmip_mlp* net0, const dmip_mlp* net1, const SampleArgs& a) {
  const int xdim = a.xdim, ydim = a.ydim;
  if (!dmip::f32_sampler_supported(mode, net0->width, net0->n_hidden, xdim, ydim))
    return no_kernel("f32 sampler", mode, net0, xdim, ydim);
  hipStream_t st = (hipStream_t)a.stream;
  dmip::F32SamplerParams p{};
  p.net[0] = f32_net(net0);
  if (net1) p.net[1] = f32_net(net1);
  p.n_hidden = net0->n_hidden;
  StreamScratch l1y;
  if (mode != DMIP_SAMPLER_CDIFFE) {
    if (int rc = f32_l1_prep(l1y, net0, a.y_dev, a.n_y, xdim, ydim, st)) return rc;
    p.l1y = (float*)l1y.ptr;
  }
  if (int rc = fill_common(p, a, st)) return rc;
  p.act = f32_act(net0);
  p.solver = a.table_dev ? (a.table_sde ? dmip::kSolverTableSde : dmip::kSolverTable) : a.solver;
  p.x0 = a.x0_dev;
  p.table = a.table_dev;
  bool ok = false;
  hipError_t e = dmip::launch_f32_sampler(p, mode, net0->width, net0->n_hidden, xdim, ydim, a.n_y, st, &ok);
  if (!ok) return fail(DMIP_ERR_UNSUPPORTED, "no compiled f32 sampler");
  if (e != hipSuccess) return hip_fail(e, "f32 sampler launch");
  return DMIP_OK;
}

// DMIP_X3K=0 selects the one-tile-per-wave fp32x3 engine (dmip_x3.h) at the k-major engine's shape too
// (A/B and parity of the two engines; not part of the ABI)
bool x3k_enabled() {
  const char* e = getenv("DMIP_X3K");
  return !(e && e[0] == '0');
}
#ifdef DMIP_WITH_X3P
// A/B library only (make diag): DMIP_X3P=1 selects the paired-tile 32x32 engine (dmip_x3p.h) instead of the
// 16x16 k-major one (dmip_x3k.h) at its shape. It measured slower (profiles/r4_ab_x3p_vs_x3k.json), so the
// product library libdmip.so does not contain it.
bool x3p_enabled() {
  const char* e = getenv("DMIP_X3P");
  return e && e[0] == '1';
}
#endif

// fp32-accurate split-fp16 samplers (dmip_x3.h): same loop, RNG and sharding as the other engines;
// arguments already validated by em_sample_impl
int em_sample_x3(int mode, const dmip_mlp* net0, const dmip_mlp* net1, const SampleArgs& a) {
  const int xdim = a.xdim, ydim = a.ydim;
  if (int rc = x3_check_range(net0, net1)) return rc;
  if (!dmip::x3_sampler_supported(mode, net0->width, net0->n_hidden, xdim, ydim) || !net0->x3_stream ||
      (mode == DMIP_SAMPLER_CDIFFE && !net0->x3_l1_full) || (net1 && !net1->x3_stream))
    return no_kernel("f32x3 sampler", mode, net0, xdim, ydim);
  hipStream_t st = (hipStream_t)a.stream;
  dmip::X3SamplerParams p{};
  p.net[0] = x3_net(net0);
  if (mode == DMIP_SAMPLER_CDIFFE) p.net[0].l1 = net0->x3_l1_full;  // every input column
  if (mode == DMIP_SAMPLER_CDIFFE && net0->x3_stream_l1r) p.net[0].stream = net0->x3_stream_l1r;  // L1R layout
  if (net1) p.net[1] = x3_net(net1);
  p.n_hidden = net0->n_hidden;
  StreamScratch bias_y;
  // Heun and the table-driven multistep sampler: the one-tile engine only (dmip_x3.h); x3s / x3k keep Euler
  const bool heun = a.solver == DMIP_SOLVER_HEUN || a.table_dev;
  if (!heun && dmip::x3s_sampler_eligible(mode, net0->width, net0->n_hidden, xdim, a.n_chains, a.n_y)) {
    // the width-64 latency engine forms the per-y bias itself (round 6: one launch and one allocation fewer)
    p.l1w = net0->w1;
    p.l1b = net0->b1;
    p.l1_in = net0->in_dim;
    p.ydim = ydim;
  } else if (mode != DMIP_SAMPLER_CDIFFE) {
    if (int rc = x3_bias_prep(bias_y, net0, a.y_dev, a.n_y, xdim, ydim, st)) return rc;
  }
  p.bias_y = (float*)bias_y.ptr;
  if (int rc = fill_common(p, a, st)) return rc;
  p.solver = a.table_dev ? (a.table_sde ? dmip::kSolverTableSde : dmip::kSolverTable) : a.solver;
  p.x0 = a.x0_dev;
  p.table = a.table_dev;
  bool ok = false;
  hipError_t e;
#ifdef DMIP_WITH_X3P
  if (!heun && mode == DMIP_SAMPLER_CDE && net0->x3p_stream && dmip::x3p_sampler_supported(mode, net0->width, net0->n_hidden, xdim) &&
      x3k_enabled() && x3p_enabled()) {
    // the paired-tile 32x32 engine at its shape (dmip_x3p.h; A/B library only)
    p.net[0].pstream = net0->x3p_stream;
    p.net[0].pl1 = net0->x3p_l1;
    p.net[0].pow = net0->x3p_ow;
    e = dmip::launch_x3p_sampler(p, xdim, a.n_y, st, &ok);
  } else
#endif
  if (!heun && mode == DMIP_SAMPLER_CDE && net0->x3k_stream &&
             dmip::x3k_sampler_supported(mode, net0->width, net0->n_hidden, xdim) && x3k_enabled()) {
    // the k-major multi-tile engine at its shape (dmip_x3k.h)
    p.net[0].kstream = net0->x3k_stream;
    p.net[0].kout = net0->x3k_out;
    e = dmip::launch_x3k_sampler(p, xdim, a.n_y, st, &ok);
  } else {
    e = dmip::launch_x3_sampler(p, mode, net0->width, net0->n_hidden, xdim, ydim, a.n_y, st, &ok);
  }
  if (!ok) return fail(DMIP_ERR_UNSUPPORTED, "no compiled f32x3 sampler");
  if (e != hipSuccess) return hip_fail(e, "f32x3 sampler launch");
  return DMIP_OK;
}

// the 16-bit samplers (dmip_kernels.hip); arguments already validated by em_sample_impl
int em_sample_16(int mode, const dmip_mlp* net0, const dmip_mlp* net1, const SampleArgs& a) {
  const int xdim = a.xdim, ydim = a.ydim;
  if (!dmip::sampler_shape_supported(mode, net0->width, net0->n_hidden, xdim, ydim))
    return no_kernel("sampler", mode, net0, xdim, ydim);
  hipStream_t st = (hipStream_t)a.stream;
  dmip::SamplerParams p{};
  StreamScratch a1;
  p.hidden = net0->hidden;
  if (mode == DMIP_SAMPLER_CDIFFE) {
    // y_t varies per chain: layer 1 takes every input column (the forward kernel's image); at width 512
    // the split layer-1 image streams through the ring ahead of the hidden chunks
    p.a1 = net0->a1_full;
    p.a1_per_y = 0;
    if (net0->width == 512) {
      if (!net0->ring_l1) return fail(DMIP_ERR_UNSUPPORTED, "no ring image for this network");
      p.hidden = net0->ring_l1;
    }
  } else {
    // y is constant per y index: fold W1_y y + b1 into a per-y layer-1 bias
    const int T = net0->width / 32;
    const int k1s = k1s_for(3 * (xdim + 1) + 2);
    if (int rc = a1.alloc((size_t)a.n_y * T * k1s * 1024, st)) return rc;
    dmip::A1PrepParams ap{};
    ap.w1 = net0->w1;
    ap.b1 = net0->b1;
    ap.y = a.y_dev;
    ap.a1 = (char*)a1.ptr;
    ap.width = net0->width;
    ap.in_dim = net0->in_dim;
    ap.xdim = xdim;
    ap.ydim = ydim;
    ap.y_col0 = xdim;
    ap.t_col = net0->in_dim - 1;
    ap.k1s = k1s;
    const hipError_t e = dmip::launch_a1_prep(ap, a.n_y, st);
    if (e != hipSuccess) return hip_fail(e, "a1_prep launch");
    p.a1 = (char*)a1.ptr;
    p.a1_per_y = 1;
  }
  p.ao = net0->ao_samp;
  p.bias_hidden = net0->bias_hidden;
  p.bias_out = net0->bias_out_samp;
  if (mode == DMIP_SAMPLER_POSTERIOR) {
    // the prior's (x, t) layer-1 image is the sampler's B1 slot layout over (x, tau)
    p.hidden2 = net1->hidden;
    p.a1_2 = net1->a1_full;
    p.ao2 = net1->ao_samp;
    p.bias_hidden2 = net1->bias_hidden;
    p.bias_out2 = net1->bias_out_samp;
  }
  p.stamps = (unsigned long long*)a.stamps;
  if (int rc = fill_common(p, a, st)) return rc;
  bool ok = false;
  hipError_t e = dmip::launch_sampler(p, mode, net0->width, net0->n_hidden, xdim, ydim, a.n_y, st, &ok);
  if (!ok) return fail(DMIP_ERR_UNSUPPORTED, "no compiled sampler");
  if (e != hipSuccess) return hip_fail(e, "em_sampler launch");
  return DMIP_OK;
}

// every sampler entry point ends here. net0: the CDE / CDiffE network or the Posterior likelihood; `prior` is used
// in Posterior mode only
int em_sample_impl(int mode, const dmip_mlp* net0, const dmip_mlp* prior, const SampleArgs& a) {
  const dmip_mlp* net1 = mode == DMIP_SAMPLER_POSTERIOR ? prior : nullptr;
  const int xdim = a.xdim, ydim = a.ydim;
  if (!net0 || !a.sde || !a.y_dev || !a.x_out_dev || (mode == DMIP_SAMPLER_POSTERIOR && !net1))
    return fail(DMIP_ERR_INVALID, "null argument");
  if (a.precision != DMIP_PREC_FP16 && a.precision != DMIP_PREC_F32 && a.precision != DMIP_PREC_F32X3)
    return fail(DMIP_ERR_INVALID, "unknown precision");
  if (a.noise_dev && mode != DMIP_SAMPLER_CDE) return fail(DMIP_ERR_INVALID, "noise injection: CDE sampler only");
  if (int rc = check_nets("sampler", net0, net1, mode == DMIP_SAMPLER_CDIFFE ? xdim + ydim : xdim, xdim, ydim, a.n_y,
                          false, a.n_chains, a.chain_offset, a.num_steps, a.sde))
    return rc;
  if (!(a.lmbd >= 0.0 && a.lmbd <= 1.0)) return fail(DMIP_ERR_INVALID, "lmbd must be in [0, 1]");
  if (a.lmbd != 0.0 && mode == DMIP_SAMPLER_CDIFFE)
    return fail(DMIP_ERR_INVALID, "lmbd != 0: CDE and Posterior samplers only");
  if (f32_act(net0) || (net1 && f32_act(net1))) {
    if (a.precision != DMIP_PREC_F32 || mode != DMIP_SAMPLER_CDE) return act_refused("em_sample");
  }
  if (a.solver == DMIP_SOLVER_HEUN &&
      !(a.precision == DMIP_PREC_F32
            ? dmip::f32_heun_supported(mode, net0->width, net0->n_hidden, xdim, f32_act(net0))
            : dmip_ode_sample_supported(mode, net0->width, net0->n_hidden, xdim, ydim, a.precision, a.solver)))
    return no_kernel("Heun sampler", mode, net0, xdim, -1, a.precision);
  if (a.table_dev && a.table_sde &&
      !(a.precision == DMIP_PREC_F32
            ? dmip::f32_multistep_sde_supported(mode, net0->width, net0->n_hidden, xdim, f32_act(net0))
            : dmip_multistep_sde_supported(mode, net0->width, net0->n_hidden, xdim, ydim, a.precision)))
    return no_kernel("stochastic multistep sampler", mode, net0, xdim, -1, a.precision);
  if (a.table_dev && !a.table_sde &&
      !(a.precision == DMIP_PREC_F32
            ? dmip::f32_multistep_supported(mode, net0->width, net0->n_hidden, xdim, f32_act(net0))
            : dmip_multistep_supported(mode, net0->width, net0->n_hidden, xdim, ydim, a.precision)))
    return no_kernel("multistep sampler", mode, net0, xdim, -1, a.precision);
  if (a.n_chains == 0) return DMIP_OK;
  if (a.precision == DMIP_PREC_F32) return em_sample_f32(mode, net0, net1, a);
  if (a.precision == DMIP_PREC_F32X3) return em_sample_x3(mode, net0, net1, a);
  return em_sample_16(mode, net0, net1, a);
}

int check_corrector(int corrector_steps, float snr) {
  if (corrector_steps < 0) return fail(DMIP_ERR_INVALID, "corrector_steps must be >= 0");
  if (corrector_steps > 0 && !(snr > 0.0f)) return fail(DMIP_ERR_INVALID, "snr must be > 0");
  return DMIP_OK;
}

// dmip_em_sample_lmbd's and dmip_ode_sample's optional snapshots
int check_snapshots(int snapshot_every, int num_steps, const float* snap_out_dev) {
  if (snapshot_every < 0 || (snapshot_every > 0 && (snapshot_every > num_steps || !snap_out_dev)))
    return fail(DMIP_ERR_INVALID, "snapshot_every must be 0 or in [1, num_steps] with a snapshot buffer");
  return DMIP_OK;
}

}  // namespace

extern "C" {

int dmip_sampler_supported(int mode, int width, int n_hidden, int xdim, int ydim) {
  return dmip::sampler_shape_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
}

int dmip_sampler_supported_f32(int mode, int width, int n_hidden, int xdim, int ydim) {
  return dmip::f32_sampler_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
}

int dmip_sampler_supported_precision(int precision, int mode, int width, int n_hidden, int xdim, int ydim) {
  switch (precision) {
    case DMIP_PREC_FP16: return dmip::sampler_shape_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
    case DMIP_PREC_F32: return dmip::f32_sampler_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
    case DMIP_PREC_F32X3: return dmip::x3_sampler_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
    default: return 0;
  }
}

int dmip_em_sample(const dmip_mlp* net, const dmip_vpsde* sde, const float* y_dev, int n_y, int ydim, int xdim,
                   int64_t n_chains, int64_t chain_offset, int num_steps, float mean, float stdv, uint64_t seed,
                   int precision, const float* noise_dev, float* x_out_dev, void* stream) {
  SampleArgs a(sde, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps, mean, stdv, seed, precision, x_out_dev,
               stream);
  a.noise_dev = noise_dev;
  return em_sample_impl(DMIP_SAMPLER_CDE, net, nullptr, a);
}

int dmip_em_sample_posterior(const dmip_mlp* prior, const dmip_mlp* likelihood, const dmip_vpsde* sde,
                             const float* y_dev, int n_y, int ydim, int xdim, int64_t n_chains, int64_t chain_offset,
                             int num_steps, float mean, float stdv, uint64_t seed, int precision, float* x_out_dev,
                             void* stream) {
  if (!prior) return fail(DMIP_ERR_INVALID, "null argument");
  const SampleArgs a(sde, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps, mean, stdv, seed, precision,
                     x_out_dev, stream);
  return em_sample_impl(DMIP_SAMPLER_POSTERIOR, likelihood, prior, a);
}

int dmip_em_sample_cdiffe(const dmip_mlp* net, const dmip_vpsde* sde, const float* y_dev, int n_y, int ydim, int xdim,
                          int64_t n_chains, int64_t chain_offset, int num_steps, float mean, float stdv, uint64_t seed,
                          int precision, int corrector_steps, float snr, float* x_out_dev, void* stream) {
  if (int rc = check_corrector(corrector_steps, snr)) return rc;
  SampleArgs a(sde, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps, mean, stdv, seed, precision, x_out_dev,
               stream);
  a.n_corr = corrector_steps;
  a.snr = snr;
  return em_sample_impl(DMIP_SAMPLER_CDIFFE, net, nullptr, a);
}

int dmip_em_sample_snapshots(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde,
                             const float* y_dev, int n_y, int ydim, int xdim, int64_t n_chains, int64_t chain_offset,
                             int num_steps, float mean, float stdv, uint64_t seed, int precision, int corrector_steps,
                             float snr, int snapshot_every, float* snap_out_dev, float* x_out_dev, void* stream) {
  if (mode != DMIP_SAMPLER_CDE && mode != DMIP_SAMPLER_POSTERIOR && mode != DMIP_SAMPLER_CDIFFE)
    return fail(DMIP_ERR_INVALID, "unknown sampler mode");
  if (snapshot_every < 1 || snapshot_every > num_steps)
    return fail(DMIP_ERR_INVALID, "snapshot_every must be in [1, num_steps]");
  if (!snap_out_dev) return fail(DMIP_ERR_INVALID, "null snapshot buffer");
  if (mode == DMIP_SAMPLER_POSTERIOR && !prior) return fail(DMIP_ERR_INVALID, "null argument");
  if (mode != DMIP_SAMPLER_CDIFFE && corrector_steps != 0)
    return fail(DMIP_ERR_INVALID, "corrector steps: CDiffE sampler only");
  if (int rc = check_corrector(corrector_steps, snr)) return rc;
  SampleArgs a(sde, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps, mean, stdv, seed, precision, x_out_dev,
               stream);
  a.n_corr = corrector_steps;
  a.snr = snr;
  a.snap_every = snapshot_every;
  a.snap_out_dev = snap_out_dev;
  return em_sample_impl(mode, net, prior, a);
}

int dmip_em_sample_lmbd(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde, const float* y_dev,
                        int n_y, int ydim, int xdim, int64_t n_chains, int64_t chain_offset, int num_steps, float mean,
                        float stdv, uint64_t seed, int precision, double lmbd, const float* noise_dev,
                        int snapshot_every, float* snap_out_dev, float* x_out_dev, void* stream) {
  if (mode != DMIP_SAMPLER_CDE && mode != DMIP_SAMPLER_POSTERIOR)
    return fail(DMIP_ERR_INVALID, "em_sample_lmbd: CDE and Posterior samplers only");
  if (mode == DMIP_SAMPLER_POSTERIOR && !prior) return fail(DMIP_ERR_INVALID, "null argument");
  if (!(lmbd >= 0.0 && lmbd <= 1.0)) return fail(DMIP_ERR_INVALID, "lmbd must be in [0, 1]");
  if (num_steps < 1) return fail(DMIP_ERR_INVALID, "num_steps must be >= 1");
  if (int rc = check_snapshots(snapshot_every, num_steps, snap_out_dev)) return rc;
  SampleArgs a(sde, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps, mean, stdv, seed, precision, x_out_dev,
               stream);
  a.noise_dev = noise_dev;
  a.snap_every = snapshot_every;
  a.snap_out_dev = snapshot_every > 0 ? snap_out_dev : nullptr;
  a.lmbd = lmbd;
  return em_sample_impl(mode, net, prior, a);
}

// Euler: what dmip_em_sample_lmbd runs (any precision); Heun: the exact-f32 and the one-tile fp32x3 engines (there is
// no 16-bit Heun kernel). The answer is for the tanh chain, as dmip_sampler_supported_precision's: a SiLU CDE network
// has its exact-f32 Heun kernel at every shape of the exact-f32 CDE sampler
int dmip_ode_sample_supported(int mode, int width, int n_hidden, int xdim, int ydim, int precision, int solver) {
  if (mode != DMIP_SAMPLER_CDE && mode != DMIP_SAMPLER_POSTERIOR) return 0;
  if (solver == DMIP_SOLVER_EULER)
    return dmip_sampler_supported_precision(precision, mode, width, n_hidden, xdim, ydim);
  if (solver != DMIP_SOLVER_HEUN) return 0;
  if (precision == DMIP_PREC_F32) return dmip::f32_heun_supported(mode, width, n_hidden, xdim, 0) ? 1 : 0;
  if (precision == DMIP_PREC_F32X3) return dmip::x3_heun_supported(mode, width, n_hidden, xdim) ? 1 : 0;
  return 0;
}

// the probability-flow ODE sampler (lmbd = 1) by solver; every argument is validated before any device work
int dmip_ode_sample(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde, const float* y_dev,
                    int n_y, int ydim, int xdim, int64_t n_chains, int64_t chain_offset, int num_steps, float mean,
                    float stdv, uint64_t seed, int precision, int solver, const float* x0_dev, int snapshot_every,
                    float* snap_out_dev, float* x_out_dev, void* stream) {
  if (mode != DMIP_SAMPLER_CDE && mode != DMIP_SAMPLER_POSTERIOR)
    return fail(DMIP_ERR_INVALID, "ode_sample: CDE and Posterior samplers only");
  if (solver != DMIP_SOLVER_EULER && solver != DMIP_SOLVER_HEUN) return fail(DMIP_ERR_INVALID, "unknown solver");
  if (num_steps < 1) return fail(DMIP_ERR_INVALID, "num_steps must be >= 1");
  if (int rc = check_snapshots(snapshot_every, num_steps, snap_out_dev)) return rc;
  if (solver == DMIP_SOLVER_EULER && x0_dev)
    return fail(DMIP_ERR_UNSUPPORTED, "ode_sample: x0_dev needs DMIP_SOLVER_HEUN (the Euler samplers start from "
                                      "injected noise: dmip_em_sample_lmbd's noise_dev)");
  if (!net || !sde || !y_dev || !x_out_dev || (mode == DMIP_SAMPLER_POSTERIOR && !prior))
    return fail(DMIP_ERR_INVALID, "null argument");
  if (solver == DMIP_SOLVER_EULER)
    return dmip_em_sample_lmbd(mode, net, prior, sde, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps, mean,
                               stdv, seed, precision, 1.0, nullptr, snapshot_every, snap_out_dev, x_out_dev, stream);
  SampleArgs a(sde, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps, mean, stdv, seed, precision, x_out_dev,
               stream);
  a.snap_every = snapshot_every;
  a.snap_out_dev = snapshot_every > 0 ? snap_out_dev : nullptr;
  a.lmbd = 1.0;
  a.solver = DMIP_SOLVER_HEUN;
  a.x0_dev = x0_dev;
  return em_sample_impl(mode, net, prior, a);
}

// the table-driven few-step samplers (dmip_device.h MultistepStep): the exact-f32 and the one-tile fp32x3 engines at
// the shapes of their Heun kernels; the answer is for the tanh chain (as dmip_ode_sample_supported's)
int dmip_multistep_supported(int mode, int width, int n_hidden, int xdim, int ydim, int precision) {
  if (mode != DMIP_SAMPLER_CDE && mode != DMIP_SAMPLER_POSTERIOR) return 0;
  if (precision == DMIP_PREC_F32) return dmip::f32_multistep_supported(mode, width, n_hidden, xdim, 0) ? 1 : 0;
  if (precision == DMIP_PREC_F32X3) return dmip::x3_multistep_supported(mode, width, n_hidden, xdim) ? 1 : 0;
  return 0;
}

// the stochastic variant's kernels (SOLVER_TABLE_SDE), at the same shapes
int dmip_multistep_sde_supported(int mode, int width, int n_hidden, int xdim, int ydim, int precision) {
  if (mode != DMIP_SAMPLER_CDE && mode != DMIP_SAMPLER_POSTERIOR) return 0;
  if (precision == DMIP_PREC_F32) return dmip::f32_multistep_sde_supported(mode, width, n_hidden, xdim, 0) ? 1 : 0;
  if (precision == DMIP_PREC_F32X3) return dmip::x3_multistep_sde_supported(mode, width, n_hidden, xdim) ? 1 : 0;
  return 0;
}

// DPM-Solver++(2M) / DDIM from a step table (sde: with the noise column and a draw per step); every argument is
// validated before any device work, in dmip_ode_sample's order. The kernels take every time-dependent quantity from the
// table, so there is no dmip_vpsde here
static int multistep_sample_impl(bool sde, int mode, const dmip_mlp* net, const dmip_mlp* prior, const float* y_dev,
                                 int n_y, int ydim, int xdim, int64_t n_chains, int64_t chain_offset, int num_steps,
                          const float* table_dev, int table_cols, float mean, float stdv, uint64_t seed, int precision,
                          const float* x0_dev, int snapshot_every, float* snap_out_dev, float* x_out_dev, void* stream) {
  if (mode != DMIP_SAMPLER_CDE && mode != DMIP_SAMPLER_POSTERIOR)
    return fail(DMIP_ERR_INVALID, sde ? "multistep_sde_sample: CDE and Posterior samplers only"
                                      : "multistep_sample: CDE and Posterior samplers only");
  if (table_cols != DMIP_MULTISTEP_COLS)
    return fail(DMIP_ERR_INVALID, sde ? "multistep_sde_sample: table_cols must be DMIP_MULTISTEP_COLS"
                                      : "multistep_sample: table_cols must be DMIP_MULTISTEP_COLS");
  if (num_steps < 1) return fail(DMIP_ERR_INVALID, "num_steps must be >= 1");
  if (int rc = check_snapshots(snapshot_every, num_steps, snap_out_dev)) return rc;
  if (!net || !table_dev || !y_dev || !x_out_dev || (mode == DMIP_SAMPLER_POSTERIOR && !prior))
    return fail(DMIP_ERR_INVALID, "null argument");
  if (precision == DMIP_PREC_FP16)
    return fail(DMIP_ERR_UNSUPPORTED,
                sde ? "multistep_sde_sample: no 16-bit kernel (DMIP_PREC_F32X3 or DMIP_PREC_F32)"
                    : "multistep_sample: no 16-bit kernel (DMIP_PREC_F32X3 or DMIP_PREC_F32)");
  static const dmip_vpsde no_sde{0.0, 0.0, 1.0};  // (the launch's schedule fields are unused by SOLVER_TABLE[_SDE])
  SampleArgs a(&no_sde, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps, mean, stdv, seed, precision,
               x_out_dev, stream);
  a.snap_every = snapshot_every;
  a.snap_out_dev = snapshot_every > 0 ? snap_out_dev : nullptr;
  a.lmbd = 1.0;
  a.x0_dev = x0_dev;
  a.table_dev = table_dev;
  a.table_sde = sde;
  return em_sample_impl(mode, net, prior, a);
}

int dmip_multistep_sample(int mode, const dmip_mlp* net, const dmip_mlp* prior, const float* y_dev, int n_y, int ydim,
                          int xdim, int64_t n_chains, int64_t chain_offset, int num_steps, const float* table_dev,
                          int table_cols, float mean, float stdv, uint64_t seed, int precision, const float* x0_dev,
                          int snapshot_every, float* snap_out_dev, float* x_out_dev, void* stream) {
  return multistep_sample_impl(false, mode, net, prior, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps,
                               table_dev, table_cols, mean, stdv, seed, precision, x0_dev, snapshot_every, snap_out_dev,
                               x_out_dev, stream);
}

// the stochastic few-step samplers: the same table with column 7 = cn, one draw per step (include/dmip.h)
int dmip_multistep_sde_sample(int mode, const dmip_mlp* net, const dmip_mlp* prior, const float* y_dev, int n_y,
                              int ydim, int xdim, int64_t n_chains, int64_t chain_offset, int num_steps,
                              const float* table_dev, int table_cols, float mean, float stdv, uint64_t seed,
                              int precision, const float* x0_dev, int snapshot_every, float* snap_out_dev,
                              float* x_out_dev, void* stream) {
  return multistep_sample_impl(true, mode, net, prior, y_dev, n_y, ydim, xdim, n_chains, chain_offset, num_steps,
                               table_dev, table_cols, mean, stdv, seed, precision, x0_dev, snapshot_every, snap_out_dev,
                               x_out_dev, stream);
}

int dmip_em_sample_stamps(const dmip_mlp* net, const dmip_vpsde* sde, const float* y_dev, int n_y, int ydim,
                          int xdim, int64_t n_chains, int num_steps, uint64_t seed, float* x_out_dev,
                          uint64_t* stamps_dev, void* stream) {
  if (!stamps_dev) return fail(DMIP_ERR_INVALID, "null stamps buffer");
  SampleArgs a(sde, y_dev, n_y, ydim, xdim, n_chains, /*chain_offset=*/0, num_steps, /*mean=*/0.0f, /*stdv=*/1.0f,
               seed, DMIP_PREC_FP16, x_out_dev, stream);
  a.stamps = stamps_dev;
  return em_sample_impl(DMIP_SAMPLER_CDE, net, nullptr, a);
}

}  // extern "C"

// ------------------------------------------------------------------- scatterometry surrogate: forward, MH, DPS
namespace {

int surrogate_check(const dmip_surrogate* s, int64_t n) {
  if (!s) return fail(DMIP_ERR_INVALID, "null surrogate handle");
  if (n < 0) return fail(DMIP_ERR_INVALID, "n < 0");
  return DMIP_OK;
}

int noise_check(const dmip_scat_noise* nz, dmip::SurrogateParams& p) {
  if (!nz) return fail(DMIP_ERR_INVALID, "null noise model");
  if (!(nz->b > 0.0f) || !(nz->a >= 0.0f) || !(nz->lambd_bd >= 0.0f))
    return fail(DMIP_ERR_INVALID, "noise model needs b > 0, a >= 0, lambd_bd >= 0");
  p.a = nz->a;
  p.b2 = (float)((double)nz->b * (double)nz->b);  // python b**2, rounded once to f32 (torch scalar add)
  p.lam = nz->lambd_bd;
  return DMIP_OK;
}

// what dmip_mh_sample and the fp32x3 path of dmip_mh_sample_ex check alike (the noise model lands in `p`)
int mh_check(const dmip_surrogate* s, const dmip_scat_noise* noise, dmip::SurrogateParams& p, const float* y_dev,
             const float* x_out_dev, int n_y, int64_t n_chains, int64_t chain_offset, int num_steps, float noise_std) {
  if (int rc = surrogate_check(s, n_chains)) return rc;
  if (int rc = noise_check(noise, p)) return rc;
  if (!y_dev || !x_out_dev) return fail(DMIP_ERR_INVALID, "null argument");
  if (n_y < 1 || n_y > 65535) return fail(DMIP_ERR_INVALID, "n_y must be in [1, 65535]");
  if (chain_offset < 0) return fail(DMIP_ERR_INVALID, "negative chain offset");
  if (num_steps < 0) return fail(DMIP_ERR_INVALID, "num_steps must be >= 0");
  if (!(noise_std >= 0.0f)) return fail(DMIP_ERR_INVALID, "noise_std must be >= 0");
  return DMIP_OK;
}

// the sizes dmip_dps_sample and the fp32x3 path of dmip_dps_sample_ex check alike, after their handles
int dps_check_sizes(int n_y, int64_t n_chains, int64_t chain_offset, int num_steps, const dmip_vpsde* sde, float zeta) {
  if (n_y < 1 || n_y > 65535) return fail(DMIP_ERR_INVALID, "n_y must be in [1, 65535]");
  if (n_chains < 0 || chain_offset < 0) return fail(DMIP_ERR_INVALID, "negative chain count/offset");
  if (num_steps < 1) return fail(DMIP_ERR_INVALID, "num_steps must be >= 1");
  if (!(sde->T > 0.0)) return fail(DMIP_ERR_INVALID, "T must be > 0");
  if (!(zeta >= 0.0f)) return fail(DMIP_ERR_INVALID, "zeta must be >= 0");
  return DMIP_OK;
}

// the chains of an MH, MALA or DPS launch over the surrogate, whatever kernel runs them (DPS: no start states)
dmip::MhChains fill_chains(int64_t n_chains, int64_t chain_offset, int num_steps, float noise_std, uint64_t seed,
                           const float* x_init_dev, const float* noise_dev, const float* unif_dev, float* x_out_dev) {
  return dmip::MhChains{n_chains, chain_offset, num_steps, noise_std, seed, x_init_dev, noise_dev, unif_dev, x_out_dev};
}

int dps_prior_refused() {
  return fail(DMIP_ERR_UNSUPPORTED, "DPS prior must be an x,t network (MLP2) with xdim 3 and hidden layers [256]*3");
}

}  // namespace

extern "C" {

int dmip_surrogate_forward(const dmip_surrogate* s, const float* x_dev, int64_t n, float* f_out_dev, void* stream) {
  if (int rc = surrogate_check(s, n)) return rc;
  if (n == 0) return DMIP_OK;
  if (!x_dev || !f_out_dev) return fail(DMIP_ERR_INVALID, "null argument");
  dmip::SurrogateParams p{};
  surrogate_params(s, p);
  p.x = x_dev;
  p.n = n;
  p.f_out = f_out_dev;
  hipError_t e = dmip::launch_surrogate_eval(p, 0, surrogate_n_wg(n, (hipStream_t)stream), (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "surrogate_forward launch");
}

int dmip_log_posterior(const dmip_surrogate* s, const dmip_scat_noise* noise, const float* x_dev, const float* y_dev,
                       int64_t y_stride, int64_t n, float* e_out_dev, float* grad_out_dev, void* stream) {
  if (int rc = surrogate_check(s, n)) return rc;
  dmip::SurrogateParams p{};
  if (int rc = noise_check(noise, p)) return rc;
  if (y_stride != 0 && y_stride != dmip::kSurYdim) return fail(DMIP_ERR_INVALID, "y_stride must be 0 or 23");
  if (n == 0) return DMIP_OK;
  if (!x_dev || !y_dev || !e_out_dev) return fail(DMIP_ERR_INVALID, "null argument");
  surrogate_params(s, p);
  p.x = x_dev;
  p.y = y_dev;
  p.y_stride = y_stride;
  p.n = n;
  p.e_out = e_out_dev;
  p.g_out = grad_out_dev;
  hipError_t e = dmip::launch_surrogate_eval(p, grad_out_dev ? 2 : 1, surrogate_n_wg(n, (hipStream_t)stream), (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "log_posterior launch");
}

int dmip_mh_sample(const dmip_surrogate* s, const dmip_scat_noise* noise, const float* y_dev, int n_y,
                   int64_t n_chains, int64_t chain_offset, int num_steps, float noise_std, uint64_t seed,
                   const float* x_init_dev, const float* noise_dev, const float* unif_dev, float* x_out_dev,
                   float* e_out_dev, void* stream) {
  dmip::SurrogateParams p{};
  if (int rc = mh_check(s, noise, p, y_dev, x_out_dev, n_y, n_chains, chain_offset, num_steps, noise_std)) return rc;
  if ((noise_dev == nullptr) != (unif_dev == nullptr))
    return fail(DMIP_ERR_INVALID, "inject both the proposal normals and the uniforms, or neither");
  if (n_chains == 0) return DMIP_OK;
  surrogate_params(s, p);
  p.y = y_dev;
  p.ch = fill_chains(n_chains, chain_offset, num_steps, noise_std, seed, x_init_dev, noise_dev, unif_dev, x_out_dev);
  p.e_out = e_out_dev;
  hipError_t e = dmip::launch_mh(p, n_y, (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "mh_sample launch");
}

int dmip_mh_sample_ex(const dmip_surrogate* s, const dmip_scat_noise* noise, const float* y_dev, int n_y,
                      int64_t n_chains, int64_t chain_offset, int num_steps, float noise_std, uint64_t seed,
                      const float* x_init_dev, const float* noise_dev, const float* unif_dev, int precision,
                      float* x_out_dev, float* e_out_dev, void* stream) {
  if (precision == DMIP_PREC_F32)
    return dmip_mh_sample(s, noise, y_dev, n_y, n_chains, chain_offset, num_steps, noise_std, seed, x_init_dev,
                          noise_dev, unif_dev, x_out_dev, e_out_dev, stream);
  if (precision != DMIP_PREC_F32X3) return fail(DMIP_ERR_INVALID, "MH precision: DMIP_PREC_F32 or DMIP_PREC_F32X3");
  dmip::SurrogateParams sp{};
  if (int rc = mh_check(s, noise, sp, y_dev, x_out_dev, n_y, n_chains, chain_offset, num_steps, noise_std)) return rc;
  if (noise_dev || unif_dev) return fail(DMIP_ERR_UNSUPPORTED, "fp32x3 MH: injected draws need DMIP_PREC_F32");
  if (!s->x3_img) return x3_range_refused("fp32x3 MH", "|w|", s->x3_range);
  if (n_chains == 0) return DMIP_OK;
  hipStream_t st = (hipStream_t)stream;
  dmip::MhX3Params p{};
  p.simg = s->x3_img;
  p.sl1 = s->x3_l1;
  p.sbias = s->x3_bias;
  p.y = y_dev;
  p.ch = fill_chains(n_chains, chain_offset, num_steps, noise_std, seed, x_init_dev, /*noise_dev=*/nullptr,
                     /*unif_dev=*/nullptr, x_out_dev);
  p.a = sp.a;
  p.b2 = sp.b2;
  p.lam = sp.lam;
  p.e_out = e_out_dev;
  if (int rc = status_word_or_fail(p.err, st)) return rc;
  hipError_t e = dmip::launch_mh_x3(p, n_y, st);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "mh_sample (fp32x3) launch");
}

int dmip_mala_sample(const dmip_surrogate* s, const dmip_scat_noise* noise, const float* y_dev, int n_y,
                     int64_t n_chains, int64_t chain_offset, int num_steps, int lang_steps, double stepsize,
                     double lambd, uint64_t seed, const float* x_init_dev, const float* eta_dev,
                     const float* unif_dev, float* x_out_dev, float* e_out_dev, int32_t* acc_out_dev, void* stream) {
  dmip::MalaParams q{};
  if (int rc = mh_check(s, noise, q.s, y_dev, x_out_dev, n_y, n_chains, chain_offset, num_steps, 0.0f)) return rc;
  if (lang_steps < 1) return fail(DMIP_ERR_INVALID, "lang_steps must be >= 1");
  if (!std::isfinite(stepsize) || !(stepsize > 0.0) || !((float)stepsize > 0.0f) || !std::isfinite((float)stepsize))
    return fail(DMIP_ERR_INVALID, "stepsize must be finite and > 0");
  if (!(lambd >= 0.0 && lambd <= 1.0)) return fail(DMIP_ERR_INVALID, "lambd must be in [0, 1]");
  if ((eta_dev == nullptr) != (unif_dev == nullptr))
    return fail(DMIP_ERR_INVALID, "inject both the Langevin normals and the uniforms, or neither");
  if (n_chains == 0) return DMIP_OK;
  surrogate_params(s, q.s);
  q.s.y = y_dev;
  q.s.ch = fill_chains(n_chains, chain_offset, num_steps, /*noise_std=*/0.0f, seed, x_init_dev, /*noise_dev=*/eta_dev,
                       unif_dev, x_out_dev);
  q.s.e_out = e_out_dev;
  q.lang_steps = lang_steps;
  // python scalars of the reference (models/SNF.py:294-297): each constant rounded once from double
  q.h = (float)stepsize;
  q.c = (float)std::sqrt(2.0 * stepsize);
  q.lam_e = (float)lambd;
  q.lam_q = (float)((1.0 - lambd) * 0.5);
  q.acc_out = acc_out_dev;
  hipError_t e = dmip::launch_mala(q, n_y, (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "mala_sample launch");
}

// (the two DPS entry points refuse a bad guidance mode and a SiLU prior in opposite orders, so only what follows
// their handle checks is shared: dps_check_sizes)
int dmip_dps_sample(const dmip_mlp* prior, const dmip_surrogate* fwd, const dmip_scat_noise* noise,
                    const dmip_vpsde* sde, const float* y_dev, int n_y, int64_t n_chains, int64_t chain_offset,
                    int num_steps, float mean, float stdv, uint64_t seed, int mode, float zeta, float* x_out_dev,
                    void* stream) {
  if (!prior || !fwd || !sde || !y_dev || !x_out_dev) return fail(DMIP_ERR_INVALID, "null argument");
  if (mode != DMIP_DPS_NLL && mode != DMIP_DPS_NORM) return fail(DMIP_ERR_INVALID, "unknown DPS guidance mode");
  if (f32_act(prior)) return act_refused("dps_sample");
  dmip::DpsParams p{};
  if (mode == DMIP_DPS_NLL) {
    if (int rc = noise_check(noise, p.s)) return rc;
  }
  if (!prior->dps_l1) return dps_prior_refused();
  if (int rc = dps_check_sizes(n_y, n_chains, chain_offset, num_steps, sde, zeta)) return rc;
  if (n_chains == 0) return DMIP_OK;
  surrogate_params(fwd, p.s);
  p.mode = mode;
  p.s.y = y_dev;
  p.s.ch = fill_chains(n_chains, chain_offset, num_steps, /*noise_std=*/0.0f, seed, /*x_init_dev=*/nullptr,
                       /*noise_dev=*/nullptr, /*unif_dev=*/nullptr, x_out_dev);
  p.pl1 = prior->dps_l1;
  p.pw2 = prior->dps_w2;
  p.pw3 = prior->dps_w3;
  p.pw4 = prior->dps_w4;
  p.pbias = prior->dps_bias;
  fill_schedule(*sde, num_steps, p.T, p.bmin, p.bdiff, p.delta, &p.sqrt_delta);
  p.mean = mean;
  p.stdv = stdv;
  p.zeta = zeta;
  hipError_t e = dmip::launch_dps(p, n_y, (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "dps_sample launch");
}

int dmip_dps_sample_ex(const dmip_mlp* prior, const dmip_surrogate* fwd, const dmip_scat_noise* noise,
                       const dmip_vpsde* sde, const float* y_dev, int n_y, int64_t n_chains, int64_t chain_offset,
                       int num_steps, float mean, float stdv, uint64_t seed, int mode, float zeta, int precision,
                       float* x_out_dev, void* stream) {
  if (precision == DMIP_PREC_F32)
    return dmip_dps_sample(prior, fwd, noise, sde, y_dev, n_y, n_chains, chain_offset, num_steps, mean, stdv, seed,
                           mode, zeta, x_out_dev, stream);
  if (precision != DMIP_PREC_F32X3) return fail(DMIP_ERR_INVALID, "DPS precision: DMIP_PREC_F32 or DMIP_PREC_F32X3");
  if (!prior || !fwd || !sde || !y_dev || !x_out_dev) return fail(DMIP_ERR_INVALID, "null argument");
  if (f32_act(prior)) return act_refused("dps_sample_ex");
  if (mode != DMIP_DPS_NLL && mode != DMIP_DPS_NORM) return fail(DMIP_ERR_INVALID, "unknown DPS guidance mode");
  dmip::DpsX3Params p{};
  if (mode == DMIP_DPS_NLL) {
    dmip::SurrogateParams sp{};
    if (int rc = noise_check(noise, sp)) return rc;
    p.a = sp.a;
    p.b2 = sp.b2;
  }
  if (!prior->dps_l1) return dps_prior_refused();
  if (!prior->dps_x3_img || !fwd->x3_img)
    return x3_range_refused("fp32x3 DPS", "|w|", std::max(prior->dps_x3_range, fwd->x3_range));
  if (int rc = dps_check_sizes(n_y, n_chains, chain_offset, num_steps, sde, zeta)) return rc;
  if (n_chains == 0) return DMIP_OK;
  hipStream_t st = (hipStream_t)stream;
  p.pimg = prior->dps_x3_img;
  p.simg = fwd->x3_img;
  p.pl1 = prior->dps_x3_l1;
  p.sl1 = fwd->x3_l1;
  p.pbias = prior->dps_x3_bias;
  p.sbias = fwd->x3_bias;
  p.y = y_dev;
  p.n_chains = n_chains;
  p.chain_offset = chain_offset;
  p.num_steps = num_steps;
  fill_schedule(*sde, num_steps, p.T, p.bmin, p.bdiff, p.delta, &p.sqrt_delta);
  p.mean = mean;
  p.stdv = stdv;
  p.zeta = zeta;
  p.mode = mode;
  p.seed = seed;
  p.x_out = x_out_dev;
  if (int rc = status_word_or_fail(p.err, st)) return rc;
  hipError_t e = dmip::launch_dps_x3(p, n_y, st);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "dps_sample (fp32x3) launch");
}

int dmip_rng_words(uint64_t seed, int64_t chain_offset, uint64_t stream_id, int64_t n_chains, int n_words,
                   uint32_t* out_dev, void* stream) {
  if (!out_dev || n_chains < 0 || n_words < 0) return fail(DMIP_ERR_INVALID, "bad argument");
  if (n_chains == 0 || n_words == 0) return DMIP_OK;
  hipError_t e = dmip::launch_rng_words(seed, chain_offset, stream_id, n_chains, n_words, out_dev, (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "rng_words launch");
}

int dmip_rng_normals(uint64_t seed, int64_t chain_offset, uint64_t stream_id, int64_t n_chains, int n_pairs,
                     float* out_dev, void* stream) {
  if (!out_dev || n_chains < 0 || n_pairs < 0) return fail(DMIP_ERR_INVALID, "bad argument");
  if (n_chains == 0 || n_pairs == 0) return DMIP_OK;
  hipError_t e = dmip::launch_rng_normals(seed, chain_offset, stream_id, n_chains, n_pairs, out_dev, (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "rng_normals launch");
}

int dmip_schedule(int num_steps, const dmip_vpsde* sde, float* out_dev, void* stream) {
  if (!out_dev || !sde || num_steps < 1) return fail(DMIP_ERR_INVALID, "bad argument");
  hipError_t e = dmip::launch_schedule(num_steps, (float)sde->T, (float)sde->beta_min,
                                       (float)(sde->beta_max - sde->beta_min), out_dev, (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "schedule launch");
}

}  // extern "C"
