// libdmip.so C-ABI, the probability-flow entry points: log p(x | y) of given rows (dmip_flow_logp[_ex]), samples with
// their log-density (dmip_flow_sample[_ex]), their paired forms with one observation per row (dmip_flow_logp_pairs,
// dmip_flow_sample_pairs) and the *_supported queries. One implementation, parameterised by two facts: the
// log-density of given rows or samples, and one y per y index or one per row. Argument validation first, then
// stream-ordered launches.
#include <type_traits>

#include "dmip_capi_common.h"
#include "dmip_pairs.h"

using namespace dmip_capi;

namespace {

// What every flow entry point takes, then what only some of them set: the rows of a log-density call, the chains of a
// sampling call. `n`: rows or chains (per y index; the paired forms have one y per row and n_y = 1 for the networks'
// check)
struct FlowArgs {
  int mode;
  const dmip_mlp *net, *prior;
  const dmip_vpsde* sde;
  const float* y_dev;
  int ydim, xdim;
  int64_t n;
  int num_steps, precision;
  void* stream;
  FlowArgs(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde, const float* y_dev, int ydim,
           int xdim, int64_t n, int num_steps, int precision, void* stream)
      : mode(mode), net(net), prior(prior), sde(sde), y_dev(y_dev), ydim(ydim), xdim(xdim), n(n), num_steps(num_steps),
        precision(precision), stream(stream) {}
  int n_y = 1;
  const float* x_dev = nullptr;  // the rows [n_y][n][xdim], their log p and (or null) their latents x_S
  float *logp_out_dev = nullptr, *latent_out_dev = nullptr;
  int64_t chain_offset = 0;  // the chains: the RNG's index of chain 0, the base density, start states or null
  float mean = 0.0f, stdv = 1.0f;
  uint64_t seed = 0;
  const float* x0_dev = nullptr;
  float *x_out_dev = nullptr, *logq_out_dev = nullptr;
};

// What the four kinds of entry point word differently, [samples][paired]
struct FlowKind {
  const char* who;     // the entry point's name in its messages
  const char* count;   // the refusal of n < 1 among the entry point's own arguments; null: n == 0 is OK and n < 0 is
                       // left to the networks' check
  const char* silu;    // the SiLU refusal, after "<who>: the tanh chain only "
  const char* kernel;  // no_kernel's kind
  const char* missing;  // the launch found no kernel
};
const FlowKind kKinds[2][2] = {
    {{"flow_logp", nullptr, "(no SiLU log-likelihood kernel)", "log-likelihood kernel",
      "no compiled log-likelihood kernel"},
     {"flow_logp_pairs", "n must be >= 1", "(no SiLU kernel)", "paired flow kernel",
      "no compiled paired log-likelihood kernel"}},
    {{"flow_sample", "n_chains must be >= 1", "(no SiLU kernel)", "flow_sample kernel",
      "no compiled flow_sample kernel"},
     {"flow_sample_pairs", "n must be >= 1", "(no SiLU kernel)", "paired flow kernel",
      "no compiled paired flow_sample kernel"}}};

// Every argument is validated before any device work, in the entry point's own order: the sampling and the paired
// forms check their count (and stdv) before the null arguments, dmip_flow_logp leaves its count to check_nets. Out:
// the Posterior prior (else null) and the engine. The precision is exact f32 (dmip_flow.hip, dmip_flow_sample.hip) or
// the fp32x3 engine (dmip_x3_flow.h) -- which DMIP_PREC_FP16 / BF16 run as well: there is no 16-bit flow kernel (as
// dmip_ode_sample's Heun routing has none)
int flow_check(const FlowKind& k, bool sample, bool paired, const FlowArgs& a, const dmip_mlp*& net1, bool& x3) {
  const bool post = a.mode == DMIP_SAMPLER_POSTERIOR;
  if (a.mode != DMIP_SAMPLER_CDE && !post)
    return fail(DMIP_ERR_INVALID, std::string(k.who) + ": CDE and Posterior estimators only");
  if (a.num_steps < 1) return fail(DMIP_ERR_INVALID, "num_steps must be >= 1");
  if (k.count && a.n < 1) return fail(DMIP_ERR_INVALID, k.count);
  if (sample && !(a.stdv > 0.0f)) return fail(DMIP_ERR_INVALID, "stdv must be > 0");
  if (!a.net || !a.sde || !a.y_dev || (post && !a.prior) ||
      (sample ? !a.x_out_dev || !a.logq_out_dev : !a.x_dev || !a.logp_out_dev))
    return fail(DMIP_ERR_INVALID, "null argument");
  if (a.precision != DMIP_PREC_FP16 && a.precision != DMIP_PREC_F32 && a.precision != DMIP_PREC_F32X3)
    return fail(DMIP_ERR_INVALID, "unknown precision");
  const dmip_mlp* net = a.net;
  net1 = post ? a.prior : nullptr;
  if (int rc = check_nets(k.who, net, net1, a.xdim, a.xdim, a.ydim, paired ? 1 : a.n_y, !sample, a.n, a.chain_offset,
                          a.num_steps, a.sde))
    return rc;
  if (f32_act(net) || (net1 && f32_act(net1)))
    return fail(DMIP_ERR_UNSUPPORTED, std::string(k.who) + ": the tanh chain only " + k.silu);
  x3 = a.precision != DMIP_PREC_F32;
  if (!(x3               ? dmip::x3_flow_supported(a.mode, net->width, net->n_hidden, a.xdim, a.ydim)
        : sample && !paired ? dmip::f32_flow_sample_supported(a.mode, net->width, net->n_hidden, a.xdim, a.ydim)
                            : dmip::f32_flow_supported(a.mode, net->width, net->n_hidden, a.xdim, a.ydim)))
    return no_kernel(k.kernel, a.mode, net, a.xdim, -1, x3 ? DMIP_PREC_F32X3 : -1);
  if (!x3) return DMIP_OK;
  // what em_sample_x3 checks before an fp32x3 launch: the networks have their split images
  if (int rc = x3_check_range(net, net1)) return rc;
  if (!net->x3_stream || (net1 && !net1->x3_stream))
    return no_kernel(k.kernel, a.mode, net, a.xdim, -1, DMIP_PREC_F32X3);
  return DMIP_OK;
}

// ---- the paired forms: one observation per row (dmip_pairs.h)
// rows per slab: the [rows][W] layer-1 bias scratch stays within 32 MiB (test hook, not ABI: DMIP_PAIRS_SLAB_ROWS=k
// forces k rows per slab). Rows are independent, so the slabs of a call give the bits of one launch
int64_t pairs_slab_rows(int width) {
  if (const char* e = getenv("DMIP_PAIRS_SLAB_ROWS")) {
    const long long v = atoll(e);
    if (v >= 1) return (int64_t)v;
  }
  return (int64_t)((32u << 20) / ((size_t)width * sizeof(float)));
}
// (the kernels index the scratch with 32-bit offsets: a forced slab stays below 2^31 floats)
int64_t pairs_slab_bound(int64_t slab, int width) { return std::min<int64_t>(slab, ((int64_t)1 << 31) / width - 1); }

// a slab's layer-1 biases c_i (and, exact f32, the shared zero-bias layer-1 image) on the stream
int pairs_prep(StreamScratch& bias, StreamScratch& l1, const dmip_mlp* net, const float* y_dev, int64_t rows, int xdim,
               int ydim, bool x3, hipStream_t st) {
  const int k1q = (xdim + 2 + 3) / 4;
  if (int rc = bias.alloc((size_t)rows * net->width * sizeof(float), st)) return rc;
  if (!x3)
    if (int rc = l1.alloc((size_t)(net->width / 16) * k1q * 64 * sizeof(float), st)) return rc;
  dmip::PairsPrepParams pp{net->w1, net->b1, y_dev, (float*)bias.ptr, (float*)l1.ptr, rows, net->width, net->in_dim,
                           xdim, ydim, k1q, x3 ? (double)dmip::kPairsTanhScale : 1.0};
  const hipError_t e = dmip::launch_pairs_prep(pp, st);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "paired layer-1 bias prep launch");
}

// the rows or the chains [r0, r0 + rows) of a call, whichever engine runs them (the per-y forms: all of them, per y)
template <bool Sample>
auto flow_work(const FlowArgs& a, int64_t r0, int64_t rows) {
  const size_t x_off = (size_t)r0 * a.xdim;
  if constexpr (Sample) {
    dmip::FlowChains c{a.x0_dev ? a.x0_dev + x_off : nullptr, a.x_out_dev + x_off, a.logq_out_dev + r0, rows,
                       a.chain_offset + r0, a.num_steps};
    fill_schedule(*a.sde, a.num_steps, c.T, c.bmin, c.bdiff, c.delta);
    c.mean = a.mean;
    c.stdv = a.stdv;
    c.seed = a.seed;
    c.base = -0.5 * (double)a.xdim * 1.8378770664093453 - (double)a.xdim * std::log((double)a.stdv);  // log 2 pi
    return c;
  } else {
    dmip::FlowRows r{a.x_dev + x_off, a.logp_out_dev + r0, a.latent_out_dev ? a.latent_out_dev + x_off : nullptr, rows,
                     a.num_steps};
    fill_schedule(*a.sde, a.num_steps, r.T, r.bmin, r.bdiff, r.h);
    return r;
  }
}

// the eight launches: a per-y parameter struct goes out as it is, or inside its paired struct (.x / .f) with the rows'
// layer-1 biases beside it
template <bool Paired>
hipError_t flow_launch(const dmip::X3FlowParams& q, const float* row_bias, const FlowArgs& a, hipStream_t st, bool* ok) {
  const dmip_mlp* n = a.net;
  if constexpr (Paired)
    return dmip::launch_x3_flow_pairs({q, row_bias}, a.mode, n->width, n->n_hidden, a.xdim, a.ydim, st, ok);
  else
    return dmip::launch_x3_flow(q, a.mode, n->width, n->n_hidden, a.xdim, a.ydim, a.n_y, st, ok);
}
template <bool Paired>
hipError_t flow_launch(const dmip::X3FlowSampleParams& q, const float* row_bias, const FlowArgs& a, hipStream_t st,
                       bool* ok) {
  const dmip_mlp* n = a.net;
  if constexpr (Paired)
    return dmip::launch_x3_flow_sample_pairs({q, row_bias}, a.mode, n->width, n->n_hidden, a.xdim, a.ydim, st, ok);
  else
    return dmip::launch_x3_flow_sample(q, a.mode, n->width, n->n_hidden, a.xdim, a.ydim, a.n_y, st, ok);
}
template <bool Paired>
hipError_t flow_launch(const dmip::F32FlowParams& q, const float* row_bias, const FlowArgs& a, hipStream_t st, bool* ok) {
  const dmip_mlp* n = a.net;
  if constexpr (Paired)
    return dmip::launch_f32_flow_pairs({q, row_bias}, a.mode, n->width, n->n_hidden, a.xdim, a.ydim, st, ok);
  else
    return dmip::launch_f32_flow(q, a.mode, n->width, n->n_hidden, a.xdim, a.ydim, a.n_y, st, ok);
}
template <bool Paired>
hipError_t flow_launch(const dmip::F32FlowSampleParams& q, const float* row_bias, const FlowArgs& a, hipStream_t st,
                       bool* ok) {
  const dmip_mlp* n = a.net;
  if constexpr (Paired)
    return dmip::launch_f32_flow_sample_pairs({q, row_bias}, a.mode, n->width, n->n_hidden, a.xdim, a.ydim, st, ok);
  else
    return dmip::launch_f32_flow_sample(q, a.mode, n->width, n->n_hidden, a.xdim, a.ydim, a.n_y, st, ok);
}

// what a flow launch needs beside its rows or chains: the images' pointers and the engine's layer-1 data, one filler
// per engine (the fp32x3 one with the device status word)
template <typename P>
int fill_x3(P& p, const dmip_mlp* net, const dmip_mlp* net1, const StreamScratch& bias, hipStream_t st) {
  p.net[0] = x3_net(net);
  if (net1) p.net[1] = x3_net(net1);
  p.n_hidden = net->n_hidden;
  p.bias_y = (const float*)bias.ptr;
  return status_word_or_fail(p.err, st);
}
template <typename P>
int fill_f32(P& p, const dmip_mlp* net, const dmip_mlp* net1, const StreamScratch& l1) {
  p.net[0] = f32_net(net);
  if (net1) p.net[1] = f32_net(net1);
  p.n_hidden = net->n_hidden;
  p.l1y = (const float*)l1.ptr;
  return DMIP_OK;
}

// One slab: the layer-1 prep (per y: the fp32x3 engine's bias or the exact-f32 engine's image; paired: the rows' biases
// and, exact f32, the shared image), the selected engine's parameters, the launch. The scratch is freed on the stream
// behind the launch
template <bool Sample, bool Paired>
int flow_slab(const FlowKind& k, const FlowArgs& a, const dmip_mlp* net1, bool x3, int64_t r0, int64_t rows) {
  hipStream_t st = (hipStream_t)a.stream;
  const dmip_mlp* net = a.net;
  StreamScratch bias, l1;
  if (int rc = Paired ? pairs_prep(bias, l1, net, a.y_dev + (size_t)r0 * a.ydim, rows, a.xdim, a.ydim, x3, st)
               : x3   ? x3_bias_prep(bias, net, a.y_dev, a.n_y, a.xdim, a.ydim, st)
                      : f32_l1_prep(l1, net, a.y_dev, a.n_y, a.xdim, a.ydim, st))
    return rc;
  std::conditional_t<Sample, dmip::X3FlowSampleParams, dmip::X3FlowParams> px{};  // the selected engine's is filled
  std::conditional_t<Sample, dmip::F32FlowSampleParams, dmip::F32FlowParams> pf{};
  if constexpr (Sample)
    px.chains = pf.chains = flow_work<true>(a, r0, rows);
  else
    px.rows = pf.rows = flow_work<false>(a, r0, rows);
  if (int rc = x3 ? fill_x3(px, net, net1, bias, st) : fill_f32(pf, net, net1, l1)) return rc;
  bool ok = false;
  const hipError_t e = x3 ? flow_launch<Paired>(px, (const float*)bias.ptr, a, st, &ok)
                          : flow_launch<Paired>(pf, (const float*)bias.ptr, a, st, &ok);
  if (!ok) return fail(DMIP_ERR_UNSUPPORTED, k.missing);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, (std::string(k.who) + " launch").c_str());
}

// every flow entry point ends here. The per-y forms are one slab of all n rows or chains per y
template <bool Sample, bool Paired>
int flow_impl(const FlowArgs& a) {
  const FlowKind& k = kKinds[Sample][Paired];
  const dmip_mlp* net1 = nullptr;
  bool x3 = false;
  if (int rc = flow_check(k, Sample, Paired, a, net1, x3)) return rc;
  if (a.n == 0) return DMIP_OK;
  const int64_t slab = Paired ? pairs_slab_bound(pairs_slab_rows(a.net->width), a.net->width) : a.n;
  for (int64_t r0 = 0; r0 < a.n; r0 += slab)
    if (int rc = flow_slab<Sample, Paired>(k, a, net1, x3, r0, std::min<int64_t>(slab, a.n - r0))) return rc;
  return DMIP_OK;
}

template <bool Paired>
int flow_logp(FlowArgs a, int n_y, const float* x_dev, float* logp_out_dev, float* latent_out_dev) {
  a.n_y = n_y;
  a.x_dev = x_dev;
  a.logp_out_dev = logp_out_dev;
  a.latent_out_dev = latent_out_dev;
  return flow_impl<false, Paired>(a);
}

template <bool Paired>
int flow_sample(FlowArgs a, int n_y, int64_t chain_offset, float mean, float stdv, uint64_t seed, const float* x0_dev,
                float* x_out_dev, float* logq_out_dev) {
  a.n_y = n_y;
  a.chain_offset = chain_offset;
  a.mean = mean;
  a.stdv = stdv;
  a.seed = seed;
  a.x0_dev = x0_dev;
  a.x_out_dev = x_out_dev;
  a.logq_out_dev = logq_out_dev;
  return flow_impl<true, Paired>(a);
}

// the tanh chain's answer, as dmip_sampler_supported_precision's
int flow_supported_precision(int precision, int mode, int width, int n_hidden, int xdim, int ydim) {
  if (precision == DMIP_PREC_F32) return dmip::f32_flow_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
  if (precision == DMIP_PREC_F32X3 || precision == DMIP_PREC_FP16)
    return dmip::x3_flow_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
  return 0;
}

}  // namespace

extern "C" {

int dmip_flow_logp_supported(int mode, int width, int n_hidden, int xdim, int ydim) {
  return dmip::f32_flow_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
}

int dmip_flow_logp_supported_precision(int precision, int mode, int width, int n_hidden, int xdim, int ydim) {
  return flow_supported_precision(precision, mode, width, n_hidden, xdim, ydim);
}

int dmip_flow_logp(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde, const float* x_dev,
                   const float* y_dev, int n_y, int ydim, int xdim, int64_t n, int num_steps, float* logp_out_dev,
                   float* latent_out_dev, void* stream) {
  return flow_logp<false>({mode, net, prior, sde, y_dev, ydim, xdim, n, num_steps, DMIP_PREC_F32, stream}, n_y, x_dev,
                          logp_out_dev, latent_out_dev);
}

int dmip_flow_logp_ex(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde, const float* x_dev,
                      const float* y_dev, int n_y, int ydim, int xdim, int64_t n, int num_steps, float* logp_out_dev,
                      float* latent_out_dev, int precision, void* stream) {
  return flow_logp<false>({mode, net, prior, sde, y_dev, ydim, xdim, n, num_steps, precision, stream}, n_y, x_dev,
                          logp_out_dev, latent_out_dev);
}

int dmip_flow_sample_supported(int mode, int width, int n_hidden, int xdim, int ydim) {
  return dmip::f32_flow_sample_supported(mode, width, n_hidden, xdim, ydim) ? 1 : 0;
}

int dmip_flow_sample_supported_precision(int precision, int mode, int width, int n_hidden, int xdim, int ydim) {
  return flow_supported_precision(precision, mode, width, n_hidden, xdim, ydim);
}

int dmip_flow_sample(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde, const float* y_dev,
                     int n_y, int ydim, int xdim, int64_t n_chains, int64_t chain_offset, int num_steps, float mean,
                     float stdv, uint64_t seed, const float* x0_dev, float* x_out_dev, float* logq_out_dev,
                     void* stream) {
  return flow_sample<false>({mode, net, prior, sde, y_dev, ydim, xdim, n_chains, num_steps, DMIP_PREC_F32, stream}, n_y,
                            chain_offset, mean, stdv, seed, x0_dev, x_out_dev, logq_out_dev);
}

int dmip_flow_sample_ex(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde,
                        const float* y_dev, int n_y, int ydim, int xdim, int64_t n_chains, int64_t chain_offset,
                        int num_steps, float mean, float stdv, uint64_t seed, const float* x0_dev, float* x_out_dev,
                        float* logq_out_dev, int precision, void* stream) {
  return flow_sample<false>({mode, net, prior, sde, y_dev, ydim, xdim, n_chains, num_steps, precision, stream}, n_y,
                            chain_offset, mean, stdv, seed, x0_dev, x_out_dev, logq_out_dev);
}

int dmip_flow_pairs_supported(int precision, int mode, int width, int n_hidden, int xdim, int ydim) {
  return flow_supported_precision(precision, mode, width, n_hidden, xdim, ydim);
}

int dmip_flow_logp_pairs(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde,
                         const float* x_dev, const float* y_dev, int ydim, int xdim, int64_t n, int num_steps,
                         float* logp_out_dev, float* latent_out_dev, int precision, void* stream) {
  return flow_logp<true>({mode, net, prior, sde, y_dev, ydim, xdim, n, num_steps, precision, stream}, 1, x_dev,
                         logp_out_dev, latent_out_dev);
}

int dmip_flow_sample_pairs(int mode, const dmip_mlp* net, const dmip_mlp* prior, const dmip_vpsde* sde,
                           const float* y_dev, int ydim, int xdim, int64_t n, int64_t chain_offset, int num_steps,
                           float mean, float stdv, uint64_t seed, const float* x0_dev, float* x_out_dev,
                           float* logq_out_dev, int precision, void* stream) {
  return flow_sample<true>({mode, net, prior, sde, y_dev, ydim, xdim, n, num_steps, precision, stream}, 1, chain_offset,
                           mean, stdv, seed, x0_dev, x_out_dev, logq_out_dev);
}

}  // extern "C"
