// libdmip.so C-ABI, guided posterior sampling for a linear-Gaussian problem from a prior score network alone
// (dmip_dps_linear.hip, dmip_x3_dps_linear.hip), and the same with the Tweedie-covariance guidance (dmip_dps_tweedie.hip,
// dmip_x3_dps_tweedie.hip). Argument validation first, then one stream-ordered launch.
#include "dmip_capi_common.h"

using namespace dmip_capi;

namespace {

// What the two entry points share, after their own null-pointer and table checks and before any device work: the ranges,
// the network's kind, and whether a kernel and an image exist for it. `what` names the entry point in the messages.
int check_dps(const dmip_mlp* prior, const dmip_vpsde* sde, int ydim, int n_y, int64_t n_chains, int64_t chain_offset,
              int num_steps, float zeta, int precision, const std::string& what) {
  if (num_steps < 1) return fail(DMIP_ERR_INVALID, "num_steps must be >= 1");
  if (ydim < 1 || ydim > dmip::kDpsLinearMaxY) return fail(DMIP_ERR_INVALID, "ydim must be in [1, 32]");
  if (!(zeta >= 0.0f) || !std::isfinite(zeta)) return fail(DMIP_ERR_INVALID, "zeta must be finite and >= 0");
  if (n_y < 1 || n_y > 65535) return fail(DMIP_ERR_INVALID, "n_y must be in [1, 65535]");
  if (n_chains < 0 || chain_offset < 0) return fail(DMIP_ERR_INVALID, "negative chain count/offset");
  if (!(sde->T > 0.0)) return fail(DMIP_ERR_INVALID, "T must be > 0");
  if (prior->layout != DMIP_INPUT_X_T || prior->out_dim != prior->xdim || prior->in_dim != prior->xdim + 1)
    return fail(DMIP_ERR_INVALID, what + " prior must be an x,t network with out_dim == xdim");
  if (f32_act(prior)) return fail(DMIP_ERR_UNSUPPORTED, what + ": the tanh chain only (no SiLU kernel)");
  if (precision != DMIP_PREC_F32 && precision != DMIP_PREC_F32X3 && precision != DMIP_PREC_FP16)
    return fail(DMIP_ERR_UNSUPPORTED, what + ": no kernel for this precision (DMIP_PREC_F32 or DMIP_PREC_F32X3)");
  const bool x3 = precision != DMIP_PREC_F32;
  const int xdim = prior->xdim;
  if (!dmip::dps_linear_supported(prior->width, prior->n_hidden, xdim, ydim))
    return fail(DMIP_ERR_UNSUPPORTED, "no compiled " + what + " kernel for width " + std::to_string(prior->width) +
                                          ", layers " + std::to_string(prior->n_hidden) + ", xdim " +
                                          std::to_string(xdim));
  if (x3 && prior->x3_range > 0.0)
    return x3_range_refused(what + " (fp32x3)", "scaled |w|", prior->x3_range);
  if (x3 ? !prior->x3_stream : (!prior->f32_l1 || prior->f32_k1q != (xdim + 2 + 3) / 4))
    return fail(DMIP_ERR_UNSUPPORTED, what + ": the prior has no image for this precision");
  return DMIP_OK;
}

dmip::DpsLinearChains dps_chains(const dmip_vpsde* sde, const float* A_dev, const float* B_dev, int n_B,
                                 const float* yres_dev, int ydim, int64_t n_chains, int64_t chain_offset, int num_steps,
                                 float mean, float stdv, uint64_t seed, int step_rule, float zeta, float* x_out_dev) {
  dmip::DpsLinearChains c{};
  c.A = A_dev;
  c.B = B_dev;
  c.yres = yres_dev;
  c.x_out = x_out_dev;
  c.n = n_chains;
  c.chain_offset = chain_offset;
  c.num_steps = num_steps;
  c.ydim = ydim;
  c.n_B = n_B;
  c.step_rule = step_rule;
  fill_schedule(*sde, num_steps, c.T, c.bmin, c.bdiff, c.delta, &c.sqrt_delta);
  c.mean = mean;
  c.stdv = stdv;
  c.zeta = zeta;
  c.seed = seed;
  return c;
}

}  // namespace

extern "C" {

// the tanh chain's answer (a SiLU prior is refused by the entry point); DMIP_PREC_FP16 runs the fp32x3 kernel, as
// the flow entry points
int dmip_dps_linear_supported(int width, int n_hidden, int xdim, int ydim, int precision) {
  if (precision != DMIP_PREC_F32 && precision != DMIP_PREC_F32X3 && precision != DMIP_PREC_FP16) return 0;
  return dmip::dps_linear_supported(width, n_hidden, xdim, ydim) ? 1 : 0;
}

// every argument is validated before any device work
int dmip_dps_linear_sample(const dmip_mlp* prior, const dmip_vpsde* sde, const float* A_dev, const float* B_dev, int n_B,
                           const float* yres_dev, int ydim, int n_y, int64_t n_chains, int64_t chain_offset,
                           int num_steps, float mean, float stdv, uint64_t seed, int step_rule, float zeta,
                           int precision, float* x_out_dev, void* stream) {
  if (!prior || !sde || !A_dev || !B_dev || !yres_dev || !x_out_dev) return fail(DMIP_ERR_INVALID, "null argument");
  if (step_rule != DMIP_DPS_STEP_BETA && step_rule != DMIP_DPS_STEP_NORM)
    return fail(DMIP_ERR_INVALID, "unknown dps_linear step rule");
  if (n_B != 1 && n_B != num_steps) return fail(DMIP_ERR_INVALID, "n_B must be 1 or num_steps");
  if (int rc = check_dps(prior, sde, ydim, n_y, n_chains, chain_offset, num_steps, zeta, precision, "dps_linear"))
    return rc;
  if (n_chains == 0) return DMIP_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool x3 = precision != DMIP_PREC_F32;
  const dmip::DpsLinearChains c = dps_chains(sde, A_dev, B_dev, n_B, yres_dev, ydim, n_chains, chain_offset, num_steps,
                                             mean, stdv, seed, step_rule, zeta, x_out_dev);
  bool ok = false;
  hipError_t e;
  if (x3) {
    dmip::X3DpsLinearParams p{};
    p.net = x3_net(prior);
    p.n_hidden = prior->n_hidden;
    p.chains = c;
    if (int rc = status_word_or_fail(p.err, st)) return rc;
    e = dmip::launch_x3_dps_linear(p, prior->width, prior->xdim, n_y, st, &ok);
  } else {
    dmip::F32DpsLinearParams p{};
    p.net = f32_net(prior);
    p.n_hidden = prior->n_hidden;
    p.chains = c;
    e = dmip::launch_f32_dps_linear(p, prior->width, prior->xdim, n_y, st, &ok);
  }
  if (!ok) return fail(DMIP_ERR_UNSUPPORTED, "no compiled dps_linear kernel");
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "dps_linear launch");
}

// the Tweedie-covariance guidance: the shapes, precisions, validation and status classes of dps_linear; B is one
// matrix and the step rule is DMIP_DPS_STEP_BETA
int dmip_dps_tweedie_supported(int width, int n_hidden, int xdim, int ydim, int precision) {
  return dmip_dps_linear_supported(width, n_hidden, xdim, ydim, precision);
}

int dmip_dps_tweedie_sample(const dmip_mlp* prior, const dmip_vpsde* sde, const float* A_dev, const float* B_dev,
                            const float* H_dev, const float* yres_dev, int ydim, int n_y, int64_t n_chains,
                            int64_t chain_offset, int num_steps, float mean, float stdv, uint64_t seed, float zeta,
                            int precision, float* x_out_dev, void* stream) {
  if (!prior || !sde || !A_dev || !B_dev || !H_dev || !yres_dev || !x_out_dev)
    return fail(DMIP_ERR_INVALID, "null argument");
  if (int rc = check_dps(prior, sde, ydim, n_y, n_chains, chain_offset, num_steps, zeta, precision, "dps_tweedie"))
    return rc;
  if (n_chains == 0) return DMIP_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool x3 = precision != DMIP_PREC_F32;
  dmip::DpsTweedieChains c{};
  c.lin = dps_chains(sde, A_dev, B_dev, 1, yres_dev, ydim, n_chains, chain_offset, num_steps, mean, stdv, seed,
                     DMIP_DPS_STEP_BETA, zeta, x_out_dev);
  c.H = H_dev;
  bool ok = false;
  hipError_t e;
  if (x3) {
    dmip::X3DpsTweedieParams p{};
    p.net = x3_net(prior);
    p.n_hidden = prior->n_hidden;
    p.chains = c;
    if (int rc = status_word_or_fail(p.err, st)) return rc;
    e = dmip::launch_x3_dps_tweedie(p, prior->width, prior->xdim, n_y, st, &ok);
  } else {
    dmip::F32DpsTweedieParams p{};
    p.net = f32_net(prior);
    p.n_hidden = prior->n_hidden;
    p.chains = c;
    e = dmip::launch_f32_dps_tweedie(p, prior->width, prior->xdim, n_y, st, &ok);
  }
  if (!ok) return fail(DMIP_ERR_UNSUPPORTED, "no compiled dps_tweedie kernel");
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "dps_tweedie launch");
}

}  // extern "C"
