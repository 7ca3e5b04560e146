// Host-side AddressSanitizer driver for libdmip's C-ABI (make asan; run by tests/test_asan.py).
// Exercises every entry point's argument validation with null / out-of-range / inconsistent
// arguments -- the paths that return before any device work -- plus the error-string plumbing, so
// ASan sees the validation code's reads of caller arrays (widths, weight tables) and the
// thread-local error buffer. Exits 0 when every call returned the documented status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "../../include/dmip.h"

static int failures = 0;

static void expect(int got, int want, const char* what) {
  if (got != want) {
    std::printf("FAIL %s: status %d, want %d (%s)\n", what, got, want, dmip_last_error());
    ++failures;
  }
}

// the status and dmip_last_error's text of a refusal
static void refused(int got, int want, const char* msg, const char* what) {
  if (got != want || std::strcmp(dmip_last_error(), msg) != 0) {
    std::printf("FAIL %s: status %d, want %d; message '%s', want '%s'\n", what, got, want, dmip_last_error(), msg);
    ++failures;
  }
}

// The sampler, flow, DPS and MH entry points' refusals that need no handle, in the order each entry point checks
// (where two arguments are wrong, the first check's message).
static void sampler_refusals() {
  const dmip_vpsde sde{0.1, 20.0, 1.0};
  const dmip_scat_noise nz{0.2f, 0.01f, 1000.f}, nz_bad{0.2f, 0.0f, 1000.f};
  float buf[4] = {};
  uint64_t stamps[4] = {};
  const int INV = DMIP_ERR_INVALID, UNS = DMIP_ERR_UNSUPPORTED;
  const int CDE = DMIP_SAMPLER_CDE, POST = DMIP_SAMPLER_POSTERIOR, CDIFFE = DMIP_SAMPLER_CDIFFE;
  const char* null_arg = "null argument";
  const char* snap01 = "snapshot_every must be 0 or in [1, num_steps] with a snapshot buffer";
  // dmip_em_sample*, every null in turn
  refused(dmip_em_sample(nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, nullptr, buf, nullptr), INV, null_arg,
          "em_sample: null net");
  refused(dmip_em_sample(nullptr, nullptr, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 7, nullptr, buf, nullptr), INV,
          null_arg, "em_sample: null before precision");
  refused(dmip_em_sample_posterior(nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 1, buf, nullptr), INV,
          null_arg, "posterior: null prior");
  refused(dmip_em_sample_cdiffe(nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, -1, 0.f, buf, nullptr), INV,
          "corrector_steps must be >= 0", "cdiffe: corrector before snr");
  refused(dmip_em_sample_cdiffe(nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1, 0.f, buf, nullptr), INV,
          "snr must be > 0", "cdiffe: snr");
  refused(dmip_em_sample_cdiffe(nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1, 0.16f, buf, nullptr), INV,
          null_arg, "cdiffe: null net");
  refused(dmip_em_sample_stamps(nullptr, &sde, buf, 1, 2, 2, 10, 10, 1, buf, nullptr, nullptr), INV,
          "null stamps buffer", "stamps: null buffer");
  refused(dmip_em_sample_stamps(nullptr, &sde, buf, 1, 2, 2, 10, 10, 1, buf, stamps, nullptr), INV, null_arg,
          "stamps: null net");
  // dmip_em_sample_snapshots
  refused(dmip_em_sample_snapshots(7, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 0, 0.16f, 0,
                                   nullptr, buf, nullptr),
          INV, "unknown sampler mode", "snapshots: mode before snapshot_every");
  for (int every : {0, 11})
    refused(dmip_em_sample_snapshots(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 0, 0.16f,
                                     every, nullptr, buf, nullptr),
            INV, "snapshot_every must be in [1, num_steps]", "snapshots: every before null buffer");
  refused(dmip_em_sample_snapshots(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 0, 0.16f, 2,
                                   nullptr, buf, nullptr),
          INV, "null snapshot buffer", "snapshots: null buffer");
  refused(dmip_em_sample_snapshots(POST, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1, 0.16f, 2,
                                   buf, buf, nullptr),
          INV, null_arg, "snapshots: null prior before corrector");
  refused(dmip_em_sample_snapshots(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1, 0.16f, 2,
                                   buf, buf, nullptr),
          INV, "corrector steps: CDiffE sampler only", "snapshots: corrector, CDE");
  refused(dmip_em_sample_snapshots(CDIFFE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, -1, 0.f, 2,
                                   buf, buf, nullptr),
          INV, "corrector_steps must be >= 0", "snapshots: corrector < 0");
  refused(dmip_em_sample_snapshots(CDIFFE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1, 0.f, 2,
                                   buf, buf, nullptr),
          INV, "snr must be > 0", "snapshots: snr");
  refused(dmip_em_sample_snapshots(CDIFFE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1, 0.16f,
                                   2, buf, buf, nullptr),
          INV, null_arg, "snapshots: null net");
  // dmip_em_sample_lmbd
  refused(dmip_em_sample_lmbd(CDIFFE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1.5, nullptr, 0,
                              nullptr, buf, nullptr),
          INV, "em_sample_lmbd: CDE and Posterior samplers only", "lmbd: mode before lmbd");
  refused(dmip_em_sample_lmbd(POST, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1.5, nullptr, 0,
                              nullptr, buf, nullptr),
          INV, null_arg, "lmbd: null prior before lmbd");
  for (double l : {1.5, -0.25, std::nan("")})
    refused(dmip_em_sample_lmbd(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 0, 0.f, 1.f, 1, 0, l, nullptr, 0,
                                nullptr, buf, nullptr),
            INV, "lmbd must be in [0, 1]", "lmbd: lmbd before num_steps");
  refused(dmip_em_sample_lmbd(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 0, 0.f, 1.f, 1, 0, 1.0, nullptr, -1,
                              nullptr, buf, nullptr),
          INV, "num_steps must be >= 1", "lmbd: num_steps before snapshot_every");
  refused(dmip_em_sample_lmbd(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1.0, nullptr, -1,
                              buf, buf, nullptr),
          INV, snap01, "lmbd: snapshot_every < 0");
  refused(dmip_em_sample_lmbd(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1.0, nullptr, 11,
                              buf, buf, nullptr),
          INV, snap01, "lmbd: snapshot_every > num_steps");
  refused(dmip_em_sample_lmbd(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1.0, nullptr, 2,
                              nullptr, buf, nullptr),
          INV, snap01, "lmbd: snapshots without a buffer");
  refused(dmip_em_sample_lmbd(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1.0, nullptr, 2,
                              buf, buf, nullptr),
          INV, null_arg, "lmbd: null net");
  // dmip_ode_sample
  const char* x0_euler =
      "ode_sample: x0_dev needs DMIP_SOLVER_HEUN (the Euler samplers start from "
      "injected noise: dmip_em_sample_lmbd's noise_dev)";
  refused(dmip_ode_sample(CDIFFE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 2, 7, nullptr, 0,
                          nullptr, buf, nullptr),
          INV, "ode_sample: CDE and Posterior samplers only", "ode: mode before solver");
  refused(dmip_ode_sample(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 0, 0.f, 1.f, 1, 2, 7, buf, 0, nullptr, buf,
                          nullptr),
          INV, "unknown solver", "ode: solver before num_steps");
  refused(dmip_ode_sample(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 0, 0.f, 1.f, 1, 2, DMIP_SOLVER_HEUN,
                          nullptr, 11, buf, buf, nullptr),
          INV, "num_steps must be >= 1", "ode: num_steps before snapshot_every");
  for (int solver : {DMIP_SOLVER_EULER, DMIP_SOLVER_HEUN}) {
    refused(dmip_ode_sample(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 2, solver, buf, 11, buf,
                            buf, nullptr),
            INV, snap01, "ode: snapshot_every before x0");
    refused(dmip_ode_sample(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 2, solver, nullptr, 2,
                            nullptr, buf, nullptr),
            INV, snap01, "ode: snapshots without a buffer");
    refused(dmip_ode_sample(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 2, solver, nullptr, 0,
                            nullptr, buf, nullptr),
            INV, null_arg, "ode: null net");
    refused(dmip_ode_sample(POST, nullptr, nullptr, nullptr, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 2, solver, nullptr,
                            0, nullptr, nullptr, nullptr),
            INV, null_arg, "ode: nulls, Posterior");
  }
  refused(dmip_ode_sample(CDE, nullptr, nullptr, &sde, buf, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 2, DMIP_SOLVER_EULER, buf,
                          0, nullptr, buf, nullptr),
          UNS, x0_euler, "ode: x0 with Euler before null net");
  expect(dmip_ode_sample_supported(CDIFFE, 64, 3, 2, 2, DMIP_PREC_F32, DMIP_SOLVER_HEUN), 0, "ode_supported: CDiffE");
  expect(dmip_ode_sample_supported(CDE, 64, 3, 2, 2, DMIP_PREC_FP16, DMIP_SOLVER_HEUN), 0, "ode_supported: 16-bit Heun");
  expect(dmip_ode_sample_supported(CDE, 64, 3, 2, 2, DMIP_PREC_F32, 7), 0, "ode_supported: solver");
  expect(dmip_ode_sample_supported(CDE, 64, 3, 2, 2, DMIP_PREC_FP16, DMIP_SOLVER_EULER),
         dmip_sampler_supported_precision(DMIP_PREC_FP16, CDE, 64, 3, 2, 2), "ode_supported: Euler");
  expect(dmip_sampler_supported_precision(7, CDE, 64, 3, 2, 2), 0, "supported: precision");
  // dmip_flow_logp
  refused(dmip_flow_logp(CDIFFE, nullptr, nullptr, &sde, buf, buf, 1, 2, 2, 4, 0, buf, nullptr, nullptr), INV,
          "flow_logp: CDE and Posterior estimators only", "flow: mode before num_steps");
  refused(dmip_flow_logp(CDE, nullptr, nullptr, &sde, buf, buf, 1, 2, 2, 4, 0, buf, nullptr, nullptr), INV,
          "num_steps must be >= 1", "flow: num_steps before null net");
  refused(dmip_flow_logp(CDE, nullptr, nullptr, &sde, buf, buf, 1, 2, 2, 4, 8, buf, nullptr, nullptr), INV, null_arg,
          "flow: null net");
  refused(dmip_flow_logp(POST, nullptr, nullptr, &sde, buf, buf, 1, 2, 2, 4, 8, nullptr, nullptr, nullptr), INV,
          null_arg, "flow: null prior / output");
  // the other flow entry points: each one's sequence mode, num_steps, count, stdv, null argument, precision, two faults
  // at a time (`fake` stands for a handle where the check under test comes before the handle is read)
  const dmip_mlp* fake = reinterpret_cast<const dmip_mlp*>(buf);
  const char* steps1 = "num_steps must be >= 1";
  const char* stdv0 = "stdv must be > 0";
  const char* prec_unknown = "unknown precision";
  auto logp_ex = [&](int mode, const dmip_mlp* net, int steps, int prec) {
    return dmip_flow_logp_ex(mode, net, nullptr, &sde, buf, buf, 1, 2, 2, 4, steps, buf, nullptr, prec, nullptr);
  };
  refused(logp_ex(CDIFFE, nullptr, 0, 7), INV, "flow_logp: CDE and Posterior estimators only",
          "flow_logp_ex: mode before num_steps");
  refused(logp_ex(CDE, nullptr, 0, 7), INV, steps1, "flow_logp_ex: num_steps before null net");
  refused(logp_ex(CDE, nullptr, 8, 7), INV, null_arg, "flow_logp_ex: null net before precision");
  refused(logp_ex(POST, fake, 8, 7), INV, null_arg, "flow_logp_ex: null prior before precision");
  refused(logp_ex(CDE, fake, 8, 7), INV, prec_unknown, "flow_logp_ex: precision before the handle");
  refused(logp_ex(CDE, fake, 8, -1), INV, prec_unknown, "flow_logp_ex: precision < 0");
  auto smp = [&](bool ex, int mode, const dmip_mlp* net, int steps, int64_t n_chains, float stdv, int prec) {
    return ex ? dmip_flow_sample_ex(mode, net, nullptr, &sde, buf, 1, 2, 2, n_chains, 0, steps, 0.f, stdv, 1, nullptr,
                                    buf, buf, prec, nullptr)
              : dmip_flow_sample(mode, net, nullptr, &sde, buf, 1, 2, 2, n_chains, 0, steps, 0.f, stdv, 1, nullptr, buf,
                                 buf, nullptr);
  };
  for (bool ex : {false, true}) {
    refused(smp(ex, CDIFFE, nullptr, 0, 4, 1.f, 1), INV, "flow_sample: CDE and Posterior estimators only",
            "flow_sample: mode before num_steps");
    refused(smp(ex, CDE, nullptr, 0, 0, 1.f, 1), INV, steps1, "flow_sample: num_steps before n_chains");
    for (int64_t n : {0, -3})
      refused(smp(ex, CDE, nullptr, 8, n, 0.f, 1), INV, "n_chains must be >= 1", "flow_sample: n_chains before stdv");
    for (float s : {0.f, -1.f, std::nanf("")})
      refused(smp(ex, CDE, nullptr, 8, 4, s, 1), INV, stdv0, "flow_sample: stdv before null net");
    refused(smp(ex, CDE, nullptr, 8, 4, 1.f, 7), INV, null_arg, "flow_sample: null net before precision");
    refused(smp(ex, POST, fake, 8, 4, 1.f, 7), INV, null_arg, "flow_sample: null prior before precision");
  }
  refused(smp(true, CDE, fake, 8, 4, 1.f, 7), INV, prec_unknown, "flow_sample_ex: precision before the handle");
  refused(dmip_flow_sample_ex(CDE, fake, nullptr, &sde, buf, 1, 2, 2, 4, 0, 8, 0.f, 1.f, 1, nullptr, buf, nullptr, 1,
                              nullptr),
          INV, null_arg, "flow_sample_ex: null logq");
  const char* n1 = "n must be >= 1";
  auto logp_pairs = [&](int mode, const dmip_mlp* net, int steps, int64_t n, int prec) {
    return dmip_flow_logp_pairs(mode, net, nullptr, &sde, buf, buf, 2, 2, n, steps, buf, nullptr, prec, nullptr);
  };
  refused(logp_pairs(CDIFFE, nullptr, 0, 2, 1), INV, "flow_logp_pairs: CDE and Posterior estimators only",
          "flow_logp_pairs: mode before num_steps");
  refused(logp_pairs(CDE, nullptr, 0, 0, 1), INV, steps1, "flow_logp_pairs: num_steps before n");
  for (int64_t n : {0, -3}) refused(logp_pairs(CDE, nullptr, 8, n, 7), INV, n1, "flow_logp_pairs: n before null net");
  refused(logp_pairs(CDE, nullptr, 8, 2, 7), INV, null_arg, "flow_logp_pairs: null net before precision");
  refused(logp_pairs(POST, fake, 8, 2, 7), INV, null_arg, "flow_logp_pairs: null prior before precision");
  refused(logp_pairs(CDE, fake, 8, 2, 7), INV, prec_unknown, "flow_logp_pairs: precision before the handle");
  auto smp_pairs = [&](int mode, const dmip_mlp* net, int steps, int64_t n, float stdv, int prec) {
    return dmip_flow_sample_pairs(mode, net, nullptr, &sde, buf, 2, 2, n, 0, steps, 0.f, stdv, 1, nullptr, buf, buf,
                                  prec, nullptr);
  };
  refused(smp_pairs(CDIFFE, nullptr, 0, 2, 1.f, 1), INV, "flow_sample_pairs: CDE and Posterior estimators only",
          "flow_sample_pairs: mode before num_steps");
  refused(smp_pairs(CDE, nullptr, 0, 0, 1.f, 1), INV, steps1, "flow_sample_pairs: num_steps before n");
  for (int64_t n : {0, -3}) refused(smp_pairs(CDE, nullptr, 8, n, 0.f, 1), INV, n1, "flow_sample_pairs: n before stdv");
  for (float s : {0.f, -1.f, std::nanf("")})
    refused(smp_pairs(CDE, nullptr, 8, 2, s, 1), INV, stdv0, "flow_sample_pairs: stdv before null net");
  refused(smp_pairs(CDE, nullptr, 8, 2, 1.f, 7), INV, null_arg, "flow_sample_pairs: null net before precision");
  refused(smp_pairs(POST, fake, 8, 2, 1.f, 7), INV, null_arg, "flow_sample_pairs: null prior before precision");
  refused(smp_pairs(CDE, fake, 8, 2, 1.f, 7), INV, prec_unknown, "flow_sample_pairs: precision before the handle");
  // MH
  refused(dmip_surrogate_forward(nullptr, buf, 4, buf, nullptr), INV, "null surrogate handle", "surrogate_forward: null");
  refused(dmip_log_posterior(nullptr, &nz_bad, buf, buf, 5, -1, buf, nullptr, nullptr), INV, "null surrogate handle",
          "log_posterior: handle first");
  refused(dmip_mh_sample(nullptr, &nz_bad, nullptr, 0, -1, -1, -1, -1.f, 1, nullptr, buf, nullptr, nullptr, nullptr,
                         nullptr),
          INV, "null surrogate handle", "mh: handle first");
  for (int prec : {DMIP_PREC_F32, DMIP_PREC_F32X3})
    refused(dmip_mh_sample_ex(nullptr, &nz, buf, 1, 10, 0, 5, 0.5f, 1, nullptr, nullptr, nullptr, prec, buf, nullptr,
                              nullptr),
            INV, "null surrogate handle", "mh_ex: null handle");
  refused(dmip_mh_sample_ex(nullptr, nullptr, nullptr, 0, 10, 0, 5, 0.5f, 1, nullptr, nullptr, nullptr, DMIP_PREC_FP16,
                            nullptr, nullptr, nullptr),
          INV, "MH precision: DMIP_PREC_F32 or DMIP_PREC_F32X3", "mh_ex: precision first");
  // DPS
  refused(dmip_dps_sample(nullptr, nullptr, &nz_bad, &sde, buf, 0, -1, 0, 0, 0.f, 1.f, 1, 7, -1.f, buf, nullptr), INV,
          null_arg, "dps: null first");
  for (int prec : {DMIP_PREC_F32, DMIP_PREC_F32X3})
    refused(dmip_dps_sample_ex(nullptr, nullptr, &nz, &sde, buf, 1, 10, 0, 5, 0.f, 1.f, 1, 7, 1.f, prec, buf, nullptr),
            INV, null_arg, "dps_ex: null before mode");
  refused(dmip_dps_sample_ex(nullptr, nullptr, &nz, &sde, buf, 1, 10, 0, 5, 0.f, 1.f, 1, 0, 1.f, DMIP_PREC_FP16, buf,
                             nullptr),
          INV, "DPS precision: DMIP_PREC_F32 or DMIP_PREC_F32X3", "dps_ex: precision first");
}

int main() {
  expect(dmip_abi_version(), DMIP_ABI_VERSION, "abi version");
  sampler_refusals();
  const int w3[3] = {64, 64, 64}, wneq[3] = {64, 32, 64}, w1[1] = {96};
  const float* null4[4] = {nullptr, nullptr, nullptr, nullptr};
  dmip_mlp* net = nullptr;
  expect(dmip_mlp_create(5, 2, 3, w3, 0, 0, 2, null4, null4, &net), DMIP_ERR_INVALID, "create: null layers");
  expect(dmip_mlp_create(5, 2, 3, wneq, 0, 0, 2, null4, null4, &net), DMIP_ERR_UNSUPPORTED, "create: widths");
  expect(dmip_mlp_create(5, 2, 3, w3, 1, 0, 2, null4, null4, &net), DMIP_ERR_UNSUPPORTED, "create: act");
  expect(dmip_mlp_create(5, 40, 3, w3, 0, 0, 2, null4, null4, &net), DMIP_ERR_UNSUPPORTED, "create: out_dim");
  expect(dmip_mlp_create(5, 2, 0, w3, 0, 0, 2, null4, null4, &net), DMIP_ERR_INVALID, "create: n_hidden");
  expect(dmip_mlp_create(5, 2, 1, w1, 0, 7, 2, null4, null4, &net), DMIP_ERR_INVALID, "create: layout");
  expect(dmip_mlp_create(5, 2, 1, w1, 0, 1, 2, null4, null4, &net), DMIP_ERR_INVALID, "create: X_T in_dim");
  expect(dmip_mlp_create(5, 2, 3, nullptr, 0, 0, 2, null4, null4, &net), DMIP_ERR_INVALID, "create: null widths");
  if (net != nullptr) ++failures;
  dmip_vpsde sde{0.1, 20.0, 1.0};
  expect(dmip_mlp_forward(nullptr, nullptr, nullptr, 0, nullptr, 0, 4, nullptr, 0, nullptr), DMIP_ERR_INVALID,
         "forward: null");
  expect(dmip_em_sample(nullptr, &sde, nullptr, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, nullptr, nullptr, nullptr),
         DMIP_ERR_INVALID, "em_sample: null");
  expect(dmip_em_sample_posterior(nullptr, nullptr, &sde, nullptr, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 1, nullptr,
                                  nullptr),
         DMIP_ERR_INVALID, "posterior: null");
  expect(dmip_em_sample_cdiffe(nullptr, &sde, nullptr, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, -1, 0.16f, nullptr,
                               nullptr),
         DMIP_ERR_INVALID, "cdiffe: corrector steps");
  expect(dmip_em_sample_cdiffe(nullptr, &sde, nullptr, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 1, 0.f, nullptr, nullptr),
         DMIP_ERR_INVALID, "cdiffe: snr");
  dmip_loss_cfg cfg{};
  expect(dmip_loss_grad(5, 2, 3, w3, 2, nullptr, nullptr, &sde, &cfg, nullptr, nullptr, nullptr, nullptr, 16, nullptr,
                        nullptr, nullptr),
         DMIP_ERR_INVALID, "loss_grad: null");
  expect(dmip_loss_grad_supported(5, 2, 3, w3, 2), 1, "loss_grad_supported");
  expect(dmip_loss_grad_supported(5, 2, 3, wneq, 2), 0, "loss_grad_supported widths");
  expect(dmip_histogram(nullptr, 10, 3, 75, -1.0, 1.0, 1, nullptr, nullptr), DMIP_ERR_INVALID, "histogram: null");
  dmip_surrogate* sur = nullptr;
  const int w256[3] = {256, 256, 256};
  expect(dmip_surrogate_create(3, 23, 3, w256, null4, null4, &sur), DMIP_ERR_INVALID, "surrogate: null layers");
  expect(dmip_surrogate_create(2, 23, 3, w256, null4, null4, &sur), DMIP_ERR_UNSUPPORTED, "surrogate: shape");
  dmip_scat_noise nz{0.2f, 0.01f, 1000.f};
  expect(dmip_log_posterior(nullptr, &nz, nullptr, nullptr, 0, 4, nullptr, nullptr, nullptr), DMIP_ERR_INVALID,
         "log_posterior: null");
  expect(dmip_mh_sample(nullptr, &nz, nullptr, 1, 10, 0, 5, 0.5f, 1, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr),
         DMIP_ERR_INVALID, "mh: null");
  expect(dmip_dps_sample(nullptr, nullptr, &nz, &sde, nullptr, 1, 10, 0, 5, 0.f, 1.f, 1, 0, 1.f, nullptr, nullptr),
         DMIP_ERR_INVALID, "dps: null");
  expect(dmip_rng_words(1, 0, 0, 10, 4, nullptr, nullptr), DMIP_ERR_INVALID, "rng_words: null");
  expect(dmip_schedule(0, &sde, nullptr, nullptr), DMIP_ERR_INVALID, "schedule: steps");
  expect(dmip_sampler_supported(0, 256, 3, 3, 23), 1, "supported bf16");
  expect(dmip_sampler_supported_f32(2, 512, 3, 3, 23), 1, "supported f32");
  expect(dmip_sampler_supported(2, 512, 3, 3, 23), 1, "supported bf16 CDiffE width 512");
  float dummy[4];
  expect(dmip_em_sample_snapshots(0, nullptr, nullptr, &sde, nullptr, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 0, 0.16f,
                                  0, dummy, nullptr, nullptr),
         DMIP_ERR_INVALID, "snapshots: every");
  expect(dmip_em_sample_snapshots(0, nullptr, nullptr, &sde, nullptr, 1, 2, 2, 10, 0, 10, 0.f, 1.f, 1, 0, 0, 0.16f,
                                  2, nullptr, nullptr, nullptr),
         DMIP_ERR_INVALID, "snapshots: null buffer");
  dmip_train_plan* plan = nullptr;
  expect(dmip_train_plan_create(nullptr, &plan), DMIP_ERR_INVALID, "train_plan: null desc");
  dmip_train_plan_desc d{};
  expect(dmip_train_plan_create(&d, &plan), DMIP_ERR_INVALID, "train_plan: null pointers");
  expect(dmip_train_plan_step(nullptr, nullptr, nullptr, nullptr), DMIP_ERR_INVALID, "train_plan: null step");
  expect(dmip_train_plan_destroy(nullptr), DMIP_OK, "train_plan: destroy null");
  // the error buffer is thread-local: concurrent failures keep their own messages
  std::string a, b;
  std::thread t1([&] {
    dmip_schedule(0, &sde, nullptr, nullptr);
    a = dmip_last_error();
  });
  std::thread t2([&] {
    dmip_mlp_create(5, 2, 3, wneq, 0, 0, 2, null4, null4, &net);
    b = dmip_last_error();
  });
  t1.join();
  t2.join();
  if (a == b || a.empty() || b.empty()) {
    std::printf("FAIL thread-local errors: '%s' / '%s'\n", a.c_str(), b.c_str());
    ++failures;
  }
  std::printf("%s: %d failure(s)\n", failures ? "FAIL" : "ok", failures);
  return failures ? 1 : 0;
}
