// libdmip.so C-ABI, training and evaluation entry points: the config-5 loss + gradient kernel and the exact-f32
// stacked-jet step, the training draws, Adam, the captured training-step graph, the histogram, and the GEMM-composed
// PosteriorLoss step.
#include <utility>

#include "dmip_capi_common.h"

using namespace dmip_capi;

static bool train_shape_ok(int in_dim, int out_dim, int n_hidden, const int* widths, int xdim) {
  if (!widths || (n_hidden != 2 && n_hidden != 3)) return false;
  for (int i = 0; i < n_hidden; ++i)
    if (widths[i] != dmip::kTrainWidth) return false;
  return xdim == dmip::kTrainXdim && out_dim == dmip::kTrainXdim &&
         in_dim == dmip::kTrainXdim + dmip::kTrainYdim + 1;
}

extern "C" int dmip_loss_grad_supported(int in_dim, int out_dim, int n_hidden, const int* widths, int xdim) {
  return train_shape_ok(in_dim, out_dim, n_hidden, widths, xdim) ? 1 : 0;
}

// Scratch of a loss + gradient launch sequence: null = stream-ordered allocation per call (the C-ABI
// entry points); query = report the bytes only (no launch); else the caller's persistent buffer (the
// captured training-step graph, dmip_train_plan).
struct Workspace {
  char* ptr = nullptr;
  size_t bytes = 0;
  bool query = false;
};

static int loss_grad_bf16_impl(int in_dim, int out_dim, int n_hidden, const int* widths, int xdim,
                               const float* const* weights_dev, const float* const* biases_dev, const dmip_vpsde* sde,
                               const dmip_loss_cfg* cfg, const float* x_dev, const float* y_dev, const float* t_dev,
                               const float* eps_dev, int64_t batch, float* grad_out_dev, float* loss_out_dev,
                               void* stream, Workspace* ws, const dmip::TrainFuse* fuse = nullptr) {
  if (!weights_dev || !biases_dev || !sde || !cfg || !x_dev || !y_dev || !t_dev || !eps_dev || !grad_out_dev ||
      !loss_out_dev)
    return fail(DMIP_ERR_INVALID, "null argument");
  if (!train_shape_ok(in_dim, out_dim, n_hidden, widths, xdim))
    return fail(DMIP_ERR_UNSUPPORTED, "no compiled training kernel for this network (compiled: in 5, out 2, xdim 2, "
                                      "widths 64, 2 or 3 hidden layers)");
  for (int i = 0; i <= n_hidden; ++i)
    if (!weights_dev[i] || !biases_dev[i]) return fail(DMIP_ERR_INVALID, "null layer pointer");
  if (batch < 1) return fail(DMIP_ERR_INVALID, "batch must be >= 1");
  if (cfg->kind < DMIP_LOSS_DSM || cfg->kind > DMIP_LOSS_PINN2) return fail(DMIP_ERR_INVALID, "unknown loss kind");
  const bool needs_pde = cfg->kind != DMIP_LOSS_DSM;
  if (needs_pde && cfg->pde != DMIP_PDE_FPE && cfg->pde != DMIP_PDE_CFPE)
    return fail(DMIP_ERR_INVALID, "pde must be DMIP_PDE_FPE or DMIP_PDE_CFPE for this loss");
  for (int m : {cfg->pde_metric, cfg->ic_metric})
    if (m != DMIP_METRIC_L1 && m != DMIP_METRIC_L2) return fail(DMIP_ERR_INVALID, "metric must be L1 or L2");
  if (!(sde->beta_min > 0.0)) return fail(DMIP_ERR_INVALID, "beta_min must be > 0");
  hipStream_t st = (hipStream_t)stream;
  dmip::TrainParams p{};
  for (int i = 0; i <= n_hidden; ++i) p.w[i] = weights_dev[i], p.b[i] = biases_dev[i];
  p.x = x_dev;
  p.y = y_dev;
  p.t = t_dev;
  p.eps = eps_dev;
  p.n = batch;
  p.inv_n = (float)(1.0 / (double)batch);
  p.bmin = (float)sde->beta_min;
  p.bdiff = (float)(sde->beta_max - sde->beta_min);
  p.has_dsm = cfg->kind == DMIP_LOSS_DSM || cfg->kind == DMIP_LOSS_DSM_PDE || cfg->kind == DMIP_LOSS_PINN;
  p.has_ic = cfg->kind == DMIP_LOSS_PINN || cfg->kind == DMIP_LOSS_PINN2;
  p.pde = needs_pde ? cfg->pde : 0;
  p.pde_l1 = cfg->pde_metric == DMIP_METRIC_L1;
  p.ic_l1 = cfg->ic_metric == DMIP_METRIC_L1;
  p.lam = cfg->lam;
  p.lam2 = cfg->lam2;
  for (int i = 0; i < 4; ++i) p.icA[i] = cfg->ic_A[i], p.icS[i] = cfg->ic_Sinv[i];
  p.icb[0] = cfg->ic_b[0];
  p.icb[1] = cfg->ic_b[1];
  // one workgroup per CU (LDS-bound; one wave per SIMD), 16-sample tiles strided over the waves
  int n_cu = 256;
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dmip::stream_device(st));
  if (n_cu < 1) n_cu = 256;
  const int64_t tiles = (batch + 15) / 16;
  const int64_t per_wg = dmip::train_waves_per_wg();
  int n_wg = (int)std::min<int64_t>((int64_t)n_cu, (tiles + per_wg - 1) / per_wg);
  if (n_wg < 1) n_wg = 1;
  const size_t part_bytes =
      (size_t)n_wg * dmip::train_partials_per_wg() * dmip::train_partial_stride(n_hidden) * sizeof(float);
  // one scratch allocation: the partial rows, then the packed LDS image of the weights
  const size_t part_pad = (part_bytes + 255) / 256 * 256;
  const size_t packed_pad = ((size_t)dmip::train_packed_bytes(n_hidden) + 255) / 256 * 256;
  const size_t need = part_pad + packed_pad + dmip::train_adj_bytes(batch);
  if (ws && ws->query) {
    ws->bytes = need;
    return DMIP_OK;
  }
  float* partials = nullptr;
  hipError_t e = hipSuccess;
  if (ws) {
    if (ws->bytes < need) return fail(DMIP_ERR_INVALID, "workspace too small");
    partials = (float*)ws->ptr;
  } else if ((e = hipMallocAsync((void**)&partials, need, st)) != hipSuccess) {
    return fail(DMIP_ERR_ALLOC, std::string("hipMallocAsync: ") + hipGetErrorString(e));
  }
  p.packed = (char*)partials + part_pad;
  p.adj = dmip::train_adj_bytes(batch) ? (float*)((char*)partials + part_pad + packed_pad) : nullptr;
  e = fuse ? dmip::launch_loss_grad_fused(p, n_hidden, grad_out_dev, loss_out_dev, partials, n_wg, *fuse, st)
           : dmip::launch_loss_grad(p, n_hidden, grad_out_dev, loss_out_dev, partials, n_wg, st);
  if (!ws) (void)hipFreeAsync(partials, st);
  if (e != hipSuccess) return hip_fail(e, "loss_grad launch");
  return DMIP_OK;
}

static int loss_grad_f32_impl(int in_dim, int out_dim, int n_hidden, const int* widths, int xdim,
                              const float* const* weights_dev, const float* const* biases_dev, const dmip_vpsde* sde,
                              const dmip_loss_cfg* cfg, const float* x_dev, const float* y_dev, const float* t_dev,
                              const float* eps_dev, const float* ic_target_dev, int64_t batch, float* grad_out_dev,
                              float* loss_out_dev, void* stream, Workspace* ws) {
  if (!widths || !weights_dev || !biases_dev || !sde || !cfg || !x_dev || !y_dev || !t_dev || !eps_dev ||
      !grad_out_dev || !loss_out_dev)
    return fail(DMIP_ERR_INVALID, "null argument");
  if (n_hidden < 1 || n_hidden > dmip::kJetsMaxLayers - 1) return fail(DMIP_ERR_UNSUPPORTED, "n_hidden must be in [1, 8]");
  if (out_dim != xdim) return fail(DMIP_ERR_UNSUPPORTED, "f32 training: score networks with out_dim == xdim");
  if (xdim < 1 || xdim > (cfg->kind == DMIP_LOSS_DSM ? dmip::kJetsMaxDsmDim : 4))
    return fail(DMIP_ERR_UNSUPPORTED, "f32 training: xdim in [1, 4] (DSMLoss: [1, 64])");
  const int ydim = in_dim - xdim - 1;
  if (ydim < 0) return fail(DMIP_ERR_INVALID, "in_dim must be xdim + ydim + 1");
  for (int i = 0; i < n_hidden; ++i)
    if (widths[i] < 1 || widths[i] > 4096) return fail(DMIP_ERR_INVALID, "hidden widths must be in [1, 4096]");
  for (int i = 0; i <= n_hidden; ++i)
    if (!weights_dev[i] || !biases_dev[i]) return fail(DMIP_ERR_INVALID, "null layer pointer");
  if (batch < 1) return fail(DMIP_ERR_INVALID, "batch must be >= 1");
  if (cfg->kind < DMIP_LOSS_DSM || cfg->kind > DMIP_LOSS_PINN2) return fail(DMIP_ERR_INVALID, "unknown loss kind");
  const bool has_pde = cfg->kind != DMIP_LOSS_DSM;
  const bool has_ic = cfg->kind == DMIP_LOSS_PINN || cfg->kind == DMIP_LOSS_PINN2;
  if (has_pde && cfg->pde != DMIP_PDE_FPE && cfg->pde != DMIP_PDE_CFPE)
    return fail(DMIP_ERR_INVALID, "pde must be DMIP_PDE_FPE or DMIP_PDE_CFPE for this loss");
  if (has_ic && !ic_target_dev && (xdim != 2 || ydim != 2))
    return fail(DMIP_ERR_INVALID, "initial-condition target required (the built-in one is the linear problem's, 2-D)");
  if (!(sde->beta_min > 0.0)) return fail(DMIP_ERR_INVALID, "beta_min must be > 0");
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = batch;
  dmip::JetsParams p{};
  p.batch = B;
  p.xdim = xdim;
  p.ydim = ydim;
  p.out_dim = out_dim;
  p.bmin = (float)sde->beta_min;
  p.bdiff = (float)(sde->beta_max - sde->beta_min);
  p.lam = cfg->lam;
  p.lam2 = cfg->lam2;
  p.has_dsm = cfg->kind != DMIP_LOSS_PINN2;
  p.pde = has_pde ? cfg->pde : 0;
  p.pde_l1 = cfg->pde_metric == DMIP_METRIC_L1;
  p.ic_l1 = cfg->ic_metric == DMIP_METRIC_L1;
  for (int i = 0; i < 4; ++i) p.icA[i] = cfg->ic_A[i], p.icS[i] = cfg->ic_Sinv[i];
  p.icb[0] = cfg->ic_b[0];
  p.icb[1] = cfg->ic_b[1];
  p.x = x_dev;
  p.y = y_dev;
  p.t = t_dev;
  p.eps = eps_dev;
  p.ic_target = ic_target_dev;
  const bool fpe = has_pde && cfg->pde == DMIP_PDE_FPE;
  p.blk_v = has_pde ? 1 : -1;
  p.blk_c = has_ic ? (has_pde ? 2 : 1) : -1;
  p.n_bwd = 1 + (has_pde ? 1 : 0) + (has_ic ? 1 : 0);
  p.blk_e = p.n_bwd;
  p.n_e = fpe ? xdim : 0;
  p.n_pair = fpe ? xdim * (xdim + 1) / 2 : 0;
  p.n_streams = p.n_bwd + p.n_e + p.n_pair;
  int wmax = in_dim + 1;
  for (int i = 0; i < n_hidden; ++i) wmax = std::max(wmax, widths[i] + 1);
  p.splits = 64;  // the cap: each weight-gradient GEMM picks its own split count (dmip_jets.hip wgrad_splits)
  const int64_t nS = p.n_streams, nb = p.n_bwd;
  std::vector<std::pair<float**, size_t>> plan;
  for (int l = 0; l <= n_hidden; ++l) plan.emplace_back(&p.h[l], (size_t)nS * B * ((l == 0 ? in_dim : widths[l - 1]) + 1));
  for (int l = 0; l < n_hidden; ++l) plan.emplace_back(&p.aux[l], (size_t)3 * B * widths[l]);
  plan.emplace_back(&p.scal, (size_t)B * 8);
  plan.emplace_back(&p.x_t, (size_t)B * xdim);
  plan.emplace_back(&p.z, (size_t)nS * B * wmax);
  plan.emplace_back(&p.a_out, (size_t)nS * B * out_dim);
  plan.emplace_back(&p.zbar, (size_t)nb * B * out_dim);
  plan.emplace_back(&p.zbar_a, (size_t)nb * B * wmax);
  plan.emplace_back(&p.zbar_b, (size_t)nb * B * wmax);
  plan.emplace_back(&p.hbar, (size_t)nb * B * wmax);
  plan.emplace_back(&p.rows, (size_t)B * 3);
  plan.emplace_back(&p.part, (size_t)p.splits * wmax * wmax);
  size_t total = 0;
  for (auto& q : plan) total += (q.second * sizeof(float) + 255) / 256 * 256;
  if (ws && ws->query) {
    ws->bytes = total;
    return DMIP_OK;
  }
  char* scratch = nullptr;
  hipError_t e = hipSuccess;
  if (ws) {
    if (ws->bytes < total) return fail(DMIP_ERR_INVALID, "workspace too small");
    scratch = ws->ptr;
  } else if ((e = hipMallocAsync((void**)&scratch, total, st)) != hipSuccess) {
    return fail(DMIP_ERR_ALLOC, std::string("hipMallocAsync: ") + hipGetErrorString(e));
  }
  size_t o = 0;
  for (auto& q : plan) {
    *q.first = (float*)(scratch + o);
    o += (q.second * sizeof(float) + 255) / 256 * 256;
  }
  p.loss_out = loss_out_dev;
  e = dmip::launch_jets_loss_grad(p, n_hidden, widths, weights_dev, biases_dev, grad_out_dev, st);
  if (!ws) (void)hipFreeAsync(scratch, st);
  if (e != hipSuccess) return hip_fail(e, "loss_grad_f32 launch");
  return DMIP_OK;
}

extern "C" {

int dmip_loss_grad(int in_dim, int out_dim, int n_hidden, const int* widths, int xdim,
                   const float* const* weights_dev, const float* const* biases_dev, const dmip_vpsde* sde,
                   const dmip_loss_cfg* cfg, const float* x_dev, const float* y_dev, const float* t_dev,
                   const float* eps_dev, int64_t batch, float* grad_out_dev, float* loss_out_dev, void* stream) {
  return loss_grad_bf16_impl(in_dim, out_dim, n_hidden, widths, xdim, weights_dev, biases_dev, sde, cfg, x_dev,
                             y_dev, t_dev, eps_dev, batch, grad_out_dev, loss_out_dev, stream, nullptr);
}

int dmip_loss_grad_f32(int in_dim, int out_dim, int n_hidden, const int* widths, int xdim,
                       const float* const* weights_dev, const float* const* biases_dev, const dmip_vpsde* sde,
                       const dmip_loss_cfg* cfg, const float* x_dev, const float* y_dev, const float* t_dev,
                       const float* eps_dev, const float* ic_target_dev, int64_t batch, float* grad_out_dev,
                       float* loss_out_dev, void* stream) {
  return loss_grad_f32_impl(in_dim, out_dim, n_hidden, widths, xdim, weights_dev, biases_dev, sde, cfg, x_dev, y_dev,
                            t_dev, eps_dev, ic_target_dev, batch, grad_out_dev, loss_out_dev, stream, nullptr);
}

}  // extern "C"

static int draws_params(uint64_t seed, uint64_t stream_id, int64_t batch, int xdim, int debias, const dmip_vpsde* sde,
                        double t_epsilon, float t_add, float* t_out_dev, float* eps_out_dev, dmip::TrainDrawsParams& p) {
  if (!sde || !t_out_dev || !eps_out_dev) return fail(DMIP_ERR_INVALID, "null argument");
  if (batch < 0 || xdim < 1 || xdim > 4) return fail(DMIP_ERR_INVALID, "batch >= 0 and xdim in [1, 4]");
  if (!(sde->T > 0.0) || !(sde->beta_min > 0.0)) return fail(DMIP_ERR_INVALID, "bad SDE parameters");
  p = dmip::TrainDrawsParams{};
  p.batch = batch;
  p.xdim = xdim;
  p.debias = debias ? 1 : 0;
  p.seed = seed;
  p.stream_id = stream_id;
  p.t_add = t_add;
  p.T = (float)sde->T;
  const double a = sde->beta_max - sde->beta_min, b = sde->beta_min, te = t_epsilon;
  const double B_te = 0.5 * a * te * te + b * te;
  const double r_te = (b + a * te) / (1.0 - std::exp(-B_te));
  const double A_te = std::log(std::expm1(B_te));
  const double B_T = 0.5 * a * sde->T * sde->T + b * sde->T;
  p.a = (float)a;
  p.b = (float)b;
  p.te = (float)te;
  p.r_te = (float)r_te;
  p.A_te = (float)A_te;
  p.Z = (float)(te * r_te + std::log(std::expm1(B_T)) - A_te);
  p.t = t_out_dev;
  p.eps = eps_out_dev;
  return DMIP_OK;
}

static int adam_params(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2,
                       double eps, int64_t step, dmip::AdamParams& p) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !numel) return fail(DMIP_ERR_INVALID, "null argument");
  if (n_tensors < 1 || n_tensors > dmip::kAdamMaxTensors)
    return fail(DMIP_ERR_UNSUPPORTED, "n_tensors must be in [1, 16]");
  if (step < 1) return fail(DMIP_ERR_INVALID, "step must be >= 1 (torch increments before the update)");
  p = dmip::AdamParams{};
  p.n = n_tensors;
  p.off[0] = 0;
  for (int k = 0; k < n_tensors; ++k) {
    if (!params[k] || !grads[k] || !exp_avg[k] || !exp_avg_sq[k] || numel[k] < 0)
      return fail(DMIP_ERR_INVALID, "null tensor or negative size");
    p.param[k] = params[k];
    p.grad[k] = grads[k];
    p.m[k] = exp_avg[k];
    p.v[k] = exp_avg_sq[k];
    p.off[k + 1] = p.off[k] + numel[k];
  }
  // torch.optim.Adam's scalars, in Python double like torch computes them
  const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
  p.step_size = (float)(lr / bc1);
  p.bc2_sqrt = (float)std::sqrt(bc2);
  p.w1 = (float)(1.0 - beta1);
  p.beta2 = (float)beta2;
  p.w2 = (float)(1.0 - beta2);
  p.eps = (float)eps;
  p.lr_d = lr;
  p.beta1_d = beta1;
  p.beta2_d = beta2;
  return DMIP_OK;
}

// ----------------------------------------------------------------- captured training-step graph
struct dmip_train_plan {
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph = nullptr;
  int64_t batch = 0;
  int xdim = 0, ydim = 0;
  float *x = nullptr, *y = nullptr;          // staging: the batch is copied in at each replay
  float *t = nullptr, *eps = nullptr, *loss = nullptr;  // caller-owned
  char* ws = nullptr;
  dmip::StepCounters* ctr = nullptr;
  int device = 0;
  // the draws launch stages the batch itself: each step points that kernel node's x_src / y_src at the caller's
  // batch (hipGraphExecKernelNodeSetParams) instead of two copy nodes; `stage_node` null: copies (fallback)
  hipGraphNode_t stage_node = nullptr;
  hipKernelNodeParams stage_kp{};
  int stage_nargs = 0;
  alignas(16) char stage_args[3][1024];      // the node's argument values (TrainDrawsParams first)
  void* stage_argv[3] = {};
};

// makes `dev` the current device for the guard's scope (and restores the caller's)
struct DeviceGuard {
  int prev = -1, dev = -1;
  explicit DeviceGuard(int d) : dev(d) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev && dev >= 0) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0 && prev != dev && dev >= 0) (void)hipSetDevice(prev);
  }
};

// the device that owns a device pointer (the current device if the runtime cannot tell)
static int pointer_device(const void* p) {
  hipPointerAttribute_t a{};
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (!p) return cur;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // clear only the error this query left (a non-device pointer)
    return cur;
  }
  return a.device >= 0 ? a.device : cur;
}

static void plan_free(dmip_train_plan* pl) {
  if (!pl) return;
  if (pl->exec) (void)hipGraphExecDestroy(pl->exec);
  if (pl->graph) (void)hipGraphDestroy(pl->graph);
  for (void* q : {(void*)pl->x, (void*)pl->y, (void*)pl->ws, (void*)pl->ctr})
    if (q) (void)hipFree(q);
  delete pl;
}

extern "C" {

int dmip_train_draws(uint64_t seed, uint64_t stream_id, int64_t batch, int xdim, int debias, const dmip_vpsde* sde,
                     double t_epsilon, float t_add, float* t_out_dev, float* eps_out_dev, void* stream) {
  dmip::TrainDrawsParams p{};
  const int rc = draws_params(seed, stream_id, batch, xdim, debias, sde, t_epsilon, t_add, t_out_dev, eps_out_dev, p);
  if (rc != DMIP_OK || batch == 0) return rc;
  hipError_t e = dmip::launch_train_draws(p, (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "train_draws launch");
}

int dmip_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2, double eps,
                   int64_t step, void* stream) {
  dmip::AdamParams p{};
  const int rc = adam_params(n_tensors, params, grads, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, step, p);
  if (rc != DMIP_OK) return rc;
  hipError_t e = dmip::launch_adam(p, (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "adam launch");
}

int dmip_train_plan_create(const dmip_train_plan_desc* d, dmip_train_plan** out) {
  if (!d || !out || !d->widths || !d->weights_dev || !d->biases_dev || !d->t_dev || !d->eps_dev || !d->loss_dev)
    return fail(DMIP_ERR_INVALID, "null argument");
  *out = nullptr;
  if (d->batch < 1) return fail(DMIP_ERR_INVALID, "batch must be >= 1");
  if (d->precision != DMIP_PREC_BF16 && d->precision != DMIP_PREC_F32) return fail(DMIP_ERR_INVALID, "unknown precision");
  const int ydim = d->in_dim - d->xdim - 1;
  if (d->xdim < 1 || d->xdim > 4 || ydim < 0) return fail(DMIP_ERR_INVALID, "xdim in [1, 4] and in_dim = xdim + ydim + 1");
  const bool has_ic = d->cfg.kind == DMIP_LOSS_PINN || d->cfg.kind == DMIP_LOSS_PINN2;
  if (has_ic && (d->xdim != 2 || ydim != 2))
    return fail(DMIP_ERR_UNSUPPORTED, "captured steps take the built-in (linear-problem) initial condition only");
  const bool bf16 = d->precision == DMIP_PREC_BF16;
  if (bf16 && !train_shape_ok(d->in_dim, d->out_dim, d->n_hidden, d->widths, d->xdim))
    return fail(DMIP_ERR_UNSUPPORTED, "no compiled bf16 training kernel for this network");
  dmip::AdamParams ap{};
  int rc = adam_params(d->n_tensors, d->params, d->grads, d->exp_avg, d->exp_avg_sq, d->numel, d->lr, d->beta1,
                       d->beta2, d->eps, 1, ap);
  if (rc != DMIP_OK) return rc;
  for (int k = 1; k < d->n_tensors; ++k)
    if (d->grads[k] != d->grads[0] + ap.off[k])
      return fail(DMIP_ERR_INVALID, "grads must be consecutive views of one flat buffer (reference parameter order)");
  // everything the plan allocates, and its capture stream, live on the parameters' device, whatever the
  // caller's current device is (the weights, optimizer state and the replay stream are that device's)
  const DeviceGuard guard(pointer_device(d->weights_dev[0]));
  auto* pl = new dmip_train_plan();
  pl->batch = d->batch;
  pl->xdim = d->xdim;
  pl->ydim = ydim;
  pl->t = d->t_dev;
  pl->eps = d->eps_dev;
  pl->loss = d->loss_dev;
  pl->device = guard.dev;
  const int64_t B = d->batch;
  auto alloc = [&](void** q, size_t bytes) { return hipMalloc(q, bytes < 4 ? 4 : bytes); };
  hipError_t e = hipSuccess;
  if ((e = alloc((void**)&pl->x, (size_t)B * d->xdim * 4)) != hipSuccess ||
      (e = alloc((void**)&pl->y, (size_t)B * ydim * 4)) != hipSuccess ||
      (e = alloc((void**)&pl->ctr, sizeof(dmip::StepCounters))) != hipSuccess) {
    plan_free(pl);
    return fail(DMIP_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  dmip::StepCounters c0{0ull, (long long)d->step0};
  if ((e = hipMemcpy(pl->ctr, &c0, sizeof(c0), hipMemcpyHostToDevice)) != hipSuccess) {
    plan_free(pl);
    return hip_fail(e, "counter init");
  }
  // workspace of the loss sequence, sized by a query pass
  Workspace ws;
  ws.query = true;
  const dmip::TrainFuse* fuse = nullptr;  // bf16: the fused prologue / reduction + Adam launches (set below)
  auto loss_seq = [&](hipStream_t st, Workspace* w) {
    return bf16 ? loss_grad_bf16_impl(d->in_dim, d->out_dim, d->n_hidden, d->widths, d->xdim, d->weights_dev,
                                      d->biases_dev, &d->sde, &d->cfg, pl->x, pl->y, pl->t, pl->eps, B,
                                      d->grads[0], pl->loss, st, w, fuse)
                : loss_grad_f32_impl(d->in_dim, d->out_dim, d->n_hidden, d->widths, d->xdim, d->weights_dev,
                                     d->biases_dev, &d->sde, &d->cfg, pl->x, pl->y, pl->t, pl->eps, nullptr, B,
                                     d->grads[0], pl->loss, st, w);
  };
  if ((rc = loss_seq(nullptr, &ws)) != DMIP_OK) {
    plan_free(pl);
    return rc;
  }
  if ((e = alloc((void**)&pl->ws, ws.bytes)) != hipSuccess) {
    plan_free(pl);
    return fail(DMIP_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  ws.ptr = pl->ws;
  ws.query = false;
  dmip::TrainDrawsParams dp{};
  if ((rc = draws_params(d->seed, d->first_draw, B, d->xdim, d->debias, &d->sde, d->t_epsilon, d->t_add, pl->t,
                         pl->eps, dp)) != DMIP_OK) {
    plan_free(pl);
    return rc;
  }
  dp.draw_ctr = &pl->ctr->draw;
  ap.step_ctr = &pl->ctr->step;
  // the draws launch stages the batch (x_src / y_src set per step in its kernel node)
  dp.x_src = pl->x, dp.y_src = pl->y, dp.x_dst = pl->x, dp.y_dst = pl->y, dp.ydim = ydim;
  // bf16 (the config-5 kernel): four launches -- the pack in the draws launch, Adam and the counters in the
  // gradient reduction (dmip::TrainFuse); exact f32: draws -> loss + gradients -> Adam -> advance the counters
  const dmip::TrainFuse fz{dp, ap, pl->ctr};
  if (bf16 && dmip::train_split()) fuse = &fz;
  hipStream_t cs = nullptr;
  if ((e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking)) != hipSuccess) {
    plan_free(pl);
    return hip_fail(e, "capture stream");
  }
  hipGraph_t g = nullptr;
  e = hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed);
  if (e == hipSuccess) {
    hipError_t le = hipSuccess;
    int lrc = DMIP_OK;
    if (fuse) {
      lrc = loss_seq(cs, &ws);
    } else {
      le = dmip::launch_train_draws(dp, cs);
      lrc = le == hipSuccess ? loss_seq(cs, &ws) : DMIP_ERR_HIP;
      if (lrc == DMIP_OK && (le = dmip::launch_adam(ap, cs)) == hipSuccess) le = dmip::launch_counters_advance(pl->ctr, cs);
    }
    e = hipStreamEndCapture(cs, &g);
    if (e == hipSuccess && (le != hipSuccess || lrc != DMIP_OK)) e = le != hipSuccess ? le : hipErrorUnknown;
  }
  if (e == hipSuccess) e = hipGraphInstantiate(&pl->exec, g, nullptr, nullptr, 0);
  (void)hipStreamDestroy(cs);
  if (e != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    plan_free(pl);
    return hip_fail(e, "training-step graph capture");
  }
  pl->graph = g;
  // the staging kernel node: its arguments are kept here and re-pointed at each step's batch
  const void* stage_fn = fuse ? dmip::train_plan_prologue_func(d->n_hidden) : dmip::train_draws_func();
  size_t nn = 0;
  if (hipGraphGetNodes(g, nullptr, &nn) == hipSuccess && nn > 0) {
    std::vector<hipGraphNode_t> nodes(nn);
    if (hipGraphGetNodes(g, nodes.data(), &nn) == hipSuccess)
      for (size_t i = 0; i < nn && !pl->stage_node; ++i) {
        hipGraphNodeType ty;
        hipKernelNodeParams kp{};
        if (hipGraphNodeGetType(nodes[i], &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) continue;
        if (hipGraphKernelNodeGetParams(nodes[i], &kp) != hipSuccess || kp.func != stage_fn || !kp.kernelParams) continue;
        // prologue (TrainDrawsParams, TrainParams, int) or draws (TrainDrawsParams)
        const size_t sizes[3] = {sizeof(dmip::TrainDrawsParams), sizeof(dmip::TrainParams), sizeof(int)};
        const int nargs = fuse ? 3 : 1;
        for (int a = 0; a < nargs; ++a) {
          std::memcpy(pl->stage_args[a], kp.kernelParams[a], sizes[a]);
          pl->stage_argv[a] = pl->stage_args[a];
        }
        pl->stage_kp = kp;
        pl->stage_kp.kernelParams = pl->stage_argv;
        pl->stage_kp.extra = nullptr;
        pl->stage_nargs = nargs;
        pl->stage_node = nodes[i];
      }
  }
  (void)hipGetLastError();
  *out = pl;
  return DMIP_OK;
}

int dmip_train_plan_step(dmip_train_plan* pl, const float* x_dev, const float* y_dev, void* stream) {
  if (!pl || !x_dev || (pl->ydim > 0 && !y_dev)) return fail(DMIP_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const DeviceGuard guard(pl->device);
  hipError_t e = hipSuccess;
  if (pl->stage_node) {  // the draws launch copies the batch in: point its node at this step's x / y
    auto* dp = (dmip::TrainDrawsParams*)pl->stage_args[0];
    dp->x_src = x_dev;
    dp->y_src = pl->ydim > 0 ? y_dev : pl->y;
    e = hipGraphExecKernelNodeSetParams(pl->exec, pl->stage_node, &pl->stage_kp);
  } else {
    e = hipMemcpyAsync(pl->x, x_dev, (size_t)pl->batch * pl->xdim * 4, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && pl->ydim > 0)
      e = hipMemcpyAsync(pl->y, y_dev, (size_t)pl->batch * pl->ydim * 4, hipMemcpyDeviceToDevice, st);
  }
  if (e == hipSuccess) e = hipGraphLaunch(pl->exec, st);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "training-step graph launch");
}

int dmip_train_plan_set_counters(dmip_train_plan* pl, uint64_t draws_done, int64_t steps_done, void* stream) {
  if (!pl) return fail(DMIP_ERR_INVALID, "null argument");
  if (steps_done < 0) return fail(DMIP_ERR_INVALID, "steps_done must be >= 0");
  // stream-ordered after earlier replays; the source is copied before this call returns
  const dmip::StepCounters c{(unsigned long long)draws_done, (long long)steps_done};
  hipError_t e = hipMemcpyAsync(pl->ctr, &c, sizeof(c), hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "counter update");
}

int dmip_train_plan_destroy(dmip_train_plan* pl) {
  if (!pl) return DMIP_OK;
  const DeviceGuard guard(pl->device);
  (void)hipDeviceSynchronize();  // no replay may still be running on the plan's device
  plan_free(pl);
  return DMIP_OK;
}

int dmip_histogram(const float* x_dev, int64_t n, int d, int nbins, double lo, double hi, int n_hist,
                   uint32_t* counts_dev, void* stream) {
  if (!x_dev || !counts_dev) return fail(DMIP_ERR_INVALID, "null argument");
  if (d < 1 || d > 3 || nbins < 1 || nbins > 4096 || n < 0 || n_hist < 1 || n_hist > 65535 || !(hi > lo))
    return fail(DMIP_ERR_INVALID, "bad histogram shape or range");
  if (n == 0) return DMIP_OK;
  hipError_t e = dmip::launch_histogram(x_dev, n, d, nbins, lo, hi, n_hist, (unsigned int*)counts_dev,
                                        (hipStream_t)stream);
  return e == hipSuccess ? DMIP_OK : hip_fail(e, "histogram launch");
}

}  // extern "C"

// ---- A18: PosteriorLoss value + parameter gradients (GEMM-composed exact-f32 step, dmip_gemm.hip)
namespace {

struct MlpDims {
  int L;                      // hidden layers; linear layers 0..L
  std::vector<int> in, out;   // per linear layer
};

// one network's forward over the batch: layer inputs [B][in+1] (ones column last), hidden outputs
// with their activation derivatives, output [B][out]
struct MlpTape {
  std::vector<float*> h;      // h[l]: input matrix of layer l, [B][in_l + 1]; h[0] is the caller's
  std::vector<float*> d;      // d[l]: act'(z_l) of hidden layer l, [B][out_l]
  float* out = nullptr;       // [B][out_L]
};

hipError_t mlp_forward_f32(const MlpDims& dm, const float* const* W, const float* const* b, MlpTape& tp, int64_t B,
                           hipStream_t st) {
  for (int l = 0; l <= dm.L; ++l) {
    dmip::GemmParams g{};
    g.a = tp.h[l];
    g.lda = dm.in[l] + 1;
    g.b = W[l];
    g.ldb = dm.in[l];
    g.m = B;
    g.n = dm.out[l];
    g.k = dm.in[l];
    g.bias = b[l];
    if (l < dm.L) {
      g.c = tp.h[l + 1];
      g.ldc = dm.out[l] + 1;
      g.epi = l == 0 ? dmip::GEMM_EPI_BIAS_TANH2 : dmip::GEMM_EPI_BIAS_TANH;
      g.aux_out = tp.d[l];
      g.ldaux = dm.out[l];
    } else {
      g.c = tp.out;
      g.ldc = dm.out[l];
      g.epi = dmip::GEMM_EPI_BIAS;
    }
    hipError_t e = dmip::launch_gemm_f32(g, false, true, 1, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// reverse pass from the output adjoint `adj` [B][out_L]: with grads != null, [dW_l | db_l] into the
// flat reference-order gradient buffer; with in_grad != null, d/d(input) [B][in_0] (no parameter grads)
hipError_t mlp_backward_f32(const MlpDims& dm, const float* const* W, const MlpTape& tp, const float* adj, int64_t B,
                            float* delta_a, float* delta_b, float* grads, float* in_grad, float* part, int splits,
                            hipStream_t st) {
  std::vector<size_t> off(dm.L + 2, 0);
  for (int l = 0; l <= dm.L; ++l) off[l + 1] = off[l] + (size_t)dm.out[l] * dm.in[l] + dm.out[l];
  const float* dl = adj;  // adjoint of layer l's output, [B][out_l]
  float* bufs[2] = {delta_a, delta_b};
  for (int l = dm.L; l >= 0; --l) {
    hipError_t e;
    if (grads) {
      dmip::GemmParams g{};
      g.a = dl;
      g.lda = dm.out[l];
      g.b = tp.h[l];
      g.ldb = dm.in[l] + 1;
      g.m = dm.out[l];
      g.n = dm.in[l] + 1;
      g.k = B;
      g.c = grads + off[l];
      g.ldc = dm.in[l];
      g.epi = dmip::GEMM_EPI_WGRAD;
      g.bias_out = grads + off[l] + (size_t)dm.out[l] * dm.in[l];
      g.part = part;
      if ((e = dmip::launch_gemm_f32(g, true, false, dmip::gemm_wgrad_splits(g.m, g.n, g.k, splits), st)) != hipSuccess)
        return e;
    }
    if (l == 0 && !in_grad) break;
    dmip::GemmParams g{};
    g.a = dl;
    g.lda = dm.out[l];
    g.b = W[l];
    g.ldb = dm.in[l];
    g.m = B;
    g.n = dm.in[l];
    g.k = dm.out[l];
    if (l > 0) {
      float* nxt = bufs[l & 1];
      g.c = nxt;
      g.ldc = dm.in[l];
      g.epi = dmip::GEMM_EPI_MUL_AUX;
      g.aux_in = tp.d[l - 1];
      g.ldaux = dm.in[l];
      if ((e = dmip::launch_gemm_f32(g, false, false, 1, st)) != hipSuccess) return e;
      dl = nxt;
    } else {
      g.c = in_grad;
      g.ldc = dm.in[0];
      g.epi = dmip::GEMM_EPI_NONE;
      if ((e = dmip::launch_gemm_f32(g, false, false, 1, st)) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

}  // namespace

extern "C" {

int dmip_posterior_loss_grad(int xdim, int ydim, int n_hidden, const int* widths, const float* const* prior_w,
                             const float* const* prior_b, const float* const* lik_w, const float* const* lik_b,
                             const dmip_surrogate* fwd, const dmip_scat_noise* noise, float lam, const dmip_vpsde* sde,
                             const float* x_dev, const float* y_dev, const float* t_dev, const float* eps_dev,
                             int64_t batch, float* grad_prior_dev, float* grad_lik_dev, float* loss_out_dev,
                             float* target_out_dev, void* stream) {
  if (!widths || !prior_w || !prior_b || !lik_w || !lik_b || !fwd || !noise || !sde || !x_dev || !y_dev || !t_dev ||
      !eps_dev || !grad_prior_dev || !grad_lik_dev || !loss_out_dev)
    return fail(DMIP_ERR_INVALID, "null argument");
  if (xdim != dmip::kSurXdim || ydim != dmip::kSurYdim)
    return fail(DMIP_ERR_UNSUPPORTED, "PosteriorLoss: the scatterometry surrogate's shapes (xdim 3, ydim 23)");
  if (n_hidden < 1 || n_hidden > 8) return fail(DMIP_ERR_UNSUPPORTED, "n_hidden must be in [1, 8]");
  for (int i = 0; i < n_hidden; ++i)
    if (widths[i] < 1 || widths[i] > 4096) return fail(DMIP_ERR_INVALID, "hidden widths must be in [1, 4096]");
  for (int i = 0; i <= n_hidden; ++i)
    if (!prior_w[i] || !prior_b[i] || !lik_w[i] || !lik_b[i]) return fail(DMIP_ERR_INVALID, "null layer pointer");
  if (batch < 1) return fail(DMIP_ERR_INVALID, "batch must be >= 1");
  if (!(noise->b > 0.0f) || !(noise->a >= 0.0f)) return fail(DMIP_ERR_INVALID, "noise model needs b > 0, a >= 0");
  if (!(sde->beta_min > 0.0)) return fail(DMIP_ERR_INVALID, "beta_min must be > 0");
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = batch;
  MlpDims dp, dl;  // prior MLP2 (x, t) and likelihood MLP (x, y, t)
  dp.L = dl.L = n_hidden;
  for (int l = 0; l <= n_hidden; ++l) {
    const int in_w = l == 0 ? 0 : widths[l - 1], out_w = l == n_hidden ? xdim : widths[l];
    dp.in.push_back(l == 0 ? xdim + 1 : in_w);
    dl.in.push_back(l == 0 ? xdim + ydim + 1 : in_w);
    dp.out.push_back(out_w);
    dl.out.push_back(out_w);
  }
  int wmax = xdim + ydim + 2;
  for (int i = 0; i < n_hidden; ++i) wmax = std::max(wmax, widths[i] + 1);
  const int splits = 64;  // the cap of every weight-gradient GEMM's own split count (gemm_wgrad_splits)
  // scratch (one allocation, carved in 256-byte aligned pieces)
  std::vector<std::pair<float**, size_t>> plan;
  auto need = [&](float** p, size_t n) { plan.emplace_back(p, n); };
  MlpTape tp, tl;
  tp.h.assign(n_hidden + 1, nullptr);
  tl.h.assign(n_hidden + 1, nullptr);
  tp.d.assign(n_hidden, nullptr);
  tl.d.assign(n_hidden, nullptr);
  for (int l = 0; l <= n_hidden; ++l) {
    need(&tp.h[l], (size_t)B * (dp.in[l] + 1));
    need(&tl.h[l], (size_t)B * (dl.in[l] + 1));
  }
  for (int l = 0; l < n_hidden; ++l) {
    need(&tp.d[l], (size_t)B * widths[l]);
    need(&tl.d[l], (size_t)B * widths[l]);
  }
  float *sp = nullptr, *sl = nullptr, *alpha = nullptr, *stdv = nullptr, *xt = nullptr, *x0 = nullptr, *u = nullptr,
        *jtu = nullptr, *tgt = nullptr, *ap = nullptr, *al = nullptr, *rows = nullptr, *da = nullptr, *db = nullptr,
        *part = nullptr;
  need(&sp, (size_t)B * xdim);
  need(&sl, (size_t)B * xdim);
  need(&alpha, B);
  need(&stdv, B);
  need(&xt, (size_t)B * xdim);
  need(&x0, (size_t)B * xdim);
  need(&u, (size_t)B * xdim);
  need(&jtu, (size_t)B * (xdim + 1));
  need(&tgt, (size_t)B * xdim);
  need(&ap, (size_t)B * xdim);
  need(&al, (size_t)B * xdim);
  need(&rows, (size_t)B * 2);
  need(&da, (size_t)B * wmax);
  need(&db, (size_t)B * wmax);
  need(&part, (size_t)splits * (size_t)wmax * (size_t)wmax);
  size_t total = 0;
  for (auto& q : plan) total += (q.second * sizeof(float) + 255) / 256 * 256;
  char* scratch = nullptr;
  hipError_t e = hipMallocAsync((void**)&scratch, total, st);
  if (e != hipSuccess) return fail(DMIP_ERR_ALLOC, std::string("hipMallocAsync: ") + hipGetErrorString(e));
  {
    size_t o = 0;
    for (auto& q : plan) {
      *q.first = (float*)(scratch + o);
      o += (q.second * sizeof(float) + 255) / 256 * 256;
    }
  }
  tp.out = sp;
  tl.out = sl;
  dmip::PosteriorParams pp{};
  pp.batch = B;
  pp.xdim = xdim;
  pp.ydim = ydim;
  pp.bmin = (float)sde->beta_min;
  pp.bdiff = (float)(sde->beta_max - sde->beta_min);
  pp.lam = lam;
  pp.x = x_dev;
  pp.y = y_dev;
  pp.t = t_dev;
  pp.eps = eps_dev;
  pp.alpha = alpha;
  pp.stdv = stdv;
  pp.x_t = xt;
  pp.prior_in = tp.h[0];
  pp.lik_in = tl.h[0];
  pp.s_prior = sp;
  pp.s_lik = sl;
  pp.x0 = x0;
  pp.u = u;
  pp.jtu = jtu;
  pp.target = target_out_dev ? target_out_dev : tgt;
  pp.adj_prior = ap;
  pp.adj_lik = al;
  pp.rows = rows;
  pp.loss_out = loss_out_dev;
  dmip::SurrogateParams sq{};
  surrogate_params(fwd, sq);
  sq.a = noise->a;
  sq.b2 = (float)((double)noise->b * (double)noise->b);
  sq.x = x0;
  sq.y = y_dev;
  sq.y_stride = ydim;
  sq.n = B;
  sq.g_out = u;
  auto run = [&]() -> hipError_t {
    hipError_t r;
    for (int l = 1; l <= n_hidden; ++l) {
      if ((r = dmip::launch_ones_column(tp.h[l], B, dp.in[l] + 1, st)) != hipSuccess) return r;
      if ((r = dmip::launch_ones_column(tl.h[l], B, dl.in[l] + 1, st)) != hipSuccess) return r;
    }
    if ((r = dmip::launch_posterior_stage(pp, 0, st)) != hipSuccess) return r;  // x_t, network inputs
    if ((r = mlp_forward_f32(dp, prior_w, prior_b, tp, B, st)) != hipSuccess) return r;
    if ((r = mlp_forward_f32(dl, lik_w, lik_b, tl, B, st)) != hipSuccess) return r;
    if ((r = dmip::launch_posterior_stage(pp, 1, st)) != hipSuccess) return r;  // Tweedie x0
    if ((r = dmip::launch_surrogate_eval(sq, 3, surrogate_n_wg(B, st), st)) != hipSuccess) return r;  // u = J_F^T v
    // J_s^T u: the prior's reverse pass to its input, no parameter gradients
    if ((r = mlp_backward_f32(dp, prior_w, tp, u, B, da, db, nullptr, jtu, part, splits, st)) != hipSuccess) return r;
    if ((r = dmip::launch_posterior_stage(pp, 2, st)) != hipSuccess) return r;  // target, adjoints, rows
    if ((r = mlp_backward_f32(dp, prior_w, tp, ap, B, da, db, grad_prior_dev, nullptr, part, splits, st)) != hipSuccess)
      return r;
    if ((r = mlp_backward_f32(dl, lik_w, tl, al, B, da, db, grad_lik_dev, nullptr, part, splits, st)) != hipSuccess)
      return r;
    return dmip::launch_posterior_stage(pp, 3, st);  // loss reduction
  };
  e = run();
  (void)hipFreeAsync(scratch, st);
  if (e != hipSuccess) return hip_fail(e, "posterior_loss_grad launch");
  return DMIP_OK;
}

}  // extern "C"
