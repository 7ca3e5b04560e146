// libdmip.so C-ABI (include/dmip.h), handles and library state: dmip_mlp_create and dmip_surrogate_create (validate,
// pack on the host with dmip_pack.h, upload every image, publish the handle), the network forward, the error text and
// the device status words. The sampling entry points are in dmip_capi_sample.cpp, the probability-flow ones in
// dmip_capi_flow.cpp, linear guided sampling in dmip_capi_dps_linear.cpp, the training ones in dmip_capi_train.cpp.
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <tuple>

#include "dmip_capi_common.h"

using namespace dmip_capi;

namespace {

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

// one host image and the device buffer it goes to
struct Upload {
  DevMem* dst;
  const void* src;
  size_t bytes;
  template <typename T>
  Upload(DevMem& d, const std::vector<T>& v) : dst(&d), src(v.data()), bytes(v.size() * sizeof(T)) {}
};
#define UP(name) Upload(net->name, im.name)  // an image and the handle's buffer share one name

// uploads every non-empty image; an empty one leaves its buffer null (that engine is absent for this network)
int upload_all(std::initializer_list<Upload> ups) {
  for (const Upload& u : ups) {
    if (u.bytes == 0) continue;
    hipError_t e = hipMalloc(&u.dst->ptr, u.bytes);
    if (e != hipSuccess) return fail(DMIP_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    if ((e = hipMemcpy(u.dst->ptr, u.src, u.bytes, hipMemcpyHostToDevice)) != hipSuccess) return hip_fail(e, "hipMemcpy");
  }
  return DMIP_OK;
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

  const dmip_pack::MlpImages im = dmip_pack::pack_mlp({in_dim, out_dim, n_hidden, W, input_layout, xdim}, weights, biases);
  std::unique_ptr<dmip_mlp> net(new (std::nothrow) dmip_mlp);
  if (!net) return fail(DMIP_ERR_ALLOC, "host allocation");
  net->in_dim = in_dim;
  net->out_dim = out_dim;
  net->n_hidden = n_hidden;
  net->width = W;
  net->act_mode = act_mode;
  net->layout = input_layout;
  net->xdim = xdim;
  net->k1s_full = im.k1s_full;
  net->f32_k1q = im.f32_k1q;
  net->f32_ot = im.f32_ot;
  net->x3_range = im.x3_range;
  net->dps_x3_range = im.dps_x3_range;
  if (const int rc = upload_all(
          {UP(ring_l1), UP(hidden), UP(ao_samp), UP(ao_full), UP(bias_hidden), UP(bias_out_samp), UP(bias_out_full),
           UP(a1_full), UP(w1), UP(b1), UP(dps_l1), UP(dps_w2), UP(dps_w3), UP(dps_w4), UP(dps_bias), UP(dps_x3_img),
           UP(dps_x3_l1), UP(dps_x3_bias), UP(f32_l1), UP(f32_stream), UP(f32_bias), UP(x3_l1), UP(x3_l1_full),
           UP(x3_stream), UP(x3_stream_l1r), UP(x3_bias), UP(x3k_stream), UP(x3k_out), UP(x3p_stream), UP(x3p_l1),
           UP(x3p_ow)}))
    return rc;
  *out = net.release();
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
  const dmip_pack::SurrogateImages im = dmip_pack::pack_surrogate(weights, biases);
  std::unique_ptr<dmip_surrogate> net(new (std::nothrow) dmip_surrogate);
  if (!net) return fail(DMIP_ERR_ALLOC, "host allocation");
  net->x3_range = im.x3_range;
  if (const int rc = upload_all({UP(l1), UP(bias), UP(img[0]), UP(img[1]), UP(img[2]), UP(img[3]), UP(img[4]),
                                 UP(img[5]), UP(img[6]), UP(x3_img), UP(x3_l1), UP(x3_bias)}))
    return rc;
  *out = net.release();
  return DMIP_OK;
}

int dmip_surrogate_destroy(dmip_surrogate* s) {
  delete s;
  return DMIP_OK;
}

}  // extern "C"
