"""ctypes binding of libdmip.so (include/dmip.h).

The library is built in-tree (Makefile / __graft_entry__.build()) next to this file. It must be
loaded AFTER `import torch` so that it binds to the HIP runtime torch already loaded (both carry
SONAME libamdhip64.so.7; the dynamic loader then reuses torch's copy and device pointers and
streams are shared). There is no fallback: if the library is missing, every device entry point
raises.
"""
import collections
import ctypes
import os
import threading

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DMIP_LIB", os.path.join(_HERE, "libdmip.so"))

DMIP_OK, DMIP_ERR_INVALID, DMIP_ERR_UNSUPPORTED, DMIP_ERR_HIP, DMIP_ERR_ALLOC = range(5)
DMIP_INPUT_X_Y_T, DMIP_INPUT_X_T = 0, 1
DMIP_ACT_TANH_TWICE_FIRST, DMIP_ACT_TANH, DMIP_ACT_SILU_TWICE_FIRST = 0, 1, 2
DMIP_PREC_FP16, DMIP_PREC_F32, DMIP_PREC_F32X3 = 0, 1, 2
# DMIP_PREC_BF16 (include/dmip.h): the same value -- the config-5 training kernel's split-bf16 arithmetic, and the
# samplers' deprecated name of DMIP_PREC_FP16 (their 16-bit engine computes its hidden and output layers in fp16)
DMIP_PREC_BF16 = DMIP_PREC_FP16
PRECISIONS = {"fp16": DMIP_PREC_FP16, "bf16": DMIP_PREC_BF16, "fp32": DMIP_PREC_F32, "fp32x3": DMIP_PREC_F32X3}
DMIP_SAMPLER_CDE, DMIP_SAMPLER_POSTERIOR, DMIP_SAMPLER_CDIFFE = 0, 1, 2
ABI_VERSION = 9
DMIP_LOSS_DSM, DMIP_LOSS_DSM_PDE, DMIP_LOSS_PINN, DMIP_LOSS_PINN2 = 0, 1, 2, 3
DMIP_PDE_NONE, DMIP_PDE_FPE, DMIP_PDE_CFPE = 0, 1, 2
DMIP_METRIC_L1, DMIP_METRIC_L2 = 0, 1

# every symbol include/dmip.h declares (checked by tests/test_capi.py)
EXPORTED = (
    "dmip_mlp_create", "dmip_mlp_destroy", "dmip_mlp_forward", "dmip_em_sample", "dmip_rng_words",
    "dmip_rng_normals", "dmip_schedule", "dmip_last_error", "dmip_abi_version", "dmip_sampler_supported",
    "dmip_em_sample_stamps", "dmip_em_sample_posterior", "dmip_em_sample_cdiffe", "dmip_loss_grad",
    "dmip_loss_grad_supported", "dmip_histogram", "dmip_surrogate_create", "dmip_surrogate_destroy",
    "dmip_surrogate_forward", "dmip_log_posterior", "dmip_mh_sample", "dmip_dps_sample", "dmip_device_status",
    "dmip_sampler_supported_f32", "dmip_posterior_loss_grad", "dmip_loss_grad_f32", "dmip_train_draws",
    "dmip_adam_step", "dmip_em_sample_snapshots", "dmip_train_plan_create", "dmip_train_plan_step",
    "dmip_train_plan_set_counters", "dmip_train_plan_destroy", "dmip_sampler_supported_precision",
    "dmip_dps_sample_ex", "dmip_mh_sample_ex", "dmip_em_sample_lmbd", "dmip_flow_logp", "dmip_flow_logp_supported",
    "dmip_ode_sample", "dmip_ode_sample_supported", "dmip_flow_sample", "dmip_flow_sample_supported",
    "dmip_flow_logp_ex", "dmip_flow_sample_ex", "dmip_flow_logp_supported_precision",
    "dmip_flow_sample_supported_precision", "dmip_mala_sample", "dmip_dps_linear_supported", "dmip_dps_linear_sample",
    "dmip_multistep_sample", "dmip_multistep_supported", "dmip_flow_pairs_supported", "dmip_flow_logp_pairs",
    "dmip_flow_sample_pairs", "dmip_multistep_sde_sample", "dmip_multistep_sde_supported",
    "dmip_dps_tweedie_supported", "dmip_dps_tweedie_sample",
)
DMIP_SOLVER_EULER, DMIP_SOLVER_HEUN = 0, 1
SOLVERS = {"euler": DMIP_SOLVER_EULER, "heun": DMIP_SOLVER_HEUN}
# the table-driven few-step samplers of the probability-flow ODE (dmip_multistep_sample): Python-side names, not values
# of dmip_solver. A row of their step table: tau | p q | cx c0 c1 | g | cn (include/dmip.h; cn, the noise coefficient,
# is read by dmip_multistep_sde_sample alone)
TABLE_SOLVERS = ("dpm2m", "ddim")
DMIP_MULTISTEP_COLS = 8
DMIP_DPS_NLL, DMIP_DPS_NORM = 0, 1
DMIP_DPS_STEP_BETA, DMIP_DPS_STEP_NORM = 0, 1


class DmipVpsde(ctypes.Structure):
    _fields_ = [("beta_min", ctypes.c_double), ("beta_max", ctypes.c_double), ("T", ctypes.c_double)]


class DmipLossCfg(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("pde", ctypes.c_int), ("pde_metric", ctypes.c_int),
                ("ic_metric", ctypes.c_int), ("lam", ctypes.c_float), ("lam2", ctypes.c_float),
                ("ic_A", ctypes.c_float * 4), ("ic_b", ctypes.c_float * 2), ("ic_Sinv", ctypes.c_float * 4)]


class DmipTrainPlanDesc(ctypes.Structure):
    """dmip_train_plan_desc (include/dmip.h)."""
    _fields_ = [("in_dim", ctypes.c_int), ("out_dim", ctypes.c_int), ("n_hidden", ctypes.c_int),
                ("widths", ctypes.c_void_p), ("xdim", ctypes.c_int), ("weights_dev", ctypes.c_void_p),
                ("biases_dev", ctypes.c_void_p), ("sde", DmipVpsde), ("cfg", DmipLossCfg),
                ("precision", ctypes.c_int), ("batch", ctypes.c_int64), ("seed", ctypes.c_uint64),
                ("first_draw", ctypes.c_uint64), ("debias", ctypes.c_int), ("t_epsilon", ctypes.c_double),
                ("t_add", ctypes.c_float), ("n_tensors", ctypes.c_int), ("params", ctypes.c_void_p),
                ("grads", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("numel", ctypes.c_void_p), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("step0", ctypes.c_int64),
                ("t_dev", ctypes.c_void_p), ("eps_dev", ctypes.c_void_p), ("loss_dev", ctypes.c_void_p)]


class DmipScatNoise(ctypes.Structure):
    _fields_ = [("a", ctypes.c_float), ("b", ctypes.c_float), ("lambd_bd", ctypes.c_float)]


_c_void_p = ctypes.c_void_p
_i32, _i64, _u64t = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
_f32 = ctypes.c_float

_lib = None
_lock = threading.Lock()
calls = collections.Counter()  # instrumentation: proves the HIP path ran (calls of each wrapper below)


def _declare(lib):
    lib.dmip_last_error.restype = ctypes.c_char_p
    lib.dmip_sampler_supported.argtypes = [_i32, _i32, _i32, _i32, _i32]
    lib.dmip_sampler_supported_f32.argtypes = [_i32, _i32, _i32, _i32, _i32]
    lib.dmip_sampler_supported_precision.argtypes = [_i32, _i32, _i32, _i32, _i32, _i32]  # ABI >= 6 (EXPORTED)
    lib.dmip_device_status.argtypes = [_c_void_p]
    lib.dmip_train_draws.argtypes = [_u64t, _u64t, _i64, _i32, _i32, ctypes.POINTER(DmipVpsde), ctypes.c_double, _f32,
                                     _c_void_p, _c_void_p, _c_void_p]
    lib.dmip_adam_step.argtypes = [_i32, ctypes.POINTER(_c_void_p), ctypes.POINTER(_c_void_p), ctypes.POINTER(_c_void_p),
                                   ctypes.POINTER(_c_void_p), ctypes.POINTER(_i64), ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, ctypes.c_double, _i64, _c_void_p]
    lib.dmip_loss_grad_f32.argtypes = [_i32, _i32, _i32, ctypes.POINTER(_i32), _i32, ctypes.POINTER(_c_void_p),
                                       ctypes.POINTER(_c_void_p), ctypes.POINTER(DmipVpsde), ctypes.POINTER(DmipLossCfg),
                                       _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p,
                                       _c_void_p, _c_void_p]
    _pp = ctypes.POINTER(_c_void_p)
    lib.dmip_posterior_loss_grad.argtypes = [_i32, _i32, _i32, ctypes.POINTER(_i32), _pp, _pp, _pp, _pp, _c_void_p,
                                             ctypes.POINTER(DmipScatNoise), _f32, ctypes.POINTER(DmipVpsde),
                                             _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p,
                                             _c_void_p, _c_void_p, _c_void_p]
    lib.dmip_mlp_create.argtypes = [_i32, _i32, _i32, ctypes.POINTER(_i32), _i32, _i32, _i32,
                                    ctypes.POINTER(_c_void_p), ctypes.POINTER(_c_void_p),
                                    ctypes.POINTER(_c_void_p)]
    lib.dmip_mlp_destroy.argtypes = [_c_void_p]
    lib.dmip_mlp_forward.argtypes = [_c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _i32, _i64,
                                     _c_void_p, _i32, _c_void_p]
    lib.dmip_em_sample.argtypes = [_c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32, _i32, _i32,
                                   _i64, _i64, _i32, _f32, _f32, _u64t, _i32, _c_void_p, _c_void_p,
                                   _c_void_p]
    lib.dmip_em_sample_posterior.argtypes = [_c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32,
                                             _i32, _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _i32, _c_void_p,
                                             _c_void_p]
    lib.dmip_em_sample_cdiffe.argtypes = [_c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32, _i32, _i32,
                                          _i64, _i64, _i32, _f32, _f32, _u64t, _i32, _i32, _f32, _c_void_p,
                                          _c_void_p]
    if hasattr(lib, "dmip_em_sample_snapshots"):  # (absent from older builds loaded by A/B timing scripts)
        lib.dmip_em_sample_snapshots.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32,
                                                 _i32, _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _i32, _i32, _f32,
                                                 _i32, _c_void_p, _c_void_p, _c_void_p]
    if hasattr(lib, "dmip_em_sample_lmbd"):  # (absent from older builds loaded by A/B timing scripts)
        lib.dmip_em_sample_lmbd.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32, _i32,
                                            _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _i32, ctypes.c_double, _c_void_p,
                                            _i32, _c_void_p, _c_void_p, _c_void_p]
        lib.dmip_flow_logp.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _c_void_p, _i32,
                                       _i32, _i32, _i64, _i32, _c_void_p, _c_void_p, _c_void_p]
        lib.dmip_flow_logp_supported.argtypes = [_i32, _i32, _i32, _i32, _i32]
    if hasattr(lib, "dmip_ode_sample"):  # (absent from older builds loaded by A/B timing scripts)
        lib.dmip_ode_sample.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32, _i32,
                                        _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _i32, _i32, _c_void_p, _i32,
                                        _c_void_p, _c_void_p, _c_void_p]
        lib.dmip_ode_sample_supported.argtypes = [_i32] * 7
    if hasattr(lib, "dmip_flow_sample"):  # (absent from older builds loaded by A/B timing scripts)
        lib.dmip_flow_sample.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32, _i32,
                                         _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _c_void_p, _c_void_p, _c_void_p,
                                         _c_void_p]
        lib.dmip_flow_sample_supported.argtypes = [_i32, _i32, _i32, _i32, _i32]
    if hasattr(lib, "dmip_flow_logp_ex"):  # (absent from older builds loaded by A/B timing scripts)
        lib.dmip_flow_logp_ex.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _c_void_p,
                                          _i32, _i32, _i32, _i64, _i32, _c_void_p, _c_void_p, _i32, _c_void_p]
        lib.dmip_flow_sample_ex.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32,
                                            _i32, _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _c_void_p, _c_void_p,
                                            _c_void_p, _i32, _c_void_p]
        lib.dmip_flow_logp_supported_precision.argtypes = [_i32] * 6
        lib.dmip_flow_sample_supported_precision.argtypes = [_i32] * 6
    if hasattr(lib, "dmip_flow_logp_pairs"):  # (absent from older builds loaded by A/B timing scripts)
        lib.dmip_flow_pairs_supported.argtypes = [_i32] * 6
        lib.dmip_flow_logp_pairs.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _c_void_p,
                                             _i32, _i32, _i64, _i32, _c_void_p, _c_void_p, _i32, _c_void_p]
        lib.dmip_flow_sample_pairs.argtypes = [_i32, _c_void_p, _c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32,
                                               _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _c_void_p, _c_void_p,
                                               _c_void_p, _i32, _c_void_p]
    if hasattr(lib, "dmip_train_plan_create"):
        lib.dmip_train_plan_create.argtypes = [ctypes.POINTER(DmipTrainPlanDesc), ctypes.POINTER(_c_void_p)]
        lib.dmip_train_plan_step.argtypes = [_c_void_p, _c_void_p, _c_void_p, _c_void_p]
        lib.dmip_train_plan_set_counters.argtypes = [_c_void_p, _u64t, _i64, _c_void_p]
        lib.dmip_train_plan_destroy.argtypes = [_c_void_p]
    lib.dmip_loss_grad.argtypes = [_i32, _i32, _i32, ctypes.POINTER(_i32), _i32, ctypes.POINTER(_c_void_p),
                                   ctypes.POINTER(_c_void_p), ctypes.POINTER(DmipVpsde), ctypes.POINTER(DmipLossCfg),
                                   _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p,
                                   _c_void_p]
    lib.dmip_histogram.argtypes = [_c_void_p, _i64, _i32, _i32, ctypes.c_double, ctypes.c_double, _i32, _c_void_p,
                                   _c_void_p]
    lib.dmip_loss_grad_supported.argtypes = [_i32, _i32, _i32, ctypes.POINTER(_i32), _i32]
    lib.dmip_em_sample_stamps.argtypes = [_c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _i32, _i32, _i32,
                                          _i64, _i32, _u64t, _c_void_p, _c_void_p, _c_void_p]
    lib.dmip_rng_words.argtypes = [_u64t, _i64, _u64t, _i64, _i32, _c_void_p, _c_void_p]
    lib.dmip_rng_normals.argtypes = [_u64t, _i64, _u64t, _i64, _i32, _c_void_p, _c_void_p]
    lib.dmip_schedule.argtypes = [_i32, ctypes.POINTER(DmipVpsde), _c_void_p, _c_void_p]
    lib.dmip_surrogate_create.argtypes = [_i32, _i32, _i32, ctypes.POINTER(_i32), ctypes.POINTER(_c_void_p),
                                          ctypes.POINTER(_c_void_p), ctypes.POINTER(_c_void_p)]
    lib.dmip_surrogate_destroy.argtypes = [_c_void_p]
    lib.dmip_surrogate_forward.argtypes = [_c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p]
    lib.dmip_log_posterior.argtypes = [_c_void_p, ctypes.POINTER(DmipScatNoise), _c_void_p, _c_void_p, _i64, _i64,
                                       _c_void_p, _c_void_p, _c_void_p]
    lib.dmip_mh_sample.argtypes = [_c_void_p, ctypes.POINTER(DmipScatNoise), _c_void_p, _i32, _i64, _i64, _i32, _f32,
                                   _u64t, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]
    lib.dmip_dps_sample.argtypes = [_c_void_p, _c_void_p, ctypes.POINTER(DmipScatNoise), ctypes.POINTER(DmipVpsde),
                                    _c_void_p, _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _i32, _f32, _c_void_p,
                                    _c_void_p]
    lib.dmip_dps_sample_ex.argtypes = [_c_void_p, _c_void_p, ctypes.POINTER(DmipScatNoise), ctypes.POINTER(DmipVpsde),
                                       _c_void_p, _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _i32, _f32, _i32,
                                       _c_void_p, _c_void_p]
    if hasattr(lib, "dmip_mh_sample_ex"):  # ABI >= 9
        lib.dmip_mh_sample_ex.argtypes = [_c_void_p, ctypes.POINTER(DmipScatNoise), _c_void_p, _i32, _i64, _i64, _i32,
                                          _f32, _u64t, _c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p,
                                          _c_void_p]
    if hasattr(lib, "dmip_mala_sample"):  # additive within ABI 9
        lib.dmip_mala_sample.argtypes = [_c_void_p, ctypes.POINTER(DmipScatNoise), _c_void_p, _i32, _i64, _i64, _i32,
                                         _i32, ctypes.c_double, ctypes.c_double, _u64t, _c_void_p, _c_void_p,
                                         _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]
    if hasattr(lib, "dmip_dps_linear_sample"):  # additive within ABI 9
        lib.dmip_dps_linear_supported.argtypes = [_i32] * 5
        lib.dmip_dps_linear_sample.argtypes = [_c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _c_void_p, _i32,
                                               _c_void_p, _i32, _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _i32, _f32,
                                               _i32, _c_void_p, _c_void_p]
    if hasattr(lib, "dmip_multistep_sample"):  # additive within ABI 9
        lib.dmip_multistep_supported.argtypes = [_i32] * 6
        lib.dmip_multistep_sample.argtypes = [_i32, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _i64, _i64, _i32,
                                              _c_void_p, _i32, _f32, _f32, _u64t, _i32, _c_void_p, _i32, _c_void_p,
                                              _c_void_p, _c_void_p]
    if hasattr(lib, "dmip_multistep_sde_sample"):  # additive within ABI 9
        lib.dmip_multistep_sde_supported.argtypes = [_i32] * 6
        lib.dmip_multistep_sde_sample.argtypes = [_i32, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _i64, _i64,
                                                  _i32, _c_void_p, _i32, _f32, _f32, _u64t, _i32, _c_void_p, _i32,
                                                  _c_void_p, _c_void_p, _c_void_p]
    if hasattr(lib, "dmip_dps_tweedie_sample"):  # additive within ABI 9
        lib.dmip_dps_tweedie_supported.argtypes = [_i32] * 5
        lib.dmip_dps_tweedie_sample.argtypes = [_c_void_p, ctypes.POINTER(DmipVpsde), _c_void_p, _c_void_p, _c_void_p,
                                                _c_void_p, _i32, _i32, _i64, _i64, _i32, _f32, _f32, _u64t, _f32, _i32,
                                                _c_void_p, _c_void_p]
    for name in EXPORTED:  # every entry point returns int but dmip_last_error
        if name != "dmip_last_error" and hasattr(lib, name):
            getattr(lib, name).restype = _i32


class _OlderBuild:
    """An older build of the library loaded for a same-box timing A/B (DMIP_LIB=<path> DMIP_LIB_AB=1, scripts/): the
    entry points it lacks take their ctypes declarations and fail when called. Never the product path."""

    def __init__(self, handle):
        self._handle, self._absent = handle, {}

    def __getattr__(self, name):
        try:
            return getattr(self._handle, name)
        except AttributeError:
            return self._absent.setdefault(name, _Absent(name))


class _Absent:
    def __init__(self, name):
        self.name = name

    def __call__(self, *args):
        raise RuntimeError(f"dmip: {LIB_PATH} (A/B build) has no {self.name}")


def lib():
    """The loaded library; raises RuntimeError if it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"dmip: HIP library not found at {LIB_PATH}; build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` or `make` at the repo root")
                handle = ctypes.CDLL(LIB_PATH)
                missing = [n for n in EXPORTED if not hasattr(handle, n)]
                ab = os.environ.get("DMIP_LIB_AB") == "1"
                if missing and ab:
                    handle = _OlderBuild(handle)
                elif missing:
                    raise RuntimeError(f"dmip: {LIB_PATH} is not ABI {ABI_VERSION}: missing {', '.join(missing)} "
                                       "(rebuild with `make` at the repo root)")
                elif not ab and handle.dmip_abi_version() != ABI_VERSION:
                    raise RuntimeError(f"dmip: {LIB_PATH} is ABI {handle.dmip_abi_version()}, this package needs "
                                       f"{ABI_VERSION} (rebuild with `make` at the repo root)")
                _declare(handle)
                _lib = handle
    return _lib


def check(rc):
    if rc == DMIP_OK:
        return
    msg = lib().dmip_last_error().decode(errors="replace")
    if rc in (DMIP_ERR_INVALID, DMIP_ERR_UNSUPPORTED):
        raise ValueError(f"dmip: {msg}")
    raise RuntimeError(f"dmip: {msg} (status {rc})")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _u64(v):
    return ctypes.c_uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


def _h(handle):
    """The dmip_mlp* of an optional MlpHandle (the Posterior prior; None elsewhere)."""
    return handle.h if handle is not None else None


def stream_of(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_device(t, what="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"dmip: {what} must be on a HIP device (got {getattr(t, 'device', type(t))});"
                           " the dmip kernels have no CPU path")


def vpsde(beta_min, beta_max, T):
    return DmipVpsde(float(beta_min), float(beta_max), float(T))


class MlpHandle:
    """Owns a dmip_mlp* (packed device weights) for one snapshot of a network's parameters."""

    def __init__(self, layers, in_dim, out_dim, xdim, input_layout, device, act=DMIP_ACT_TANH_TWICE_FIRST):
        L = len(layers) - 1
        widths = (_i32 * L)(*[int(layers[i][0].shape[0]) for i in range(L)])
        with torch.cuda.device(device):
            ws = [w.detach().float().contiguous().cpu() for w, _ in layers]
            bs = [b.detach().float().contiguous().cpu() for _, b in layers]
            wp = (_c_void_p * (L + 1))(*[w.data_ptr() for w in ws])
            bp = (_c_void_p * (L + 1))(*[b.data_ptr() for b in bs])
            out = _c_void_p()
            check(lib().dmip_mlp_create(in_dim, out_dim, L, widths, act, input_layout, xdim, wp, bp,
                                        ctypes.byref(out)))
        self.h = out
        self.device = device
        self.width = int(layers[0][0].shape[0])
        self.n_hidden = L
        self.in_dim, self.out_dim, self.xdim = in_dim, out_dim, xdim
        self.act = act

    def __del__(self):
        h = getattr(self, "h", None)
        if h and _lib is not None:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            _lib.dmip_mlp_destroy(h)
            self.h = None


def precision_code(precision):
    """'fp16' (16-bit MFMA operands, the fastest mode: split-bf16 layer 1, fp16 hidden and output layers; 'bf16' is
    its deprecated name), 'fp32x3' (fp32-accurate products as three fp16 MFMAs, the reference-precision throughput
    mode) or 'fp32' (exact f32 MFMA, bit-level parity mode)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
    return PRECISIONS[precision]


def mlp_forward(handle, x, y, t, out, y_stride, t_stride, precision="fp32"):
    calls["mlp_forward"] += 1
    check(lib().dmip_mlp_forward(handle.h, ptr(x), ptr(y), y_stride, ptr(t), t_stride, x.shape[0],
                                 ptr(out), precision_code(precision), stream_of(x.device)))


def em_sample(handle, sde, y, n_chains, chain_offset, num_steps, mean, std, seed, out, noise=None,
              precision="fp16"):
    calls["em_sample"] += 1
    _status_pending.add(_dev_index(y.device))
    n_y, ydim = y.shape
    check(lib().dmip_em_sample(handle.h, ctypes.byref(sde), ptr(y), n_y, ydim, handle.xdim,
                               int(n_chains), int(chain_offset), int(num_steps), float(mean), float(std), _u64(seed),
                               precision_code(precision), ptr(noise), ptr(out), stream_of(y.device)))


def em_sample_posterior(prior, likelihood, sde, y, n_chains, chain_offset, num_steps, mean, std, seed, out,
                        precision="fp16"):
    calls["em_sample_posterior"] += 1
    _status_pending.add(_dev_index(y.device))
    n_y, ydim = y.shape
    check(lib().dmip_em_sample_posterior(prior.h, likelihood.h, ctypes.byref(sde), ptr(y), n_y, ydim,
                                         likelihood.xdim, int(n_chains), int(chain_offset), int(num_steps),
                                         float(mean), float(std), _u64(seed), precision_code(precision), ptr(out),
                                         stream_of(y.device)))


def em_sample_cdiffe(handle, sde, y, n_chains, chain_offset, num_steps, mean, std, seed, out, corrector_steps=0,
                     snr=0.16, precision="fp16"):
    calls["em_sample_cdiffe"] += 1
    _status_pending.add(_dev_index(y.device))
    n_y, ydim = y.shape
    check(lib().dmip_em_sample_cdiffe(handle.h, ctypes.byref(sde), ptr(y), n_y, ydim, handle.xdim,
                                      int(n_chains), int(chain_offset), int(num_steps), float(mean), float(std),
                                      _u64(seed), precision_code(precision), int(corrector_steps), float(snr),
                                      ptr(out), stream_of(y.device)))


def em_sample_snapshots(mode, net, prior, sde, y, n_chains, chain_offset, num_steps, mean, std, seed, snapshot_every,
                        snaps, out, corrector_steps=0, snr=0.16, precision="fp16"):
    """dmip_em_sample_snapshots: the fused sampler of `mode` that also writes x after every
    snapshot_every-th step into snaps [num_steps // snapshot_every][n_y][n_chains][xdim]."""
    calls["em_sample_snapshots"] += 1
    _status_pending.add(_dev_index(y.device))
    n_y, ydim = y.shape
    check(lib().dmip_em_sample_snapshots(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(y), n_y, ydim, net.xdim,
                                         int(n_chains), int(chain_offset), int(num_steps), float(mean), float(std),
                                         _u64(seed), precision_code(precision), int(corrector_steps), float(snr),
                                         int(snapshot_every), ptr(snaps), ptr(out), stream_of(y.device)))


def em_sample_lmbd(mode, net, prior, sde, y, n_chains, chain_offset, num_steps, mean, std, seed, lmbd, out, noise=None,
                   snapshot_every=0, snaps=None, precision="fp16"):
    """dmip_em_sample_lmbd: the fused CDE / Posterior sampler of the lambda family (sdes.py:77-87; lmbd = 1 the
    probability-flow ODE), optionally with trajectory snapshots."""
    calls["em_sample_lmbd"] += 1
    _status_pending.add(_dev_index(y.device))
    n_y, ydim = y.shape
    check(lib().dmip_em_sample_lmbd(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(y), n_y, ydim, net.xdim,
                                    int(n_chains), int(chain_offset), int(num_steps), float(mean), float(std),
                                    _u64(seed), precision_code(precision), float(lmbd), ptr(noise),
                                    int(snapshot_every), ptr(snaps), ptr(out), stream_of(y.device)))


def solver_code(solver):
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {sorted(SOLVERS)}, got {solver!r}")
    return SOLVERS[solver]


def ode_sample_supported(width, n_hidden, xdim, ydim=0, mode=DMIP_SAMPLER_CDE, precision="fp32x3", solver="heun"):
    return bool(lib().dmip_ode_sample_supported(mode, width, n_hidden, xdim, ydim, precision_code(precision),
                                                solver_code(solver)))


def ode_sample(mode, net, prior, sde, y, n_chains, chain_offset, num_steps, mean, std, seed, out, solver="heun",
               x0=None, snapshot_every=0, snaps=None, precision="fp32x3"):
    """dmip_ode_sample: the fused CDE / Posterior sampler of the probability-flow ODE; "heun" is the second-order
    solver (x0 (n_y, n_chains, xdim) replaces the chain's own start state), "euler" dmip_em_sample_lmbd at lmbd = 1."""
    calls["ode_sample"] += 1
    _status_pending.add(_dev_index(y.device))
    n_y, ydim = y.shape
    check(lib().dmip_ode_sample(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(y), n_y, ydim, net.xdim,
                                int(n_chains), int(chain_offset), int(num_steps), float(mean), float(std), _u64(seed),
                                precision_code(precision), solver_code(solver), ptr(x0), int(snapshot_every),
                                ptr(snaps), ptr(out), stream_of(y.device)))


def multistep_supported(width, n_hidden, xdim, ydim=0, mode=DMIP_SAMPLER_CDE, precision="fp32x3"):
    return bool(lib().dmip_multistep_supported(mode, width, n_hidden, xdim, ydim, precision_code(precision)))


def _multistep(name, mode, net, prior, y, n_chains, chain_offset, num_steps, table, mean, std, seed, out, x0,
               snapshot_every, snaps, precision):
    """The body of multistep_sample and multistep_sde_sample: `name` is the wrapper's (its `calls` key, the name in its
    message and, behind dmip_, its entry point)."""
    if tuple(table.shape) != (int(num_steps), DMIP_MULTISTEP_COLS) or table.dtype != torch.float32 or \
            not table.is_contiguous() or table.device != y.device:
        raise ValueError(f"{name}: table must be a contiguous f32 (num_steps, DMIP_MULTISTEP_COLS) tensor on y's "
                         "device")
    calls[name] += 1
    _status_pending.add(_dev_index(y.device))
    n_y, ydim = y.shape
    check(getattr(lib(), "dmip_" + name)(int(mode), net.h, _h(prior), ptr(y), n_y, ydim, net.xdim, int(n_chains),
                                         int(chain_offset), int(num_steps), ptr(table), int(table.shape[1]),
                                         float(mean), float(std), _u64(seed), precision_code(precision), ptr(x0),
                                         int(snapshot_every), ptr(snaps), ptr(out), stream_of(y.device)))


def multistep_sample(mode, net, prior, y, n_chains, chain_offset, num_steps, table, mean, std, seed, out, x0=None,
                     snapshot_every=0, snaps=None, precision="fp32x3"):
    """dmip_multistep_sample: the fused CDE / Posterior few-step sampler of the probability-flow ODE (DPM-Solver++(2M),
    DDIM) from `table`, a contiguous f32 device tensor (num_steps, DMIP_MULTISTEP_COLS) (estimators.multistep_table);
    x0 (n_y, n_chains, xdim) replaces the chain's own start state."""
    _multistep("multistep_sample", mode, net, prior, y, n_chains, chain_offset, num_steps, table, mean, std, seed, out,
               x0, snapshot_every, snaps, precision)


def multistep_sde_supported(width, n_hidden, xdim, ydim=0, mode=DMIP_SAMPLER_CDE, precision="fp32x3"):
    return bool(lib().dmip_multistep_sde_supported(mode, width, n_hidden, xdim, ydim, precision_code(precision)))


def multistep_sde_sample(mode, net, prior, y, n_chains, chain_offset, num_steps, table, mean, std, seed, out, x0=None,
                         snapshot_every=0, snaps=None, precision="fp32x3"):
    """dmip_multistep_sde_sample: the fused stochastic few-step sampler (SDE-DPM-Solver++(2M), ancestral / eta-DDIM)
    from `table` as multistep_sample, whose column 7 is the noise coefficient (estimators.multistep_table(eta=)). A
    chain draws the Euler sampler's normals: x0's first (consumed also when `x0` replaces the start state), then one
    set after each step's network evaluation."""
    _multistep("multistep_sde_sample", mode, net, prior, y, n_chains, chain_offset, num_steps, table, mean, std, seed,
               out, x0, snapshot_every, snaps, precision)


def flow_logp_supported(width, n_hidden, xdim, ydim=0, mode=DMIP_SAMPLER_CDE, precision="fp32"):
    """Whether dmip_flow_logp[_ex] has a kernel: "fp32" the exact-f32 engine, "fp32x3" (and "fp16" / "bf16", which
    run it) the split engine."""
    if precision == "fp32":
        return bool(lib().dmip_flow_logp_supported(mode, width, n_hidden, xdim, ydim))
    return bool(lib().dmip_flow_logp_supported_precision(precision_code(precision), mode, width, n_hidden, xdim, ydim))


def flow_logp(mode, net, prior, sde, x, y, num_steps, logp, latent=None, precision="fp32"):
    """dmip_flow_logp: log p(x | y) of x (n_y, n, xdim) under ys (n_y, ydim) into logp (n_y, n) [and x_S into latent].
    precision "fp32" is that entry point; any other goes through dmip_flow_logp_ex (the fp32x3 kernels)."""
    code = precision_code(precision)
    calls["flow_logp"] += 1
    _status_pending.add(_dev_index(y.device))  # (parallel.guarded then reads the status word after the launch)
    n_y, ydim = y.shape
    if code == DMIP_PREC_F32:
        check(lib().dmip_flow_logp(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(x), ptr(y), n_y, ydim, net.xdim,
                                   int(x.shape[1]), int(num_steps), ptr(logp), ptr(latent), stream_of(y.device)))
        return
    check(lib().dmip_flow_logp_ex(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(x), ptr(y), n_y, ydim, net.xdim,
                                  int(x.shape[1]), int(num_steps), ptr(logp), ptr(latent), code, stream_of(y.device)))


def flow_sample_supported(width, n_hidden, xdim, ydim=0, mode=DMIP_SAMPLER_CDE, precision="fp32"):
    """flow_logp_supported's answer for dmip_flow_sample[_ex]."""
    if precision == "fp32":
        return bool(lib().dmip_flow_sample_supported(mode, width, n_hidden, xdim, ydim))
    return bool(lib().dmip_flow_sample_supported_precision(precision_code(precision), mode, width, n_hidden, xdim,
                                                           ydim))


def flow_sample(mode, net, prior, sde, y, n_chains, chain_offset, num_steps, mean, std, seed, out, logq, x0=None,
                precision="fp32"):
    """dmip_flow_sample: Heun samples of the probability-flow ODE into out (n_y, n_chains, xdim) with their
    log-density into logq (n_y, n_chains); x0 (n_y, n_chains, xdim) replaces the chains' own start states. precision
    "fp32" is that entry point (exact f32); any other goes through dmip_flow_sample_ex (the fp32x3 kernels)."""
    code = precision_code(precision)
    calls["flow_sample"] += 1
    _status_pending.add(_dev_index(y.device))  # (parallel.guarded then reads the status word after the launch)
    n_y, ydim = y.shape
    if code == DMIP_PREC_F32:
        check(lib().dmip_flow_sample(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(y), n_y, ydim, net.xdim,
                                     int(n_chains), int(chain_offset), int(num_steps), float(mean), float(std),
                                     _u64(seed), ptr(x0), ptr(out), ptr(logq), stream_of(y.device)))
        return
    check(lib().dmip_flow_sample_ex(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(y), n_y, ydim, net.xdim,
                                    int(n_chains), int(chain_offset), int(num_steps), float(mean), float(std),
                                    _u64(seed), ptr(x0), ptr(out), ptr(logq), code, stream_of(y.device)))


def flow_pairs_supported(width, n_hidden, xdim, ydim=0, mode=DMIP_SAMPLER_CDE, precision="fp32"):
    """flow_logp_supported's answer for the paired entry points (dmip_flow_logp_pairs, dmip_flow_sample_pairs)."""
    return bool(lib().dmip_flow_pairs_supported(precision_code(precision), mode, width, n_hidden, xdim, ydim))


def flow_logp_pairs(mode, net, prior, sde, x, y, num_steps, logp, latent=None, precision="fp32"):
    """dmip_flow_logp_pairs: log p(x_i | y_i) of x (n, xdim) under y (n, ydim), one observation per row, into logp
    (n,) [and x_S into latent (n, xdim)]."""
    calls["flow_logp_pairs"] += 1
    _status_pending.add(_dev_index(y.device))  # (parallel.guarded then reads the status word after the launch)
    n, ydim = y.shape
    check(lib().dmip_flow_logp_pairs(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(x), ptr(y), ydim, net.xdim,
                                     int(n), int(num_steps), ptr(logp), ptr(latent), precision_code(precision),
                                     stream_of(y.device)))


def flow_sample_pairs(mode, net, prior, sde, y, chain_offset, num_steps, mean, std, seed, out, logq, x0=None,
                      precision="fp32"):
    """dmip_flow_sample_pairs: one Heun sample of the probability-flow ODE per row of y (n, ydim) into out (n, xdim)
    with its log-density into logq (n,); x0 (n, xdim) replaces the rows' own start states."""
    calls["flow_sample_pairs"] += 1
    _status_pending.add(_dev_index(y.device))  # (parallel.guarded then reads the status word after the launch)
    n, ydim = y.shape
    check(lib().dmip_flow_sample_pairs(int(mode), net.h, _h(prior), ctypes.byref(sde), ptr(y), ydim, net.xdim, int(n),
                                       int(chain_offset), int(num_steps), float(mean), float(std), _u64(seed), ptr(x0),
                                       ptr(out), ptr(logq), precision_code(precision), stream_of(y.device)))


def sampler_supported(width, n_hidden, xdim, ydim=0, mode=DMIP_SAMPLER_CDE, precision="fp16"):
    return bool(lib().dmip_sampler_supported_precision(precision_code(precision), mode, width, n_hidden, xdim, ydim))


# devices with a launch of a status-writing kernel (the samplers, MH, DPS) whose status word has not been read since;
# clear_range_status skips the read (a stream synchronise and a copy) when there is none
_status_pending = set()


def _dev_index(device):
    d = torch.device(device)
    return d.index if d.index is not None else torch.cuda.current_device()


def device_status(device):
    """Synchronise the device's current stream and raise if a kernel reported an asynchronous failure
    (dmip_device_status: the balanced sampler's hand-over timeout, or an fp32x3 chain outside the fp16 range).
    Reading clears the status word."""
    try:
        check(lib().dmip_device_status(stream_of(device)))
    finally:
        _status_pending.discard(_dev_index(device))


def is_range_error(e):
    """The fp32x3 split's fp16-range refusal (pack time, ValueError) or report (device status, RuntimeError)."""
    return isinstance(e, (ValueError, RuntimeError)) and "fp16 range" in str(e)


def clear_range_status(device):
    """Read and clear the device status word before a launch whose range report will be read: a stale fp16-range
    report of an earlier launch (whose caller did not read it) is dropped; any other stale failure raises. Nothing to
    read (no status-writing launch of this process since the last read): returns at once."""
    if _dev_index(device) not in _status_pending:
        return
    try:
        device_status(device)
    except RuntimeError as e:
        if not is_range_error(e):
            raise


def rng_normals(seed, chain_offset, stream_id, n_chains, n_pairs, out):
    """(n_chains, 2 n_pairs) standard normals of the kernels' chain-keyed generator (dmip_rng_normals)."""
    check(lib().dmip_rng_normals(_u64(seed), int(chain_offset), _u64(stream_id), int(n_chains), int(n_pairs), ptr(out),
                                 stream_of(out.device)))


def loss_grad_supported(in_dim, out_dim, widths, xdim):
    w = (_i32 * len(widths))(*widths)
    return bool(lib().dmip_loss_grad_supported(in_dim, out_dim, len(widths), w, xdim))


def loss_grad(layers, in_dim, out_dim, xdim, sde, cfg, x, y, t, eps, grad_out, loss_out):
    """layers: [(weight, bias), ...] device fp32 tensors (the torch parameters)."""
    calls["loss_grad"] += 1
    L = len(layers) - 1
    widths = (_i32 * L)(*[int(layers[i][0].shape[0]) for i in range(L)])
    wp = (_c_void_p * (L + 1))(*[w.data_ptr() for w, _ in layers])
    bp = (_c_void_p * (L + 1))(*[b.data_ptr() for _, b in layers])
    check(lib().dmip_loss_grad(in_dim, out_dim, L, widths, xdim, wp, bp, ctypes.byref(sde), ctypes.byref(cfg),
                               ptr(x), ptr(y), ptr(t), ptr(eps), int(x.shape[0]), ptr(grad_out), ptr(loss_out),
                               stream_of(x.device)))


def loss_grad_f32(layers, in_dim, out_dim, xdim, sde, cfg, x, y, t, eps, grad_out, loss_out, ic_target=None):
    """dmip_loss_grad_f32: the exact-f32 stacked-jet training step at any width."""
    calls["loss_grad_f32"] += 1
    L = len(layers) - 1
    widths = (_i32 * L)(*[int(layers[i][0].shape[0]) for i in range(L)])
    wp = (_c_void_p * (L + 1))(*[w.data_ptr() for w, _ in layers])
    bp = (_c_void_p * (L + 1))(*[b.data_ptr() for _, b in layers])
    check(lib().dmip_loss_grad_f32(in_dim, out_dim, L, widths, xdim, wp, bp, ctypes.byref(sde), ctypes.byref(cfg),
                                   ptr(x), ptr(y), ptr(t), ptr(eps), ptr(ic_target), int(x.shape[0]), ptr(grad_out),
                                   ptr(loss_out), stream_of(x.device)))


def histogram(x, nbins, lo, hi, counts):
    """x: (n_hist, n, d) fp32 device tensor; counts: (n_hist, nbins**d) int32 device tensor (accumulated)."""
    calls["histogram"] += 1
    n_hist, n, d = x.shape
    check(lib().dmip_histogram(ptr(x), int(n), int(d), int(nbins), float(lo), float(hi), int(n_hist), ptr(counts),
                               stream_of(x.device)))


# ------------------------------------------------------------------------- scatterometry surrogate
class SurrogateHandle:
    """Owns a dmip_surrogate* (packed f32 MFMA images of the frozen forward model)."""

    def __init__(self, layers, device):
        widths = (_i32 * 3)(*[int(layers[i][0].shape[0]) for i in range(3)])
        with torch.cuda.device(device):
            ws = [w.detach().float().contiguous().cpu() for w, _ in layers]
            bs = [b.detach().float().contiguous().cpu() for _, b in layers]
            wp = (_c_void_p * 4)(*[w.data_ptr() for w in ws])
            bp = (_c_void_p * 4)(*[b.data_ptr() for b in bs])
            out = _c_void_p()
            check(lib().dmip_surrogate_create(int(layers[0][0].shape[1]), int(layers[-1][0].shape[0]), 3, widths,
                                              wp, bp, ctypes.byref(out)))
        self.h = out
        self.device = device

    def __del__(self):
        h = getattr(self, "h", None)
        if h and _lib is not None:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            _lib.dmip_surrogate_destroy(h)
            self.h = None


def scat_noise(a, b, lambd_bd):
    return DmipScatNoise(float(a), float(b), float(lambd_bd))


def surrogate_forward(handle, x, out):
    calls["surrogate_forward"] += 1
    check(lib().dmip_surrogate_forward(handle.h, ptr(x), int(x.shape[0]), ptr(out), stream_of(x.device)))


def log_posterior(handle, noise, x, y, y_stride, e_out, grad_out=None):
    calls["log_posterior"] += 1
    check(lib().dmip_log_posterior(handle.h, ctypes.byref(noise), ptr(x), ptr(y), int(y_stride), int(x.shape[0]),
                                   ptr(e_out), ptr(grad_out), stream_of(x.device)))


def mh_sample(handle, noise, y, n_chains, chain_offset, num_steps, noise_std, seed, x_out, x_init=None,
              inj_noise=None, inj_unif=None, e_out=None, precision="fp32"):
    """dmip_mh_sample_ex: "fp32" the exact-f32 kernel, "fp32x3" the split-fp16 one (dmip_dps_x3.hip mh_x3_kernel)."""
    calls["mh_sample"] += 1
    _status_pending.add(_dev_index(y.device))
    check(lib().dmip_mh_sample_ex(handle.h, ctypes.byref(noise), ptr(y), int(y.shape[0]), int(n_chains),
                                  int(chain_offset), int(num_steps), float(noise_std), _u64(seed), ptr(x_init),
                                  ptr(inj_noise), ptr(inj_unif), precision_code(precision), ptr(x_out), ptr(e_out),
                                  stream_of(y.device)))


def mala_sample(handle, noise, y, n_chains, chain_offset, num_steps, lang_steps, stepsize, lambd, seed, x_out,
                x_init=None, inj_eta=None, inj_unif=None, e_out=None, acc_out=None):
    """dmip_mala_sample: fused Metropolis-adjusted Langevin chains (csrc/dmip_surrogate.hip mala_kernel), exact f32."""
    calls["mala_sample"] += 1
    _status_pending.add(_dev_index(y.device))
    check(lib().dmip_mala_sample(handle.h, ctypes.byref(noise), ptr(y), int(y.shape[0]), int(n_chains),
                                 int(chain_offset), int(num_steps), int(lang_steps), float(stepsize), float(lambd),
                                 _u64(seed), ptr(x_init), ptr(inj_eta), ptr(inj_unif), ptr(x_out), ptr(e_out),
                                 ptr(acc_out), stream_of(y.device)))


def dps_sample(prior, surrogate, noise, sde, y, n_chains, chain_offset, num_steps, mean, std, seed, mode, zeta, out,
               precision="fp32"):
    """dmip_dps_sample_ex: "fp32" the exact-f32 kernel, "fp32x3" the split-fp16 one (dmip_dps_x3.hip)."""
    calls["dps_sample"] += 1
    _status_pending.add(_dev_index(y.device))
    check(lib().dmip_dps_sample_ex(prior.h, surrogate.h, ctypes.byref(noise), ctypes.byref(sde), ptr(y),
                                   int(y.shape[0]), int(n_chains), int(chain_offset), int(num_steps), float(mean),
                                   float(std), _u64(seed), int(mode), float(zeta), precision_code(precision), ptr(out),
                                   stream_of(y.device)))


def dps_linear_supported(width, n_hidden, xdim, ydim, precision="fp32x3"):
    return bool(lib().dmip_dps_linear_supported(width, n_hidden, xdim, ydim, precision_code(precision)))


def dps_linear_sample(prior, sde, A, B, yres, n_chains, chain_offset, num_steps, mean, std, seed, step_rule, zeta, out,
                      precision="fp32x3"):
    """dmip_dps_linear_sample: guided posterior samples of a linear-Gaussian problem from the prior (x, t) network
    alone into out (n_y, n_chains, xdim). A (ydim, xdim), B (n_B, ydim, xdim) the guidance table, yres (n_y, ydim)
    = y - b: contiguous f32 device tensors. "fp32" the exact-f32 kernel, any other precision the fp32x3 one."""
    calls["dps_linear_sample"] += 1
    _status_pending.add(_dev_index(yres.device))
    check(lib().dmip_dps_linear_sample(prior.h, ctypes.byref(sde), ptr(A), ptr(B), int(B.shape[0]), ptr(yres),
                                       int(yres.shape[1]), int(yres.shape[0]), int(n_chains), int(chain_offset),
                                       int(num_steps), float(mean), float(std), _u64(seed), int(step_rule),
                                       float(zeta), precision_code(precision), ptr(out), stream_of(yres.device)))


def dps_tweedie_supported(width, n_hidden, xdim, ydim, precision="fp32x3"):
    return bool(lib().dmip_dps_tweedie_supported(width, n_hidden, xdim, ydim, precision_code(precision)))


def dps_tweedie_sample(prior, sde, A, B, H, yres, n_chains, chain_offset, num_steps, mean, std, seed, zeta, out,
                       precision="fp32x3"):
    """dmip_dps_tweedie_sample: dps_linear_sample with the Tweedie-covariance guidance. A (ydim, xdim), B (ydim, xdim)
    = Sigma^-1 A, H (xdim, xdim) = A^T Sigma^-1 A, yres (n_y, ydim) = y - b: contiguous f32 device tensors."""
    calls["dps_tweedie_sample"] += 1
    _status_pending.add(_dev_index(yres.device))
    check(lib().dmip_dps_tweedie_sample(prior.h, ctypes.byref(sde), ptr(A), ptr(B), ptr(H), ptr(yres),
                                        int(yres.shape[1]), int(yres.shape[0]), int(n_chains), int(chain_offset),
                                        int(num_steps), float(mean), float(std), _u64(seed), float(zeta),
                                        precision_code(precision), ptr(out), stream_of(yres.device)))


def posterior_loss_grad(prior_layers, lik_layers, surrogate, noise, lam, sde, x, y, t, eps, grad_prior, grad_lik,
                        loss_out, target_out=None):
    """dmip_posterior_loss_grad (A18): layers = [(weight, bias)] device fp32 tensors of the prior (MLP2) and
    likelihood (MLP) networks; writes the flat reference-order gradients, loss_out[3] and optionally the
    likelihood target."""
    calls["posterior_loss_grad"] += 1
    L = len(prior_layers) - 1
    widths = (_i32 * L)(*[int(prior_layers[i][0].shape[0]) for i in range(L)])
    arr = lambda ts: (_c_void_p * (L + 1))(*[v.data_ptr() for v in ts])
    check(lib().dmip_posterior_loss_grad(
        int(x.shape[1]), int(y.shape[1]), L, widths, arr([w for w, _ in prior_layers]), arr([b for _, b in prior_layers]),
        arr([w for w, _ in lik_layers]), arr([b for _, b in lik_layers]), surrogate.h, ctypes.byref(noise),
        float(lam), ctypes.byref(sde), ptr(x), ptr(y), ptr(t), ptr(eps), int(x.shape[0]), ptr(grad_prior),
        ptr(grad_lik), ptr(loss_out), ptr(target_out), stream_of(x.device)))
