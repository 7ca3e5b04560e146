"""The cases of the non-default VP-SDE tests: what tests/test_gpu_sde_params.py runs on the device and
tests/test_sde_params_host.py checks on the CPU (that every reference moves by at least 50 bounds when any one of
beta_min, beta_max, T falls back to its default). A plain module: models, references and bounds, nothing device-side.

Every bound is the one the project asserts for the same kernel against the same reference at the default SDE; the
name of the test it comes from stands beside it. Relative bounds are of max(1, max |ref|), as there.
"""
import functools
import importlib

import numpy as np
import torch

import flow_ref as FR
import flow_sample_ref as FS
import heun_ref as HR
import oracle as O

DEFAULT = (0.1, 20.0, 1.0)
# (beta_min, beta_max, T). A: every value exact in f32, T < 1; B: beta_min and beta_max - beta_min inexact in f32, T > 1
SDES = {"A": (0.5, 4.0, 0.75), "B": (1.1, 25.0, 1.25)}
FACTOR = 50.0      # a reference with one parameter at its default misses the test SDE's by this many bounds
MEAN, STD = 0.3, 1.5


def variants(sde):
    """{name: sde with that one parameter reset to the default}."""
    return {name: tuple(DEFAULT[j] if j == i else sde[j] for j in range(3))
            for i, name in enumerate(("beta_min", "beta_max", "T"))}


def kw(sde):
    return dict(beta_min=sde[0], beta_max=sde[1], T=sde[2])


def set_sde(dmip, m, sde):
    """m.sde = PluginReverseSDE(VariancePreservingSDE(beta_min, beta_max, T), m.sde.a, T): what a user writes. The
    two-network scores (PosteriorScore, DPS's prior drift) hold the forward process for their own g: it is replaced
    too, so that the eager module and the kernels see one SDE."""
    sdes = importlib.import_module(dmip.__name__ + ".sdes")
    base = sdes.VariancePreservingSDE(*sde)
    m.sde = sdes.PluginReverseSDE(base, m.sde.a, T=sde[2], debias=m.sde.debias)
    if hasattr(m.sde.a, "forward_sde"):
        m.sde.a.forward_sde = base
    return m


def rel(out, ref):
    return float(np.abs(np.asarray(out, np.float64) - np.asarray(ref, np.float64)).max()
                 / max(1.0, float(np.abs(ref).max())))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(1e-30, np.linalg.norm(b)))


# ------------------------------------------------------------------------------------------ Euler samplers
# id: (class, W, xdim, ydim, n, precision, bound, sample_device keywords). Three hidden layers, S = 6 steps,
# mean 0.3, std 1.5. Bounds: fp16 tests/test_gpu_parity.py *_vs_oracle_product_rng (1e-4 / 7e-4 / 1.2e-4); exact f32
# tests/test_gpu_f32.py test_f32_*_sampler_vs_oracle (1e-4); fp32x3 tests/test_gpu_x3.py test_x3_*_vs_oracle and
# tests/test_gpu_x3k.py test_x3k_vs_oracle_ragged (1e-4).
EULER_STEPS = 6
EULER = {
    "fp16-cde64": ("CDE", 64, 2, 2, 333, "fp16", 1e-4, {}),
    "fp16-post64": ("Posterior", 64, 2, 2, 333, "fp16", 7e-4, {}),
    "fp16-cdiffe64": ("CDiffE", 64, 2, 2, 333, "fp16", 1.2e-4, {}),
    "fp32-cde64": ("CDE", 64, 2, 2, 333, "fp32", 1e-4, {}),
    "fp32-cde256": ("CDE", 256, 3, 23, 131, "fp32", 1e-4, {}),
    "fp32-post64": ("Posterior", 64, 2, 2, 333, "fp32", 1e-4, {}),
    "fp32-cdiffe64": ("CDiffE", 64, 2, 2, 333, "fp32", 1e-4, {}),
    "fp32-cdiffe256-pc": ("CDiffE", 256, 3, 23, 131, "fp32", 1e-4, dict(corrector_steps=1, snr=0.3)),
    "x3s-cde64": ("CDE", 64, 2, 2, 49, "fp32x3", 1e-4, {}),            # the latency engine (dmip_x3s.h)
    "x3-cde128": ("CDE", 128, 3, 23, 131, "fp32x3", 1e-4, {}),         # the one-tile engine (dmip_x3.h)
    "x3-post256": ("Posterior", 256, 3, 23, 131, "fp32x3", 1e-4, {}),
    "x3-cdiffe64": ("CDiffE", 64, 2, 2, 333, "fp32x3", 1e-4, {}),
    "x3k-cde256-49": ("CDE", 256, 3, 23, 49, "fp32x3", 1e-4, {}),      # k-major + x3k_coef_kernel
    "x3k-cde256-1000": ("CDE", 256, 3, 23, 1000, "fp32x3", 1e-4, {}),
}
EULER_SEED = 4711


def _cls(dmip, name):
    return getattr(dmip, "PosteriorDiffusionEstimator" if name == "Posterior" else name)


def euler_model(dmip, cid):
    """(a fresh model at the default SDE, params, prior params or None, ys (2, ydim)); parameters are created on the
    CPU under a seed fixed by the shape, so the host test and the device test hold the same networks. Models are
    built anew on every call (the tests change their SDE and device); only the numpy references below are cached."""
    cls, W, xd, yd, n, prec, bound, extra = EULER[cid]
    torch.manual_seed(7000 + W + 10 * xd + {"CDE": 0, "Posterior": 1, "CDiffE": 2}[cls])
    m = _cls(dmip, cls)(xd, yd, [W] * 3)
    if extra.get("corrector_steps"):
        # as tests/test_gpu_f32.py test_f32_cdiffe_predictor_corrector_vs_oracle: a small, smooth output layer keeps
        # the corrector's comparison well conditioned
        with torch.no_grad():
            last = [l for l in m.sde.a if isinstance(l, torch.nn.Linear)][-1]
            last.weight.mul_(0.05)
            last.bias.fill_(0.5)
    if cls == "Posterior":
        params, prior = HR.params_of(m.sde.a.likelihood_net), HR.params_of(m.sde.a.prior_net)
    else:
        params, prior = HR.params_of(m.sde.a), None
    ys = np.random.default_rng(W + yd).uniform(0, 1, (2, yd)).astype(np.float32)
    return m, params, prior, ys


@functools.lru_cache(maxsize=None)
def euler_ref(dmip, cid, sde, k=0):
    """The oracle's chains of observation k (RNG stream k), read-only."""
    cls, W, xd, yd, n, prec, bound, extra = EULER[cid]
    _, params, prior, ys = euler_model(dmip, cid)
    common = dict(mean=MEAN, std=STD, stream=k, **kw(sde))
    if cls == "CDE":
        ref = O.cde_sample(params, ys[k], n, EULER_STEPS, EULER_SEED, **common)
    elif cls == "Posterior":
        ref = O.posterior_sample(prior, params, ys[k], n, EULER_STEPS, EULER_SEED, **common)
    else:
        ref = O.cdiffe_sample(params, ys[k], n, EULER_STEPS, EULER_SEED, **common, **extra)
    ref.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------ Heun
# tests/test_gpu_heun.py test_parity_with_the_restatement: HR.BOUND[prec] max(1, |ref|), x0 injected, S = 5
HEUN = {"cde64": ("cde", 64, 2, 2, 333), "cde256": ("cde", 256, 3, 23, 100), "post64": ("posterior", 64, 2, 2, 333)}
HEUN_STEPS = HR.PARITY_STEPS


def heun_model(dmip, cid):
    return HR.parity_case(dmip, *HEUN[cid])  # (m, params, prior, y, x0)


@functools.lru_cache(maxsize=None)
def heun_ref(dmip, cid, sde, dtype=np.float64):
    _, params, prior, y, x0 = heun_model(dmip, cid)
    ref = HR.heun_sample(params, x0, y, HEUN_STEPS, prior, dtype=dtype, **kw(sde))
    ref.setflags(write=False)
    return ref


# the unfused loop (a shape without a fused sampler, as tests/test_gpu_heun.py
# test_shape_without_a_kernel_steps_through_the_loop builds it): Heun from x0 and the lmbd = 1 Euler loop from the
# loop's own start states, both to HR.BOUND["fp32"] (tests/test_gpu_capi_paths.py test_lmbd1_launch_vs_restatement)
LOOP_N, LOOP_STEPS, LOOP_SEED, LOOP_STREAM = 200, 5, 4, 1 << 62


def loop_model(dmip):
    torch.manual_seed(96)
    m = dmip.CDE(4, 5, [64] * 3)
    g = torch.Generator().manual_seed(5)
    y, x0 = torch.randn(5, generator=g).numpy(), torch.randn(LOOP_N, 4, generator=g).numpy()
    return m, HR.params_of(m.sde.a), y, x0


@functools.lru_cache(maxsize=None)
def loop_ref(dmip, solver, sde):
    _, params, y, x0 = loop_model(dmip)
    if solver == "heun":
        return HR.heun_sample(params, x0, y, LOOP_STEPS, **kw(sde))
    x0 = HR.x0_of_seed(LOOP_SEED, LOOP_N, 4, stream=LOOP_STREAM, mean=MEAN, std=STD)
    return HR.euler_sample(params, x0, y, LOOP_STEPS, **kw(sde))


# ------------------------------------------------------------------------------------------ flow kernels
# flow_tol below, 4 e_cpu + 1e-6 [max(1, max |f64|)], is the gate that tests/flow_cases.py replaced and never exceeds
# (unscaled for the exact-f32 log_prob, scaled for the rest): a variant that moves past it moves past today's gate
FLOW = {"cde64": ("CDE", 17, 311), "post64": ("Posterior", 5, 312)}   # (class, rows, weight seed): width 64, (2, 2)
FLOW_STEPS = 6


def flow_model(dmip, cid):
    cls, n, seed = FLOW[cid]
    m = _cls(dmip, cls)(2, 2, [64] * 3)
    params = O.reference_weights([5, 64, 64, 64, 2], seed)
    prior = None
    lins = lambda net: [l for l in net if isinstance(l, torch.nn.Linear)]  # noqa: E731
    if cls == "Posterior":
        prior = O.reference_weights([3, 64, 64, 64, 2], seed + 50)
        pairs = list(zip(lins(m.sde.a.likelihood_net), params)) + list(zip(lins(m.sde.a.prior_net), prior))
    else:
        pairs = list(zip(lins(m.sde.a), params))
    with torch.no_grad():
        for lin, (W, b) in pairs:
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))
    g = np.random.default_rng(seed)
    x = g.normal(size=(n, 2)).astype(np.float32)
    y = g.normal(size=2).astype(np.float32)
    return m, params, prior, x, y


@functools.lru_cache(maxsize=None)
def flow_logp_ref(dmip, cid, sde, dtype=np.float64):
    """(logp (n,), latent (n, 2)) of flow_ref.log_prob."""
    _, params, prior, x, y = flow_model(dmip, cid)
    return FR.log_prob(params, x, y, FLOW_STEPS, prior, dtype=dtype, **kw(sde))


@functools.lru_cache(maxsize=None)
def flow_sample_ref(dmip, cid, sde, dtype=np.float64):
    """(x_S (n, 2), logq (n,)) of flow_sample_ref.sample_with_logq from x0 = 0.3 + 1.5 * (the case's rows)."""
    _, params, prior, x, y = flow_model(dmip, cid)
    return FS.sample_with_logq(params, flow_x0(dmip, cid), y, FLOW_STEPS, prior, dtype=dtype, mean=MEAN, std=STD,
                               **kw(sde))


def flow_x0(dmip, cid):
    x = flow_model(dmip, cid)[3]
    return (x * np.float32(STD) + np.float32(MEAN)).astype(np.float32)


def flow_tol(ref64, ref32, scaled):
    ref64, ref32 = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    return 4 * np.abs(ref32 - ref64).max() + 1e-6 * (max(1.0, np.abs(ref64).max()) if scaled else 1.0)


# ------------------------------------------------------------------------------------------ DPS
# tests/test_gpu_surrogate.py test_dps_vs_oracle_product_rng: 1e-3 max(1, |ref|), its guidance pairs, S = 5
# SDE C is DPS's own: the Tweedie estimate divides by mean_weight(T), e^-10 at B, which leaves fp16's range in the first
# step (the default path then resamples in exact f32). C keeps B's inexact beta_min and its T above 1 with a milder
# beta_max (mean_weight(T) = e^-3.4), so that the split engine and dps_x3_coef_kernel are compared there too.
DPS_SDES = dict(SDES, C=(1.1, 8.0, 1.25))



def dps_falls_back(tag, guidance, zeta):
    """Whether the fp32x3 engine leaves fp16's range and the default path resamples in exact f32: never at A, always
    at B, and at C for the pair whose chains themselves pass 65504 ('nll' at zeta = 1: max |ref| 1e6)."""
    return tag == "B" or (tag == "C" and (guidance, zeta) == ("nll", 1.0))


DPS_PAIRS = [("nll", 1.0), ("nll", 0.0), ("norm", 0.05)]
DPS_N, DPS_STEPS, DPS_SEED, DPS_BOUND = 64, 5, 21, 1e-3


def dps_model(dmip, guidance, zeta, forward_model=None):
    torch.manual_seed(3)
    m = dmip.DPS(3, 23, [256] * 3, forward_model, zeta=zeta, guidance=guidance)
    with torch.no_grad():  # (as the default-SDE test: a small, smooth output layer keeps EM + guidance from chaos)
        last = [l for l in m.prior_net if isinstance(l, torch.nn.Linear)][-1]
        last.weight.mul_(0.1)
        last.bias.fill_(0.1)
    return m, HR.params_of(m.prior_net)


def dps_ys():
    from conftest import GOLDEN
    return np.load(f"{GOLDEN}/data_scat.npz")["y_test"][2:4].astype(np.float32)


@functools.lru_cache(maxsize=None)
def dps_ref(dmip, guidance, zeta, sde, k=0):
    """oracle.dps_sample's chains of observation k (RNG stream k)."""
    from conftest import GOLDEN
    _, prior = dps_model(dmip, guidance, zeta)
    sur = O.surrogate_params_from_npz(np.load(f"{GOLDEN}/surrogate.npz"))
    return O.dps_sample(prior, sur, dps_ys()[k], DPS_N, DPS_STEPS, DPS_SEED, zeta=zeta, mode=guidance, stream=k,
                        **kw(sde))


# ------------------------------------------------------------------------------------------ training
LOSS_CFGS = {"pinn": dict(kind="pinn", pde="FPE", pde_metric="L1", ic_metric="L2", lam=1e-3, lam2=0.1),
             "dsm": dict(kind="dsm")}
LIN_IC = dict(ic_A=[[1, 0.5], [0, 1]], ic_b=[0.3, 0.5], ic_Sinv=np.eye(2) / 0.3)
GRAD_KEYS = ("0_weight", "0_bias", "3_weight", "3_bias", "5_weight", "5_bias", "7_weight", "7_bias")


def loss_objects(dmip):
    sp = dmip.LinearForwardProblem().score_posterior
    return {"pinn": dmip.PINNLoss(sp, lam=1e-3, lam2=0.1, pde_loss="FPE", ic_metric="L2", pde_metric="L1"),
            "dsm": dmip.DSMLoss()}


def oracle_loss_case(dmip, T):
    """tests/test_gpu_train_f32.py test_f32_loss_grad_vs_oracle's (100, 2 hidden, n = 777) with t on [1e-4, T]."""
    W, NL, n = 100, 2, 777
    torch.manual_seed(W + NL)
    m = dmip.CDE(2, 2, [W] * NL)
    g = np.random.default_rng(n)
    x = g.normal(size=(n, 2)).astype(np.float32)
    y = (x @ np.array([[1, 0.5], [0, 1]], np.float32).T + np.array([0.3, 0.5], np.float32)
         + 0.3 * g.normal(size=(n, 2))).astype(np.float32)
    t = (1e-4 + g.uniform(size=(n, 1)) * (T - 1e-4)).astype(np.float32)
    eps = g.normal(size=(n, 2)).astype(np.float32)
    return m, HR.params_of(m.sde.a), (x, y, t, eps)


@functools.lru_cache(maxsize=None)
def oracle_loss_ref(dmip, T, sde):
    """(loss, [dW, db, ...]) of oracle.loss_grad (PINNLoss, FPE, L2 / L1) on oracle_loss_case(T)'s batch."""
    _, params, batch = oracle_loss_case(dmip, T)
    loss, _, grads = O.loss_grad(params, *batch, **LOSS_CFGS["pinn"], **LIN_IC, beta_min=sde[0], beta_max=sde[1])
    return loss, [a for wb in grads for a in wb]


def posterior_loss_case(dmip, T):
    """tests/test_gpu_posterior_loss.py test_posterior_loss_vs_oracle's recipe at (64, 2 hidden, B = 333)."""
    from conftest import GOLDEN
    W, NL, B = 64, 2, 333
    torch.manual_seed(W + NL)
    m = dmip.PosteriorDiffusionEstimator(3, 23, [W] * NL)
    g = np.random.default_rng(B)
    x = g.uniform(-1, 1, (B, 3)).astype(np.float32)
    y = np.load(f"{GOLDEN}/data_scat.npz")["y_test"][g.integers(0, 100, B)].astype(np.float32)
    t = g.uniform(1e-4, T, (B, 1)).astype(np.float32)
    eps = g.normal(size=(B, 3)).astype(np.float32)
    return m, HR.params_of(m.sde.a.prior_net), HR.params_of(m.sde.a.likelihood_net), (x, y, t, eps)


@functools.lru_cache(maxsize=None)
def posterior_loss_ref(dmip, T, sde):
    from conftest import GOLDEN
    _, pp, pl, batch = posterior_loss_case(dmip, T)
    sur = O.surrogate_params_from_npz(np.load(f"{GOLDEN}/surrogate.npz"))
    return O.posterior_loss_grad(pp, pl, sur, *batch, 0.2, 0.01, 0.01, beta_min=sde[0], beta_max=sde[1])


# dmip_train_draws: (tag, t_epsilon) x debias x B; tests/test_gpu_train_step.py test_train_draws_vs_oracle's bounds
DRAWS = [("A", 5e-3), ("B", 1e-3)]
DRAWS_B = [1, 4099]
# (draw stream 8: there the single u of the B = 1 case lands mid-range, where all three parameters move its t; a u next
# to 1 gives t = T whatever the betas are)
DRAWS_SEED, DRAWS_K, T_RTOL, T_ATOL, EPS_ATOL = 0x1234_5678_9ABC, 8, 1e-4, 1e-6, 2e-5


def draws_ref(sde, t_eps, debias, B, xdim=2, seed=DRAWS_SEED, k=DRAWS_K):
    return O.train_draws(seed, k, B, xdim, debias, sde[0], sde[1], t_eps, sde[2])
