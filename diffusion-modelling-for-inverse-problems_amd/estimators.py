"""CDE / CDiffE / PosteriorDiffusionEstimator with the reference's construct-and-sample API
(models/diffusion.py:14-229).

Sampling is the hot path and runs on the HIP device only: one launch of the fused persistent
reverse-SDE kernel for all num_steps, the chain state never leaving the registers --
  * CDE: dmip_em_sample;
  * PosteriorDiffusionEstimator: dmip_em_sample_posterior (prior + likelihood networks in one kernel);
  * CDiffE (repaired sampler): dmip_em_sample_cdiffe;
  * DPS (BASELINE config 4, prior score net + forward-model guidance): dmip_dps_sample;
  * LinearDPS (a prior score net guided towards a linear-Gaussian measurement): dmip_dps_linear_sample.
CDE and PosteriorDiffusionEstimator sample the whole lambda family of the reference's PluginReverseSDE
(sdes.py:77-87) with `lmbd=`: 0 the reverse SDE (the default), 1 the deterministic probability-flow ODE
(dmip_em_sample_lmbd), and `model.log_prob(x, y)` is the model's own log-density log p(x | y) along that ODE
(dmip_flow_logp, exact f32); `model.sample_with_log_prob(y, n)` draws samples of that ODE together with their
log-density in one launch (dmip_flow_sample, exact f32). Both take `precision="fp32x3"` for the same scheme on the
split-fp16 engine (dmip_flow_logp_ex / dmip_flow_sample_ex); their default is exact f32 whatever `model.precision` is.
`solver="heun"` samples that ODE with second-order steps (dmip_ode_sample); `solver="dpm2m"` (DPM-Solver++(2M)) and
`"ddim"` with one network evaluation per step on a grid uniform in the log-SNR (dmip_multistep_sample, from the step
table of `multistep_table`).
Precision (`model.precision`, or `precision=` per call; default from $DMIP_PRECISION, else "fp32x3"):
  "fp32x3" -- the reference's fp32 arithmetic at the fp16 matrix rate: every product as three fp16 MFMAs
             (W_hi h_hi + W_hi h_lo + W_lo h_hi, fp32 accumulation; csrc/dmip_x3.h), tanh by exp2 + rcp.
             Error per product 2^-23 of sum |w h|, as an fp32 fmaf chain. The default.
  "fp32"   -- exact f32 (v_mfma_f32_16x16x4_f32, an fmaf chain, libm tanh): the bit-level parity mode.
  "fp16"   -- 16-bit MFMA operands (fp16 hidden and output layers, split-bf16 layer 1): the fastest
             mode, ~1e-3 relative per network evaluation. ("bf16" is its deprecated name.)
A shape without a fused kernel in the requested precision runs the next more accurate one that has one
(fp16 -> fp32x3 -> fp32). Shapes with no fused kernel at all step through per-step launches of the
network kernel (dmip_mlp_forward, exact f32) with the SDE update as device tensor ops and the kernels'
chain-keyed RNG (so sharding stays bit-identical there too).
There is no CPU sampling path: without a HIP device the samplers raise.

RNG: the reference draws x0 and the per-step noise from torch's global generator. Here every chain
has its own counter-keyed stream (seed, global chain index, y index); the seed itself is drawn from
torch's global generator, so torch.manual_seed(s) still makes a sampling call reproducible, and the
samples of a chain do not depend on how chains are split over workgroups or GPUs.
"""
import os

import numpy as np
import torch
from torch import nn

from . import _lib
from . import sdes
from .losses import PosteriorLoss
from .nets import MLP, MLP2, PosteriorScore

device = 'cuda' if torch.cuda.is_available() else 'cpu'


class _FusedStep:
    """A batch whose loss and parameter gradients came from the fused kernel (training.py)."""

    def __init__(self, loss, info, stepped=False):
        self.loss, self.info, self.stepped = loss, info, stepped  # stepped: the optimizer update ran too


def _draw_seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def canonical_precision(precision):
    """The sampler precision's name: "bf16" is the deprecated name of "fp16" (the 16-bit engine computes its
    hidden and output layers in fp16)."""
    return "fp16" if precision == "bf16" else precision


def default_precision():
    return canonical_precision(os.environ.get("DMIP_PRECISION", "fp32x3"))


# a precision whose fused kernel is missing for a shape falls back to a more accurate one, never a less
# accurate one: fp16 -> fp32x3 -> fp32
_MORE_ACCURATE = {"fp16": ("fp32x3", "fp32"), "fp32x3": ("fp32",), "fp32": ()}


def _check_lmbd(lmbd, model):
    """lmbd of sdes.py:77-87 as a float in [0, 1]; CDE and PosteriorDiffusionEstimator only (CDiffE's repaired
    sampler and DPS's guidance are this project's own semantics: no ODE form of them)."""
    lmbd = float(lmbd)
    if not 0.0 <= lmbd <= 1.0:
        raise ValueError(f"lmbd must be in [0, 1], got {lmbd}")
    if lmbd != 0.0 and not isinstance(model, (CDE, PosteriorDiffusionEstimator)):
        raise ValueError(f"{type(model).__name__}: lmbd != 0 is implemented for CDE and PosteriorDiffusionEstimator only")
    return lmbd


def _check_eta(eta):
    """eta of the stochastic few-step samplers as a float: finite and >= 0."""
    try:
        eta = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"eta must be a finite float >= 0, got {eta!r}") from None
    if not (np.isfinite(eta) and eta >= 0.0):
        raise ValueError(f"eta must be a finite float >= 0, got {eta!r}")
    return eta


MULTISTEP_GRIDS = ("logsnr", "uniform")


def _check_grid(grid, t_end, T):
    """t_end of a few-step sampling call as a float: None is 1e-3 T; 0 < t_end < T."""
    if grid not in MULTISTEP_GRIDS:
        raise ValueError(f"grid must be one of {MULTISTEP_GRIDS}, got {grid!r}")
    t_end = 1e-3 * T if t_end is None else float(t_end)
    if not 0.0 < t_end < T:
        raise ValueError(f"t_end must be in (0, T = {T}), got {t_end}")
    return t_end


def _check_solver(solver, lmbd, model, x0=None, noise=None, grid="logsnr", t_end=None, eta=0.0):
    """The effective lmbd of a sampling call. solver="heun" is the second-order sampler of the probability-flow ODE
    (dmip_ode_sample): lmbd left at its default or given as 1.0, CDE and PosteriorDiffusionEstimator only, no noise
    to inject. x0= (the chains' start states) needs it, or one of the few-step solvers "dpm2m" / "ddim"
    (dmip_multistep_sample), which integrate the same ODE under the same rules and alone take grid= and t_end=, and
    eta= (their stochastic variants, dmip_multistep_sde_sample)."""
    eta = _check_eta(eta)
    if eta != 0.0 and solver not in _lib.TABLE_SOLVERS:
        raise ValueError(f"eta= belongs to solver='dpm2m' / 'ddim', got solver={solver!r}")
    if solver in _lib.TABLE_SOLVERS:
        if not isinstance(model, (CDE, PosteriorDiffusionEstimator)):
            raise ValueError(f"{type(model).__name__}: solver='{solver}' is implemented for CDE and "
                             "PosteriorDiffusionEstimator only")
        if float(lmbd) not in (0.0, 1.0):
            raise ValueError(f"solver='{solver}' integrates the probability-flow ODE (lmbd = 1), got lmbd={lmbd}")
        if noise is not None and eta != 0.0:
            raise ValueError(f"solver='{solver}' with eta={eta} draws its step noise from the chain's generator: "
                             "noise= injection is not implemented for it (start states go in x0=)")
        if noise is not None:
            raise ValueError(f"solver='{solver}' draws no noise per step: pass the start states as x0=, not noise=")
        _check_grid(grid, t_end, float(model.sde.T))
        return 1.0
    if solver not in _lib.SOLVERS:
        raise ValueError(f"solver must be one of {sorted(_lib.SOLVERS) + list(_lib.TABLE_SOLVERS)}, got {solver!r}")
    if grid != "logsnr" or t_end is not None:
        raise ValueError("grid= and t_end= belong to solver='dpm2m' / 'ddim' (the other samplers run the uniform grid)")
    if solver == "heun":
        if not isinstance(model, (CDE, PosteriorDiffusionEstimator)):
            raise ValueError(f"{type(model).__name__}: solver='heun' is implemented for CDE and "
                             "PosteriorDiffusionEstimator only")
        if float(lmbd) not in (0.0, 1.0):
            raise ValueError(f"solver='heun' integrates the probability-flow ODE (lmbd = 1), got lmbd={lmbd}")
        if noise is not None:
            raise ValueError("solver='heun' draws no noise per step: pass the start states as x0=")
        return 1.0
    if x0 is not None:
        raise ValueError("x0= needs solver='heun'; the Euler samplers take their start states through the noise= "
                         "argument (slot 0 of the injected normals)")
    return _check_lmbd(lmbd, model)


def multistep_table(solver, grid, num_steps, beta_min, beta_max, T, t_end=None, eta=0.0):
    """The step table of dmip_multistep_sample in float64, (num_steps, 8): row i is tau_i | p_i q_i | cx_i c0_i c1_i |
    g_i | cn_i with d = p x + q a and x' = cx x + c0 d + c1 d_prev + cn xi (include/dmip.h), for solver "dpm2m"
    (DPM-Solver++(2M)) or "ddim" (c1 = 0) of the VP-SDE (beta_min, beta_max, T) on
      grid "logsnr"   tau_0 = T .. tau_{S-1} = t_end uniform in the log-SNR lambda = log(alpha / sigma), then 0 (lambda
                      inverts in closed form for the linear beta schedule); t_end defaults to 1e-3 T
      grid "uniform"  the samplers' own f32 grid tau_i = T - T linspace(0, 1, S + 1)[i], whose last step reaches 0
                      (t_end is checked and unused).
    The times are rounded to the f32 the network sees first and every coefficient is formed from those, so the table
    and the network agree on tau. num_steps is the number of network evaluations; the last step, to sigma = 0, returns
    the denoised estimate and is first order for both solvers.
    eta >= 0 (finite) selects the stochastic variants (dmip_multistep_sde_sample reads column 7, the deterministic
    entry point ignores it): for i < S - 1, with h = lambda_{i+1} - lambda_i,
      cx = (sigma' / sigma) e^{-eta h},  c0 + c1 = -alpha' expm1(-(1 + eta) h),  cn = sigma' sqrt(-expm1(-2 eta h))
    and c1 = -(c0 + c1) / (2 r) for "dpm2m". eta = 0 is the deterministic table, bit for bit (cn = 0); eta = 1 is
    SDE-DPM-Solver++(2M) ("dpm2m") and ancestral sampling, the DDIM paper's eta = 1 ("ddim"). Between 0 and 1 this
    exponent convention (k-diffusion's dpmpp_2m_sde) is the definition, not the DDIM paper's linear eta. For every eta,
    cx alpha_i + c0 + c1 = alpha_{i+1} and cx^2 sigma_i^2 + cn^2 = sigma_{i+1}^2: a step maps the exact marginal of a
    point mass to the exact marginal."""
    eta = _check_eta(eta)
    if solver not in _lib.TABLE_SOLVERS:
        raise ValueError(f"solver must be one of {_lib.TABLE_SOLVERS}, got {solver!r}")
    S, T = int(num_steps), float(T)
    bmin, bd = float(beta_min), float(beta_max) - float(beta_min)
    t_end = _check_grid(grid, t_end, T)
    if S < 1:
        raise ValueError("num_steps must be >= 1")
    B = lambda t: 0.5 * t * t * bd + t * bmin                      # the integral of beta: alpha = exp(-B / 2)
    lam = lambda t: -0.5 * B(t) - 0.5 * np.log(-np.expm1(-B(t)))   # log(alpha / sigma)
    if grid == "uniform":
        Tf = torch.tensor(T, dtype=torch.float32)
        tau = (Tf - torch.linspace(0, 1, S + 1, dtype=torch.float32) * Tf)[:S].double().numpy()  # the kernels' step_coef
    else:
        lams = np.linspace(lam(T), lam(t_end), S) if S > 1 else np.array([lam(T)])
        Bl = np.logaddexp(0.0, -2.0 * lams)                        # alpha^2 = 1 / (1 + exp(-2 lambda))
        tau = 2.0 * Bl / (bmin + np.sqrt(bmin * bmin + 2.0 * bd * Bl))
        tau[0] = T
        if S > 1:
            tau[-1] = t_end
        tau = tau.astype(np.float32).astype(np.float64)
    if not (np.all(np.diff(tau) < 0) and tau[-1] > 0):
        raise ValueError(f"multistep_table: the grid's f32 times are not strictly decreasing to t_end = {t_end} "
                         f"(num_steps = {S} is too many for this grid)")
    alpha, sigma2 = np.exp(-0.5 * B(tau)), -np.expm1(-B(tau))
    sigma, lm, g = np.sqrt(sigma2), lam(tau), np.sqrt(bmin + bd * tau)
    tab = np.zeros((S, _lib.DMIP_MULTISTEP_COLS))
    tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 6] = tau, 1.0 / alpha, sigma2 / (g * alpha), g
    h = np.diff(lm)                                                # h_i = lambda_{i+1} - lambda_i > 0, i < S - 1
    if eta == 0.0:
        E = -alpha[1:] * np.expm1(-h)
        tab[:-1, 3], tab[:-1, 4] = sigma[1:] / sigma[:-1], E
    else:
        E = -alpha[1:] * np.expm1(-(1.0 + eta) * h)
        tab[:-1, 3], tab[:-1, 4] = sigma[1:] / sigma[:-1] * np.exp(-eta * h), E
        tab[:-1, 7] = sigma[1:] * np.sqrt(-np.expm1(-2.0 * eta * h))
    if solver == "dpm2m" and S > 2:
        w = 0.5 * h[1:] / h[:-1]                                   # 1 / (2 r_i), r_i = h_{i-1} / h_i, i = 1 .. S - 2
        tab[1:-1, 4], tab[1:-1, 5] = E[1:] * (1.0 + w), -E[1:] * w
    tab[-1, 3:6] = 0.0, 1.0, 0.0                                   # x_S = d_{S-1} (and cn = 0)
    return tab


def _x0_tensor(x0, ys, num_samples, xdim, dev):
    """x0 as a contiguous f32 device tensor (n_y, num_samples, xdim); (num_samples, xdim) is accepted for one y."""
    if x0 is None:
        return None
    x0 = torch.as_tensor(x0).to(device=dev, dtype=torch.float32)
    if x0.ndim == 2 and ys.shape[0] == 1:
        x0 = x0[None]
    if tuple(x0.shape) != (ys.shape[0], int(num_samples), xdim):
        raise ValueError("x0 must have shape (n_y, num_samples, xdim), or (num_samples, xdim) for one y")
    return x0.contiguous()


def _fused_precision(precision, mode, width, n_hidden, xdim, ydim, acts=(_lib.DMIP_ACT_TANH_TWICE_FIRST,),
                     solver="euler", eta=0.0):
    """The precision a fused kernel runs this shape in: the requested one, else the next more accurate
    one that is compiled (_MORE_ACCURATE); None when none is (per-step loop). `acts`: the networks' activation
    chains -- a SiLU network has the exact-f32 CDE sampler only (include/dmip.h dmip_act), and its Heun kernel at
    every shape of that sampler. solver="heun": fp32x3 (the one-tile engine) or fp32; "fp16" runs fp32x3 (there is
    no 16-bit Heun kernel); "dpm2m" / "ddim" likewise (dmip_multistep_supported; dmip_multistep_sde_supported at
    eta != 0)."""
    _lib.precision_code(precision)
    precision = canonical_precision(precision)
    if any(a != _lib.DMIP_ACT_TANH_TWICE_FIRST for a in acts):
        ok = mode == _lib.DMIP_SAMPLER_CDE and _lib.sampler_supported(width, n_hidden, xdim, ydim, mode, "fp32")
        return "fp32" if ok else None
    for prec in (precision,) + _MORE_ACCURATE[precision]:
        if solver in _lib.TABLE_SOLVERS and eta != 0.0:
            ok = _lib.multistep_sde_supported(width, n_hidden, xdim, ydim, mode, prec)
        elif solver in _lib.TABLE_SOLVERS:
            ok = _lib.multistep_supported(width, n_hidden, xdim, ydim, mode, prec)
        elif solver == "heun":
            ok = _lib.ode_sample_supported(width, n_hidden, xdim, ydim, mode, prec)
        else:
            ok = _lib.sampler_supported(width, n_hidden, xdim, ydim, mode, prec)
        if ok:
            return prec
    return None


def _nets_and_mode(model, error, cdiffe=False):
    """(networks, sampler mode) of a model with a fused kernel: [prior, likelihood] for the Posterior estimator, the
    score network for CDE (and CDiffE where the caller has a kernel for it); raises `error` for any other model."""
    if isinstance(model, PosteriorDiffusionEstimator):
        return [model.sde.a.prior_net, model.sde.a.likelihood_net], _lib.DMIP_SAMPLER_POSTERIOR
    if isinstance(model, CDE):
        return [model.sde.a], _lib.DMIP_SAMPLER_CDE
    if cdiffe and isinstance(model, CDiffE):
        return [model.sde.a], _lib.DMIP_SAMPLER_CDIFFE
    raise error


def _flow_precision(precision):
    """The precision of log_prob / sample_with_log_prob: None is "fp32" (what they ran before they took one)."""
    precision = "fp32" if precision is None else precision
    _lib.precision_code(precision)  # ValueError for an unknown name, before anything else
    return precision


def _flow_hint(precision):
    return "" if precision == "fp32" else f' at precision="{precision}" (precision="fp32" has the exact-f32 kernels)'


def _fused_launch(mode, net, prior, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed, out, prec,
                  lmbd=0.0, solver="euler", x0=None, noise=None, table=None, eta=0.0, snapshot_every=0, snaps=None,
                  corrector_steps=0, snr=0.16):
    """The fused launch of sample_device and, with snapshots, of sample_trajectory: dmip_multistep_sample for "dpm2m" /
    "ddim" (`table`: their step table on the device; dmip_multistep_sde_sample at eta != 0), dmip_ode_sample for Heun,
    dmip_em_sample_lmbd for lmbd != 0, else the reverse SDE's own entry point: dmip_em_sample_snapshots with snapshots
    (CDiffE and its corrector included), dmip_em_sample / dmip_em_sample_posterior without."""
    if solver in _lib.TABLE_SOLVERS:
        launch = _lib.multistep_sde_sample if eta != 0.0 else _lib.multistep_sample
        launch(mode, net, prior, ys, num_samples, chain_offset, num_steps, table, mean, std, seed, out, x0,
               snapshot_every, snaps, prec)
    elif solver == "heun":
        _lib.ode_sample(mode, net, prior, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed, out, "heun",
                        x0, snapshot_every, snaps, prec)
    elif lmbd != 0.0:
        _lib.em_sample_lmbd(mode, net, prior, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed, lmbd,
                            out, noise, snapshot_every, snaps, prec)
    elif snaps is not None:
        _lib.em_sample_snapshots(mode, net, prior, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed,
                                 snapshot_every, snaps, out, corrector_steps, snr, prec)
    elif mode == _lib.DMIP_SAMPLER_POSTERIOR:
        _lib.em_sample_posterior(prior, net, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed, out, prec)
    else:
        _lib.em_sample(net, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed, out, noise, prec)
    return out


class BaseClassDiffusionModel:
    """models/diffusion.py:14-58."""

    def __init__(self, xdim, ydim):
        self.xdim = xdim
        self.ydim = ydim
        self.sde = None
        self.precision = default_precision()  # "fp32x3" | "fp32" | "fp16": arithmetic of the sampler's networks

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    # ----------------------------------------------------------------- sampling API
    def forward(self, y, num_samples=2000, num_steps=200, mean=0, std=1, precision=None, lmbd=0.0,
                solver="euler", grid="logsnr", t_end=None, eta=0.0):
        """Posterior samples for one observation y (ydim,): np.ndarray (num_samples, xdim) float32
        (models/diffusion.py:27-46). Under torch.distributed with world_size > 1 the chains are
        sharded over the ranks and every rank returns all num_samples (parallel.sample_sharded).
        `precision` overrides self.precision for this call; `lmbd` in [0, 1] selects the reverse process of
        sdes.py:77-87 (0: the reverse SDE, 1: the deterministic probability-flow ODE; CDE and Posterior only).
        `solver="heun"` samples that ODE with Heun's second-order steps (two network evaluations per step; about
        an eighth of the Euler steps reach the same accuracy: DESIGN.md 3e), sharded like every other call.
        `solver="dpm2m"` (DPM-Solver++(2M)) and `"ddim"` sample it with one evaluation per step on a grid uniform in
        the log-SNR (`grid="logsnr"`, ending at `t_end`, default 1e-3 T, before the last step to 0; `grid="uniform"`
        is the other samplers' grid): num_steps is then the number of evaluations.
        `eta` > 0 with those two solvers draws fresh noise at every step (the stochastic few-step samplers:
        eta = 1 is SDE-DPM-Solver++(2M) for "dpm2m" and ancestral sampling, the DDIM paper's eta = 1, for "ddim";
        between 0 and 1 eta is k-diffusion's exponent convention, x keeps e^{-eta h} of its noise per step, not the DDIM
        paper's linear eta; multistep_table). eta = 0 is the deterministic sampler."""
        from . import parallel
        lmbd = _check_solver(solver, lmbd, self, grid=grid, t_end=t_end, eta=eta)
        # (sample_sharded's launch is guarded: the device status word was read after it, so an asynchronous kernel
        # failure has raised already rather than coming back as silent NaNs)
        kw = {"lmbd": lmbd} if lmbd != 0.0 else {}
        if solver != "euler":
            kw["solver"] = solver
        if solver in _lib.TABLE_SOLVERS:
            kw.update(grid=grid, t_end=t_end)
            if float(eta) != 0.0:
                kw["eta"] = float(eta)
        x = parallel.sample_sharded(self, y, num_samples, num_steps, mean, std, precision=precision, **kw)
        return x.cpu().numpy()

    def sample_trajectory(self, y, num_samples=2000, num_steps=200, snapshot_every=10, mean=0, std=1, seed=None,
                          chain_offset=0, precision=None, corrector_steps=0, snr=0.16, lmbd=0.0, solver="euler",
                          grid="logsnr", t_end=None, eta=0.0):
        """The fused sampler with trajectory snapshots (dmip_em_sample_snapshots): returns device tensors
        (x (n_y, num_samples, xdim), snaps (num_steps // snapshot_every, n_y, num_samples, xdim)), snaps[k]
        = the chains after step (k + 1) * snapshot_every of the loop of models/diffusion.py:27-46 (the
        reference returns only the final state). Same chains, RNG and sharding as sample_device; `lmbd` as
        forward (dmip_em_sample_lmbd with snapshots); `solver="heun"`: the states after each full Heun step
        (dmip_ode_sample); `solver="dpm2m"` / `"ddim"` with `grid` and `t_end` as forward: the states after each of
        their steps (dmip_multistep_sample; with `eta` != 0 dmip_multistep_sde_sample, the noise included)."""
        lmbd = _check_solver(solver, lmbd, self, grid=grid, t_end=t_end, eta=eta)
        eta = float(eta)
        nets, mode = _nets_and_mode(self, NotImplementedError(f"{type(self).__name__}: no fused trajectory sampler"),
                                    cdiffe=True)
        if corrector_steps and mode != _lib.DMIP_SAMPLER_CDIFFE:
            raise ValueError("corrector steps: CDiffE only")
        dev, ys, sde, out = self._prepare(y, num_samples, num_steps, nets)
        net, prior = self._handles(nets, dev)
        if prior is not None and (prior.width, prior.n_hidden) != (net.width, net.n_hidden):
            raise ValueError("prior and likelihood networks must have the same hidden layers")
        prec = _fused_precision(precision or self.precision, mode, net.width, net.n_hidden, self.xdim, self.ydim,
                                [h.act for h in (net, prior) if h is not None], solver, eta)
        if prec is None:
            raise ValueError("no fused sampler for this network shape / activation")
        snaps = torch.empty(int(num_steps) // int(snapshot_every), ys.shape[0], int(num_samples), self.xdim,
                            device=dev, dtype=torch.float32)
        seed = _draw_seed() if seed is None else seed
        # (the reverse SDE's own entry point, dmip_em_sample_snapshots, makes this check itself; to the others 0 means
        # no snapshots)
        if (solver != "euler" or lmbd != 0.0) and not 1 <= int(snapshot_every) <= int(num_steps):
            raise ValueError("snapshot_every must be in [1, num_steps]")
        table = self._multistep_table(solver, grid, num_steps, t_end, dev, eta) if solver in _lib.TABLE_SOLVERS else None
        _fused_launch(mode, net, prior, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed, out, prec, lmbd,
                      solver, None, None, table, eta, snapshot_every, snaps, corrector_steps, snr)
        return out, snaps

    def log_prob(self, x, y, num_steps=200, return_latent=False, precision=None):
        """The model's own log-density log p(x | y) by the instantaneous change of variables along the
        probability-flow ODE (lmbd = 1; Song et al. 2021, section 4.3): num_steps Heun steps from x to the latent
        x_S ~ N(0, I), the divergence of the score network exact (forward tangents), in exact f32 in one launch
        (dmip_flow_logp). x (n, xdim) with one y (ydim,) -> a float32 device tensor (n,); x (n_y, n, xdim) with ys
        (n_y, ydim) -> (n_y, n). return_latent=True: (logp, x_S), x_S shaped as x. CDE and
        PosteriorDiffusionEstimator; like sampling there is no CPU path, and a shape or activation without a
        compiled kernel raises ValueError. precision: None is "fp32" (exact f32); "fp32x3" runs the same scheme on
        the split-fp16 engine (dmip_flow_logp_ex; "fp16" / "bf16" run it too: there is no 16-bit kernel) -- a row
        beyond the split's range then raises "fp16 range", as an explicit precision="fp32x3" sampler call does."""
        nets, mode, precision = self._flow_nets("log_prob", "flow_logp_supported", precision)
        from . import parallel
        x = torch.as_tensor(x)
        single = x.ndim == 2
        dev = x.device if x.is_cuda else self._exec_device(y)
        dev, ys, sde, _ = self._prepare(torch.as_tensor(y).to(dev), 0, num_steps, nets)
        xs = x.to(device=dev, dtype=torch.float32)
        xs = (xs[None] if single else xs).contiguous()
        if xs.ndim != 3 or xs.shape[0] != ys.shape[0] or xs.shape[2] != self.xdim:
            raise ValueError("x must be (n, xdim) for one y (ydim,), or (n_y, n, xdim) for ys (n_y, ydim)")
        net, prior = self._handles(nets, dev)
        logp = torch.empty(xs.shape[0], xs.shape[1], device=dev, dtype=torch.float32)
        latent = torch.empty_like(xs) if return_latent else None
        # guarded: the device status word is read after the launch
        parallel.guarded(dev, lambda: _lib.flow_logp(mode, net, prior, sde, xs, ys, num_steps, logp, latent,
                                                     precision))
        if single:
            logp, latent = logp[0], (latent[0] if return_latent else None)
        return (logp, latent) if return_latent else logp

    def sample_with_log_prob(self, y, num_samples, num_steps=200, mean=0, std=1, seed=None, chain_offset=0, x0=None,
                             precision=None):
        """Samples x ~ q(. | y) of the probability-flow ODE together with their model log-density log q(x | y), in
        exact f32 in one launch (dmip_flow_sample): the steps of sample_device(solver="heun", precision="fp32") --
        the same x at the same seed -- with the divergence of the drift (exact, forward tangents) integrated beside
        them on the same grid, so the pair is consistent by construction (log_prob re-integrates on the forward grid
        and agrees to second order in 1 / num_steps). Device tensors (x (n_y, num_samples, xdim), logq (n_y,
        num_samples)) for ys (n_y, ydim); ((num_samples, xdim), (num_samples,)) for one y (ydim,). `seed`,
        `chain_offset` and `x0` as sample_device: shards of a run are bit-identical to the whole run, and the base
        density N(mean, std^2 I) is evaluated at the f32 start state whichever way it came. With the unnormalised
        log posterior at x these are importance weights (evaluate.importance_report). CDE and
        PosteriorDiffusionEstimator; there is no CPU path, and a shape or activation without a compiled kernel
        raises ValueError. precision: None is "fp32"; "fp32x3" (and "fp16" / "bf16", which run it) is the split-fp16
        engine (dmip_flow_sample_ex): the x of sample_device(solver="heun", precision="fp32x3") at the same seed, and
        "fp16 range" raised for a chain beyond the split's range."""
        def own_checks():  # (made after the model's and the precision's, before the kernel's: _flow_nets)
            n_y = torch.as_tensor(y).reshape(-1, self.ydim).shape[0]
            if x0 is not None:
                shape = tuple(torch.as_tensor(x0).shape)
                if shape != (n_y, int(num_samples), self.xdim) and \
                        not (n_y == 1 and shape == (int(num_samples), self.xdim)):
                    raise ValueError("x0 must have shape (n_y, num_samples, xdim), or (num_samples, xdim) for one y")
            if int(num_samples) < 1 or int(num_steps) < 1:
                raise ValueError("sample_with_log_prob: num_samples and num_steps must be >= 1")
            if not float(std) > 0.0:
                raise ValueError(f"sample_with_log_prob: std must be > 0, got {std}")

        nets, mode, precision = self._flow_nets("sample_with_log_prob", "flow_sample_supported", precision,
                                                own_checks)
        single = torch.as_tensor(y).ndim == 1
        from . import parallel
        dev, ys, sde, out = self._prepare(y, num_samples, num_steps, nets)
        x0 = _x0_tensor(x0, ys, num_samples, self.xdim, dev)
        net, prior = self._handles(nets, dev)
        logq = torch.empty(ys.shape[0], int(num_samples), device=dev, dtype=torch.float32)
        seed = _draw_seed() if seed is None else seed
        # guarded: the device status word is read after the launch
        parallel.guarded(dev, lambda: _lib.flow_sample(mode, net, prior, sde, ys, num_samples, chain_offset, num_steps,
                                                       mean, std, seed, out, logq, x0, precision))
        return (out[0], logq[0]) if single else (out, logq)

    # what each flow query's kernel is called in "no compiled <...>" and in the tanh-chain refusal
    _FLOW_KERNELS = {"flow_logp_supported": ("log-likelihood kernel", "log-likelihood kernel"),
                     "flow_sample_supported": ("kernel", "kernel"), "flow_pairs_supported": ("paired kernel", "kernel")}

    def _flow_nets(self, who, supported, precision, own_checks=None):
        """What log_prob, sample_with_log_prob and their paired forms refuse before any device work: a model without
        an ODE form, an unknown precision, [the caller's own argument checks, where it makes them here,] hidden layers
        or a precision without a kernel (`supported`: the _lib query's name), an activation chain other than tanh.
        Returns (nets, mode, precision)."""
        nets, mode = _nets_and_mode(self, ValueError(f"{type(self).__name__}: {who} is implemented for CDE and "
                                                     "PosteriorDiffusionEstimator only"))
        precision = _flow_precision(precision)
        if own_checks is not None:
            own_checks()
        missing, tanh_only = self._FLOW_KERNELS[supported]
        layers = [list(n.hidden_layers) for n in nets]
        widths = set(w for hl in layers for w in hl)
        if len(widths) != 1 or len(set(len(hl) for hl in layers)) != 1 or \
                not getattr(_lib, supported)(layers[0][0], len(layers[0]), self.xdim, self.ydim, mode, precision):
            raise ValueError(f"{who}: no compiled {missing} for hidden layers {layers}, xdim {self.xdim}"
                             + _flow_hint(precision))
        if any(n.dmip_act != _lib.DMIP_ACT_TANH_TWICE_FIRST for n in nets):
            raise ValueError(f"{who}: the {tanh_only} computes the tanh chain only")
        return nets, mode, precision

    def _handles(self, nets, dev):
        """(net, prior): the handles of _nets_and_mode's networks on `dev`; prior is None but for the Posterior."""
        handles = [n.dmip_handle(dev, self.xdim) for n in nets]
        return handles[-1], (handles[0] if len(handles) > 1 else None)

    def _pairs_y(self, who, y):
        y = torch.as_tensor(y)
        if y.ndim != 2 or y.shape[1] != self.ydim or y.shape[0] < 1:
            raise ValueError(f"{who}: y must be (n, ydim) with n >= 1, one observation per row")
        return y

    def log_prob_pairs(self, x, y, num_steps=200, return_latent=False, precision=None):
        """log p(x_i | y_i) for n pairs, one observation per row: x (n, xdim), y (n, ydim) -> a float32 device tensor
        (n,); return_latent=True: (logp, x_S (n, xdim)). The scheme, precisions and refusals of log_prob; what
        log_prob(x[:, None, :], y)[:, 0] computes, in one launch over all rows instead of one workgroup per pair
        (dmip_flow_logp_pairs): y enters through a per-row layer-1 bias. A row's value does not depend on n or on the
        row's position. Single-device: shard by slicing rows. CDE and PosteriorDiffusionEstimator."""
        nets, mode, precision = self._flow_nets("log_prob_pairs", "flow_pairs_supported", precision)
        x, y = torch.as_tensor(x), self._pairs_y("log_prob_pairs", y)
        if x.ndim != 2 or x.shape[1] != self.xdim:
            raise ValueError("log_prob_pairs: x must be (n, xdim)")
        if x.shape[0] != y.shape[0]:
            raise ValueError(f"log_prob_pairs: x has {x.shape[0]} rows and y has {y.shape[0]}: one y per row of x")
        if int(num_steps) < 1:
            raise ValueError("log_prob_pairs: num_steps must be >= 1")
        from . import parallel
        dev = x.device if x.is_cuda else self._exec_device(y)
        dev, ys, sde, _ = self._prepare(y.to(dev), 0, num_steps, nets)
        xs = x.to(device=dev, dtype=torch.float32).contiguous()
        net, prior = self._handles(nets, dev)
        logp = torch.empty(xs.shape[0], device=dev, dtype=torch.float32)
        latent = torch.empty_like(xs) if return_latent else None
        # guarded: the device status word is read after the launch
        parallel.guarded(dev, lambda: _lib.flow_logp_pairs(mode, net, prior, sde, xs, ys, num_steps, logp, latent,
                                                           precision))
        return (logp, latent) if return_latent else logp

    def sample_with_log_prob_pairs(self, y, num_steps=200, mean=0, std=1, seed=None, chain_offset=0, x0=None,
                                   precision=None):
        """One draw x_i ~ q(. | y_i) per observation with its log-density: y (n, ydim) -> device tensors (x (n, xdim),
        logq (n,)), in one launch over all rows (dmip_flow_sample_pairs). The scheme, precisions and refusals of
        sample_with_log_prob. Row i draws its start from stream (seed, chain_offset + i, 0), the start of
        sample_with_log_prob(y[i], 1, seed=seed, chain_offset=chain_offset + i); x0 (n, xdim) replaces the starts.
        Shards of a run (rows sliced, chain_offset advanced) are bit-identical to the whole run. Single-device. CDE
        and PosteriorDiffusionEstimator."""
        nets, mode, precision = self._flow_nets("sample_with_log_prob_pairs", "flow_pairs_supported", precision)
        y = self._pairs_y("sample_with_log_prob_pairs", y)
        n = int(y.shape[0])
        if x0 is not None and tuple(torch.as_tensor(x0).shape) != (n, self.xdim):
            raise ValueError("sample_with_log_prob_pairs: x0 must have shape (n, xdim), one start per row of y")
        if int(num_steps) < 1:
            raise ValueError("sample_with_log_prob_pairs: num_steps must be >= 1")
        if not float(std) > 0.0:
            raise ValueError(f"sample_with_log_prob_pairs: std must be > 0, got {std}")
        from . import parallel
        dev, ys, sde, _ = self._prepare(y, 0, num_steps, nets)
        if x0 is not None:
            x0 = torch.as_tensor(x0).to(device=dev, dtype=torch.float32).contiguous()
        net, prior = self._handles(nets, dev)
        out = torch.empty(n, self.xdim, device=dev, dtype=torch.float32)
        logq = torch.empty(n, device=dev, dtype=torch.float32)
        seed = _draw_seed() if seed is None else seed
        # guarded: the device status word is read after the launch
        parallel.guarded(dev, lambda: _lib.flow_sample_pairs(mode, net, prior, sde, ys, chain_offset, num_steps, mean,
                                                             std, seed, out, logq, x0, precision))
        return out, logq

    def _multistep_table(self, solver, grid, num_steps, t_end, dev, eta=0.0):
        """multistep_table of this model's VP-SDE as the kernels read it: rounded once to f32, on `dev`."""
        base = self.sde.base_sde
        tab = multistep_table(solver, grid, num_steps, base.beta_min, base.beta_max, self.sde.T, t_end, eta)
        return torch.from_numpy(tab).to(torch.float32).to(dev).contiguous()

    def _exec_device(self, y):
        if isinstance(y, torch.Tensor) and y.is_cuda:
            return y.device
        p = next(self.sde.a.parameters())
        if p.is_cuda:
            return p.device
        if torch.cuda.is_available():
            return torch.device('cuda', torch.cuda.current_device())
        raise RuntimeError("dmip: sampling needs a HIP device (the reverse-SDE sampler is a HIP kernel; "
                           "there is no CPU sampling path)")

    def _ys(self, y, dev):
        ys = torch.as_tensor(y).to(device=dev, dtype=torch.float32)
        return ys.reshape(-1, self.ydim).contiguous()

    def sample_device(self, y, num_samples, num_steps=200, mean=0, std=1, seed=None, chain_offset=0,
                      noise=None, precision=None, lmbd=0.0, solver="euler", x0=None, grid="logsnr", t_end=None,
                      eta=0.0):
        """Device-resident samples (n_y, num_samples, xdim) for ys (n_y, ydim) -- no host copy.
        `chain_offset` selects a shard of a larger run; `noise` injects standard normals
        (num_steps + 1, n_y, num_samples, xdim) (slot 0 -> x0) in place of the internal RNG;
        `precision` ("fp32x3" | "fp32" | "fp16") overrides self.precision; `lmbd` as forward (a chain's x0 and its
        RNG consumption do not depend on it: at lmbd = 1 the normals are drawn and multiplied by 0).
        `solver="heun"` (CDE and Posterior): Heun's second-order steps along the probability-flow ODE
        (dmip_ode_sample; fp32x3 on the one-tile engine, or fp32; "fp16" runs fp32x3), from the same x0 as the Euler
        samplers at the same seed -- or from `x0` (n_y, num_samples, xdim) ((num_samples, xdim) for one y; with
        chain_offset the rows of this shard), e.g. the latent of log_prob(..., return_latent=True): the two are an
        encode / decode pair.
        `solver="dpm2m"` / `"ddim"` (CDE and Posterior): the few-step samplers of that ODE from a step table
        (dmip_multistep_sample; multistep_table), num_steps network evaluations on `grid` ("logsnr", ending at `t_end`,
        or "uniform"); x0, seed, chain_offset and precision as for "heun". `eta` != 0 (forward): their stochastic
        variants (dmip_multistep_sde_sample), whose chain draws the Euler sampler's normals, x0 and every step's, from
        the same stream (the x0 draw is consumed when x0= is given, so the step noise is the same either way); noise=
        is refused.
        This body is CDE's and PosteriorDiffusionEstimator's (`_table_score` is what they word differently); CDiffE and
        the guided samplers have their own, and any other model raises NotImplementedError."""
        nets, mode = _nets_and_mode(self, NotImplementedError())
        lmbd = _check_solver(solver, lmbd, self, x0, noise, grid, t_end, eta)
        eta = float(eta)
        if noise is not None and mode != _lib.DMIP_SAMPLER_CDE:
            raise ValueError("noise injection is only implemented for the fused CDE sampler")
        dev, ys, sde, out = self._prepare(y, num_samples, num_steps, nets)
        seed = _draw_seed() if seed is None else seed
        net, prior = self._handles(nets, dev)
        x0 = _x0_tensor(x0, ys, num_samples, self.xdim, dev)
        prec = None  # (a prior and a likelihood network of unequal hidden layers have no fused kernel)
        if prior is None or (prior.width, prior.n_hidden) == (net.width, net.n_hidden):
            prec = _fused_precision(precision or self.precision, mode, net.width, net.n_hidden, self.xdim, self.ydim,
                                    [h.act for h in (prior, net) if h is not None], solver, eta)
        if noise is not None:
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(noise.shape) != (int(num_steps) + 1, ys.shape[0], int(num_samples), self.xdim):
                raise ValueError("noise must have shape (num_steps+1, n_y, num_samples, xdim)")
            if prec is None:
                raise ValueError("noise injection needs a fused CDE kernel for this shape")
        table = self._multistep_table(solver, grid, num_steps, t_end, dev, eta) if solver in _lib.TABLE_SOLVERS else None
        if prec is not None:
            return _fused_launch(mode, net, prior, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed, out,
                                 prec, lmbd, solver, x0, noise, table, eta)
        if table is not None:
            return _multistep_device_loop(self, ys, int(num_samples), seed, chain_offset, mean, std, x0, table,
                                          self._table_score, stochastic=eta != 0.0)
        base = self.sde.base_sde

        def drift(x, y, tvec):
            return (1. - 0.5 * lmbd) * base.g(tvec, x) * self.sde.a(x, y, tvec) - base.f(tvec, x)

        return _em_device_loop(self, ys, int(num_samples), int(num_steps), mean, std, seed, chain_offset,
                               drift, self.xdim, self.xdim, lmbd=lmbd, solver=solver, x0=x0)

    def _prepare(self, y, num_samples, num_steps, nets):
        dev = self._exec_device(y)
        ys = self._ys(y, dev)
        for net in nets:
            pdev = next(net.parameters()).device
            if pdev != dev:
                raise RuntimeError(f"dmip: score network is on {pdev}, y on {dev}")
        base = self.sde.base_sde
        if float(base.T) != float(self.sde.T):
            raise ValueError("PluginReverseSDE.T must equal the base SDE's T")
        out = torch.empty(ys.shape[0], int(num_samples), self.xdim, device=dev, dtype=torch.float32)
        return dev, ys, _lib.vpsde(base.beta_min, base.beta_max, self.sde.T), out

    def sample_t(self, x, eps=1e-4):
        """Training times (models/diffusion.py:48-58)."""
        if self.sde.debias:
            t_ = self.sde.base_sde.sample_debiasing_t([x.size(0), ] + [1 for _ in range(x.ndim - 1)]) + eps
            t_ = t_.to(x)
            t_[torch.where(t_ > self.sde.T)] -= eps
            t_.requires_grad = True
        else:
            t_ = eps + torch.rand([x.size(0), ] + [1 for _ in range(x.ndim - 1)], requires_grad=True).to(x) * self.sde.T
            t_[torch.where(t_ > self.sde.T)] = self.sde.T - eps
        return t_

    # ----------------------------------------------------------------- training API
    @staticmethod
    def _accumulate(logger_info, k, loss):
        if isinstance(loss, tuple):
            loss, info = loss
            for key, value in info.items():
                prev = logger_info.get(key, 0.0)
                logger_info[key] = prev * k / (k + 1) + value.item() / (k + 1)
        return loss

    def _train_loop(self, optimizer, epoch_data_loader, batch_loss):
        mean_loss = 0
        logger_info = {}
        for k, (x, y) in enumerate(epoch_data_loader()):
            out = batch_loss(x, y)
            if isinstance(out, _FusedStep):  # gradients already written by the fused kernel
                loss = self._accumulate(logger_info, k, (out.loss, out.info))
            else:
                loss = self._accumulate(logger_info, k, out)
                optimizer.zero_grad()
                loss.backward()
            if not (isinstance(out, _FusedStep) and out.stepped):
                optimizer.step()
            mean_loss = mean_loss * k / (k + 1) + loss / (k + 1)
        return mean_loss, logger_info


class CDE(BaseClassDiffusionModel):
    """Conditional diffusion estimator: score net a(x_t, y, t) (models/diffusion.py:60-105)."""

    def __init__(self, xdim, ydim, hidden_layers):
        super().__init__(xdim, ydim)
        score_net = MLP(xdim + ydim + 1, xdim, hidden_layers, nn.Tanh()).to(device)
        self.sde = sdes.PluginReverseSDE(sdes.VariancePreservingSDE(), score_net, T=1, debias=True)

    def _table_score(self, x, y, tvec, g):
        """_multistep_device_loop's a: the score network's output, as the fused kernel takes it."""
        return self.sde.a(x, y, tvec)

    def train_epoch(self, optimizer, loss_fn, epoch_data_loader):
        from .training import DeviceTrainStep, _plain_adam, device_step_enabled, device_step_ok, fused_config, \
            fused_loss_grad, loss_info
        cfg = fused_config(self, loss_fn)
        # $DMIP_TRAIN_DEVICE_STEP=1: t, eps and Adam on the device too (training.DeviceTrainStep)
        dstep = DeviceTrainStep(self, loss_fn, optimizer) \
            if cfg is not None and device_step_enabled() and _plain_adam(optimizer) is not None \
            and device_step_ok(self) else None

        def batch_loss(x, y):
            if dstep is not None:
                return _FusedStep(*loss_info(cfg.kind, dstep(x, y)), stepped=True)
            t = self.sample_t(x)
            if cfg is not None:
                # same draws as base_sde.sample (sdes.py:37-49): eps = randn_like(x)
                eps = torch.randn_like(x)
                optimizer.zero_grad()
                return _FusedStep(*fused_loss_grad(self, loss_fn, cfg, x, y, t, eps))
            x_t, target, std, g = self.sde.base_sde.sample(t, x, return_noise=True)
            if loss_fn.name == 'DSMLoss':
                return loss_fn(self.sde.a(x_t, y, t) / g, std, target).mean()
            return loss_fn(self.sde, x, y, x_t, t, target, std, g)
        return self._train_loop(optimizer, epoch_data_loader, batch_loss)


_LOOP_STREAM = 1 << 62  # RNG stream ids of the per-step loop (disjoint from the fused kernels' y indices)


def _loop_normals(seed, chain_offset, stream_id, n, d, dev):
    """(n, d) normals of the kernels' chain-keyed generator for chains [chain_offset, chain_offset + n)."""
    out = torch.empty(n, 2 * ((d + 1) // 2), device=dev, dtype=torch.float32)
    _lib.rng_normals(seed, chain_offset, stream_id, n, (d + 1) // 2, out)
    return out[:, :d]


def _em_device_loop(model, ys, num_samples, num_steps, mean, std, seed, chain_offset, drift, zdim,
                    keep, y_resample=None, lmbd=0.0, solver="euler", x0=None):
    """Reverse-SDE EM loop on device tensors for shapes without a compiled fused sampler: the
    network evaluations are dmip_mlp_forward launches in the networks' own forward precision
    (nets.MLP.dmip_precision, exact f32 unless set otherwise), the update follows
    models/diffusion.py:40-42 (same rounding order as the fused kernel). Noise comes from the
    kernels' counter-keyed generator, keyed by (seed, global chain index, stream = (y index, step)),
    so a shard of a run draws exactly the chains of the full run (bit-identical union).
    solver="heun" (lmbd = 1): the two-stage update of csrc/dmip_device.h HeunStep, two network launches per step and
    no noise; x0 (n_y, num_samples, zdim) replaces the generator's start states."""
    dev = ys.device
    base = model.sde.base_sde
    T = float(model.sde.T)
    n_y = ys.shape[0]
    outs = []
    ts = torch.linspace(0, 1, num_steps + 1) * T
    delta = T / num_steps
    off = int(chain_offset)
    with torch.no_grad():
        for k in range(n_y):
            y = ys[k]
            sid = _LOOP_STREAM + (k << 40)
            x = x0[k] if x0 is not None else _loop_normals(seed, off, sid, num_samples, zdim, dev) * std + mean
            for i in range(num_steps):
                tau = (T - ts[i]).item()
                tvec = torch.full((num_samples, 1), tau, device=dev)
                if solver == "heun":
                    k1 = drift(x, y, tvec)
                    xt = x + delta * k1
                    k2 = drift(xt, y, torch.full((num_samples, 1), (T - ts[i + 1]).item(), device=dev))
                    x = x + (0.5 * delta) * (k1 + k2)
                    continue
                eps_y = None
                if y_resample is not None:
                    eps_y = _loop_normals(seed, off, sid + (1 << 39) + i, num_samples, model.ydim, dev)
                z_in = x if y_resample is None else y_resample(x, y, tau, eps_y)
                mu = drift(z_in, y, tvec)
                sigma = base.g(tvec, z_in) if lmbd == 0.0 else (1. - lmbd) ** 0.5 * base.g(tvec, z_in)
                xi = _loop_normals(seed, off, sid + 1 + i, num_samples, z_in.shape[1], dev)
                z = z_in + delta * mu + delta ** 0.5 * sigma * xi
                x = z[:, :keep] if keep < z.shape[1] else z
            outs.append(x[:, :keep])
    return torch.stack(outs)


def _multistep_device_loop(model, ys, num_samples, seed, chain_offset, mean, std, x0, table, score, stochastic=False):
    """solver="dpm2m" / "ddim" for shapes without a compiled fused sampler: the update of csrc/dmip_device.h
    MultistepStep from the same f32 table (num_steps, 8) on the device, in its rounding order (f32 tensor ops, no
    fusion), one network launch (dmip_mlp_forward) per network and step. score(x, y, tvec, g) is a (CDE) or
    g (likelihood + prior) (Posterior). The start states are _em_device_loop's: the loop's own chain-keyed x0, or x0.
    stochastic (eta != 0): the table's column 7 times the step's normals is added last; the normals are
    _em_device_loop's, stream sid + 1 + i of the chain-keyed generator, so shards stay bit-identical to the whole."""
    dev = ys.device
    rows = table.cpu()
    outs = []
    with torch.no_grad():
        for k in range(ys.shape[0]):
            sid = _LOOP_STREAM + (k << 40)
            x = x0[k] if x0 is not None else \
                _loop_normals(seed, int(chain_offset), sid, num_samples, model.xdim, dev) * std + mean
            d_prev = torch.zeros_like(x)
            for i, (tau, p, q, cx, c0, c1, g, cn) in enumerate(rows.tolist()):
                a = score(x, ys[k], torch.full((num_samples, 1), tau, device=dev), g)
                d = p * x + q * a
                x = (cx * x + c0 * d) + c1 * d_prev
                if stochastic:
                    x = x + cn * _loop_normals(seed, int(chain_offset), sid + 1 + i, num_samples, model.xdim, dev)
                d_prev = d
            outs.append(x)
    return torch.stack(outs)


class CDiffE(BaseClassDiffusionModel):
    """Conditional diffusion over the joint z = (x, y) (models/diffusion.py:109-180).

    The reference sampler (models/diffusion.py:158-180) raises TypeError (`sde.mu` without `cond`).
    Repaired semantics, consistent with its training (models/diffusion.py:129-137): each step
    re-diffuses the observation, y_t ~ q(y_t | y) at forward time T - t_i, evaluates the joint score
    net a(x_t, y_t, T - t_i) (output xdim + ydim), takes the EM step on z_t = [x_t, y_t] and keeps x.
    """

    def __init__(self, xdim, ydim, hidden_layers):
        super().__init__(xdim, ydim)
        score_net = MLP(xdim + ydim + 1, xdim + ydim, hidden_layers, nn.Tanh()).to(device)
        self.sde = sdes.PluginReverseSDE(sdes.VariancePreservingSDE(), score_net, T=1, debias=True)

    def forward(self, y, num_samples=2000, num_steps=200, mean=0, std=1, corrector_steps=0, snr=0.16,
                precision=None, lmbd=0.0, solver="euler"):
        """As BaseClassDiffusionModel.forward; `corrector_steps` > 0 adds Langevin corrector steps
        before every predictor step (predictor-corrector sampling, BASELINE config 3; see
        dmip_em_sample_cdiffe in include/dmip.h for the definition). The step size takes the norms at
        their expected values, eps = 2 alpha snr^2 var(T - t): `snr` is not score_sde's measured-norm snr
        (that one measures |s| on the batch; for a trained score with |s| != sqrt(d)/std the same value
        gives a different step)."""
        from . import parallel
        _check_solver(solver, lmbd, self)  # (raises for lmbd != 0 or "heun": the repaired sampler has no ODE form)
        x = parallel.sample_sharded(self, y, num_samples, num_steps, mean, std,
                                    corrector_steps=corrector_steps, snr=snr, precision=precision)
        return x.cpu().numpy()  # (the guarded launch read the device status word)

    def sample_device(self, y, num_samples, num_steps=200, mean=0, std=1, seed=None, chain_offset=0,
                      noise=None, corrector_steps=0, snr=0.16, precision=None, lmbd=0.0, solver="euler", x0=None):
        _check_solver(solver, lmbd, self, x0)
        if noise is not None:
            raise ValueError("noise injection is only implemented for the fused CDE sampler")
        net = self.sde.a
        dev, ys, sde, out = self._prepare(y, num_samples, num_steps, [net])
        seed = _draw_seed() if seed is None else seed
        handle = net.dmip_handle(dev, self.xdim)
        prec = _fused_precision(precision or self.precision, _lib.DMIP_SAMPLER_CDIFFE, handle.width,
                                handle.n_hidden, self.xdim, self.ydim, [handle.act])
        if prec is not None:
            _lib.em_sample_cdiffe(handle, sde, ys, num_samples, chain_offset, num_steps, mean, std, seed, out,
                                  corrector_steps, snr, prec)
            return out
        if corrector_steps:
            raise ValueError("the predictor-corrector sampler needs a compiled fused CDiffE kernel for this shape")
        base = self.sde.base_sde
        xd = self.xdim

        def y_resample(x, y, tau, eps):
            tt = torch.full((x.shape[0], 1), tau, device=x.device)
            y_t = base.mean_weight(tt) * y + base.var(tt) ** 0.5 * eps
            return torch.cat([x[:, :xd], y_t], dim=1)

        def drift(z, y, tvec):
            a = self.sde.a(z[:, :xd].contiguous(), z[:, xd:].contiguous(), tvec)
            return base.g(tvec, z) * a - base.f(tvec, z)

        return _em_device_loop(self, ys, int(num_samples), int(num_steps), mean, std, seed, chain_offset,
                               drift, xd, xd, y_resample)

    def train_epoch(self, optimizer, loss_fn, epoch_data_loader):
        """models/diffusion.py:123-156. On a HIP device DSMLoss on the joint z = (x, y) runs through the
        exact-f32 fused loss + gradient engine (training.joint_fused_config); otherwise autograd."""
        from .training import fused_loss_grad, joint_fused_config
        cfg = joint_fused_config(self, loss_fn)

        def batch_loss(x, y):
            z = torch.concat([x, y], dim=1)
            t = self.sample_t(z)
            if cfg is not None:
                eps = torch.randn_like(z)  # base_sde.sample's draw (sdes.py:37-49)
                optimizer.zero_grad()
                return _FusedStep(*fused_loss_grad(self, loss_fn, cfg, z, None, t, eps))
            diffused, target, std, g = self.sde.base_sde.sample(t, z, return_noise=True)
            x_t, y_t = diffused[:, :self.xdim], diffused[:, self.xdim:]
            if loss_fn.name == 'DSMLoss':
                return loss_fn(self.sde.a(x_t, y_t, t) / g, std, target).mean()
            return loss_fn(self.sde, x, y, diffused, t, target, std, g)
        return self._train_loop(optimizer, epoch_data_loader, batch_loss)


class PosteriorDiffusionEstimator(BaseClassDiffusionModel):
    """Prior score + likelihood score, score = g (prior(x,t) + lik(x,y,t)) (models/diffusion.py:182-229)."""

    def __init__(self, xdim, ydim, hidden_layers):
        super().__init__(xdim, ydim)
        forward_process = sdes.VariancePreservingSDE()
        prior_net = MLP2(xdim + 1, xdim, hidden_layers, nn.Tanh()).to(device)
        likelihood_net = MLP(xdim + ydim + 1, xdim, hidden_layers, nn.Tanh()).to(device)
        score_net = PosteriorScore(prior_net, likelihood_net, forward_process)
        self.sde = sdes.PluginReverseSDE(forward_process, score_net, T=1, debias=True)
        self.loss_fn = PosteriorLoss

    def _table_score(self, x, y, tvec, g):
        """_multistep_device_loop's a = g (likelihood + prior) at the table's g, as the fused kernel forms it."""
        score = self.sde.a
        return g * (score.likelihood_net(x, y, tvec) + score.prior_net(x, tvec))

    def train_epoch(self, optimizer, loss_fn, epoch_data_loader):
        """models/diffusion.py:204-229. On a HIP device with PosteriorLoss on the scatterometry surrogate,
        each batch's loss and both networks' gradients come from dmip_posterior_loss_grad (exact f32,
        training.posterior_loss_grad); otherwise the autograd graph of losses.PosteriorLoss."""
        from .training import posterior_fused_ok, posterior_loss_grad
        fused = posterior_fused_ok(self, loss_fn)

        def batch_loss(x, y):
            t = self.sample_t(x)
            if fused:
                eps = torch.randn_like(x)  # base_sde.sample's draw (sdes.py:37-49)
                optimizer.zero_grad()
                return _FusedStep(*posterior_loss_grad(self, loss_fn, x, y, t, eps))
            return loss_fn(self.sde, x, y, t)
        return self._train_loop(optimizer, epoch_data_loader, batch_loss)


class _PriorDrift(nn.Module):
    """a(x, y, t) = g(t) prior(x, t): the unconditional drift of a prior score network (the prior half of
    PosteriorScore, nets.py:155-157); y is ignored."""

    def __init__(self, prior_net, forward_process):
        super().__init__()
        self.prior_net = prior_net
        self.forward_sde = forward_process

    def forward(self, x, y, t):
        return self.forward_sde.g(t, x) * self.prior_net(x, t)


class _PriorDiffusionModel(BaseClassDiffusionModel):
    """What the guided samplers share (DPS, LinearDPS): a prior score network MLP2(x, t) under the unconditional drift
    g prior(x, t), trained by the prior DSM."""

    def _init_prior(self, hidden_layers):
        forward_process = sdes.VariancePreservingSDE()
        prior_net = MLP2(self.xdim + 1, self.xdim, hidden_layers, nn.Tanh()).to(device)
        self.sde = sdes.PluginReverseSDE(forward_process, _PriorDrift(prior_net, forward_process), T=1, debias=True)

    @property
    def prior_net(self):
        return self.sde.a.prior_net

    def _load_prior(self, pn):
        """The weights of another model's prior network, on its device."""
        self.sde.a.prior_net.load_state_dict(pn.state_dict())
        self.sde.a.prior_net.to(next(pn.parameters()).device)
        return self

    def train_epoch(self, optimizer, loss_fn, epoch_data_loader):
        """Prior DSM epoch (the prior half of PosteriorLoss, losses.py:373-377): score = prior(x_t, t)."""
        def batch_loss(x, y):
            t = self.sample_t(x)
            x_t, target, std, g = self.sde.base_sde.sample(t, x, return_noise=True)
            return loss_fn(self.sde.a.prior_net(x_t, t), std, target).mean()
        return self._train_loop(optimizer, epoch_data_loader, batch_loss)


class DPS(_PriorDiffusionModel):
    """Diffusion posterior sampling (Chung et al. 2023; BASELINE config 4) for the scatterometry problem:
    a prior score network MLP2(x, t) (the PosteriorDiffusionEstimator's prior, trained with DSM as
    PosteriorLoss trains it, losses.py:373-377) guided at every EM step by the gradient of the
    measurement likelihood through the surrogate forward model at the Tweedie estimate
    x0_hat = (x + var s) / mean_weight -- the quantity PosteriorLoss.likelihood_target (losses.py:349-371)
    trains the reference's likelihood network towards, here computed exactly on the fly.
    Fused kernel: dmip_dps_sample_ex (include/dmip.h), one launch for all steps: fp32x3 by default (the split-fp16
    engine, J^T by a reverse pass through the prior), exact f32 with precision="fp32".

    forward_model: the surrogate nn.Sequential (load_forward_model); params: {'a', 'b', 'lambd_bd'};
    guidance: 'norm' (default; Chung et al.'s zeta / ||y - F(x0_hat)|| step on ||y - F(x0_hat)||^2) or 'nll'
    (score + zeta grad log p(y | x0_hat), the reference PosteriorLoss target; unstable for zeta >~ 0.01 on
    scatterometry because of the 1/mean_weight amplification at large diffusion times). Measured quality
    against the fused MH ground truth: DESIGN.md §4c."""

    def __init__(self, xdim, ydim, hidden_layers, forward_model=None, params=None, zeta=0.005, guidance='norm'):
        super().__init__(xdim, ydim)
        self._init_prior(hidden_layers)
        self.forward_model = forward_model
        self.params = dict(params or {'a': 0.2, 'b': 0.01, 'lambd_bd': 1000})
        self.zeta = float(zeta)
        if guidance not in ('nll', 'norm'):
            raise ValueError("guidance must be 'nll' or 'norm'")
        self.guidance = guidance

    @classmethod
    def from_posterior(cls, model, forward_model, params=None, zeta=0.005, guidance='norm'):
        """A DPS sampler on the prior network of a trained PosteriorDiffusionEstimator."""
        pn = model.sde.a.prior_net
        return cls(model.xdim, model.ydim, pn.hidden_layers, forward_model, params, zeta, guidance)._load_prior(pn)

    def sample_device(self, y, num_samples, num_steps=200, mean=0, std=1, seed=None, chain_offset=0, noise=None,
                      precision=None, lmbd=0.0, solver="euler", x0=None):
        """dmip_dps_sample_ex at `precision` (default self.precision): "fp32x3" (the reference's fp32 accuracy at
        the fp16 matrix rate, dmip_dps_x3.hip; also what "fp16" runs: there is no 16-bit DPS) or "fp32" (exact f32,
        forward tangents). At the default precision a chain outside fp16's range resamples in exact f32
        (parallel.sample_checked)."""
        _check_solver(solver, lmbd, self, x0)
        if noise is not None:
            raise ValueError("noise injection is only implemented for the fused CDE sampler")
        from .problems import surrogate_handle
        pn = self.sde.a.prior_net
        dev, ys, sde, out = self._prepare(y, num_samples, num_steps, [pn])
        if self.forward_model is None:
            raise ValueError("DPS needs the forward model (load_forward_model) for its guidance")
        sur = surrogate_handle(self.forward_model, dev)
        if sur is None:
            raise ValueError("DPS: forward_model is not the scatterometry surrogate shape (3 -> 256^3 -> 23)")
        seed = _draw_seed() if seed is None else seed
        prior = pn.dmip_handle(dev, self.xdim)
        p = self.params
        prec = canonical_precision(precision or self.precision)
        _lib.dps_sample(prior, sur, _lib.scat_noise(p['a'], p['b'], p['lambd_bd']), sde, ys, num_samples,
                        chain_offset, num_steps, mean, std, seed,
                        _lib.DMIP_DPS_NLL if self.guidance == 'nll' else _lib.DMIP_DPS_NORM, self.zeta, out,
                        precision="fp32" if prec == "fp32" else "fp32x3")
        return out


_LINEAR_GUIDANCES = ('pigdm', 'nll', 'norm', 'tweedie')


def _spd_matrix(Sigma, M):
    """Sigma (a scalar, a length-M diagonal or an M x M matrix) as a float64 M x M array; ValueError unless it is
    symmetric positive definite."""
    S = np.asarray(1.0 if Sigma is None else (Sigma.detach().cpu().numpy() if isinstance(Sigma, torch.Tensor)
                                              else Sigma), np.float64)
    if S.ndim == 0:
        S = float(S) * np.eye(M)
    elif S.shape == (M,):
        S = np.diag(S)
    elif S.shape != (M, M):
        raise ValueError(f"Sigma must be a scalar, a length-{M} diagonal or a {M} x {M} matrix, got shape {S.shape}")
    if not np.all(np.isfinite(S)) or not np.allclose(S, S.T, rtol=1e-12, atol=0.0):
        raise ValueError("Sigma must be finite and symmetric")
    try:
        np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        raise ValueError("Sigma must be symmetric positive definite") from None
    return S


def linear_guidance_table(A, Sigma, guidance, num_steps, beta_min, beta_max, T):
    """The guidance table of dmip_dps_linear_sample in float64: (B [n_B][M][D], step rule).
      'pigdm'  B_i = (Sigma + v_i A A^T)^-1 A for every step of the reverse grid, lambda_i = zeta delta beta_i
      'nll'    B = Sigma^-1 A, one matrix, the same rule
      'norm'   B = 2 A, one matrix, lambda = zeta / |r|
    v_i = var(tau_i) = 1 - exp(-tau_i^2 (beta_max - beta_min) / 2 - tau_i beta_min) at the samplers' f32 times
    tau_i = T - T linspace(0, 1, S + 1)[i]."""
    A = np.asarray(A, np.float64)
    if guidance == 'norm':
        return 2.0 * A[None], _lib.DMIP_DPS_STEP_NORM
    if guidance == 'nll':
        return np.linalg.solve(Sigma, A)[None], _lib.DMIP_DPS_STEP_BETA
    if guidance != 'pigdm':  # ('tweedie' has no per-step table: linear_tweedie_table)
        raise ValueError("guidance must be one of ('pigdm', 'nll', 'norm')")
    S = int(num_steps)
    Tf = torch.tensor(float(T), dtype=torch.float32)
    tau = (Tf - torch.linspace(0, 1, S + 1, dtype=torch.float32) * Tf)[:S].double().numpy()  # the kernels' step_coef
    v = -np.expm1(-0.5 * tau * tau * (float(beta_max) - float(beta_min)) - tau * float(beta_min))
    AAt = A @ A.T
    return np.stack([np.linalg.solve(Sigma + vi * AAt, A) for vi in v]), _lib.DMIP_DPS_STEP_BETA


def linear_tweedie_table(A, Sigma):
    """The matrices of dmip_dps_tweedie_sample in float64: (B [M][D], H [D][D]) = (Sigma^-1 A, A^T Sigma^-1 A). They
    depend on neither the number of steps nor the SDE."""
    A = np.asarray(A, np.float64)
    B = np.linalg.solve(np.asarray(Sigma, np.float64), A)
    return B, A.T @ B


class LinearDPS(_PriorDiffusionModel):
    """Guided posterior sampling for a linear-Gaussian problem y = A x + b + eta, eta ~ N(0, Sigma), from a prior score
    network MLP2(x, t) alone: one trained prior serves every A, b, Sigma and y. Per step, at the Tweedie estimate
    x0_hat = (x + var s) / mean_weight, the residual r = y - b - A x0_hat enters the EM step through
    G = -(I + var J^T) B_i^T r / mean_weight (J = ds/dx, all of it, from the network's forward tangents):
      guidance='pigdm' (default)  B_i = (Sigma + var(tau_i) A A^T)^-1 A: the likelihood of y given x_tau with the
                                  covariance of x0 given x_tau kept; exact for a Gaussian prior
      guidance='nll'              B = Sigma^-1 A: the DPS likelihood, which drops that term
      guidance='norm'             B = 2 A with the step zeta / ||r|| (Chung et al. Alg. 1)
      guidance='tweedie'          'pigdm' with the covariance of x0 given x_tau from Tweedie's second-order formula,
                                  C = (var / mean_weight^2)(I + var J), where 'pigdm' puts var I (right only for a
                                  prior that is N(0, I) in the network's coordinates): u solves (I + A^T Sigma^-1 A C) u
                                  = A^T Sigma^-1 r, one D x D system per chain and step, and G = -(I + var J^T) u /
                                  mean_weight. Exact for a Gaussian prior of any mean and covariance, and stable at
                                  zeta = 1 on an untrained prior, where 'pigdm' overflows. Its kernel
                                  is dmip_dps_tweedie_sample
    Fused kernel: dmip_dps_linear_sample (include/dmip.h), one launch for all steps, for every network shape of the
    flow kernels (widths 64 to 512, 1 to 3 hidden layers, xdim 2 or 3) and ydim up to 32; there is no per-step path.

    A (ydim, xdim); b (ydim,) or None (zero); Sigma a scalar, a (ydim,) diagonal or a (ydim, ydim) matrix (None: the
    identity), symmetric positive definite."""

    def __init__(self, xdim, ydim, hidden_layers, A, b=None, Sigma=None, zeta=1.0, guidance='pigdm'):
        super().__init__(xdim, ydim)
        if not 1 <= int(ydim) <= 32:
            raise ValueError(f"LinearDPS: ydim must be in [1, 32], got {ydim}")
        if guidance not in _LINEAR_GUIDANCES:
            raise ValueError(f"guidance must be one of {_LINEAR_GUIDANCES}")
        as64 = lambda v: np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float64)
        self.A = as64(A)
        if self.A.shape != (ydim, xdim):
            raise ValueError(f"A must have shape (ydim, xdim) = ({ydim}, {xdim}), got {self.A.shape}")
        self.b = np.zeros(ydim) if b is None else as64(b).reshape(-1)
        if self.b.shape != (ydim,):
            raise ValueError(f"b must have {ydim} entries, got {self.b.size}")
        if not (np.all(np.isfinite(self.A)) and np.all(np.isfinite(self.b))):
            raise ValueError("A and b must be finite")
        self.Sigma = _spd_matrix(Sigma, ydim)
        zeta = float(zeta)
        if not (zeta >= 0.0 and np.isfinite(zeta)):
            raise ValueError(f"zeta must be finite and >= 0, got {zeta}")
        self.zeta = zeta
        self.guidance = guidance
        self._init_prior(hidden_layers)
        self._table = None       # (key, A, B, b, step rule): device tensors of the last (num_steps, SDE, guidance, device)
                                 # ('tweedie': (key, A, B, H, b) of the last device)
        self.table_uploads = 0   # instrumentation: how often the table went to a device

    @classmethod
    def from_posterior(cls, model, A, b=None, Sigma=None, zeta=1.0, guidance='pigdm'):
        """A LinearDPS sampler on the prior network of a trained PosteriorDiffusionEstimator (or DPS / LinearDPS)."""
        pn = model.sde.a.prior_net
        return cls(model.xdim, int(np.shape(A)[0]), pn.hidden_layers, A, b, Sigma, zeta, guidance)._load_prior(pn)

    @classmethod
    def for_problem(cls, problem, hidden_layers, zeta=1.0, guidance='pigdm'):
        """The sampler of a LinearForwardProblem: its A, b and Sigma."""
        return cls(problem.xdim, problem.ydim, hidden_layers, problem.A, problem.b, problem.Sigma, zeta, guidance)

    def guidance_table(self, num_steps, dev):
        """(A, B, b, step rule) on `dev`: A (ydim, xdim) and B (n_B, ydim, xdim) as f32 (built in float64, rounded
        once), b as float64 (y - b is formed in float64 and rounded once). Cached on the model for the last
        (num_steps, SDE, guidance, device): repeated calls upload nothing."""
        base = self.sde.base_sde
        key = (int(num_steps), float(base.beta_min), float(base.beta_max), float(self.sde.T), self.guidance, str(dev))
        if self._table is None or self._table[0] != key:
            B, rule = linear_guidance_table(self.A, self.Sigma, self.guidance, num_steps, base.beta_min, base.beta_max,
                                            self.sde.T)
            up = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v)).to(dt).to(dev).contiguous()
            self._table = (key, up(self.A, torch.float32), up(B, torch.float32), up(self.b, torch.float64), rule)
            self.table_uploads += 1
        return self._table[1:]

    def tweedie_table(self, dev):
        """(A, B, H, b) of guidance='tweedie' on `dev`: A, B = Sigma^-1 A (ydim, xdim) and H = A^T Sigma^-1 A (xdim,
        xdim) as f32 (built in float64, rounded once), b as float64. No entry depends on num_steps or the SDE: cached
        per device."""
        key = ('tweedie', str(dev))
        if self._table is None or self._table[0] != key:
            B, H = linear_tweedie_table(self.A, self.Sigma)
            up = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v)).to(dt).to(dev).contiguous()
            self._table = (key, up(self.A, torch.float32), up(B, torch.float32), up(H, torch.float32),
                           up(self.b, torch.float64))
            self.table_uploads += 1
        return self._table[1:]

    def sample_device(self, y, num_samples, num_steps=200, mean=0, std=1, seed=None, chain_offset=0, noise=None,
                      precision=None, lmbd=0.0, solver="euler", x0=None):
        """dmip_dps_linear_sample (guidance='tweedie': dmip_dps_tweedie_sample) at `precision` (default self.precision): "fp32x3" (also what "fp16" runs: there is
        no 16-bit kernel) or "fp32" (exact f32). At the default precision a chain outside fp16's range resamples in
        exact f32 (parallel.sample_checked). A shape without a kernel raises ValueError."""
        _check_solver(solver, lmbd, self, x0)
        if noise is not None:
            raise ValueError("noise injection is only implemented for the fused CDE sampler")
        if int(num_samples) < 1 or int(num_steps) < 1:
            raise ValueError("LinearDPS: num_samples and num_steps must be >= 1")
        prec = canonical_precision(precision or self.precision)
        _lib.precision_code(prec)
        prec = "fp32" if prec == "fp32" else "fp32x3"
        pn = self.prior_net
        dev, ys, sde, out = self._prepare(y, num_samples, num_steps, [pn])
        layers = pn.hidden_layers
        tweedie = self.guidance == 'tweedie'
        supported = _lib.dps_tweedie_supported if tweedie else _lib.dps_linear_supported
        if len(set(layers)) != 1 or pn.dmip_act != _lib.DMIP_ACT_TANH_TWICE_FIRST or \
                not supported(layers[0], len(layers), self.xdim, self.ydim, prec):
            raise ValueError(f"LinearDPS: no compiled kernel for hidden layers {layers}, xdim {self.xdim}, ydim "
                             f"{self.ydim} (equal widths 64 / 128 / 256 / 512, 1 to 3 layers, xdim 2 or 3, nn.Tanh)")
        prior = pn.dmip_handle(dev, self.xdim)
        seed = _draw_seed() if seed is None else seed
        if tweedie:
            A, B, H, b = self.tweedie_table(dev)
            yres = (ys.double() - b).float().contiguous()
            _lib.dps_tweedie_sample(prior, sde, A, B, H, yres, num_samples, chain_offset, num_steps, mean, std, seed,
                                    self.zeta, out, precision=prec)
            return out
        A, B, b, rule = self.guidance_table(num_steps, dev)
        yres = (ys.double() - b).float().contiguous()
        _lib.dps_linear_sample(prior, sde, A, B, yres, num_samples, chain_offset, num_steps, mean, std, seed, rule,
                               self.zeta, out, precision=prec)
        return out
