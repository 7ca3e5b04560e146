"""Numpy restatement of the second-order sampler of the probability-flow ODE (include/dmip.h dmip_ode_sample,
csrc/dmip_device.h HeunStep), for the tests. A plain module.

Scheme (the sampler's reverse grid tau_i = T - linspace_f32(S)[i] T for i = 0..S, tau_S = 0; delta = T / S;
lmbd = 1, so g_mu = 0.5 g):
    m(x, i) = g_mu_i a(x, y, tau_i) - (-0.5 beta_i) x
    k1 = m(x_i, i);  x~ = x_i + delta k1;  k2 = m(x~, i + 1);  x_{i+1} = x_i + (0.5 delta)(k1 + k2)
a is the CDE network, or g_i (likelihood + prior) at each stage's own g for the Posterior estimator.
`dtype` float64 is the scheme itself (the yardstick: tau is the f32 grid the kernels see, everything else in f64);
float32 rounds every operation where the kernels do:
    m = fl(fl(g_mu a) - fl(fl(-0.5 beta) x)), g_mu = fl(0.5 g);  x~ = fl(x + fl(delta k1));
    x' = fl(x + fl(fl(0.5 delta) fl(k1 + k2)))
A plain MLP forward (no Jacobians: flow_ref.mlp_jet is far too slow for 2048-step references).
"""
import numpy as np

import oracle as O

F32 = np.float32


def mlp(params, inp, dtype=np.float64, act="tanh"):
    """nets.py:17-35: Linear -> act -> act -> [Linear -> act] * (L - 2) -> Linear, every product in `dtype`."""
    h = np.asarray(inp, dtype)
    L = len(params)
    for li, (W, b) in enumerate(params):
        h = (h @ np.asarray(W, dtype).T + np.asarray(b, dtype)).astype(dtype)
        if li < L - 1:
            for _ in range(2 if li == 0 else 1):
                h = (np.tanh(h) if act == "tanh" else h / (1.0 + np.exp(-h))).astype(dtype)
    return h


def grid(num_steps, T=1.0, dtype=np.float64, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """tau_i, beta_i, g_i for i = 0..S: tau is the kernels' f32 grid; beta and g in the f32 rounding order of
    step_coef (dtype float32: bmin and bdiff = beta_max - beta_min, taken in double, each rounded to f32 once) or in
    f64 from that tau."""
    _, tau = O.schedule(num_steps, T)
    if dtype == np.float32:
        return tau, O.vp_beta(tau, beta_min, beta_max), O.vp_g(tau, beta_min, beta_max)
    tau = tau.astype(np.float64)
    beta = beta_min + (beta_max - beta_min) * tau
    return tau, beta, np.sqrt(beta)


def score(params, x, y, tau, g, prior_params=None, dtype=np.float64, act="tanh"):
    """a(x, y, tau): the CDE network, or g (likelihood + prior) (nets.py:155-157)."""
    n = x.shape[0]
    t = np.full((n, 1), tau, dtype)
    yy = np.broadcast_to(np.asarray(y, dtype).reshape(1, -1), (n, np.asarray(y).size))
    a = mlp(params, np.concatenate([x, yy, t], 1), dtype, act)
    if prior_params is not None:
        s = (a + mlp(prior_params, np.concatenate([x, t], 1), dtype, act)).astype(dtype)
        a = (dtype(g) * s).astype(dtype)
    return a


def _slope(x, a, beta, g, dtype):
    if dtype == np.float32:
        g_mu = F32(F32(0.5) * g)
        return ((g_mu * a).astype(F32) - (F32(F32(-0.5) * beta) * x).astype(F32)).astype(F32)
    return 0.5 * g * a + 0.5 * beta * x


def heun_sample(params, x0, y, num_steps, prior_params=None, T=1.0, dtype=np.float64, snapshot_every=0, act="tanh",
                beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """x_S (n, d) from x0 (n, d) under one observation y; with snapshot_every > 0 also the states after every
    snapshot_every-th full step, (S // snapshot_every, n, d)."""
    x = np.asarray(x0, dtype).copy()
    tau, beta, g = grid(num_steps, T, dtype, beta_min, beta_max)
    delta = dtype(T / num_steps)
    half = dtype(dtype(0.5) * delta)
    snaps = []
    for i in range(num_steps):
        a = score(params, x, y, tau[i], g[i], prior_params, dtype, act)
        k1 = _slope(x, a, beta[i], g[i], dtype)
        xt = (x + (delta * k1).astype(dtype)).astype(dtype)
        a = score(params, xt, y, tau[i + 1], g[i + 1], prior_params, dtype, act)
        k2 = _slope(xt, a, beta[i + 1], g[i + 1], dtype)
        x = (x + (half * (k1 + k2).astype(dtype)).astype(dtype)).astype(dtype)
        if snapshot_every and (i + 1) % snapshot_every == 0:
            snaps.append(x.copy())
    return (x, np.stack(snaps)) if snapshot_every else x


def euler_sample(params, x0, y, num_steps, prior_params=None, T=1.0, act="tanh", beta_min=O.BETA_MIN,
                 beta_max=O.BETA_MAX):
    """The lmbd = 1 Euler sampler in f64 (flow_ref.ode_sample without the Jacobians)."""
    x = np.asarray(x0, np.float64).copy()
    tau, beta, g = grid(num_steps, T, beta_min=beta_min, beta_max=beta_max)
    delta = T / num_steps
    for i in range(num_steps):
        a = score(params, x, y, tau[i], g[i], prior_params, np.float64, act)
        x = x + delta * _slope(x, a, beta[i], g[i], np.float64)
    return x


def x0_of_seed(seed, n, xdim, chain_offset=0, stream=0, mean=0.0, std=1.0):
    """The samplers' own start states: mean + std times the first normals of each chain's stream."""
    st = O.rng_init(seed, np.arange(chain_offset, chain_offset + n), stream)
    return (O.rng_normals(st, xdim) * F32(std) + F32(mean)).astype(F32)


def params_of(net):
    """[(W, b), ...] float32 numpy of a package MLP / MLP2 (nets.py linear_layers)."""
    return [(w.detach().cpu().numpy().astype(F32), b.detach().cpu().numpy().astype(F32))
            for w, b in net.linear_layers()]


def max_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# the parity cases of tests/test_gpu_heun.py (bound 1): random weights, three hidden layers, S = 5; the project's
# bound for ten evaluations of these engines (tests/test_gpu_lmbd.py) against the f64 restatement
PARITY_STEPS = 5
PARITY_CASES = [("cde", 64, 2, 2, 700), ("cde", 256, 3, 23, 100), ("cde", 512, 3, 23, 50),
                ("posterior", 64, 2, 2, 333), ("posterior", 256, 3, 23, 100)]
BOUND = {"fp32": 1e-4, "fp32x3": 1e-3}


def parity_case(dmip, kind, W, xd, yd, n, hidden=3):
    """(model, params, prior_params, y (yd,), x0 (n, xd)) of a parity case: torch's default initialisation under a
    seed fixed by the shape (the same on the CPU and beside a GPU: parameters are created on the CPU)."""
    import torch
    torch.manual_seed(1000 * W + 10 * xd + (kind == "posterior"))
    if kind == "cde":
        m = dmip.CDE(xd, yd, [W] * hidden)
        params, prior = params_of(m.sde.a), None
    else:
        m = dmip.PosteriorDiffusionEstimator(xd, yd, [W] * hidden)
        params, prior = params_of(m.sde.a.likelihood_net), params_of(m.sde.a.prior_net)
    g = torch.Generator().manual_seed(W + n)
    y = torch.randn(yd, generator=g).numpy()
    x0 = torch.randn(n, xd, generator=g).numpy()
    return m, params, prior, y, x0
