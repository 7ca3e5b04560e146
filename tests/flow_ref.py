"""Numpy restatement of the probability-flow log-likelihood (include/dmip.h dmip_flow_logp) and of the lambda
family's one-step arithmetic (csrc/dmip_device.h step_coef / em_update), for the tests. A plain module.

Scheme (forward time grid tau_k = linspace_f32(S)[k] T, h = T / S; Heun's explicit trapezoid):
    v(x, tau)    = -1/2 beta(tau) x - 1/2 g(tau) a(x, y, tau)
    divv(x, tau) = -1/2 beta(tau) d - 1/2 g(tau) sum_i da_i/dx_i
    k1 = v(x_k, tau_k); x~ = x_k + h k1; k2 = v(x~, tau_{k+1}); x_{k+1} = x_k + (h/2)(k1 + k2)
    I += (h/2)(divv(x_k, tau_k) + divv(x~, tau_{k+1}));  log p = -(d/2) log 2 pi - |x_S|^2 / 2 + I
a is the CDE network, or g(tau) (prior(x, tau) + likelihood(x, y, tau)) for the Posterior estimator
(nets.py:155-157). The divergence comes from analytic forward tangents through the MLP (as oracle.mlp2_jet).
`dtype` float64 is the scheme itself; float32 evaluates every network product, activation and update in f32 (I in
f64, as the kernel) and measures what f32 rounding costs.
"""
import numpy as np

import oracle as O

LOG_2PI = 1.8378770664093453


def mlp_jet(params, inp, d, dtype=np.float64):
    """a = MLP(inp) (double tanh on layer 1) and J[n, i, k] = da_i / d inp_k for the first d input columns."""
    W = [np.asarray(p[0], dtype) for p in params]
    b = [np.asarray(p[1], dtype) for p in params]
    inp = np.asarray(inp, dtype)
    z = inp @ W[0].T + b[0]
    t1 = np.tanh(z)
    h = np.tanh(t1)
    dh = ((1 - h * h) * (1 - t1 * t1))[:, :, None] * W[0][None, :, :d]
    for l in range(1, len(W) - 1):
        z = h @ W[l].T + b[l]
        dz = np.einsum("ij,njk->nik", W[l], dh)
        h = np.tanh(z)
        dh = (1 - h * h)[:, :, None] * dz
    return h @ W[-1].T + b[-1], np.einsum("ij,njk->nik", W[-1], dh)


def score_div(params, x, y, tau, g, prior_params=None, dtype=np.float64):
    """a(x, y, tau) (n, d) and sum_i da_i/dx_i (n,) of the CDE network `params`, or of the Posterior pair."""
    n, d = x.shape
    t = np.full((n, 1), tau, dtype)
    yy = np.broadcast_to(np.asarray(y, dtype), (n, np.asarray(y).shape[-1]))
    a, J = mlp_jet(params, np.concatenate([x, yy, t], 1), d, dtype)
    dv = np.trace(J, axis1=1, axis2=2)
    if prior_params is not None:
        ap, Jp = mlp_jet(prior_params, np.concatenate([x, t], 1), d, dtype)
        a, dv = g * (a + ap), g * (dv + np.trace(Jp, axis1=1, axis2=2))
    return a.astype(dtype), dv.astype(dtype)


def flow_grid(num_steps, T=1.0, dtype=np.float64, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """tau_k, beta_k, g_k (k = 0..S) and h: the f32 linspace of the sampler's schedule, the rest in `dtype` (bmin and
    bdiff = beta_max - beta_min, taken in double, each rounded to `dtype` once, as flow_coef does)."""
    tau = (O.linspace_f32(num_steps) * np.float32(T)).astype(np.float32).astype(dtype)
    beta = dtype(beta_min) + dtype(beta_max - beta_min) * tau
    return tau, beta.astype(dtype), np.sqrt(beta).astype(dtype), dtype(T / num_steps)


def log_prob(params, x, y, num_steps, prior_params=None, T=1.0, dtype=np.float64, beta_min=O.BETA_MIN,
             beta_max=O.BETA_MAX):
    """(logp (n,) float64, latent x_S (n, d) in dtype) of rows x (n, d) under one observation y."""
    x = np.asarray(x, dtype)
    n, d = x.shape
    tau, beta, g, h = flow_grid(num_steps, T, dtype, beta_min, beta_max)
    half = dtype(0.5)
    I = np.zeros(n, np.float64)
    for k in range(num_steps):
        a, dv = score_div(params, x, y, tau[k], g[k], prior_params, dtype)
        k1 = -(half * g[k] * a + half * beta[k] * x)
        d1 = -(half * beta[k] * dtype(d) + half * g[k] * dv)
        xt = (x + h * k1).astype(dtype)
        a, dv = score_div(params, xt, y, tau[k + 1], g[k + 1], prior_params, dtype)
        k2 = -(half * g[k + 1] * a + half * beta[k + 1] * xt)
        d2 = -(half * beta[k + 1] * dtype(d) + half * g[k + 1] * dv)
        x = (x + (half * h) * (k1 + k2)).astype(dtype)
        I += np.float64(half * h) * (d1.astype(np.float64) + d2.astype(np.float64))
    xs = x.astype(np.float64)
    return -0.5 * d * LOG_2PI - 0.5 * (xs * xs).sum(1) + I, x


def ode_sample(params, x0, y, num_steps, prior_params=None, T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """The sampler's Euler loop at lmbd = 1 in float64 (models/diffusion.py:38-42 with sdes.py:77-87): from the
    latent x0 back to data space; the round trip's other half."""
    x = np.asarray(x0, np.float64)
    ts = (O.linspace_f32(num_steps) * np.float32(T)).astype(np.float64)
    delta = T / num_steps
    for i in range(num_steps):
        tau = T - ts[i]
        beta = beta_min + (beta_max - beta_min) * tau
        g = np.sqrt(beta)
        a, _ = score_div(params, x, y, tau, g, prior_params, np.float64)
        x = x + delta * (0.5 * g * a + 0.5 * beta * x)
    return x


def lmbd_step_f32(x, a, xi, tau, delta, lmbd, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """One reverse step's mu, sigma and x_next in the kernels' f32 rounding order (csrc/dmip_device.h):
    c_mu = f32(1 - 0.5 lmbd), c_sig = f32(sqrt(1 - lmbd)) (double, rounded once), g_mu = fl(c_mu g),
    g_sig = fl(c_sig g), mu = fl(fl(g_mu a) - fl(fl(-0.5 beta) x)), sigma = g_sig,
    x' = fl(fl(x + fl(delta mu)) + fl(fl(sqrt(delta) g_sig) xi))."""
    F = np.float32
    x, a, xi = (np.asarray(v, F) for v in (x, a, xi))
    beta = O.vp_beta(F(tau), beta_min, beta_max)
    g = O.vp_g(F(tau), beta_min, beta_max)
    g_mu = (F(1.0 - 0.5 * lmbd) * g).astype(F)
    g_sig = (F((1.0 - lmbd) ** 0.5) * g).astype(F)
    mu = ((g_mu * a).astype(F) - ((F(-0.5) * beta).astype(F) * x).astype(F)).astype(F)
    drift = (x + (F(delta) * mu).astype(F)).astype(F)
    xn = (drift + ((F(delta ** 0.5) * g_sig).astype(F) * xi).astype(F)).astype(F)
    return mu, np.broadcast_to(g_sig, x.shape).astype(F), xn
