"""The Euler-Maruyama samplers in float64 (oracle.cde_sample, posterior_sample, cdiffe_sample restated), for the
tests. A plain module beside heun_ref.py and flow_ref.py: the yardstick of tests/accuracy_cases.py.

Scheme (reverse grid tau_i = T - linspace_f32(S)[i] T, delta = T / S, beta_i = beta_min + (beta_max - beta_min) tau_i,
g_i = sqrt(beta_i); lmbd in [0, 1] as flow_ref.lmbd_step_f32 states it, 0 the reverse SDE):
    mu = (1 - lmbd / 2) g_i a(x, y, tau_i) + beta_i x / 2
    x <- x + delta mu + sqrt(delta) sqrt(1 - lmbd) g_i xi
a is the CDE network, g_i (prior + likelihood) for the Posterior estimator, and for CDiffE the first xdim outputs of
the joint network at y_t = sd_i eps + mw_i y (mw = exp(-B / 2), sd^2 = 1 - exp(-B), B = tau^2 (beta_max - beta_min) / 2
+ tau beta_min; eps fresh normals), after `corrector_steps` Langevin steps
    x <- x + es a(x, y_t, tau_i) / g_i + sqrt(2 es) z,   es = 2 exp(-beta_i delta) snr^2 sd_i^2
Everything is float64 but what the kernels are handed in f32, promoted exactly: the time grid (oracle.schedule), the
generator's normals (oracle.rng_init / rng_normals, drawn in the oracle's order: x0; then per step eps (CDiffE), z per
corrector step, xi), the weights, y, and the f32 scalars mean, std and snr of the C interface.
"""
import numpy as np

import heun_ref as HR
import oracle as O

F32, F64 = np.float32, np.float64


def _f(v):
    return F64(F32(v))


def _start(seed, n, xdim, chain_offset, stream, mean, std):
    st = O.rng_init(seed, np.arange(chain_offset, chain_offset + n), stream)
    return st, O.rng_normals(st, xdim).astype(F64) * _f(std) + _f(mean)


def em_step(x, a, xi, beta, g, delta, lmbd=0.0):
    mu = (1.0 - 0.5 * lmbd) * g * a + 0.5 * beta * x
    return x + delta * mu + np.sqrt(delta) * np.sqrt(1.0 - lmbd) * g * xi


def _em(a_fn, st, x, xdim, num_steps, T, beta_min, beta_max, lmbd):
    tau, beta, g = HR.grid(num_steps, T, F64, beta_min, beta_max)
    delta = T / num_steps
    for i in range(num_steps):
        a = a_fn(x, tau[i], g[i])
        xi = O.rng_normals(st, xdim).astype(F64)  # (drawn at lmbd = 1 too, and multiplied by 0, as the kernels do)
        x = em_step(x, a, xi, beta[i], g[i], delta, lmbd)
    return x


def _net_input(x, y, tau):
    """cat[x, y, tau] (nets.py:32-35), or cat[x, tau] without y (nets.py:52-57); y is (ydim,) or one row per chain."""
    n = x.shape[0]
    cols = [x, np.full((n, 1), tau, F64)]
    if y is not None:
        y = np.asarray(y, F64)
        cols.insert(1, np.broadcast_to(y.reshape(-1, y.shape[-1]), (n, y.shape[-1])))
    return np.concatenate(cols, 1)


def cde_sample(params, y, num_samples, num_steps, seed, mean=0.0, std=1.0, chain_offset=0, stream=0, T=1.0,
               beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, lmbd=0.0):
    xdim = params[-1][0].shape[0]
    st, x = _start(seed, num_samples, xdim, chain_offset, stream, mean, std)
    return _em(lambda x, tau, g: HR.mlp(params, _net_input(x, y, tau)), st, x, xdim, num_steps, T, beta_min, beta_max,
               lmbd)


def posterior_sample(prior_params, lik_params, y, num_samples, num_steps, seed, mean=0.0, std=1.0, chain_offset=0,
                     stream=0, T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, lmbd=0.0):
    xdim = lik_params[-1][0].shape[0]
    st, x = _start(seed, num_samples, xdim, chain_offset, stream, mean, std)

    def a_fn(x, tau, g):
        return g * (HR.mlp(prior_params, _net_input(x, None, tau)) + HR.mlp(lik_params, _net_input(x, y, tau)))

    return _em(a_fn, st, x, xdim, num_steps, T, beta_min, beta_max, lmbd)


def cdiffe_sample(params, y, num_samples, num_steps, seed, mean=0.0, std=1.0, chain_offset=0, stream=0, T=1.0,
                  beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, corrector_steps=0, snr=0.16):
    y = np.asarray(y, F64).reshape(1, -1)
    ydim = y.shape[1]
    xdim = params[0][0].shape[1] - ydim - 1
    st, x = _start(seed, num_samples, xdim, chain_offset, stream, mean, std)
    tau, beta, g = HR.grid(num_steps, T, F64, beta_min, beta_max)
    delta = T / num_steps
    for i in range(num_steps):
        B = 0.5 * tau[i] * tau[i] * (beta_max - beta_min) + tau[i] * beta_min
        mw, var = np.exp(-0.5 * B), -np.expm1(-B)
        y_t = O.rng_normals(st, ydim).astype(F64) * np.sqrt(var) + mw * y
        a_fn = lambda x: HR.mlp(params, _net_input(x, y_t, tau[i]))[:, :xdim]  # noqa: E731
        for _ in range(corrector_steps):
            sc = a_fn(x) / g[i]
            z = O.rng_normals(st, xdim).astype(F64)
            es = 2.0 * np.exp(-beta[i] * delta) * _f(snr) ** 2 * var
            x = x + es * sc + np.sqrt(2.0 * es) * z
        a = a_fn(x)
        xi = O.rng_normals(st, xdim).astype(F64)
        x = em_step(x, a, xi, beta[i], g[i], delta)
    return x
