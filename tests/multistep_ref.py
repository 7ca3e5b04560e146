"""Numpy restatement of the few-step samplers of the probability-flow ODE, DPM-Solver++(2M) and DDIM (include/dmip.h
dmip_multistep_sample, csrc/dmip_device.h MultistepStep), for the tests. A plain module.

Scheme, on a grid tau_0 = T > tau_1 > ... > tau_{S-1} > tau_S = 0 with alpha, sigma the VP mean weight and std,
lambda = log(alpha / sigma), g = sqrt(beta), h_i = lambda_{i+1} - lambda_i and a = g score (the CDE network, or
g (likelihood + prior) for the Posterior estimator):
    d_i     = (x_i + (sigma_i^2 / g_i) a_i) / alpha_i
    x_{i+1} = (sigma_{i+1} / sigma_i) x_i - alpha_{i+1} expm1(-h_i) D_i        i < S - 1
    D_i     = d_i ("ddim", and step 0) | (1 + 1/(2r)) d_i - (1/(2r)) d_{i-1}, r = h_{i-1} / h_i ("dpm2m")
    x_S     = d_{S-1}
`direct_sample` is that, in float64, from alpha, sigma and lambda of its own grid (`grid`: its own inverse of lambda),
without the table. `table_sample` is the kernels' table-driven update from the package's table
(estimators.multistep_table), d = p x + q a, x' = cx x + c0 d + c1 d_prev: in float64 from the float64 table, or
(dtype float32) from the table rounded once to f32 in the kernels' rounding order,
    d = fl(fl(p x) + fl(q a));   x' = fl(fl(fl(cx x) + fl(c0 d)) + fl(c1 d_prev))
with the network in f32 (heun_ref.mlp) and, for the Posterior estimator, a = fl(g (likelihood + prior)).
Both grids hold the f32 times the network sees.
"""
import numpy as np

import heun_ref as HR
import oracle as O

F32, F64 = np.float32, np.float64
SOLVERS = ("dpm2m", "ddim")


def vp(tau, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """(alpha, sigma, lambda, g) of the VP-SDE at tau, float64."""
    tau = np.asarray(tau, F64)
    B = 0.5 * tau * tau * (beta_max - beta_min) + tau * beta_min
    alpha, sigma = np.exp(-0.5 * B), np.sqrt(-np.expm1(-B))
    return alpha, sigma, np.log(alpha) - np.log(sigma), np.sqrt(beta_min + (beta_max - beta_min) * tau)


def tau_of_lambda(lam, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """The inverse of lambda(tau): alpha^2 = sigmoid(2 lambda), B = -log alpha^2, then the positive root of
    (beta_max - beta_min) tau^2 / 2 + beta_min tau = B."""
    B = np.log1p(np.exp(-2.0 * np.asarray(lam, F64)))
    bd = beta_max - beta_min
    return (np.sqrt(beta_min * beta_min + 2.0 * bd * B) - beta_min) / bd if bd != 0.0 else B / beta_min


def grid(kind, num_steps, T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, t_end=None):
    """tau_0 .. tau_{S-1} as float64 holding f32 values (tau_S = 0 is implied)."""
    S = int(num_steps)
    if kind == "uniform":
        return O.schedule(S, T)[1][:S].astype(F64)
    assert kind == "logsnr", kind
    t_end = 1e-3 * T if t_end is None else t_end
    if S == 1:
        return np.array([T], F32).astype(F64)
    l0, l1 = vp(T, beta_min, beta_max)[2], vp(t_end, beta_min, beta_max)[2]
    tau = tau_of_lambda(l0 + (l1 - l0) * np.arange(S) / (S - 1), beta_min, beta_max)
    tau[0], tau[-1] = T, t_end
    return tau.astype(F32).astype(F64)


def direct_sample(params, x0, y, num_steps, solver="dpm2m", grid_kind="logsnr", prior_params=None, T=1.0,
                  beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, t_end=None, snapshot_every=0, act="tanh"):
    """x_S (n, d) in float64 from x0 (n, d) under one y, straight from alpha, sigma and lambda; with snapshot_every
    also the states after every snapshot_every-th step."""
    assert solver in SOLVERS, solver
    S = int(num_steps)
    tau = grid(grid_kind, S, T, beta_min, beta_max, t_end)
    alpha, sigma, lam, g = vp(tau, beta_min, beta_max)
    x = np.asarray(x0, F64).copy()
    d_prev, snaps = None, []
    for i in range(S):
        a = HR.score(params, x, y, tau[i], g[i], prior_params, F64, act)
        d = (x + (sigma[i] ** 2 / g[i]) * a) / alpha[i]
        if i == S - 1:
            x = d
        else:
            h = lam[i + 1] - lam[i]
            D = d
            if solver == "dpm2m" and i > 0:
                r = (lam[i] - lam[i - 1]) / h
                D = (1.0 + 0.5 / r) * d - (0.5 / r) * d_prev
            x = (sigma[i + 1] / sigma[i]) * x - alpha[i + 1] * np.expm1(-h) * D
        d_prev = d
        if snapshot_every and (i + 1) % snapshot_every == 0:
            snaps.append(x.copy())
    return (x, np.stack(snaps)) if snapshot_every else x


def table_sample(params, x0, y, table, prior_params=None, dtype=F64, snapshot_every=0, act="tanh"):
    """The table-driven update. table (S, 8) float64 (estimators.multistep_table); dtype float32 rounds it once and
    every operation after it, as the kernels do."""
    tab = np.asarray(table, F64).astype(dtype)
    x = np.asarray(x0, dtype).copy()
    d_prev, snaps = np.zeros_like(x), []
    for i, (tau, p, q, cx, c0, c1, g, _) in enumerate(tab):
        a = HR.score(params, x, y, tau, g, prior_params, dtype, act)
        d = ((p * x).astype(dtype) + (q * a).astype(dtype)).astype(dtype)
        x = (((cx * x).astype(dtype) + (c0 * d).astype(dtype)).astype(dtype) + (c1 * d_prev).astype(dtype)).astype(dtype)
        d_prev = d
        if snapshot_every and (i + 1) % snapshot_every == 0:
            snaps.append(x.copy())
    return (x, np.stack(snaps)) if snapshot_every else x


def table_of(dmip, solver, grid_kind, num_steps, T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, t_end=None):
    return dmip.estimators.multistep_table(solver, grid_kind, num_steps, beta_min, beta_max, T, t_end)


# the parity cases of tests/test_gpu_multistep.py: heun_ref.PARITY_CASES at six evaluations
PARITY_STEPS = 6
