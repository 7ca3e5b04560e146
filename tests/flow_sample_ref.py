"""Numpy restatement of the samples-with-log-density scheme (include/dmip.h dmip_flow_sample,
csrc/dmip_flow_sample.hip), for the tests. A plain module.

The state update is heun_ref's (the Heun sampler of the probability-flow ODE on the reverse grid tau_i, beta_i, g_i,
i = 0..S, delta = T / S), bit for bit in either dtype; beside it, with flow_ref.score_div's exact divergence,
    dm(x, i) = 1/2 g_i sum_j da_j/dx_j (x, y, tau_i) + 1/2 beta_i d
    J += (delta/2) (dm(x_i, i) + dm(x~, i + 1))                                 (float64 sum, 2 S terms)
    log q(x_S | y) = -(d/2) log 2 pi - d log std - 1/2 |(x_0 - mean) / std|^2 - J
(for the Posterior pair a = g_i (likelihood + prior), so score_div's divergence carries g_i already). `dtype`
float64 is the scheme itself; float32 rounds the networks, the state update and dm where the kernel does (J, the base
term and the final sum stay in float64, as in the kernel) and measures what f32 rounding costs. x_0, mean and std are
the f32 values the kernel sees in both.
"""
import numpy as np

import flow_ref as FR
import heun_ref as HR
import oracle as O

F32 = np.float32


def sample_with_logq(params, x0, y, num_steps, prior_params=None, T=1.0, dtype=np.float64, mean=0.0, std=1.0,
                     beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """(x_S (n, d) in dtype, logq (n,) float64) from the start states x0 (n, d) under one observation y."""
    x0 = np.asarray(x0, F32)
    x = x0.astype(dtype)
    n, d = x.shape
    tau, beta, g = HR.grid(num_steps, T, dtype, beta_min, beta_max)
    delta = dtype(T / num_steps)
    half = dtype(dtype(0.5) * delta)
    z = (x0.astype(np.float64) - np.float64(F32(mean))) / np.float64(F32(std))
    J = np.zeros(n, np.float64)

    def slope_div(xx, i):
        a, dv = FR.score_div(params, xx, y, tau[i], g[i], prior_params, dtype)
        dm = (dtype(0.5) * g[i] * dv + dtype(0.5) * beta[i] * dtype(d)).astype(dtype)
        return HR._slope(xx, a, beta[i], g[i], dtype), dm

    for i in range(num_steps):
        k1, d1 = slope_div(x, i)
        xt = (x + (delta * k1).astype(dtype)).astype(dtype)
        k2, d2 = slope_div(xt, i + 1)
        x = (x + (half * (k1 + k2).astype(dtype)).astype(dtype)).astype(dtype)
        J += np.float64(half) * (d1.astype(np.float64) + d2.astype(np.float64))
    base = -0.5 * d * FR.LOG_2PI - d * np.log(np.float64(F32(std))) - 0.5 * (z * z).sum(1)
    return x, base - J
