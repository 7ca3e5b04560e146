"""Numpy restatement of the stochastic few-step samplers, SDE-DPM-Solver++(2M) and ancestral / eta-DDIM (include/dmip.h
dmip_multistep_sde_sample, csrc/dmip_device.h MultistepStep), for the tests. A plain module beside multistep_ref.py,
whose grid and VP functions it uses.

Scheme, in multistep_ref's notation, with eta >= 0 and xi_i standard normal, for i < S - 1:
    x_{i+1} = (sigma_{i+1} / sigma_i) e^{-eta h_i} x_i + alpha_{i+1} (1 - e^{-(1 + eta) h_i}) D_i
              + sigma_{i+1} sqrt(1 - e^{-2 eta h_i}) xi_i
    D_i     = d_i ("ddim", and step 0) | (1 + 1/(2r)) d_i - (1/(2r)) d_{i-1}, r = h_{i-1} / h_i ("dpm2m")
    x_S     = d_{S-1}
`direct_sample` is that in float64 from alpha, sigma and lambda of its own grid, without the table. `table_sample` is
the kernels' update from the package's table (estimators.multistep_table(eta=)), in float64 or (dtype float32) from
the table rounded once to f32 in the kernels' rounding order, the noise added last:
    d = fl(fl(p x) + fl(q a));   x' = fl(fl(fl(fl(cx x) + fl(c0 d)) + fl(c1 d_prev)) + fl(cn xi))
Both take the per-step normals xi (S, n, d) as an argument (the last step's are unused: cn = 0 there).
`chain_normals` draws them as the kernels do, from the chain's own stream after its x0. `gaussian_stats` is the closed
form of the scheme on data N(0, I), where the exact a is -g x.
"""
import numpy as np

import heun_ref as HR
import multistep_ref as MR
import oracle as O

F32, F64 = np.float32, np.float64
SOLVERS = MR.SOLVERS


def chain_normals(seed, n, xdim, num_steps, chain_offset=0, stream=0, mean=0.0, std=1.0):
    """(x0 (n, d) f32, xi (S, n, d) f32) of chains [chain_offset, chain_offset + n) under y index `stream`, in the order
    the samplers consume their generator (oracle.em_sample(rng_state=)): x0 = std n + mean from the first draw, then
    one draw per step, the last step's included."""
    st = O.rng_init(seed, np.arange(chain_offset, chain_offset + n), stream)
    x0 = (O.rng_normals(st, xdim) * F32(std) + F32(mean)).astype(F32)
    xi = np.stack([O.rng_normals(st, xdim).copy() for _ in range(int(num_steps))])
    return x0, xi


def coefficients(solver, eta, tau, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """(cx, c0, c1, cn), each (S - 1,), of steps 0 .. S - 2 on the grid tau, straight from the scheme (exp, not expm1)."""
    alpha, sigma, lam, _ = MR.vp(tau, beta_min, beta_max)
    h = lam[1:] - lam[:-1]
    cx = sigma[1:] / sigma[:-1] * np.exp(-eta * h)
    E = alpha[1:] * (1.0 - np.exp(-(1.0 + eta) * h))
    cn = sigma[1:] * np.sqrt(1.0 - np.exp(-2.0 * eta * h))
    c0, c1 = E.copy(), np.zeros_like(E)
    if solver == "dpm2m" and len(h) > 1:
        w = 0.5 * h[1:] / h[:-1]
        c0[1:], c1[1:] = E[1:] * (1.0 + w), -E[1:] * w
    return cx, c0, c1, cn


def direct_sample(params, x0, y, num_steps, xi, solver="dpm2m", eta=1.0, grid_kind="logsnr", prior_params=None, T=1.0,
                  beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, t_end=None, snapshot_every=0, act="tanh", score_fn=None):
    """x_S (n, d) in float64 from x0 and the normals xi (S, n, d) under one y; with snapshot_every also the states after
    every snapshot_every-th step. score_fn(x, tau, g) replaces the network's a."""
    assert solver in SOLVERS, solver
    S = int(num_steps)
    tau = MR.grid(grid_kind, S, T, beta_min, beta_max, t_end)
    alpha, sigma, lam, g = MR.vp(tau, beta_min, beta_max)
    x = np.asarray(x0, F64).copy()
    xi = np.asarray(xi, F64)
    d_prev, snaps = None, []
    for i in range(S):
        a = score_fn(x, tau[i], g[i]) if score_fn else HR.score(params, x, y, tau[i], g[i], prior_params, F64, act)
        d = (x + (sigma[i] ** 2 / g[i]) * a) / alpha[i]
        if i == S - 1:
            x = d
        else:
            h = lam[i + 1] - lam[i]
            D = d
            if solver == "dpm2m" and i > 0:
                r = (lam[i] - lam[i - 1]) / h
                D = (1.0 + 0.5 / r) * d - (0.5 / r) * d_prev
            x = (sigma[i + 1] / sigma[i]) * np.exp(-eta * h) * x + alpha[i + 1] * (1.0 - np.exp(-(1.0 + eta) * h)) * D \
                + sigma[i + 1] * np.sqrt(1.0 - np.exp(-2.0 * eta * h)) * xi[i]
        d_prev = d
        if snapshot_every and (i + 1) % snapshot_every == 0:
            snaps.append(x.copy())
    return (x, np.stack(snaps)) if snapshot_every else x


def table_sample(params, x0, y, table, xi, prior_params=None, dtype=F64, snapshot_every=0, act="tanh"):
    """The table-driven update with the noise term. table (S, 8) float64 (estimators.multistep_table(eta=)); dtype
    float32 rounds it once and every operation after it, as the kernels do."""
    tab = np.asarray(table, F64).astype(dtype)
    x = np.asarray(x0, dtype).copy()
    xi = np.asarray(xi, dtype)
    d_prev, snaps = np.zeros_like(x), []
    for i, (tau, p, q, cx, c0, c1, g, cn) in enumerate(tab):
        a = HR.score(params, x, y, tau, g, prior_params, dtype, act)
        d = ((p * x).astype(dtype) + (q * a).astype(dtype)).astype(dtype)
        x = (((cx * x).astype(dtype) + (c0 * d).astype(dtype)).astype(dtype) + (c1 * d_prev).astype(dtype)).astype(dtype)
        x = (x + (cn * xi[i]).astype(dtype)).astype(dtype)
        d_prev = d
        if snapshot_every and (i + 1) % snapshot_every == 0:
            snaps.append(x.copy())
    return (x, np.stack(snaps)) if snapshot_every else x


def table_of(dmip, solver, grid_kind, num_steps, eta, T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, t_end=None):
    return dmip.estimators.multistep_table(solver, grid_kind, num_steps, beta_min, beta_max, T, t_end, eta=eta)


def gaussian_score(x, tau, g):
    """a = g score of data N(0, I) under the VP-SDE: every marginal is N(0, I), so a = -g x and d = alpha x."""
    return -g * x


def gaussian_stats(solver, eta, num_steps, grid_kind="logsnr", T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX,
                   t_end=None):
    """(std(x_S), corr(x_S, x_0)) per coordinate of the scheme on data N(0, I) from x_0 ~ N(0, I), in closed form: with
    d_i = alpha_i x_i the state (x_i, d_{i-1}, x_0) follows
        x_{i+1} = (cx + c0 alpha_i) x_i + c1 d_{i-1} + cn xi_i,   d_i = alpha_i x_i,   x_0 = x_0
    so its covariance goes C -> A C A^T with cn^2 added to the x entry; the last step is x_S = alpha_{S-1} x_{S-1}."""
    S = int(num_steps)
    tau = MR.grid(grid_kind, S, T, beta_min, beta_max, t_end)
    alpha = MR.vp(tau, beta_min, beta_max)[0]
    cx, c0, c1, cn = coefficients(solver, eta, tau, beta_min, beta_max)
    C = np.array([[1.0, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 1.0]])
    for i in range(S - 1):
        A = np.array([[cx[i] + c0[i] * alpha[i], c1[i], 0.0], [alpha[i], 0.0, 0.0], [0.0, 0.0, 1.0]])
        C = A @ C @ A.T
        C[0, 0] += cn[i] ** 2
    var = alpha[-1] ** 2 * C[0, 0]
    cov = alpha[-1] * C[0, 2]
    return float(np.sqrt(var)), float(cov / np.sqrt(var * C[2, 2]))


def sample_stats(x, x0):
    """(sample std (d,), sample corr(x, x0) (d,)) per coordinate: each coordinate is an independent copy of the scalar
    chain with n samples, so each is held to the n-sample standard errors on its own."""
    x, x0 = np.asarray(x, F64), np.asarray(x0, F64)
    return x.std(axis=0), np.array([np.corrcoef(x[:, k], x0[:, k])[0, 1] for k in range(x.shape[1])])


def check_gaussian(x, x0, solver, eta, num_steps, tag=""):
    """Every coordinate's sample std and corr(x_S, x_0) within GAUSS_SE standard errors of the recursion, SE(std) =
    std / sqrt(2 n) and SE(corr) = 1 / sqrt(n); prints the deviations in standard errors first."""
    n = x.shape[0]
    std, corr = gaussian_stats(solver, eta, num_steps)
    s, c = sample_stats(x, x0)
    zs, zc = (s - std) / (std / np.sqrt(2.0 * n)), (c - corr) * np.sqrt(n)
    print(f"{tag}{solver} eta={eta} S={num_steps}: std {s} vs {std:.4f} ({zs} SE), corr {c} vs {corr:.4f} ({zc} SE)")
    assert np.all(np.isfinite(x))
    assert np.all(np.abs(zs) <= GAUSS_SE) and np.all(np.abs(zc) <= GAUSS_SE), (zs, zc)


# the Gaussian statistic's cases (tests/test_multistep_sde_host.py on the reference alone, tests/test_gpu_multistep_sde.py
# on the device): n chains, 4 standard errors, SE(std) = std / sqrt(2 n), SE(corr) = 1 / sqrt(n)
GAUSS_N = 20000
GAUSS_CASES = [(solver, eta, S) for solver in ("ddim", "dpm2m") for eta in (0.5, 1.0) for S in (6, 16)]
GAUSS_SE = 4.0
ETAS = (0.5, 1.0)
PARITY_STEPS = MR.PARITY_STEPS
