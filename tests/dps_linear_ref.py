"""The guided sampler for linear-Gaussian problems (estimators.LinearDPS, dmip_dps_linear_sample) restated in numpy:
in float64 (the reference of the accuracy gate and of the moment tests) and in float32 in the kernel's rounding order
with f32 forward tangents (the f32 side of the gate). A plain module; nothing here touches the device or the package.

Scheme, per chain and step i of the samplers' reverse grid (tau_i = T - linspace_f32(S)[i] T, delta = T / S,
beta_i = beta_min + (beta_max - beta_min) tau_i, g_i = sqrt(beta_i), alpha_i = exp(-Bt / 2), v_i = 1 - exp(-Bt) with
Bt = tau_i^2 (beta_max - beta_min) / 2 + tau_i beta_min):
    s, J = prior(x, tau_i), J[k][n] = ds_k/dx_n
    x0h  = (x + v_i s) / alpha_i
    r    = y' - A x0h,  y' = y - b
    u    = B_i^T r
    G    = -(u + v_i J^T u) / alpha_i
    x   <- x + delta (g_i^2 s + beta_i x / 2) + sqrt(delta) g_i xi - lam_i G
with the table and step rule of the guidance:
    'pigdm'  B_i = (Sigma + v_i A A^T)^-1 A,  lam_i = zeta delta beta_i
    'nll'    B   = Sigma^-1 A,                lam_i = zeta delta beta_i
    'norm'   B   = 2 A,                       lam_i = zeta / sqrt(max(|r|^2, 1e-30))
RNG: the chain's stream (seed, chain_offset + row, y index); x0 = mean + std n from its first D normals, then one draw
of D normals per step. Shared inputs of the two restatements and the kernel: the f32 time grid, the normals, the f32
table (built here in float64, rounded once), the f32 A and y', the weights, and the f32 scalars mean, std, zeta.
"""
import numpy as np

import oracle as O

F32, F64 = np.float32, np.float64
GUIDANCES = ("pigdm", "nll", "norm")
STEP_BETA, STEP_NORM = 0, 1


# ------------------------------------------------------------------------------------------ the table
def var64(tau, beta_min, beta_max):
    tau = np.asarray(tau, F64)
    return 1.0 - np.exp(-(0.5 * tau * tau * (beta_max - beta_min) + tau * beta_min))


def table64(A, Sigma, guidance, num_steps, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, T=1.0):
    """(B [n_B][M][D] float64, step rule): written from the formulas above with explicit inverses, independently of
    the package's builder."""
    A = np.asarray(A, F64)
    Sigma = np.asarray(Sigma, F64)
    if guidance == "norm":
        return (A + A).reshape((1,) + A.shape), STEP_NORM
    if guidance == "nll":
        return (np.linalg.inv(Sigma) @ A).reshape((1,) + A.shape), STEP_BETA
    assert guidance == "pigdm"
    _, tau = O.schedule(num_steps, T)
    out = np.empty((num_steps,) + A.shape, F64)
    for i in range(num_steps):
        out[i] = np.linalg.inv(Sigma + var64(tau[i], beta_min, beta_max) * (A @ A.T)) @ A
    return out, STEP_BETA


def sigma_matrix(Sigma, M):
    S = np.asarray(Sigma, F64)
    return S * np.eye(M) if S.ndim == 0 else (np.diag(S) if S.ndim == 1 else S)


# ------------------------------------------------------------------------------------------ the crafted network
EPS = 2.0 ** -9


def crafted_params(W, n_hidden, D, eps=EPS):
    """An MLP2 (x, t) -> x that computes s = -x up to the tanh chain's cubic term: layer 1 has weight eps on D identity
    units (zero t column, zero biases, zero elsewhere), the hidden layers are the identity on those units, the output
    layer is -1 / eps on them. eps is a power of two, so every weight is exact in f32 and in the fp16 split."""
    params = []
    W1 = np.zeros((W, D + 1), F32)
    W1[np.arange(D), np.arange(D)] = eps
    params.append((W1, np.zeros(W, F32)))
    for _ in range(n_hidden - 1):
        Wh = np.zeros((W, W), F32)
        Wh[np.arange(D), np.arange(D)] = 1.0
        params.append((Wh, np.zeros(W, F32)))
    Wo = np.zeros((D, W), F32)
    Wo[np.arange(D), np.arange(D)] = -1.0 / eps
    params.append((Wo, np.zeros(D, F32)))
    return params


def load_params(net, params):
    """Copy [(W, b), ...] into a package MLP2 (in place)."""
    import torch
    with torch.no_grad():
        for (w, b), (W, B) in zip(net.linear_layers(), params):
            w.copy_(torch.from_numpy(np.asarray(W, F32)))
            b.copy_(torch.from_numpy(np.asarray(B, F32)))
    return net


# ------------------------------------------------------------------------------------------ the network and its Jacobian
def jet(params, x, tau, dtype=F64, forward=None):
    """s (n, D) and J (n, D, D), J[:, k, n] = ds_k/dx_n, by forward tangents with every product in `dtype`; the
    activation derivative is formed from the rounded activations, (1 - t2^2)(1 - t1^2) on layer 1, as the kernels do.
    `forward(params, inp)` replaces the primal network (the split engine's emulation); the tangents stay `dtype`."""
    x = np.asarray(x, dtype)
    n, d = x.shape
    inp = np.concatenate([x, np.full((n, 1), tau, dtype)], 1)
    Ws = [np.asarray(p[0], dtype) for p in params]
    bs = [np.asarray(p[1], dtype) for p in params]
    one = dtype(1.0)
    z = (inp @ Ws[0].T + bs[0]).astype(dtype)
    t1 = np.tanh(z).astype(dtype)
    h = np.tanh(t1).astype(dtype)
    d1 = ((one - h * h).astype(dtype) * (one - t1 * t1).astype(dtype)).astype(dtype)
    dh = (d1[:, None, :] * Ws[0].T[None, :d, :]).astype(dtype)  # (n, d, W): tangent k of every unit
    for l in range(1, len(Ws) - 1):
        z = (h @ Ws[l].T + bs[l]).astype(dtype)
        dz = (dh.reshape(n * d, -1) @ Ws[l].T).astype(dtype).reshape(n, d, -1)
        h = np.tanh(z).astype(dtype)
        dh = ((one - h * h).astype(dtype)[:, None, :] * dz).astype(dtype)
    s = (h @ Ws[-1].T + bs[-1]).astype(dtype)
    J = (dh.reshape(n * d, -1) @ Ws[-1].T).astype(dtype).reshape(n, d, -1).transpose(0, 2, 1)  # J[:, k, n]
    if forward is not None:
        s = np.asarray(forward(params, inp.astype(F32)), dtype)
    return s, J


def exact_score(params, x, tau, dtype=F64, forward=None):
    """The exact prior score of N(0, I): s = -x, J = -I (the method's own test needs no network)."""
    x = np.asarray(x, dtype)
    n, d = x.shape
    return -x, np.broadcast_to(-np.eye(d, dtype=dtype), (n, d, d))


# ------------------------------------------------------------------------------------------ the sampler
def guidance(x, s, J, A, Bi, yres, mw, var):
    """(G, |r|^2) of one step in float64: the formulas above, vectorised over chains."""
    x0h = (x + var * s) / mw
    r = yres[None, :] - x0h @ A.T
    u = r @ Bi
    G = -(u + var * np.einsum("nik,ni->nk", J, u)) / mw
    return G, (r * r).sum(1)


def _sample64(score, params, A32, B32, rule, yres32, n, S, seed, zeta, mean, std, chain_offset, stream, T, bmin, bmax):
    st = O.rng_init(seed, np.arange(chain_offset, chain_offset + n), stream)
    D = A32.shape[1]
    x = O.rng_normals(st, D).astype(F64) * F64(F32(std)) + F64(F32(mean))
    _, tau = O.schedule(S, T)
    tau = tau.astype(F64)
    delta = T / S
    A, B, yres, zeta = A32.astype(F64), B32.astype(F64), yres32.astype(F64), F64(F32(zeta))
    for i in range(S):
        beta = bmin + (bmax - bmin) * tau[i]
        g = np.sqrt(beta)
        Bt = 0.5 * tau[i] * tau[i] * (bmax - bmin) + tau[i] * bmin
        mw, var = np.exp(-0.5 * Bt), 1.0 - np.exp(-Bt)
        s, J = score(params, x, tau[i], F64)
        G, rr = guidance(x, s, J, A, B[0 if B.shape[0] == 1 else i], yres, mw, var)
        lam = np.full(n, zeta * delta * beta) if rule == STEP_BETA else zeta / np.sqrt(np.maximum(rr, 1e-30))
        xi = O.rng_normals(st, D).astype(F64)
        x = x + delta * (g * (g * s) + 0.5 * beta * x) + np.sqrt(delta) * g * xi - lam[:, None] * G
    return x


def _sample32(score, params, A, B, rule, yres, n, S, seed, zeta, mean, std, chain_offset, stream, T, bmin, bmax,
              forward=None):
    """The kernel's order (csrc/dmip_flow_rows.h dps_linear_rows): every product and sum rounded to f32, sums over the
    measurement index first to last, the oracle's em_step, then x = fl(xe - fl(lam G))."""
    st = O.rng_init(seed, np.arange(chain_offset, chain_offset + n), stream)
    M, D = A.shape
    x = (O.rng_normals(st, D) * F32(std) + F32(mean)).astype(F32)
    _, tau = O.schedule(S, T)
    delta = float(T) / S
    d32, zeta = F32(delta), F32(zeta)
    f = lambda v: np.asarray(v, F32)
    for i in range(S):
        beta = O.vp_beta(tau[i], bmin, bmax)
        g = np.sqrt(beta).astype(F32)
        mw = F32(O.vp_mean_weight(tau[i], bmin, bmax))
        var = F32(O.vp_var(tau[i], bmin, bmax))
        s, J = score(params, x, tau[i], F32, forward)
        s, J = f(s), f(J)
        x0h = f(f(x + f(var * s)) / mw)
        Bi = B[0 if B.shape[0] == 1 else i]
        u = np.zeros((n, D), F32)
        rr = np.zeros(n, F32)
        for q in range(M):
            ax = f(A[q, 0] * x0h[:, 0])
            for k in range(1, D):
                ax = f(ax + f(A[q, k] * x0h[:, k]))
            r = f(yres[q] - ax)
            rr = f(rr + f(r * r))
            for k in range(D):
                u[:, k] = f(u[:, k] + f(Bi[q, k] * r))
        if rule == STEP_BETA:
            lam = np.full(n, f(f(zeta * d32) * beta), F32)
        else:
            lam = f(zeta / np.sqrt(np.maximum(rr, F32(1e-30))).astype(F32))
        xi = O.rng_normals(st, D)
        xe = O.em_step(x, f(g * s), tau[i], delta, bmin, bmax, xi)
        xn = np.empty_like(x)
        for k in range(D):
            jt = u[:, k].copy()
            for r_ in range(D):
                jt = f(jt + f(f(var * J[:, r_, k]) * u[:, r_]))
            G = f(-f(jt / mw))
            xn[:, k] = f(xe[:, k] - f(lam * G))
        x = xn
    return x


def sample(params, A, b, Sigma, y, num_samples, num_steps, seed, guidance="pigdm", zeta=1.0, dtype=F64, mean=0.0,
           std=1.0, chain_offset=0, stream=0, T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, score=jet, forward=None):
    """The chains of one observation y (M,) (RNG stream `stream`: its y index) in `dtype`."""
    A = np.asarray(A, F64)
    M = A.shape[0]
    B64, rule = table64(A, sigma_matrix(Sigma, M), guidance, num_steps, beta_min, beta_max, T)
    yres = (np.asarray(y, F64).reshape(-1) - (0.0 if b is None else np.asarray(b, F64).reshape(-1))).astype(F32)
    args = (score, params, A.astype(F32), B64.astype(F32), rule, yres, num_samples, num_steps, seed, zeta, mean, std,
            chain_offset, stream, float(T), float(beta_min), float(beta_max))
    if dtype == F64:
        assert forward is None
        return _sample64(*args)
    return _sample32(*args, forward=forward)


def moments(x):
    x = np.asarray(x, F64)
    return x.mean(0), np.cov(x.T)


def moment_errors(x, post_mean, post_cov):
    """(max-abs mean error, max-abs covariance error) of chains against a Gaussian posterior."""
    m, c = moments(x)
    return float(np.abs(m - np.asarray(post_mean, F64)).max()), float(np.abs(c - np.asarray(post_cov, F64)).max())
