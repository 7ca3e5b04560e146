"""LinearDPS's Tweedie-covariance guidance (guidance='tweedie', dmip_dps_tweedie_sample) restated in numpy: in float64
(the reference of the accuracy gate and of the moment tests) and in float32 in the kernel's rounding order, with the
adjugate solve written out product by product. A plain module beside dps_linear_ref (its RNG, schedule, network jet and
moment helpers are used as they are); nothing here touches the device or the package.

Scheme, per chain and step i, in dps_linear_ref's notation (alpha_i, v_i, beta_i, g_i, delta):
    s, J = prior(x, tau_i), J[k][n] = ds_k/dx_n
    x0h  = (x + v_i s) / alpha_i;  r = y' - A x0h;  w = B^T r            B = Sigma^-1 A
    K    = I + v_i J;  C = (v_i / alpha_i^2) K                           Cov[x0 | x_tau], Tweedie's second-order formula
    solve (I + H C) u = w                                                H = A^T Sigma^-1 A
    G    = -(u + v_i J^T u) / alpha_i
    x   <- x + delta (g_i^2 s + beta_i x / 2) + sqrt(delta) g_i xi - zeta delta beta_i G
Shared inputs of the two restatements and the kernel: the f32 time grid, the normals, the f32 B and H (built here in
float64 with explicit inverses, rounded once), the f32 A and y', the weights, and the f32 scalars mean, std, zeta.
"""
import numpy as np

import dps_linear_ref as R
import oracle as O

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------ the table
def table64(A, Sigma):
    """(B [M][D], H [D][D]) in float64 from the formulas above with explicit inverses, independently of the package's
    builder (which solves)."""
    A = np.asarray(A, F64)
    Sinv = np.linalg.inv(np.asarray(Sigma, F64))
    return Sinv @ A, A.T @ Sinv @ A


# ------------------------------------------------------------------------------------------ an exact Gaussian prior
def gauss_score(m, P, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX):
    """The score of x_tau for x0 ~ N(m, P): s = -(alpha^2 P + v I)^-1 (x - alpha m), J = -(alpha^2 P + v I)^-1, with the
    signature of dps_linear_ref.jet (no network is involved)."""
    m, P = np.asarray(m, F64), np.asarray(P, F64)

    def score(params, x, tau, dtype=F64, forward=None):
        Bt = 0.5 * float(tau) ** 2 * (beta_max - beta_min) + float(tau) * beta_min
        a, v = np.exp(-0.5 * Bt), 1.0 - np.exp(-Bt)
        Sinv = np.linalg.inv(a * a * P + v * np.eye(len(m)))
        x = np.asarray(x, F64)
        s = -(x - a * m) @ Sinv.T
        return s.astype(dtype), np.broadcast_to(-Sinv, (x.shape[0],) + Sinv.shape).astype(dtype)

    return score


# ------------------------------------------------------------------------------------------ the sampler
def guidance(x, s, J, A, B, H, yres, mw, var):
    """G of one step in float64: the formulas above, vectorised over chains (a general solve, not the adjugate)."""
    D = A.shape[1]
    x0h = (x + var * s) / mw
    r = yres[None, :] - x0h @ A.T
    w = r @ B
    C = (var / (mw * mw)) * (np.eye(D)[None] + var * J)
    Mx = np.eye(D)[None] + np.einsum("ij,njk->nik", H, C)
    u = np.linalg.solve(Mx, w[..., None])[..., 0]
    return -(u + var * np.einsum("nik,ni->nk", J, u)) / mw


def _sample64(score, params, A32, B32, H32, yres32, n, S, seed, zeta, mean, std, chain_offset, stream, T, bmin, bmax):
    st = O.rng_init(seed, np.arange(chain_offset, chain_offset + n), stream)
    D = A32.shape[1]
    x = O.rng_normals(st, D).astype(F64) * F64(F32(std)) + F64(F32(mean))
    _, tau = O.schedule(S, T)
    tau = tau.astype(F64)
    delta = T / S
    A, B, H, yres, zeta = A32.astype(F64), B32.astype(F64), H32.astype(F64), yres32.astype(F64), F64(F32(zeta))
    with np.errstate(all="ignore"):  # (a diverging chain ends non-finite, as on the device)
        for i in range(S):
            beta = bmin + (bmax - bmin) * tau[i]
            g = np.sqrt(beta)
            Bt = 0.5 * tau[i] * tau[i] * (bmax - bmin) + tau[i] * bmin
            mw, var = np.exp(-0.5 * Bt), 1.0 - np.exp(-Bt)
            s, J = score(params, x, tau[i], F64)
            G = guidance(x, s, J, A, B, H, yres, mw, var)
            xi = O.rng_normals(st, D).astype(F64)
            x = x + delta * (g * (g * s) + 0.5 * beta * x) + np.sqrt(delta) * g * xi - (zeta * delta * beta) * G
    return x


def solve32(Mx, w):
    """u = adj(Mx) w / det(Mx) in f32, every product and sum rounded, in the order of csrc/dmip_flow_rows.h
    tweedie_solve. Mx (n, D, D), w (n, D), D = 2 or 3."""
    f = lambda v: np.asarray(v, F32)
    D = w.shape[1]
    m = lambda i, j: Mx[:, i, j]
    u = np.empty_like(w)
    if D == 2:
        det = f(f(m(0, 0) * m(1, 1)) - f(m(0, 1) * m(1, 0)))
        u[:, 0] = f(f(f(m(1, 1) * w[:, 0]) - f(m(0, 1) * w[:, 1])) / det)
        u[:, 1] = f(f(f(m(0, 0) * w[:, 1]) - f(m(1, 0) * w[:, 0])) / det)
        return u
    assert D == 3
    cof = [[None] * 3 for _ in range(3)]
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            cof[i][j] = f(f(m(i1, j1) * m(i2, j2)) - f(m(i1, j2) * m(i2, j1)))
    det = f(f(f(m(0, 0) * cof[0][0]) + f(m(0, 1) * cof[0][1])) + f(m(0, 2) * cof[0][2]))
    for k in range(3):
        u[:, k] = f(f(f(f(cof[0][k] * w[:, 0]) + f(cof[1][k] * w[:, 1])) + f(cof[2][k] * w[:, 2])) / det)
    return u


def _sample32(score, params, A, B, H, yres, n, S, seed, zeta, mean, std, chain_offset, stream, T, bmin, bmax,
              forward=None):
    """The kernel's order (csrc/dmip_flow_rows.h dps_linear_rows over DpsTweedieChains): dps_linear_ref._sample32 with
    n_B = 1 and the beta step, and between w = B^T r and G
        cs = fl(v / fl(alpha alpha));  Kc[k][n] = fl(cs fl([k == n] + fl(v J[k][n])))
        Mx[k][n] = [k == n] + sum_r fl(H[k][r] Kc[r][n])  (r first to last, each sum rounded);  u = solve32(Mx, w)."""
    st = O.rng_init(seed, np.arange(chain_offset, chain_offset + n), stream)
    M, D = A.shape
    x = (O.rng_normals(st, D) * F32(std) + F32(mean)).astype(F32)
    _, tau = O.schedule(S, T)
    delta = float(T) / S
    d32, zeta = F32(delta), F32(zeta)
    f = lambda v: np.asarray(v, F32)
    eye = np.eye(D, dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(S):
            beta = O.vp_beta(tau[i], bmin, bmax)
            g = np.sqrt(beta).astype(F32)
            mw = F32(O.vp_mean_weight(tau[i], bmin, bmax))
            var = F32(O.vp_var(tau[i], bmin, bmax))
            s, J = score(params, x, tau[i], F32, forward)
            s, J = f(s), f(J)
            x0h = f(f(x + f(var * s)) / mw)
            w = np.zeros((n, D), F32)
            for q in range(M):
                ax = f(A[q, 0] * x0h[:, 0])
                for k in range(1, D):
                    ax = f(ax + f(A[q, k] * x0h[:, k]))
                r = f(yres[q] - ax)
                for k in range(D):
                    w[:, k] = f(w[:, k] + f(B[q, k] * r))
            cs = f(var / f(mw * mw))
            Kc = f(cs * f(eye[None] + f(var * J)))
            Mx = np.empty((n, D, D), F32)
            for k in range(D):
                for c in range(D):
                    a = np.full(n, eye[k, c], F32)
                    for r_ in range(D):
                        a = f(a + f(H[k, r_] * Kc[:, r_, c]))
                    Mx[:, k, c] = a
            u = solve32(Mx, w)
            lam = f(f(zeta * d32) * beta)
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


def sample(params, A, b, Sigma, y, num_samples, num_steps, seed, zeta=1.0, dtype=F64, mean=0.0, std=1.0,
           chain_offset=0, stream=0, T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX, score=R.jet, forward=None):
    """The chains of one observation y (M,) (RNG stream `stream`: its y index) in `dtype`: dps_linear_ref.sample's
    arguments without the guidance."""
    A = np.asarray(A, F64)
    M = A.shape[0]
    B64, H64 = table64(A, R.sigma_matrix(Sigma, M))
    yres = (np.asarray(y, F64).reshape(-1) - (0.0 if b is None else np.asarray(b, F64).reshape(-1))).astype(F32)
    args = (score, params, A.astype(F32), B64.astype(F32), H64.astype(F32), yres, num_samples, num_steps, seed, zeta,
            mean, std, chain_offset, stream, float(T), float(beta_min), float(beta_max))
    if dtype == F64:
        assert forward is None
        return _sample64(*args)
    return _sample32(*args, forward=forward)
