"""Restatement of the fused Metropolis-adjusted Langevin sampler (dmip_mala_sample, csrc/dmip_surrogate.hip
mala_kernel; the reference's anneal_to_energy with langevin_prop=True, models/SNF.py:250-300, on the energy of
get_interpolated_energy_fun, models/SNF.py:220-231), on the oracle's get_log_posterior with its explicit gradient
(oracle.scat_log_posterior(grad=True)) and the oracle's restatement of the product RNG.

    E_l(x) = l E(x) + (1 - l) |x|^2 / 2,   grad E_l(x) = l grad E(x) + (1 - l) x
    per Metropolis step, from (xx, gg) = (x, grad E_l(x)), L times:
        yy = xx - h gg + c eta;  eta' = (xx - yy + h grad E_l(yy)) / c;  ld += sum_d (eta_d^2 - eta'_d^2) / 2;  xx = yy
    accept iff u < exp(-E_l(xx) + E_l(x) + ld)

dtype float64 is the gate of the tests (the oracle's surrogate is float64 either way: only the scheme's own
arithmetic follows dtype); float32 sizes what f32 rounding of that arithmetic alone does to a path.
Draws: injected (x0 (n, 3), eta (S, L, n, 3), unif (S, n)) or the product RNG keyed (seed, chain_offset + c, stream):
x0 from three words unless given, then per step L x rng_normals(3) and one word for u = (w >> 8) 2^-24."""
import numpy as np

import oracle as O

F32 = np.float32


def interp_energy_grad(params, x, y, lambd, a=0.2, b=0.01, lambd_bd=1000.0):
    x = np.asarray(x, np.float64)
    q = 0.5 * (x ** 2).sum(1)
    if lambd == 0.0:  # the reference's branch: the posterior is not evaluated
        return q, x.copy()
    e, g = O.scat_log_posterior(params, x, y, a, b, lambd_bd, grad=True)
    if lambd == 1.0:
        return e, g
    return lambd * e + (1.0 - lambd) * q, lambd * g + (1.0 - lambd) * x


def mala_sample(params, y, num_steps, stepsize, lang_steps=1, lambd=1.0, a=0.2, b=0.01, lambd_bd=1000.0, x0=None,
                eta=None, unif=None, seed=None, n_chains=None, chain_offset=0, stream=0, dtype=np.float64):
    """Returns (x, E_l(x_S) - E_l(x_0), accepted steps per chain)."""
    T = np.dtype(dtype).type
    s = None
    if eta is None:
        s = O.rng_init(seed, np.arange(chain_offset, chain_offset + n_chains), stream)
    if x0 is None:
        inv = F32(2.0 ** -24)
        x0 = np.stack([((O.rng_next(s) >> np.uint32(8)).astype(F32) * inv * F32(2.0) - F32(1.0)).astype(F32)
                       for _ in range(3)], 1)
    h, c = T(stepsize), T(np.sqrt(2.0 * stepsize))
    eg = lambda v: tuple(np.asarray(t, dtype) for t in interp_energy_grad(params, v, y, lambd, a, b, lambd_bd))
    x = np.asarray(x0, dtype).copy()
    e_cur, g_cur = eg(x)
    e0 = e_cur.copy()
    n_acc = np.zeros(len(x), np.int32)
    for i in range(num_steps):
        xx, gg, ld = x.copy(), g_cur.copy(), np.zeros(len(x), dtype)
        for l in range(lang_steps):
            et = np.asarray(O.rng_normals(s, 3) if eta is None else eta[i, l], dtype)
            yy = xx - h * gg + c * et
            e_y, g_y = eg(yy)
            et_ = (xx - yy + h * g_y) / c
            ld = ld + T(0.5) * (et ** 2 - et_ ** 2).sum(1)
            xx, gg = yy, g_y
        if unif is None:
            u = ((O.rng_next(s) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)
        else:
            u = np.asarray(unif[i], F32)
        with np.errstate(over="ignore", invalid="ignore"):
            acc = u < np.exp(-e_y + e_cur + ld)
        x = np.where(acc[:, None], xx, x)
        g_cur = np.where(acc[:, None], gg, g_cur)
        e_cur = np.where(acc, e_y, e_cur)
        n_acc += acc
    return x, e_cur - e0, n_acc
