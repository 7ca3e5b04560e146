"""Reference data of the lambda family of reverse processes and of the probability-flow log-likelihood.

Runs where the reference checkout is (make_golden.py's import recipe); writes two fixtures beside this file:

  flow_lmbd.npz  the reference's sampling loop body (models/diffusion.py:38-42) driven with
                 sde.mu(..., lmbd) and sde.sigma(..., lmbd) (sdes.py:77-87) for lmbd in {0.5, 1.0}: x0, the per-step
                 normals and the final state for ckpt_lin (n = 32; S = 200 and S = 10) and ckpt_scat (n = 16,
                 S = 10), and one step's network output, mu and sigma tensors (they pin the rounding order).
  flow_logp.npz  log p(x | y) by Heun's explicit trapezoid along the probability-flow ODE, evaluated through the
                 reference's sde.mu(T - tau, x, y, lmbd=1.) with the divergence by autograd: logp_f64 / latent_f64
                 from the networks cast to double, logp_f32_cpu / latent_f32_cpu from the same evaluation in f32
                 (the yardstick of f32 rounding). Cases: (a) ckpt_lin, y_test[0], 37 rows from the analytic
                 posterior, S = 20; (b) ckpt_scat, 50 rows near x_test[0], S = 10; (c) ckpt_lin on the 48 x 48
                 grid of half-width 3 around the posterior mean, S = 50, with the grid integral of exp(logp);
                 (d) a Posterior pair (prior ckpt_prior_scat, likelihood seeded as G10), 21 rows over 2 ys, S = 6.

    python tests/golden/make_golden_flow.py
"""
import math
import os

import numpy as np

from make_golden import OUT, import_reference, load_state, make_cde, y_of


def linspace_times(S, T, dtype):
    import torch
    return (torch.linspace(0, 1, S + 1) * T).to(dtype)  # the f32 grid of the sampler's schedule, in both precisions


def gen_lmbd(R):
    import torch
    out = {}
    for tag, n, S, seed in (("lin", 32, 200, 91), ("lin", 32, 10, 92), ("scat", 16, 10, 93)):
        m = make_cde(R, tag)
        sde = m.sde
        y = y_of(tag)
        key = f"{tag}_S{S}"
        torch.manual_seed(seed)
        x0 = torch.randn(n, m.xdim)
        xi = torch.stack([torch.randn(n, m.xdim) for _ in range(S)])
        out.update({f"{key}_y": y.numpy(), f"{key}_x0": x0.numpy(), f"{key}_xi": xi.numpy()})
        ys = torch.zeros(n, m.ydim) + y
        delta = sde.T / S
        ts = torch.linspace(0, 1, S + 1) * sde.T
        ones = torch.ones(n, 1)
        probe = 3  # the step whose mu / sigma are kept
        for lmbd in (0.5, 1.0):
            x = x0
            with torch.no_grad():
                for i in range(S):  # models/diffusion.py:38-42
                    mu = sde.mu(ones * ts[i], x, ys, lmbd=lmbd)
                    sigma = sde.sigma(ones * ts[i], x, lmbd=lmbd)
                    if i == probe:
                        lk = f"{key}_l{lmbd}"
                        out.update({f"{lk}_step_x": x.numpy().copy(), f"{lk}_step_mu": mu.numpy().copy(),
                                    f"{lk}_step_sigma": sigma.numpy().copy(),
                                    f"{lk}_step_a": sde.a(x, ys, sde.T - ones * ts[i]).numpy().copy(),
                                    f"{lk}_step_tau": (sde.T - ones * ts[i]).numpy()[0, 0]})
                    x = x + delta * mu + delta ** 0.5 * sigma * xi[i]
            out[f"{key}_l{lmbd}_final"] = x.numpy().copy()
        out[f"{key}_probe"] = probe
    np.savez(os.path.join(OUT, "flow_lmbd.npz"), **out)
    print("flow_lmbd:", {k: v.shape for k, v in out.items() if hasattr(v, "shape") and v.ndim})


def heun_logp(sde, x, y, S, dtype):
    """The scheme of include/dmip.h dmip_flow_logp through the reference's drift: v = -mu(T - tau, x, y, lmbd = 1),
    div v by autograd (one backward per dimension); I accumulated in float64."""
    import torch
    x = x.to(dtype)
    n, d = x.shape
    ys = (torch.zeros(n, y.shape[-1]) + y).to(dtype)
    T = sde.T
    tau = linspace_times(S, T, dtype)
    h = T / S
    ones = torch.ones(n, 1, dtype=dtype)

    def v_div(xx, tk):
        xx = xx.detach().requires_grad_(True)
        with torch.enable_grad():
            v = -sde.mu(ones * (T - tk), xx, ys, lmbd=1.)
            div = sum(torch.autograd.grad(v[:, i].sum(), xx, retain_graph=i + 1 < d)[0][:, i] for i in range(d))
        return v.detach(), div.detach()

    I = torch.zeros(n, dtype=torch.float64)
    for k in range(S):
        k1, d1 = v_div(x, tau[k])
        xt = x + h * k1
        k2, d2 = v_div(xt, tau[k + 1])
        x = x + (h / 2) * (k1 + k2)
        I += (h / 2) * (d1.double() + d2.double())
    xs = x.double()
    return (-0.5 * d * math.log(2 * math.pi) - 0.5 * (xs * xs).sum(1) + I).numpy(), x.numpy()


def both(sde, x, y, S):
    """(logp_f64, latent_f64, logp_f32_cpu, latent_f32_cpu)"""
    import torch
    l32, z32 = heun_logp(sde, x, y, S, torch.float32)
    sde.double()
    l64, z64 = heun_logp(sde, x, y, S, torch.float64)
    sde.float()
    print("   e_cpu = max |logp_f32 - logp_f64| =", np.abs(l32 - l64).max(), " latent:", np.abs(z32 - z64).max())
    return l64, z64, l32.astype(np.float64), z32


def gen_logp(R):
    import torch
    out = {}
    lin = make_cde(R, "lin")
    y = y_of("lin")
    post = R.linear_problem.LinearForwardProblem().get_posterior(y, device="cpu")
    g = torch.Generator().manual_seed(61)
    mean, cov = post.mean.float(), post.covariance_matrix.float()
    xa = mean + torch.randn(37, 2, generator=g) @ torch.linalg.cholesky(cov).T
    print("(a) ckpt_lin, 37 rows, S = 20")
    l64, z64, l32, z32 = both(lin.sde, xa, y, 20)
    out.update(a_x=xa.numpy(), a_y=y.numpy(), a_S=20, a_logp_f64=l64, a_latent_f64=z64, a_logp_f32_cpu=l32,
               a_latent_f32_cpu=z32)

    scat = make_cde(R, "scat")
    ysc = y_of("scat")
    x_test0 = torch.from_numpy(np.load(os.path.join(OUT, "data_scat.npz"))["x_test"][0])
    xb = x_test0 + 0.05 * torch.randn(50, 3, generator=g)
    print("(b) ckpt_scat, 50 rows, S = 10")
    l64, z64, l32, z32 = both(scat.sde, xb, ysc, 10)
    out.update(b_x=xb.numpy(), b_y=ysc.numpy(), b_S=10, b_logp_f64=l64, b_latent_f64=z64, b_logp_f32_cpu=l32,
               b_latent_f32_cpu=z32)

    G, half = 48, 3.0
    ax = (torch.arange(G, dtype=torch.float32) + 0.5) / G * 2 * half - half  # cell centres
    gx, gy = torch.meshgrid(ax, ax, indexing="ij")
    xc = torch.stack([gx.reshape(-1), gy.reshape(-1)], 1) + mean
    cell = (2 * half / G) ** 2
    print("(c) ckpt_lin, 48 x 48 grid, S = 50")
    l64, z64, l32, z32 = both(lin.sde, xc, y, 50)
    out.update(c_x=xc.numpy(), c_y=y.numpy(), c_S=50, c_cell=cell, c_logp_f64=l64, c_logp_f32_cpu=l32,
               c_integral=float(np.exp(l64).sum() * cell))
    print("   grid integral", out["c_integral"])

    torch.manual_seed(41)  # G10's seeding of the likelihood network (make_golden.gen_posterior_loss)
    pm = R.diffusion.PosteriorDiffusionEstimator(3, 23, [256] * 3)
    load_state(pm.sde.a.prior_net, os.path.join(OUT, "ckpt_prior_scat.npz"))
    lik = np.load(os.path.join(OUT, "posterior_loss.npz"))
    for k, v in pm.sde.a.likelihood_net.state_dict().items():
        assert np.array_equal(v.numpy(), lik["lik_" + k.replace(".", "_")]), "G10 seeding drifted"
    ys2 = torch.from_numpy(np.load(os.path.join(OUT, "data_scat.npz"))["y_test"][:2])
    xd = torch.rand(2, 21, 3, generator=g) * 2 - 1
    print("(d) Posterior pair, 21 rows x 2 ys, S = 6")
    res = [both(pm.sde, xd[i], ys2[i], 6) for i in range(2)]
    out.update(d_x=xd.numpy(), d_y=ys2.numpy(), d_S=6, d_logp_f64=np.stack([r[0] for r in res]),
               d_latent_f64=np.stack([r[1] for r in res]), d_logp_f32_cpu=np.stack([r[2] for r in res]),
               d_latent_f32_cpu=np.stack([r[3] for r in res]))
    np.savez(os.path.join(OUT, "flow_logp.npz"), **out)


def main():
    import torch
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    R = import_reference()
    gen_lmbd(R)
    gen_logp(R)


if __name__ == "__main__":
    main()
