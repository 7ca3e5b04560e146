"""Generate tests/golden/sde_params.npz: the REFERENCE at two VP-SDEs that are not its default (0.1, 20, 1).

Like make_golden.py this runs only where the reference is checked out, touches it only through
make_golden.import_reference(), and writes data only. Every model is the reference's CDE(2, 2, [64] * 3) under
torch.manual_seed(0) (weights stored as net_*), with
    cde.sde = PluginReverseSDE(VariancePreservingSDE(beta_min, beta_max, T), cde.sde.a, T)

  A = (beta_min 0.5, beta_max 4.0, T 0.75)      every value exact in f32, T below 1
  B = (beta_min 1.1, beta_max 25.0, T 1.25)     beta_min and beta_max - beta_min inexact in f32, T above 1

Per SDE tag (A, B):
  {tag}_sde                   (beta_min, beta_max, T) float64
  {tag}_{ts,tau,beta,g,mw,var}_{S}, {tag}_delta_{S}   the schedule as G1 (make_golden.gen_schedule) for S in {7, 200}:
                              ts = linspace(0, 1, S + 1) * T (models/diffusion.py:34), tau = T - ts (sdes.py:78)
  {tag}_y, {tag}_z0, {tag}_xi the observation (y_test[0] of data_linear.npz), 64 x 2 standard normals (the reference's
                              torch.randn for x0) and the 10 per-step draws, under torch.manual_seed(140 + i)
  {tag}_l0.0_final            the reference's own forward(y, 64, 10, mean=0.3, std=1.5) (models/diffusion.py:27-46)
  {tag}_l0.5_final, _l1.0_final   its loop body driven with sde.mu / sde.sigma at lmbd (sdes.py:77-87) from x0 = z0
                              (mean 0, std 1), as make_golden_flow.gen_lmbd does at the default
At SDE A (the G5 recipe of make_golden.gen_pinn at this SDE; 256 rows, t = 1e-4 + u (T - 1e-4), captured eps):
  loss_{x,y,t,eps}, dsm_rows, dsm_grad_*, pinn_loss, pinn_<component>, pinn_grad_*
  with pinn = PINNLoss(score_posterior, lam=1e-3, lam2=0.1, pde_loss="FPE", ic_metric="L2", pde_metric="L1").

Usage:  python tests/golden/make_golden_sde.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

SDES = {"A": (0.5, 4.0, 0.75), "B": (1.1, 25.0, 1.25)}
N, S_TRAJ, MEAN, STD = 64, 10, 0.3, 1.5


def make_cde(R, bmin, bmax, T):
    import torch
    torch.manual_seed(0)
    cde = R.diffusion.CDE(2, 2, [64] * 3)
    cde.sde = R.sdes.PluginReverseSDE(R.sdes.VariancePreservingSDE(bmin, bmax, T), cde.sde.a, T)
    return cde


def gen_schedule(cde, tag, out):
    import torch
    sde, T = cde.sde.base_sde, cde.sde.T
    for S in (7, 200):
        ts = torch.linspace(0, 1, S + 1) * T
        tau = T - ts
        out[f"{tag}_ts_{S}"], out[f"{tag}_tau_{S}"] = ts.numpy(), tau.numpy()
        out[f"{tag}_beta_{S}"] = sde.beta(tau).numpy()
        out[f"{tag}_g_{S}"] = sde.g(tau, tau).numpy()
        out[f"{tag}_mw_{S}"] = sde.mean_weight(tau).numpy()
        out[f"{tag}_var_{S}"] = sde.var(tau).numpy()
        out[f"{tag}_delta_{S}"] = np.float64(T / S)


def gen_traj(cde, tag, seed, out):
    import torch
    y = MG.y_of("lin")
    sde, S = cde.sde, S_TRAJ
    torch.manual_seed(seed)
    z0 = torch.randn(N, 2)
    xi = torch.stack([torch.randn(N, 2) for _ in range(S)])
    out.update({f"{tag}_y": y.numpy(), f"{tag}_z0": z0.numpy(), f"{tag}_xi": xi.numpy()})
    torch.manual_seed(seed)
    out[f"{tag}_l0.0_final"] = cde(y, num_samples=N, num_steps=S, mean=MEAN, std=STD)
    ys = torch.zeros(N, 2) + y
    delta = sde.T / S
    ts = torch.linspace(0, 1, S + 1) * sde.T
    ones = torch.ones(N, 1)
    for lmbd in (0.5, 1.0):
        x = z0
        with torch.no_grad():
            for i in range(S):  # models/diffusion.py:38-42
                mu = sde.mu(ones * ts[i], x, ys, lmbd=lmbd)
                sigma = sde.sigma(ones * ts[i], x, lmbd=lmbd)
                x = x + delta * mu + delta ** 0.5 * sigma * xi[i]
        out[f"{tag}_l{lmbd}_final"] = x.numpy().copy()


def gen_loss(R, cde, out):
    import torch
    f = R.linear_problem.LinearForwardProblem()
    T = cde.sde.T
    z = np.load(os.path.join(HERE, "data_linear.npz"))
    g = torch.Generator().manual_seed(15)
    B = 256
    x = torch.from_numpy(z["x_test"][:100]).repeat(3, 1)[:B].clone()
    y = (x @ f.A.T + f.b) + 0.3 * torch.randn(B, 2, generator=g)
    t = (1e-4 + torch.rand(B, 1, generator=g) * (T - 1e-4)).requires_grad_(True)
    eps = torch.randn(B, 2, generator=g)
    out.update({"loss_x": x.numpy(), "loss_y": y.numpy(), "loss_t": t.detach().numpy(), "loss_eps": eps.numpy()})
    sde = cde.sde.base_sde
    std = sde.var(t) ** 0.5
    x_t = eps * std + sde.mean_weight(t) * x  # base_sde.sample with its randn_like captured (sdes.py:37-49)
    gg = sde.g(t, x_t)
    net = cde.sde.a
    lf = R.losses.PINNLoss(f.score_posterior, lam=1e-3, lam2=0.1, pde_loss="FPE", ic_metric="L2", pde_metric="L1")
    loss, info = lf(cde.sde, x, y, x_t, t, eps, std, gg)
    loss.backward(retain_graph=True)
    out["pinn_loss"] = loss.detach().numpy()
    for k, v in info.items():
        out[f"pinn_{k.replace(' ', '_').replace('-', '_')}"] = v.detach().numpy()
    for k, p in net.named_parameters():
        out[f"pinn_grad_{k.replace('.', '_')}"] = p.grad.numpy().copy()
        p.grad = None
    dsm = R.losses.DSMLoss()(net(x_t, y, t) / gg, std, eps)  # models/diffusion.py:83-85
    dsm.mean().backward()
    out["dsm_rows"] = dsm.detach().numpy()
    for k, p in net.named_parameters():
        out[f"dsm_grad_{k.replace('.', '_')}"] = p.grad.numpy().copy()
    print("loss fixture at SDE A: pinn", float(loss), {k: float(v) for k, v in info.items()}, "dsm", float(dsm.mean()))


def main():
    R = MG.import_reference()
    out = {}
    for i, (tag, (bmin, bmax, T)) in enumerate(SDES.items()):
        cde = make_cde(R, bmin, bmax, T)
        out[f"{tag}_sde"] = np.array([bmin, bmax, T], np.float64)
        gen_schedule(cde, tag, out)
        gen_traj(cde, tag, 140 + i, out)
        if tag == "A":
            out.update(MG.state_to_npz_dict(cde.sde.a.state_dict(), "net_"))
            gen_loss(R, cde, out)
    path = os.path.join(HERE, "sde_params.npz")
    np.savez(path, **out)
    print("sde_params.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
