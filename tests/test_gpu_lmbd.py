"""`lmbd` through the fused CDE / Posterior samplers (sdes.py:77-87; dmip_em_sample_lmbd): 0 is the reverse SDE bit
for bit, 1 the deterministic probability-flow ODE. Needs an MI355X: `pytest -m gpu`.

Bounds of the reference-trajectory tests are the project's own for the same engines without lambda
(tests/test_gpu_f32.py G3): 1e-4 max(1, |ref|) at 10 steps and 1e-3 max(1, |ref|) at 200 steps for exact f32, 1e-3 at
both lengths for fp32x3 -- lambda changes only two per-step scalars.
"""
import importlib

import numpy as np
import pytest
import torch

from conftest import state_from_npz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRECS = ["fp32", "fp32x3", "fp16"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _est():
    return importlib.import_module("diffusion-modelling-for-inverse-problems_amd.estimators")


def _raw(t):
    return t.cpu().numpy().view(np.uint32)


def _direct_lmbd(dmip, m, nets, mode, ys, n, S, seed, lmbd, prec):
    """dmip_em_sample_lmbd itself (not through sample_device's lmbd == 0 shortcut to the old entry points)."""
    dev, ysd, sde, out = m._prepare(ys, n, S, nets)
    handles = [net.dmip_handle(dev, m.xdim) for net in nets]
    net, prior = handles[-1], (handles[0] if len(handles) > 1 else None)
    p = _est()._fused_precision(prec, mode, net.width, net.n_hidden, m.xdim, m.ydim, [h.act for h in handles])
    before = dmip._lib.calls.get("em_sample_lmbd", 0)
    dmip._lib.em_sample_lmbd(mode, net, prior, sde, ysd, n, 0, S, 0, 1, seed, lmbd, out, precision=p)
    assert dmip._lib.calls["em_sample_lmbd"] == before + 1
    dmip._lib.device_status(dev)
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("W,xd,yd,n", [(64, 2, 2, 1000), (256, 3, 23, 700), (512, 3, 23, 100)])
def test_cde_lmbd0_is_bit_identical(dmip, W, xd, yd, n, prec):
    """lmbd = 0 through the new entry point equals the existing sampler bitwise (g_mu = g_sig = g)."""
    torch.manual_seed(W)
    m = dmip.CDE(xd, yd, [W] * 3)
    y = torch.randn(1, yd, device=DEV)
    S, seed = 6, 4242
    base = m.sample_device(y, n, S, seed=seed, precision=prec)
    np.testing.assert_array_equal(_raw(m.sample_device(y, n, S, seed=seed, precision=prec, lmbd=0.0)), _raw(base))
    direct = _direct_lmbd(dmip, m, [m.sde.a], dmip._lib.DMIP_SAMPLER_CDE, y, n, S, seed, 0.0, prec)
    np.testing.assert_array_equal(_raw(direct), _raw(base))
    assert np.all(np.isfinite(base.cpu().numpy()))


@pytest.mark.parametrize("prec", PRECS)
def test_posterior_lmbd0_is_bit_identical(dmip, prec):
    torch.manual_seed(7)
    m = dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)
    y = torch.randn(1, 2, device=DEV)
    n, S, seed = 333, 6, 99
    base = m.sample_device(y, n, S, seed=seed, precision=prec)
    np.testing.assert_array_equal(_raw(m.sample_device(y, n, S, seed=seed, precision=prec, lmbd=0.0)), _raw(base))
    sc = m.sde.a
    direct = _direct_lmbd(dmip, m, [sc.prior_net, sc.likelihood_net], dmip._lib.DMIP_SAMPLER_POSTERIOR, y, n, S, seed,
                          0.0, prec)
    np.testing.assert_array_equal(_raw(direct), _raw(base))


def _cde(dmip, golden, tag):
    xd, yd, hl = {"lin": (2, 2, [64] * 3), "scat": (3, 23, [256] * 3)}[tag]
    m = dmip.CDE(xd, yd, hl)
    m.sde.a.load_state_dict(state_from_npz(golden(f"ckpt_{tag}.npz")))
    return m


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("lmbd", [0.5, 1.0])
@pytest.mark.parametrize("key", ["lin_S200", "lin_S10", "scat_S10"])
def test_lmbd_trajectory_matches_reference(dmip, golden, key, lmbd, prec):
    """The reference's loop body driven with sde.mu / sde.sigma at lmbd (flow_lmbd.npz), its x0 and normals
    injected."""
    z = golden("flow_lmbd.npz")
    tag, S = key.split("_S")[0], int(key.split("_S")[1])
    m = _cde(dmip, golden, tag)
    noise = np.concatenate([z[f"{key}_x0"][None], z[f"{key}_xi"]], 0)[:, None]
    n = noise.shape[2]
    out = m.sample_device(torch.from_numpy(z[f"{key}_y"]).to(DEV), n, S, noise=torch.from_numpy(noise).to(DEV),
                          precision=prec, lmbd=lmbd)[0].cpu().numpy()
    ref = z[f"{key}_l{lmbd}_final"]
    err = np.abs(out - ref).max()
    bound = (1e-4 if (prec == "fp32" and S == 10) else 1e-3) * max(1.0, np.abs(ref).max())
    print(f"{key} lmbd={lmbd} {prec}: max |kernel - reference| = {err:.3e} (bound {bound:.1e})")
    assert np.all(np.isfinite(out)) and err < bound, err


@pytest.mark.parametrize("prec", PRECS)
def test_ode_is_deterministic_in_x0(dmip, golden, prec):
    """lmbd = 1 with injected noise: two runs sharing slot 0 (x0) and differing in every other slot are bitwise
    equal; at lmbd = 0.5 they differ."""
    m = _cde(dmip, golden, "lin")
    g = torch.Generator().manual_seed(3)
    n, S = 37, 10
    na = torch.randn(S + 1, 1, n, 2, generator=g)
    nb = torch.randn(S + 1, 1, n, 2, generator=g)
    nb[0] = na[0]
    y = torch.tensor([0.5, 1.0], device=DEV)
    a1 = m.sample_device(y, n, S, noise=na.to(DEV), precision=prec, lmbd=1.0)
    b1 = m.sample_device(y, n, S, noise=nb.to(DEV), precision=prec, lmbd=1.0)
    np.testing.assert_array_equal(_raw(a1), _raw(b1))
    ah = m.sample_device(y, n, S, noise=na.to(DEV), precision=prec, lmbd=0.5)
    bh = m.sample_device(y, n, S, noise=nb.to(DEV), precision=prec, lmbd=0.5)
    assert not np.array_equal(_raw(ah), _raw(bh))
    assert not np.array_equal(_raw(ah), _raw(a1))


@pytest.mark.parametrize("model", ["cde", "posterior"])
def test_ode_shards_are_bit_identical(dmip, golden, model):
    """lmbd = 1, chain_offset splits (0, 13) + (13, 24) equal the unsplit 37 chains bitwise (the RNG consumption
    per chain does not depend on lmbd)."""
    if model == "cde":
        m = _cde(dmip, golden, "lin")
    else:
        torch.manual_seed(11)
        m = dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)
    y = torch.tensor([[0.5, 1.0]], device=DEV)
    S, seed = 8, 2024
    full = m.sample_device(y, 37, S, seed=seed, lmbd=1.0)
    lo = m.sample_device(y, 13, S, seed=seed, chain_offset=0, lmbd=1.0)
    hi = m.sample_device(y, 24, S, seed=seed, chain_offset=13, lmbd=1.0)
    np.testing.assert_array_equal(_raw(torch.cat([lo, hi], 1)), _raw(full))
    # the same x0 as the SDE's chains: after the first step the two differ only by the noise term
    sde = m.sample_device(y, 37, S, seed=seed, lmbd=0.0)
    assert not np.array_equal(_raw(sde), _raw(full))


def test_ode_trajectory_last_snapshot_is_final_state(dmip, golden):
    m = _cde(dmip, golden, "lin")
    y = torch.tensor([0.5, 1.0], device=DEV)
    x, snaps = m.sample_trajectory(y, 50, 20, snapshot_every=5, seed=5, lmbd=1.0)
    assert snaps.shape == (4, 1, 50, 2)
    assert torch.equal(snaps[-1], x)
    np.testing.assert_array_equal(_raw(x), _raw(m.sample_device(y, 50, 20, seed=5, lmbd=1.0)))
    assert not torch.equal(snaps[0], snaps[-1])


def test_forward_takes_lmbd(dmip, golden):
    m = _cde(dmip, golden, "lin")
    torch.manual_seed(1)
    a = m(torch.tensor([0.5, 1.0]), num_samples=64, num_steps=10, lmbd=1.0)
    torch.manual_seed(1)
    b = m.forward(torch.tensor([0.5, 1.0]), num_samples=64, num_steps=10, lmbd=1.0)
    assert a.shape == (64, 2) and np.array_equal(a, b) and np.all(np.isfinite(a))
