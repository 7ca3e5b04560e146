"""Which C-ABI wrapper each sample_device / sample_trajectory call of CDE and PosteriorDiffusionEstimator ends in
(estimators._fused_launch), by the `_lib.calls` counters: exactly one key rises by one per call. And that
sample_trajectory's final state is sample_device's at the same seed, bit for bit. Width 64, 1 hidden layer, xdim 2,
8 chains, 4 steps. Needs an MI355X: `pytest -m gpu`."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, S, SEED = 8, 4, 777


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _rose(dmip, fn):
    """(fn's result, the `_lib.calls` keys that rose during it with their increments)."""
    before = collections.Counter(dmip._lib.calls)
    out = fn()
    dmip._lib.device_status(torch.device(DEV))
    return out, {k: v - before[k] for k, v in dmip._lib.calls.items() if v != before[k]}


# (solver, lmbd, eta) -> the key of sample_device; of sample_trajectory where it differs
COMBOS = [
    ("euler", 0.0, 0.0, None, "em_sample_snapshots"),  # (None: em_sample / em_sample_posterior by model)
    ("euler", 0.5, 0.0, "em_sample_lmbd", "em_sample_lmbd"),
    ("heun", 0.0, 0.0, "ode_sample", "ode_sample"),
    ("dpm2m", 0.0, 0.0, "multistep_sample", "multistep_sample"),
    ("dpm2m", 0.0, 1.0, "multistep_sde_sample", "multistep_sde_sample"),
    ("ddim", 0.0, 0.0, "multistep_sample", "multistep_sample"),
    ("ddim", 0.0, 1.0, "multistep_sde_sample", "multistep_sde_sample"),
]


@pytest.mark.parametrize("kind", ["cde", "posterior"])
def test_each_call_ends_in_its_entry_point(dmip, kind):
    torch.manual_seed(11)
    m = dmip.CDE(2, 2, [64]) if kind == "cde" else dmip.PosteriorDiffusionEstimator(2, 2, [64])
    euler_key = "em_sample" if kind == "cde" else "em_sample_posterior"
    ys = torch.tensor([[0.5, 1.0], [-0.25, 0.75]], device=DEV)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, N, 2, generator=g).to(DEV)
    noise = torch.randn(S + 1, 2, N, 2, generator=g).to(DEV)
    for solver, lmbd, eta, key, traj_key in COMBOS:
        kw = dict(lmbd=lmbd, solver=solver)
        if eta:
            kw["eta"] = eta
        key = key or euler_key
        x, rose = _rose(dmip, lambda: m.sample_device(ys, N, S, seed=SEED, **kw))
        assert rose == {key: 1}, (kind, kw, rose)
        assert tuple(x.shape) == (2, N, 2) and bool(torch.isfinite(x).all())
        (xt, snaps), rose = _rose(dmip, lambda: m.sample_trajectory(ys, N, S, snapshot_every=2, seed=SEED, **kw))
        assert rose == {traj_key: 1}, (kind, kw, rose)
        assert tuple(snaps.shape) == (2, 2, N, 2) and torch.equal(snaps[-1], xt)
        assert torch.equal(xt, x), (kind, kw, float((xt - x).abs().max()))
        if solver != "euler":  # the chains' start states in place of the generator's
            x, rose = _rose(dmip, lambda: m.sample_device(ys, N, S, seed=SEED, x0=x0, **kw))
            assert rose == {key: 1}, (kind, kw, "x0", rose)
            assert bool(torch.isfinite(x).all())
        elif kind == "cde":  # injected normals: the CDE sampler alone takes them
            x, rose = _rose(dmip, lambda: m.sample_device(ys, N, S, noise=noise, **kw))
            assert rose == {key: 1}, (kind, kw, "noise", rose)
            assert bool(torch.isfinite(x).all())
        else:
            with pytest.raises(ValueError, match="noise injection"):
                m.sample_device(ys, N, S, noise=noise, **kw)


def test_posterior_with_unequal_depths_steps_through_the_network_kernel(dmip):
    """A prior and a likelihood network of different depths have no fused kernel: every solver takes the per-step loop
    (dmip_mlp_forward launches), and no fused wrapper is called."""
    torch.manual_seed(12)
    m = dmip.PosteriorDiffusionEstimator(2, 2, [64])
    m.sde.a.prior_net = dmip.MLP2(2 + 1, 2, [64] * 2, torch.nn.Tanh()).to(DEV)
    ys = torch.tensor([[0.5, 1.0]], device=DEV)
    for solver, lmbd, eta, _, _ in COMBOS:
        kw = dict(lmbd=lmbd, solver=solver, **({"eta": eta} if eta else {}))
        x, rose = _rose(dmip, lambda: m.sample_device(ys, N, S, seed=SEED, **kw))
        assert set(rose) == {"mlp_forward"} and rose["mlp_forward"] >= 2 * S, (kw, rose)
        assert tuple(x.shape) == (1, N, 2) and bool(torch.isfinite(x).all())
