"""model.sample_with_log_prob: the fused samples-with-log-density kernel (csrc/dmip_flow_sample.hip,
dmip_flow_sample) against the f64 restatement (tests/flow_sample_ref.py), the Heun sampler, model.log_prob and
itself (seed path / x0 path, shards), and evaluate.importance_posterior. Needs an MI355X: `pytest -m gpu`.

Gate of every accuracy test, for logq and for x: the start states are injected (x0= from heun_ref.x0_of_seed: the
device's Box-Muller normals are only within 2e-5 of the oracle's), and with e_gpu = max |gpu - f64| and e_cpu =
max |f32 restatement - f64| over the same rows, flow_gpu.gate (tests/flow_cases.py derives it):
    e_gpu <= 8 max(e_cpu, 1e-7)
and never above the gate it replaced, 4 e_cpu + 1e-6 max(1, max |f64|), whose additive term was scaled because |logq|
and |x| are not O(1) here (untrained weights grow |x| to 160-195 in four steps) and which let a kernel with a lost
tangent product pass at W 512. One f64 and one f32 run of the restatement per network and y, shared (read-only) by
the cases that slice them.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import flow_ref as FR
import flow_sample_ref as FS
import heun_ref as HR
from conftest import state_from_npz
from flow_gpu import DEV, seeded
from flow_gpu import bits as _bits, dev as _dev, device_x0 as _device_x0, sample_reference as _reference
from flow_gpu import gate as _gate, lin as _lin, scat as _scat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def ev(dmip):
    return importlib.import_module(dmip.__name__ + ".evaluate")


# ------------------------------------------------------------------------------------- fixture checkpoints
@pytest.mark.parametrize("case", ["lin", "scat", "post"])
def test_fixture_checkpoints(dmip, golden, case):
    """ckpt_lin ([64]^3, d = 2, 37 rows, S = 20), ckpt_scat ([256]^3, d = 3, ydim 23, 50 rows, S = 10: the streamed
    ring) and the Posterior pair (ckpt_prior_scat + posterior_loss.npz lik_, 21 rows x 2 ys, S = 6): one flow_sample
    call each (measured e_gpu / e_cpu: DESIGN.md 3f)."""
    z = golden("flow_logp.npz")
    if case == "lin":
        m, ys, n, S, prior = _lin(dmip, golden), z["a_y"][None], 37, 20, None
        params = HR.params_of(m.sde.a)
    elif case == "scat":
        m, ys, n, S, prior = _scat(dmip, golden), z["b_y"][None], 50, 10, None
        params = HR.params_of(m.sde.a)
    else:
        m = dmip.PosteriorDiffusionEstimator(3, 23, [256] * 3)
        m.sde.a.prior_net.load_state_dict(state_from_npz(golden("ckpt_prior_scat.npz")))
        m.sde.a.likelihood_net.load_state_dict(state_from_npz(golden("posterior_loss.npz"), "lik_"))
        ys, n, S = z["d_y"], 21, 6
        params, prior = HR.params_of(m.sde.a.likelihood_net), HR.params_of(m.sde.a.prior_net)
    x0 = np.stack([HR.x0_of_seed(1234, n, m.xdim, stream=i) for i in range(len(ys))])
    before = dmip._lib.calls.get("flow_sample", 0)
    if len(ys) == 1:
        x, logq = m.sample_with_log_prob(_dev(ys[0]), n, S, x0=_dev(x0[0]))
        assert tuple(x.shape) == (n, m.xdim) and tuple(logq.shape) == (n,)
        x, logq = x[None], logq[None]
    else:
        x, logq = m.sample_with_log_prob(_dev(ys), n, S, x0=_dev(x0))
        assert tuple(x.shape) == (len(ys), n, m.xdim) and tuple(logq.shape) == (len(ys), n)
    assert dmip._lib.calls["flow_sample"] == before + 1
    assert x.dtype == logq.dtype == torch.float32 and x.is_cuda and logq.is_cuda
    for i in range(len(ys)):
        (x64, l64), (x32, l32) = _reference(params, x0[i], ys[i], S, prior)
        _gate(f"({case}, y {i}) logq", logq[i].cpu().numpy(), l64, l32)
        _gate(f"({case}, y {i}) x", x[i].cpu().numpy(), x64, x32)


# ------------------------------------------------------------------ seeded networks against the restatement
SHAPES = {  # name: (W, n_hidden, xdim, ydim, rows of the shared reference, S, weight seed)
    "w64": (64, 3, 2, 2, 37, 4, 301),
    "w128": (128, 3, 2, 2, 19, 4, 302),
    "w512x1": (512, 1, 3, 23, 21, 4, 303),
    "w512x3": (512, 3, 3, 23, 21, 4, 304),
}
_refs = {}


def _seeded(dmip, name):
    """(model, x0 (n_y, n, d), ys (3, ydim), S, per-y references) -- computed once per shape and shared, unchanged."""
    W, NL, xd, yd, n, S, seed = SHAPES[name]
    m, params = seeded(dmip, W, NL, xd, yd, seed)
    if name not in _refs:
        ys = np.random.default_rng(seed).normal(size=(3, yd)).astype(np.float32)
        n_y = 3 if name == "w64" else 1
        x0 = np.stack([HR.x0_of_seed(seed, n, xd, stream=i) for i in range(n_y)])
        x0.setflags(write=False)
        _refs[name] = (x0, ys, [_reference(params, x0[i], ys[i], S) for i in range(n_y)])
    x0, ys, ref = _refs[name]
    return m, x0, ys, S, ref


@pytest.mark.parametrize("name,n", [("w64", 1), ("w64", 3), ("w64", 5), ("w64", 17), ("w64", 37), ("w128", 19),
                                    ("w512x1", 21), ("w512x3", 21)])
def test_seeded_networks_and_ragged_rows(dmip, name, n):
    """Every compiled width class and both depths of the wide network (one hidden layer: no streamed hidden tile);
    for W 64 row counts that are no multiple of the 4-row pass. Restatement alone (CPU): max |x| 160-195, e_cpu (x)
    1.3e-5 / 2.0e-5 / 1.7e-5 and e_cpu (logq) 3.4e-7 / 5.4e-7 / 4.1e-7 for w128 / w512x1 / w512x3; w64: max |x| 119,
    e_cpu 1.6e-5 (x) and 3.2e-7 (logq) over the 37 rows, 1.4e-5 and 1.5e-7 on row 0 alone. Measured on the device:
    e_gpu / e_cpu 0.3-3.0 for logq, 1.00 for x."""
    m, x0, ys, S, ref = _seeded(dmip, name)
    (x64, l64), (x32, l32) = ref[0]
    x, logq = m.sample_with_log_prob(_dev(ys[0]), n, S, x0=_dev(x0[0, :n]))
    assert tuple(x.shape) == (n, x0.shape[2]) and tuple(logq.shape) == (n,)
    _gate(f"{name} n={n} logq", logq.cpu().numpy(), l64[:n], l32[:n])
    _gate(f"{name} n={n} x", x.cpu().numpy(), x64[:n], x32[:n])


def test_multi_y(dmip):
    """n_y = 3, a different y each: every y index reads its own layer-1 image and its own rows of x0."""
    m, x0, ys, S, ref = _seeded(dmip, "w64")
    n = 5
    x, logq = m.sample_with_log_prob(_dev(ys), n, S, x0=_dev(x0[:, :n]))
    assert tuple(x.shape) == (3, n, 2) and tuple(logq.shape) == (3, n)
    for i in range(3):
        (x64, l64), (x32, l32) = ref[i]
        _gate(f"multi-y {i} logq", logq[i].cpu().numpy(), l64[:n], l32[:n])
        _gate(f"multi-y {i} x", x[i].cpu().numpy(), x64[:n], x32[:n])
    # the ys do differ: y 1's rows under y 0 are another trajectory
    x01, _ = m.sample_with_log_prob(_dev(ys[0]), n, S, x0=_dev(x0[1, :n]))
    assert np.abs(x01.cpu().numpy() - ref[1][0][0][:n]).max() > 1e-3


# ------------------------------------------------------------------------------------- against the Heun sampler
@pytest.mark.parametrize("case", ["lin", "scat"])
def test_same_x_as_the_heun_sampler(dmip, golden, case):
    """Seed path against sample_device(solver="heun", precision="fp32") at the same seed, 100 rows, S = 8: the same
    HeunStep, engine, weight images and RNG, and an MFMA column does not depend on its neighbours (16 primal
    columns there, 4 primal + 12 tangent columns here). Measured bitwise equal on every case (max |x - x_heun| = 0),
    so equality is asserted, not the 1e-4 max(1, |ref|) bound of the parity tests."""
    m = _lin(dmip, golden) if case == "lin" else _scat(dmip, golden)
    y = _dev(golden("flow_logp.npz")["a_y" if case == "lin" else "b_y"])
    pairs = []
    for seed in (7, 2 ** 40 + 3):
        ref = m.sample_device(y, 100, 8, seed=seed, precision="fp32", solver="heun")[0]
        x, _ = m.sample_with_log_prob(y, 100, 8, seed=seed)
        d = (x - ref).abs().max().item()
        same = bool(np.array_equal(_bits(x), _bits(ref)))
        print(f"({case}, seed {seed}) max |x - x_heun| = {d:.3e}, bitwise {same}, max |ref| = {ref.abs().max().item():.4g}")
        assert torch.isfinite(x).all()
        pairs.append((x, ref))
    for x, ref in pairs:
        np.testing.assert_array_equal(_bits(x), _bits(ref))


# ------------------------------------------------------------------------------------- seed path == x0 path
@pytest.mark.parametrize("case,mean,std", [("lin", 0.0, 1.0), ("lin", 0.3, 1.5), ("scat", 0.0, 1.0)])
def test_seed_path_equals_x0_path(dmip, golden, case, mean, std):
    """The chains' own start states (dmip_rng_normals: the first xdim normals of each chain, times std plus mean)
    passed back as x0= give (x, logq) bit for bit; n_y = 2 (each y its own stream) and mean = 0.3, std = 1.5 (the
    -d log std term and the standardised residual of the base density)."""
    m = _lin(dmip, golden) if case == "lin" else _scat(dmip, golden)
    y = golden("flow_logp.npz")["a_y" if case == "lin" else "b_y"]
    ys = _dev(np.stack([y, 0.5 * y]))
    n, S, seed = 45, 5, 99
    x, logq = m.sample_with_log_prob(ys, n, S, mean=mean, std=std, seed=seed, chain_offset=11)
    x0 = torch.stack([_device_x0(dmip, seed, 11, i, n, m.xdim, mean, std) for i in range(2)])
    x2, logq2 = m.sample_with_log_prob(ys, n, S, mean=mean, std=std, seed=seed + 1, x0=x0)
    assert torch.isfinite(logq).all() and (x[0] - x[1]).abs().max().item() > 1e-3
    np.testing.assert_array_equal(_bits(x2), _bits(x))
    np.testing.assert_array_equal(_bits(logq2), _bits(logq))
    if std != 1.0:
        # the base term: the same x0 declared standard normal differs by the base densities' difference
        _, logq3 = m.sample_with_log_prob(ys, n, S, x0=x0)
        z0 = x0.double()
        z1 = (z0 - float(np.float32(mean))) / float(np.float32(std))
        want = -m.xdim * np.log(float(np.float32(std))) - 0.5 * (z1 * z1).sum(-1) + 0.5 * (z0 * z0).sum(-1)
        got = logq.double() - logq3.double()
        scale = max(1.0, logq.abs().max().item(), logq3.abs().max().item())
        assert (got - want).abs().max().item() <= 4 * 2.0 ** -24 * scale  # two f32 stores of |logq| <= scale


# ------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("path", ["seed", "x0"])
def test_shards_are_bitwise_the_whole_run(dmip, golden, path):
    """Rows 500..800 computed alone (chain_offset = 500, 301 rows) equal those rows of a 1,000-row run, and one row
    alone equals the same row among 37 (quad / column cross-talk in the DPP broadcast or the output shuffles would
    show here)."""
    m = _lin(dmip, golden)
    y = _dev(golden("flow_logp.npz")["a_y"])
    S, seed = 4, 31
    x0 = _device_x0(dmip, 5, 0, 0, 1000, 2) if path == "x0" else None
    x, logq = m.sample_with_log_prob(y, 1000, S, seed=seed, x0=x0)
    xs, ls = m.sample_with_log_prob(y, 301, S, seed=seed, chain_offset=500, x0=None if x0 is None else x0[500:801])
    np.testing.assert_array_equal(_bits(xs), _bits(x[500:801]))
    np.testing.assert_array_equal(_bits(ls), _bits(logq[500:801]))
    x37, l37 = m.sample_with_log_prob(y, 37, S, seed=seed, x0=None if x0 is None else x0[:37])
    np.testing.assert_array_equal(_bits(x37), _bits(x[:37]))
    for r in (0, 3, 4, 16, 36):
        x1, l1 = m.sample_with_log_prob(y, 1, S, seed=seed, chain_offset=r, x0=None if x0 is None else x0[r:r + 1])
        np.testing.assert_array_equal(_bits(x1), _bits(x37[r:r + 1]))
        np.testing.assert_array_equal(_bits(l1), _bits(l37[r:r + 1]))


# ------------------------------------------------------------------------------------- against log_prob
def test_consistent_with_log_prob_to_second_order(dmip, golden, monkeypatch):
    """ckpt_lin, 64 chains: e(S) = max |logq_S - model.log_prob(x_S, y, 1024)| at S = 32 and 64 has a ratio in
    [3, 5] (two second-order discretisations of one integral), and each e(S) is within twice the f64 restatement's
    own value on the same rows (the rule of the round-trip test of log_prob). (flow_ref's contractions through
    numpy's BLAS path: the same sums in another order, far faster.)"""
    monkeypatch.setattr(np, "einsum", functools.partial(np.einsum, optimize=True))
    m = _lin(dmip, golden)
    params = HR.params_of(m.sde.a)
    y = golden("flow_logp.npz")["a_y"]
    x0 = HR.x0_of_seed(1234, 64, 2)
    e_gpu, e_ref = {}, {}
    for S in (32, 64):
        x, logq = m.sample_with_log_prob(_dev(y), 64, S, x0=_dev(x0))
        logp = m.log_prob(x, _dev(y), num_steps=1024)
        e_gpu[S] = (logq.double() - logp.double()).abs().max().item()
        x64, l64 = FS.sample_with_logq(params, x0, y, S)
        e_ref[S] = np.abs(l64 - FR.log_prob(params, x64, y, 1024)[0]).max()
    print(f"e_gpu = {e_gpu}, f64 restatement {e_ref}; ratio {e_gpu[32] / e_gpu[64]:.2f}")
    assert 3.0 <= e_gpu[32] / e_gpu[64] <= 5.0, e_gpu
    for S in (32, 64):
        assert e_gpu[S] <= 2 * e_ref[S], (S, e_gpu, e_ref)


# ------------------------------------------------------------------------------------- importance_posterior
def test_importance_posterior_on_the_linear_problem(dmip, golden, ev):
    """ckpt_lin against the analytic Gaussian posterior, 4,096 chains, S = 64: every field equals an f64 numpy
    recomputation from the returned (x, logq); ess_frac in (0, 1] and log_z finite. (No gate on the ESS itself: it
    measures the checkpoint, not the kernel.)"""
    m = _lin(dmip, golden)
    y = _dev(golden("flow_lmbd.npz")["lin_S10_y"])
    post = dmip.LinearForwardProblem().get_posterior(y.cpu(), device="cpu")
    log_target = lambda x: post.log_prob(x.cpu())  # noqa: E731 -- (the drivers' way: the 2 x 2 Gaussian on the host)
    before = dmip._lib.calls.get("flow_sample", 0)
    rep = ev.importance_posterior(m, y, log_target, 4096, 64, seed=7)
    assert dmip._lib.calls["flow_sample"] == before + 1
    x, logq = rep["x"], rep["logq"]
    assert tuple(x.shape) == (4096, 2) and tuple(logq.shape) == (4096,) and x.is_cuda
    xs, lq = x.cpu().numpy().astype(np.float64), logq.cpu().numpy().astype(np.float64)
    lw = log_target(x).numpy().astype(np.float64) - lq
    w = np.exp(lw - lw.max())
    ess, log_z = w.sum() ** 2 / (w * w).sum(), np.log(w.mean()) + lw.max()
    wn = w / w.sum()
    mean = (wn[:, None] * xs).sum(0)
    cov = np.einsum("n,ni,nj->ij", wn, xs - mean, xs - mean)
    print(f"ess_frac {rep['ess_frac']:.4f}, log_z {rep['log_z']:.4f}, reverse_kl {rep['reverse_kl']:.4f}, mean "
          f"{rep['mean']}, snis_mean {rep['snis_mean']}, analytic {post.mean.cpu().numpy()}")
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())  # noqa: E731
    assert rel(rep["ess"], ess) <= 1e-9 and rel(rep["ess_frac"], ess / 4096) <= 1e-9
    assert rel(rep["log_z"], log_z) <= 1e-9 and rel(rep["reverse_kl"], -lw.mean() + log_z) <= 1e-9
    assert rel(rep["weights"], wn) <= 1e-12 and rel(rep["mean"], xs.mean(0)) <= 1e-12
    assert rel(rep["snis_mean"], mean) <= 1e-9 and rel(rep["snis_cov"], cov) <= 1e-9
    assert 0.0 < rep["ess_frac"] <= 1.0 and np.isfinite(rep["log_z"])


# ------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(dmip):
    """A SiLU network, std = 0 and CDiffE raise ValueError before any launch; so does the C-ABI for a SiLU handle."""
    y = torch.zeros(23, device=DEV)
    silu = dmip.CDE(3, 23, [256] * 3)
    silu.sde.a = dmip.MLP(3 + 23 + 1, 3, [256] * 3, torch.nn.SiLU()).to(DEV)
    before = dict(dmip._lib.calls)
    with pytest.raises(ValueError, match="tanh"):
        silu.sample_with_log_prob(y, 4, 2)
    with pytest.raises(ValueError, match="std"):
        dmip.CDE(3, 23, [256] * 3).sample_with_log_prob(y, 4, 2, std=0)
    with pytest.raises(ValueError, match="sample_with_log_prob"):
        dmip.CDiffE(3, 23, [256] * 3).sample_with_log_prob(y, 4, 2)
    assert dict(dmip._lib.calls) == before
    L = dmip._lib
    out, logq = torch.empty(1, 4, 3, device=DEV), torch.empty(1, 4, device=DEV)
    with pytest.raises(ValueError, match="tanh"):
        L.flow_sample(L.DMIP_SAMPLER_CDE, silu.sde.a.dmip_handle(torch.device(DEV), 3), None, L.vpsde(0.1, 20.0, 1.0),
                      y[None], 4, 0, 2, 0.0, 1.0, 1, out, logq)
    torch.cuda.synchronize()
