"""The fused stochastic few-step samplers, SDE-DPM-Solver++(2M) and ancestral / eta-DDIM (dmip_multistep_sde_sample;
eta= on solver="dpm2m" / "ddim") against their numpy restatement (tests/multistep_sde_ref.py) fed the oracle's normals
for the same (seed, chain, y index). Needs an MI355X: `pytest -m gpu`.

Bound 1 is tests/test_gpu_multistep.py's: HR.BOUND[prec] max(1, max |ref|) (1e-4 exact f32, 1e-3 fp32x3) against the
f64 scheme at S = 6. The f32 rounding order of the update with the noise added last stays below a quarter of the f32
bound (tests/test_multistep_sde_host.py).
"""
import functools

import numpy as np
import pytest
import torch

import accuracy_cases as AC
import dps_linear_ref as DL
import heun_ref as HR
import multistep_ref as MR
import multistep_sde_ref as R
import oracle as O
import sde_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S6 = R.PARITY_STEPS
SEED = 4242
# the gate's cases of tests/test_gpu_multistep.py
GATE = [("cde", 64, 2, 2, 49), ("cde", 256, 3, 23, 49), ("posterior", 64, 2, 2, 49), ("posterior", 256, 3, 23, 49)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _raw(t):
    return t.cpu().numpy().view(np.uint32)


def _bound(prec, ref):
    return HR.BOUND[prec] * max(1.0, float(np.abs(ref).max()))


def _mode(dmip, kind):
    return dmip._lib.DMIP_SAMPLER_CDE if kind == "cde" else dmip._lib.DMIP_SAMPLER_POSTERIOR


def _sample(dmip, m, y, n, S, solver, eta, fused=True, **kw):
    """m.sample_device(solver=, eta=) for one y -> (n, xdim) numpy; the launch counters show the path taken."""
    calls = dmip._lib.calls
    names = ("multistep_sde_sample", "mlp_forward", "multistep_sample", "ode_sample", "em_sample_lmbd", "em_sample")
    before = [calls[k] for k in names]
    out = m.sample_device(torch.as_tensor(np.asarray(y, np.float32)).to(DEV), n, S, solver=solver, eta=eta, **kw)
    dmip._lib.device_status(torch.device(DEV))
    assert [calls[k] for k in names[2:]] == before[2:]
    if fused:
        assert calls["multistep_sde_sample"] == before[0] + 1 and calls["mlp_forward"] == before[1]
    else:
        assert calls["multistep_sde_sample"] == before[0] and calls["mlp_forward"] > before[1]
    return out[0].cpu().numpy()


def _loop_normals(dmip, seed, n, xdim, S, chain_offset=0, k=0):
    """xi (S, n, d) as the per-step loop draws them: stream _LOOP_STREAM + (k << 40) + 1 + i of the chain-keyed
    generator, read back through the package's own dmip_rng_normals wrapper."""
    out = []
    for i in range(S):
        buf = torch.empty(n, 2 * ((xdim + 1) // 2), device=DEV, dtype=torch.float32)
        dmip._lib.rng_normals(seed, chain_offset, (1 << 62) + (k << 40) + 1 + i, n, (xdim + 1) // 2, buf)
        out.append(buf[:, :xdim].cpu().numpy())
    return np.stack(out)


# ------------------------------------------------------------------------------ 1. parity, x0 injected
@functools.lru_cache(maxsize=None)
def _parity_ref(dmip, case, solver, eta):
    """(model, params, prior, y, x0, the oracle's step normals, the f64 scheme on them), read-only."""
    kind, W, xd, yd, n = case
    m, params, prior, y, x0 = HR.parity_case(dmip, *case)
    xi = R.chain_normals(SEED, n, xd, S6)[1]
    ref = R.direct_sample(params, x0, y, S6, xi, solver, eta, "logsnr", prior)
    ref.setflags(write=False)
    return m, params, prior, y, x0, xi, ref


@pytest.mark.parametrize("eta", R.ETAS)
@pytest.mark.parametrize("solver", R.SOLVERS)
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("case", HR.PARITY_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_parity_with_the_restatement(dmip, case, prec, solver, eta):
    """Random weights, three hidden layers, S = 6, x0 injected, the product RNG: bound 1 against the scheme stated
    directly in float64 on the oracle's normals for the same (seed, chain, y index) -- the x0 draw is consumed although
    x0 is injected. The exact-f32 shape without a kernel (width 512, tanh) steps through the loop, which draws other
    streams: there the restatement is fed the loop's own normals."""
    kind, W, xd, yd, n = case
    m, params, prior, y, x0, xi, ref = _parity_ref(dmip, case, solver, eta)
    fused = dmip._lib.multistep_sde_supported(W, 3, xd, yd, _mode(dmip, kind), prec)
    assert fused == (not (W == 512 and prec == "fp32"))
    out = _sample(dmip, m, y, n, S6, solver, eta, fused=fused, x0=torch.from_numpy(x0), precision=prec, seed=SEED)
    if not fused:
        ref = R.direct_sample(params, x0, y, S6, _loop_normals(dmip, SEED, n, xd, S6), solver, eta, "logsnr", prior)
    err = HR.max_err(out, ref)
    print(f"{kind} W={W} {prec} {solver} eta={eta}: max |kernel - f64 restatement| = {err:.3e} "
          f"(bound {_bound(prec, ref):.1e}, max |ref| {np.abs(ref).max():.3g})")
    assert np.all(np.isfinite(out)) and err < _bound(prec, ref), err


# ------------------------------------------------------------------------------ 2. the noise stream in isolation
def _sum_table(S):
    tab = np.zeros((S, 8), np.float32)
    tab[:, 0] = np.linspace(1.0, 0.1, S)   # tau: the network is evaluated, and multiplied by p = q = c0 = c1 = 0
    tab[:, 3], tab[:, 6], tab[:, 7] = 1.0, 1.0, 1.0
    return tab


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("W,xd,yd", [(64, 2, 2), (256, 3, 23)])
def test_noise_stream_in_isolation(dmip, W, xd, yd, prec):
    """A hand-made table with p = q = c0 = c1 = 0 and cx = cn = 1, S = 5, through _lib directly: x_S = x0 + sum xi_i
    whatever the network is. Against the oracle's stream within 6 x 2e-5 (the project's tolerance on one normal; six
    draws), with and without x0=; with x0 set to the sampler's own x0 the result is the same bits, so the x0 draw is
    consumed either way. Two ys: the y index keys the stream."""
    L = dmip._lib
    S, n, seed, mean, std = 5, 333, 91, 0.0, 1.0
    torch.manual_seed(W)
    m = dmip.CDE(xd, yd, [W] * 3)
    net = m.sde.a.to(DEV).dmip_handle(torch.device(DEV), xd)
    ys = torch.randn(2, yd).to(DEV)
    tab = torch.from_numpy(_sum_table(S)).to(DEV)
    out = torch.empty(2, n, xd, device=DEV)
    L.multistep_sde_sample(L.DMIP_SAMPLER_CDE, net, None, ys, n, 0, S, tab, mean, std, seed, out, precision=prec)
    L.device_status(torch.device(DEV))
    own = np.stack([R.chain_normals(seed, n, xd, S, stream=k, mean=mean, std=std)[0] for k in range(2)])
    for k in range(2):
        x0, xi = R.chain_normals(seed, n, xd, S, stream=k, mean=mean, std=std)
        ref = x0.astype(np.float64) + xi.astype(np.float64).sum(0)
        assert HR.max_err(out[k].cpu().numpy(), ref) <= 6 * 2e-5
    assert not torch.equal(out[0], out[1])
    # x0 injected: the step noise is unchanged
    x0 = torch.randn(2, n, xd, generator=torch.Generator().manual_seed(3))
    inj = torch.empty_like(out)
    L.multistep_sde_sample(L.DMIP_SAMPLER_CDE, net, None, ys, n, 0, S, tab, mean, std, seed, inj, x0.to(DEV),
                           precision=prec)
    for k in range(2):
        xi = R.chain_normals(seed, n, xd, S, stream=k)[1]
        assert HR.max_err(inj[k].cpu().numpy(), x0[k].numpy().astype(np.float64) + xi.astype(np.float64).sum(0)) <= 6 * 2e-5
    # the sampler's own x0, read back from a zero-noise table, injected: bitwise the first run
    tab0 = _sum_table(S)
    tab0[:, 7] = 0.0
    dev_x0 = torch.empty_like(out)
    L.multistep_sde_sample(L.DMIP_SAMPLER_CDE, net, None, ys, n, 0, S, torch.from_numpy(tab0).to(DEV), mean, std, seed,
                           dev_x0, precision=prec)
    assert HR.max_err(dev_x0.cpu().numpy(), own) <= 2e-5
    again = torch.empty_like(out)
    L.multistep_sde_sample(L.DMIP_SAMPLER_CDE, net, None, ys, n, 0, S, tab, mean, std, seed, again, dev_x0,
                           precision=prec)
    L.device_status(torch.device(DEV))
    np.testing.assert_array_equal(_raw(again), _raw(out))


# ------------------------------------------------------------------------------ 3. a zero noise column
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("kind,W,xd,yd", [("cde", 64, 2, 2), ("cde", 256, 3, 23), ("posterior", 64, 2, 2),
                                          ("posterior", 256, 3, 23)])
def test_zero_noise_column_is_the_ode_kernel(dmip, kind, W, xd, yd, prec):
    """The stochastic entry point on the eta = 0 table equals dmip_multistep_sample, float for float, from the chains'
    own x0 and from an injected one: the deterministic part of the step is the same arithmetic."""
    L = dmip._lib
    n, S, seed = 500, 6, 5
    m = HR.parity_case(dmip, kind, W, xd, yd, 10)[0]
    dev = torch.device(DEV)
    if kind == "cde":
        net, prior = m.sde.a.to(DEV).dmip_handle(dev, xd), None
    else:
        net = m.sde.a.likelihood_net.to(DEV).dmip_handle(dev, xd)
        prior = m.sde.a.prior_net.to(DEV).dmip_handle(dev, xd)
    ys = torch.randn(1, yd, generator=torch.Generator().manual_seed(1)).to(DEV)
    tab = torch.from_numpy(MR.table_of(dmip, "dpm2m", "logsnr", S)).to(torch.float32).to(DEV)
    for x0 in (None, torch.randn(1, n, xd, generator=torch.Generator().manual_seed(2)).to(DEV)):
        a, b = torch.empty(1, n, xd, device=DEV), torch.empty(1, n, xd, device=DEV)
        L.multistep_sample(_mode(dmip, kind), net, prior, ys, n, 0, S, tab, 0.0, 1.0, seed, a, x0, precision=prec)
        L.multistep_sde_sample(_mode(dmip, kind), net, prior, ys, n, 0, S, tab, 0.0, 1.0, seed, b, x0, precision=prec)
        L.device_status(dev)
        assert torch.isfinite(a).all()
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())


# ------------------------------------------------------------------------------ 4. the hand-over
@pytest.mark.parametrize("prec", ["fp32x3", "fp32"])
@pytest.mark.parametrize("solver", R.SOLVERS)
def test_generator_and_history_through_the_hand_over(dmip, prec, solver):
    """tests/test_gpu_multistep.py's split run at eta = 1: width 256, 70001 chains, S = 4, so the balanced schedule cuts
    tiles between waves. Two runs are bitwise equal; three ragged chain_offset shards concatenate bitwise to the full
    run; rows of the full run equal, bitwise, launches of 1000 of the same global chains, which hold one tile per wave
    and cannot split; another seed differs. A tile resumed without its generator words would draw other noise, and a
    "dpm2m" tile resumed without d_prev would miss c1 d_prev: both have to cross the slot x[D] | rng[4] | d_prev[D]
    (checked once on scratch builds that drop either one: the first fails every case, the second "dpm2m"; DESIGN.md
    3h-2)."""
    n, S, seed = 70001, 4, 77
    torch.manual_seed(256 + n)
    m = dmip.CDE(3, 23, [256] * 3)
    y = torch.from_numpy(np.random.default_rng(5).uniform(0, 1, (1, 23)).astype(np.float32)).to(DEV)
    kw = dict(seed=seed, precision=prec, solver=solver, eta=1.0)
    before = dmip._lib.calls["multistep_sde_sample"]
    full = m.sample_device(y, n, S, **kw)
    np.testing.assert_array_equal(_raw(m.sample_device(y, n, S, **kw)), _raw(full))
    cuts = [0, n // 3 + 1, n - 333, n]
    parts = [m.sample_device(y, hi - lo, S, chain_offset=lo, **kw) for lo, hi in zip(cuts[:-1], cuts[1:])]
    np.testing.assert_array_equal(_raw(torch.cat(parts, 1)), _raw(full))
    for lo in (0, 35008, n - 1000):
        small = m.sample_device(y, 1000, S, chain_offset=lo, **kw)
        np.testing.assert_array_equal(_raw(small), _raw(full[:, lo:lo + 1000]))
    dmip._lib.device_status(torch.device(DEV))
    assert dmip._lib.calls["multistep_sde_sample"] == before + 8
    assert torch.isfinite(full).all()
    assert not np.array_equal(_raw(full), _raw(m.sample_device(y, n, S, **dict(kw, seed=seed + 1))))


# ------------------------------------------------------------------------------ 5. the f32-accuracy gate
@functools.lru_cache(maxsize=None)
def _gate_refs(dmip, case, sde):
    """(params, prior, y, x0, f64 scheme, f32 restatement) of a gate case at the VP-SDE `sde`, on the same normals."""
    kind, W, xd, yd, n = case
    _, params, prior, y, x0 = HR.parity_case(dmip, *case)
    xi = R.chain_normals(SEED, n, xd, S6)[1]
    kw = SC.kw(sde)
    r64 = R.direct_sample(params, x0, y, S6, xi, "dpm2m", 1.0, "logsnr", prior, **kw)
    r32 = R.table_sample(params, x0, y, R.table_of(dmip, "dpm2m", "logsnr", S6, 1.0, **kw), xi, prior, dtype=np.float32)
    for a in (r64, r32):
        a.setflags(write=False)
    return params, prior, y, x0, r64, r32


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("case,sde", [(c, AC.M) for c in GATE] + [(GATE[0], SC.SDES["B"])],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}-{v[1]}" if isinstance(v[0], str)
                         else "sde-%g-%g-%g" % v)
def test_f32_accuracy_gate(dmip, case, sde, prec):
    """The gate of tests/accuracy_cases.py, err(gpu) <= 8 max(err(f32 restatement), 1e-7), element-wise relative errors
    against the float64 scheme on the same normals: "dpm2m" at eta = 1, the cases of tests/test_gpu_multistep.py at the
    mild VP-SDE and one at the non-default SDE B."""
    kind, W, xd, yd, n = case
    params, prior, y, x0, r64, r32 = _gate_refs(dmip, case, sde)
    m = SC.set_sde(dmip, HR.parity_case(dmip, *case)[0], sde)
    out = _sample(dmip, m, y, n, S6, "dpm2m", 1.0, x0=torch.from_numpy(x0), precision=prec, seed=SEED)
    e_cpu, e_gpu = AC.err(r32, r64), AC.err(out, r64)
    base = max(e_cpu, AC.FLOOR)
    print(f"{kind} W={W} {prec} sde {sde}: e_gpu = {e_gpu:.3e}, e_cpu = {e_cpu:.3e}, ratio = {e_gpu / base:.2f} "
          f"(K = {AC.K:g}), max |ref| = {np.abs(r64).max():.4g}")
    assert np.all(np.isfinite(out))
    assert e_gpu <= AC.K * base, (e_gpu, e_cpu)


# ------------------------------------------------------------------------------ 6. the Gaussian statistic
@functools.lru_cache(maxsize=None)
def _gaussian_model(dmip):
    """A Posterior model with a = -g x: the prior is dps_linear_ref's crafted linear score s = -x, the likelihood net
    is zeroed."""
    m = dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)
    DL.load_params(m.sde.a.prior_net, DL.crafted_params(64, 3, 2))
    with torch.no_grad():
        for w, b in m.sde.a.likelihood_net.linear_layers():
            w.zero_()
            b.zero_()
    return m


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("solver,eta,S", R.GAUSS_CASES)
def test_gaussian_statistic_on_the_device(dmip, solver, eta, S, prec):
    """Data N(0, I) at width 64, xdim 2: 20,000 chains from their own x0 end with the sample std and corr(x_S, x_0) of
    the closed-form recursion within 4 standard errors per coordinate (tests/test_multistep_sde_host.py holds the
    reference to the same bounds). At eta = 0 the correlation is 1; a mis-scaled noise term moves the std."""
    m = _gaussian_model(dmip)
    seed = 17
    x = _sample(dmip, m, np.zeros(2, np.float32), R.GAUSS_N, S, solver, eta, precision=prec, seed=seed)
    R.check_gaussian(x, HR.x0_of_seed(seed, R.GAUSS_N, 2), solver, eta, S, f"{prec} ")


# ------------------------------------------------------------------------------ 7. snapshots
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("case", [HR.PARITY_CASES[0], HR.PARITY_CASES[3]], ids=lambda c: c[0])
def test_snapshots(dmip, case, prec):
    """sample_trajectory(eta=1): snaps[-1] is the returned state bitwise, the run is sample_device's bitwise, and every
    snapshot is the restatement's state after that many steps within bound 1 (internal RNG: the restatement starts
    from the stream's x0 and takes the stream's normals)."""
    kind, W, xd, yd, n = case
    m, params, prior, y, _ = HR.parity_case(dmip, *case)
    S, every, seed = 6, 2, 99
    x0, xi = R.chain_normals(seed, n, xd, S)
    _, ref_snaps = R.direct_sample(params, x0, y, S, xi, "dpm2m", 1.0, "logsnr", prior, snapshot_every=every)
    before = dmip._lib.calls["multistep_sde_sample"], dmip._lib.calls["multistep_sample"]
    yt = torch.from_numpy(y).to(DEV)
    kw = dict(seed=seed, precision=prec, solver="dpm2m", eta=1.0)
    x, snaps = m.sample_trajectory(yt, n, S, snapshot_every=every, **kw)
    dmip._lib.device_status(torch.device(DEV))
    assert (dmip._lib.calls["multistep_sde_sample"], dmip._lib.calls["multistep_sample"]) == (before[0] + 1, before[1])
    assert snaps.shape == (3, 1, n, xd)
    np.testing.assert_array_equal(_raw(snaps[-1]), _raw(x))
    np.testing.assert_array_equal(_raw(x), _raw(m.sample_device(yt, n, S, **kw)))
    for k in range(3):
        err = HR.max_err(snaps[k, 0].cpu().numpy(), ref_snaps[k])
        assert err < _bound(prec, ref_snaps[k]), (k, err)
    assert not torch.equal(snaps[0], snaps[-1])


# ------------------------------------------------------------------------------ 8. several ys in one launch
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
def test_two_ys_in_one_launch(dmip, prec):
    """Two observations in one launch differ; y index 0 is the single-y launch of ys[0] bitwise; y index 1 draws the
    stream of y index 1: it is the restatement of ys[1] on those normals (bound 1), not on stream 0's."""
    torch.manual_seed(11)
    m = dmip.CDE(3, 23, [128] * 2)
    params = HR.params_of(m.sde.a)
    ys = torch.randn(2, 23)
    n, S, seed = 500, 5, 5
    kw = dict(seed=seed, precision=prec, solver="dpm2m", eta=1.0)
    both = m.sample_device(ys.to(DEV), n, S, **kw)
    dmip._lib.device_status(torch.device(DEV))
    assert torch.isfinite(both).all() and not torch.equal(both[0], both[1])
    np.testing.assert_array_equal(_raw(m.sample_device(ys[0].to(DEV), n, S, **kw)[0]), _raw(both[0]))
    for k in range(2):
        x0, xi = R.chain_normals(seed, n, 3, S, stream=k)
        ref = R.direct_sample(params, x0, ys[k].numpy(), S, xi, "dpm2m", 1.0)
        assert HR.max_err(both[k].cpu().numpy(), ref) < _bound(prec, ref)
    x0, xi = R.chain_normals(seed, n, 3, S, stream=0)
    wrong = R.direct_sample(params, x0, ys[1].numpy(), S, xi, "dpm2m", 1.0)
    assert HR.max_err(both[1].cpu().numpy(), wrong) > 100 * _bound(prec, wrong)


# ------------------------------------------------------------------------------ 9, 10. the public call
def _trained_lin(dmip):
    from conftest import GOLDEN, state_from_npz
    m = dmip.CDE(2, 2, [64] * 3)
    m.sde.a.load_state_dict(state_from_npz(np.load(f"{GOLDEN}/ckpt_lin.npz")))
    m.sde.a.to(DEV)
    y = np.load(f"{GOLDEN}/flow_lmbd.npz")["lin_S10_y"].astype(np.float32)
    return m, torch.from_numpy(y).to(DEV)


def test_forward_takes_eta(dmip):
    """model(y, n, S, solver="dpm2m", eta=1.0) returns finite samples of the right shape through the sharded path: the
    chains of sample_device at the seed torch's generator hands out."""
    m, y = _trained_lin(dmip)
    before = dmip._lib.calls["multistep_sde_sample"]
    torch.manual_seed(21)
    a = m(y, 300, 16, solver="dpm2m", eta=1.0)
    torch.manual_seed(21)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    b = m.sample_device(y, 300, 16, seed=seed, solver="dpm2m", eta=1.0)[0].cpu().numpy()
    assert dmip._lib.calls["multistep_sde_sample"] == before + 2
    assert isinstance(a, np.ndarray) and a.shape == (300, 2) and a.dtype == np.float32 and np.all(np.isfinite(a))
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    c = m(y, 300, 16, solver="ddim", eta=0.5, t_end=1e-2, grid="uniform")
    assert c.shape == (300, 2) and np.all(np.isfinite(c)) and dmip._lib.calls["multistep_sde_sample"] == before + 3


def test_eta_zero_takes_the_deterministic_path(dmip):
    """eta = 0 through the public calls is today's path: dmip_multistep_sample, its counter, its bits."""
    m, y = _trained_lin(dmip)
    calls = dmip._lib.calls
    before = calls["multistep_sample"], calls["multistep_sde_sample"]
    a = m.sample_device(y, 300, 8, seed=3, solver="dpm2m")
    b = m.sample_device(y, 300, 8, seed=3, solver="dpm2m", eta=0.0)
    x, _ = m.sample_trajectory(y, 300, 8, snapshot_every=4, seed=3, solver="dpm2m", eta=0)
    torch.manual_seed(4)
    c = m(y, 300, 8, solver="ddim", eta=0.0)
    dmip._lib.device_status(torch.device(DEV))
    assert (calls["multistep_sample"], calls["multistep_sde_sample"]) == (before[0] + 4, before[1])
    np.testing.assert_array_equal(_raw(a), _raw(b))
    np.testing.assert_array_equal(_raw(a), _raw(x))
    assert c.shape == (300, 2)


# ------------------------------------------------------------------------------ 11. a shape without a kernel
@pytest.mark.parametrize("kind", ["cde", "posterior"])
def test_shape_without_a_kernel_steps_through_the_loop(dmip, kind):
    """xdim 4 has no fused sampler: one dmip_mlp_forward launch per network and step and the noise of the loop's own
    streams; bound 1 (exact f32) against the restatement fed those normals, and shards stay bit-identical."""
    torch.manual_seed(96)
    m = (dmip.CDE if kind == "cde" else dmip.PosteriorDiffusionEstimator)(4, 5, [64] * 3)
    if kind == "cde":
        params, prior = HR.params_of(m.sde.a), None
    else:
        params, prior = HR.params_of(m.sde.a.likelihood_net), HR.params_of(m.sde.a.prior_net)
    g = torch.Generator().manual_seed(5)
    y, x0 = torch.randn(5, generator=g).numpy(), torch.randn(200, 4, generator=g).numpy()
    before = dmip._lib.calls["mlp_forward"]
    out = _sample(dmip, m, y, 200, S6, "dpm2m", 1.0, fused=False, x0=torch.from_numpy(x0), precision="fp32x3", seed=8)
    assert dmip._lib.calls["mlp_forward"] == before + S6 * (1 if kind == "cde" else 2)
    ref = R.direct_sample(params, x0, y, S6, _loop_normals(dmip, 8, 200, 4, S6), "dpm2m", 1.0, "logsnr", prior)
    err = HR.max_err(out, ref)
    assert np.all(np.isfinite(out)) and err < _bound("fp32", ref), err
    yt = torch.from_numpy(y).to(DEV)
    full = m.sample_device(yt, 90, 3, seed=4, solver="dpm2m", eta=1.0)
    part = m.sample_device(yt, 50, 3, seed=4, chain_offset=40, solver="dpm2m", eta=1.0)
    np.testing.assert_array_equal(_raw(part), _raw(full[:, 40:]))
    assert not torch.equal(full, m.sample_device(yt, 90, 3, seed=4, solver="dpm2m"))
