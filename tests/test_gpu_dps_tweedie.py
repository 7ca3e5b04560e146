"""LinearDPS's Tweedie-covariance guidance on the device (dmip_dps_tweedie_sample: f32_dps_tweedie_kernel,
x3_dps_tweedie_kernel) against the numpy restatements of tests/dps_tweedie_ref.py: the project's f32-accuracy gate
(tests/accuracy_cases.py) on cases where the rule differs from 'pigdm', bit identity of shards and rows, zeta = 0, the
linear problem end to end against its closed-form posterior, the fp32x3 range report, and the Python / C interface.
The layout of tests/test_gpu_dps_linear.py, whose problem generator and gate are used as they are."""
import ctypes
import functools
import importlib
import warnings

import numpy as np
import pytest
import torch

import accuracy_cases as AC
import dps_linear_ref as R
import dps_tweedie_ref as TW
import sde_cases as SC
from conftest import load_pkg
from test_gpu_dps_linear import _gate, _params, _problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64
PRECISIONS = ("fp32", "fp32x3")
SEED = 99
ZETA = 1.0  # every case, the default SDE included: the rule needs no tuning on an untrained prior

# id: (W, NL, D, M, n, n_y, sde). 37 rows: nine full 4-row passes and a ragged one.
CASES = {f"w64-L{nl}": (64, nl, 2, 2, 37, 1, AC.M) for nl in (1, 2, 3)}
CASES.update({
    "w128-L2-d3-m5": (128, 2, 3, 5, 37, 1, AC.M),
    "w256-L3-d3-m23": (256, 3, 3, 23, 37, 1, AC.M),        # the streamed ring
    "w512-L1-d3-m32": (512, 1, 3, 32, 37, 1, AC.M),
    "w512-L2-d2-m1": (512, 2, 2, 1, 37, 1, AC.M),          # H = A^T A / Sigma has rank one
    "w64-L3-ny3": (64, 3, 2, 2, 37, 3, AC.M),              # one table, y' per y
    "w64-L3-default-sde": (64, 3, 2, 2, 37, 1, AC.DEFAULT),
})
STEPS = {cid: (6, 24) if cid in ("w64-L1", "w64-L2", "w64-L3") else (6,) for cid in CASES}
STEPS["w64-L3-default-sde"] = (50,)
RUNS = [(cid, S, prec) for cid in CASES for S in STEPS[cid] for prec in PRECISIONS]


def _model(dmip, cid, guidance="tweedie", zeta=ZETA):
    W, NL, D, M, n, n_y, sde = CASES[cid]
    A, b, Sigma = _problem(M, D)
    torch.manual_seed(W + NL + D)
    m = dmip.LinearDPS(D, M, [W] * NL, A, b, Sigma, zeta=zeta, guidance=guidance)
    SC.set_sde(dmip, m, sde)
    ys = np.random.default_rng(5).uniform(0, 1, (n_y, M)).astype(F32)
    return m, (A, b, Sigma), ys


@functools.lru_cache(maxsize=None)
def refs(cid, S):
    """(float64 restatement, f32 restatement, float64 'pigdm' chains of the same inputs), (n_y, n, D), read-only."""
    W, NL, D, M, n, n_y, sde = CASES[cid]
    m, (A, b, Sigma), ys = _model(load_pkg(), cid)
    params = _params(m)
    kw = dict(T=sde[2], beta_min=sde[0], beta_max=sde[1])
    out = [AC._frozen(np.stack([TW.sample(params, A, b, Sigma, ys[k], n, S, SEED, ZETA, dt, stream=k, **kw)
                                for k in range(n_y)])) for dt in (F64, F32)]
    with np.errstate(all="ignore"):
        out.append(AC._frozen(np.stack([R.sample(params, A, b, Sigma, ys[k], n, S, SEED, "pigdm", ZETA, F64, stream=k,
                                                 **kw) for k in range(n_y)])))
    return tuple(out)


# ------------------------------------------------------------------------------------- the parity gate
@pytest.mark.parametrize("cid,S,prec", RUNS, ids=[f"{c}-S{s}-{p}" for c, s, p in RUNS])
def test_accuracy_gate(dmip, cid, S, prec):
    """err(gpu) <= 8 max(err(f32 restatement), 1e-7) against the float64 restatement (tests/accuracy_cases.py's gate),
    both precisions, one launch, zeta = 1. The case is not one where the rule is 'pigdm': the float64 chains of the two
    differ by at least 1e-2 in the same err, and on the default SDE every one of pigdm's is beyond f32's range."""
    W, NL, D, M, n, n_y, sde = CASES[cid]
    r64, r32, p64 = refs(cid, S)
    assert np.all(np.isfinite(r64))
    if cid == "w64-L3-default-sde":  # pigdm's chains do not fit an f32: float64 carries them (|x| >= 5e39), f32 cannot
        with np.errstate(all="ignore"):
            assert not np.any(np.abs(p64) <= np.finfo(F32).max)
    else:
        gap = AC.err(p64, r64)
        print(f"{cid}, S = {S}: err(float64 pigdm, float64 tweedie) = {gap:.3g}")
        assert gap >= 1e-2, (cid, S, gap)
    m, _, ys = _model(dmip, cid)
    m.sde.a.to(DEV)
    before = dmip._lib.calls["dps_tweedie_sample"], dmip._lib.calls["dps_linear_sample"]
    x = m.sample_device(torch.from_numpy(ys).to(DEV), n, S, seed=SEED, precision=prec)
    dmip._lib.device_status(x.device)
    assert (dmip._lib.calls["dps_tweedie_sample"], dmip._lib.calls["dps_linear_sample"]) == (before[0] + 1, before[1])
    assert tuple(x.shape) == (n_y, n, D)
    _gate(x.cpu().numpy(), r64, r32, f"{cid}, S = {S}, {prec}")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_many_rounds(dmip, prec):
    """10,000 rows at width 512 (4 waves x 4 rows per workgroup): the round loop runs more than once. Two steps, one
    hidden layer; a strided subset of the rows against the restatements of those rows alone (chain_offset)."""
    cid, n, S = "w512-L1-d3-m32", 10000, 2
    W, NL, D, M, _, n_y, sde = CASES[cid]
    m, (A, b, Sigma), ys = _model(dmip, cid)
    m.sde.a.to(DEV)
    x = m.sample_device(torch.from_numpy(ys).to(DEV), n, S, seed=SEED, precision=prec)[0].cpu().numpy()
    dmip._lib.device_status(torch.device(DEV))
    params = _params(m)
    rows = list(range(0, n, 997)) + [n - 1]
    kw = dict(T=sde[2], beta_min=sde[0], beta_max=sde[1])
    r64, r32 = (np.concatenate([TW.sample(params, A, b, Sigma, ys[0], 1, S, SEED, ZETA, dt, chain_offset=r, **kw)
                                for r in rows]) for dt in (F64, F32))
    _gate(x[rows], r64, r32, f"{cid}, {n} rows, {prec}")


# ------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("cid", ["w64-L3-ny3", "w256-L3-d3-m23"])
def test_shards_rows_and_seeds_are_bit_identical(dmip, cid, prec):
    W, NL, D, M, n, n_y, sde = CASES[cid]
    m, _, ys = _model(dmip, cid)
    m.sde.a.to(DEV)
    y = torch.from_numpy(ys).to(DEV)
    S = 6
    run = lambda n_, off=0, seed=SEED: m.sample_device(y, n_, S, seed=seed, chain_offset=off, precision=prec)
    whole = run(n)
    assert torch.equal(whole, run(n))                                              # the same seed twice
    assert torch.equal(whole, torch.cat([run(21), run(n - 21, 21)], dim=1))        # two chain_offset shards
    for r in (0, 17, n - 1):
        assert torch.equal(whole[:, r:r + 1], run(1, r))                           # a row alone
    assert not torch.equal(whole, run(n, seed=SEED + 1))
    if n_y > 1:  # the y index keys the RNG stream: equal observations still give different chains
        same = m.sample_device(y[:1].expand(n_y, -1).contiguous(), n, S, seed=SEED, precision=prec)
        assert not torch.equal(same[0], same[1]) and torch.equal(same[0], whole[0])
    dmip._lib.device_status(whole.device)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_zero_zeta_switches_the_guidance_off(dmip, prec):
    """zeta = 0: the bits of 'pigdm' at zeta = 0 -- the solve enters through lam G alone."""
    cid = "w64-L3"
    W, NL, D, M, n, n_y, sde = CASES[cid]
    outs = []
    for guidance in ("tweedie", "pigdm"):
        m, _, ys = _model(dmip, cid, guidance, 0.0)
        m.sde.a.to(DEV)
        outs.append(m.sample_device(torch.from_numpy(ys).to(DEV), n, 6, seed=SEED, precision=prec))
    assert torch.equal(outs[0], outs[1])
    m, _, ys = _model(dmip, cid)
    m.sde.a.to(DEV)
    assert not torch.equal(outs[0], m.sample_device(torch.from_numpy(ys).to(DEV), n, 6, seed=SEED, precision=prec))
    dmip._lib.device_status(outs[0].device)


# ------------------------------------------------------------------------------------- the linear problem, end to end
E2E_N, E2E_S, E2E_SEED = 20000, 200, 2024
E2E_YS = ((0.7, -0.2), (-1.5, 2.0))


@functools.lru_cache(maxsize=None)
def _e2e_ref(yi):
    """The float64 restatement's chains for the same seed, on the crafted network without its idle units (they are
    identically zero: dropping them changes no bit of a float64 sum)."""
    p = load_pkg().LinearForwardProblem()
    return AC._frozen(TW.sample(R.crafted_params(2, 3, 2), p.A.numpy(), p.b.numpy(), p.Sigma.numpy(),
                                np.asarray(E2E_YS[yi], F64), E2E_N, E2E_S, E2E_SEED, 1.0, F64, stream=0))


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("yi", [0, 1])
def test_linear_problem_end_to_end(dmip, yi, prec):
    """LinearDPS.for_problem with the crafted linear-score prior, 20,000 chains x 200 steps: 'tweedie' samples
    get_posterior(y) (mean and covariance errors each at most 1/5 of 'nll''s), and the device chains' moments are
    within a tenth of one standard error of the float64 restatement's for the same seed."""
    p = dmip.LinearForwardProblem()
    y = torch.tensor(E2E_YS[yi], dtype=torch.float32)
    post = p.get_posterior(y, device="cpu")
    pm, pc = post.mean.numpy().astype(F64), post.covariance_matrix.numpy().astype(F64)
    errs, xs = {}, {}
    for guidance in ("tweedie", "nll"):
        m = dmip.LinearDPS.for_problem(p, [64] * 3, guidance=guidance)
        R.load_params(m.prior_net, R.crafted_params(64, 3, 2))
        m.sde.a.to(DEV)
        x = m.sample_device(y.to(DEV), E2E_N, E2E_S, seed=E2E_SEED, precision=prec)[0].cpu().numpy()
        dmip._lib.device_status(torch.device(DEV))
        assert np.all(np.isfinite(x))
        errs[guidance], xs[guidance] = R.moment_errors(x, pm, pc), x
    (gm, gc), (nm, nc) = errs["tweedie"], errs["nll"]
    print(f"y = {E2E_YS[yi]}, {prec}: tweedie mean err {gm:.3e}, cov err {gc:.3e}; nll mean err {nm:.3e}, "
          f"cov err {nc:.3e}; ratios {gm / nm:.3f}, {gc / nc:.3f}")
    assert gm <= nm / 5 and gc <= nc / 5
    mean_g, cov_g = R.moments(xs["tweedie"])
    mean_r, cov_r = R.moments(_e2e_ref(yi))
    se_mean = np.sqrt(np.diag(cov_r) / E2E_N)
    # standard error of a sample covariance entry of a Gaussian: sqrt((c_ii c_jj + c_ij^2) / (N - 1))
    se_cov = np.sqrt((np.outer(np.diag(cov_r), np.diag(cov_r)) + cov_r ** 2) / (E2E_N - 1))
    dm, dc = np.abs(mean_g - mean_r) / se_mean, np.abs(cov_g - cov_r) / se_cov
    print(f"  device vs float64 restatement, in standard errors: mean {dm.max():.2e}, covariance {dc.max():.2e}")
    assert dm.max() <= 0.1 and dc.max() <= 0.1


# ------------------------------------------------------------------------------------- the split's fp16 range
def test_trajectory_outside_fp16_range(dmip):
    """An output bias of 1e6 drives every chain beyond 65504 after one step (finite in f32): an explicit fp32x3 request
    raises "fp16 range"; the default precision returns the exact-f32 kernel's samples, with the warning."""
    cid = "w64-L3"
    W, NL, D, M, n, n_y, sde = CASES[cid]
    m, _, ys = _model(dmip, cid)
    with torch.no_grad():
        m.prior_net.linear_layers()[-1][1][:] = 1.0e6
    m.sde.a.to(DEV)
    y = torch.from_numpy(ys[0]).to(DEV)
    n, S = 600, 6
    assert m.precision == "fp32x3"
    torch.manual_seed(6)
    with pytest.raises(RuntimeError, match="fp16 range"):
        m(y, num_samples=n, num_steps=S, precision="fp32x3")
    dmip._lib.device_status(torch.device(DEV))  # the status word was cleared
    torch.manual_seed(6)
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        x = m(y, num_samples=n, num_steps=S)
    torch.manual_seed(6)
    xf = m(y, num_samples=n, num_steps=S, precision="fp32")
    assert np.array_equal(x, xf) and np.all(np.isfinite(x)) and np.abs(x).max() > 6.6e4


# ------------------------------------------------------------------------------------- the interface
def test_api(dmip):
    p = dmip.LinearForwardProblem()
    torch.manual_seed(3)
    m, loss = dmip.get_model_from_args({"model": "LinearDPS", "hidden_layers": [64, 64, 64], "guidance": "tweedie"},
                                       {"xdim": 2, "ydim": 2}, None, p)
    assert isinstance(m, dmip.LinearDPS) and isinstance(loss, dmip.DSMLoss) and m.guidance == "tweedie"
    m.sde.a.to(DEV)  # (an untrained prior, zeta = 1, the default SDE)
    y = torch.tensor([0.7, -0.2])
    calls = dmip._lib.calls
    before, lin = calls["dps_tweedie_sample"], calls["dps_linear_sample"]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # no fallback
        x = m(y, 100, 50)
    assert isinstance(x, np.ndarray) and x.shape == (100, 2) and x.dtype == np.float32 and np.all(np.isfinite(x))
    assert calls["dps_tweedie_sample"] == before + 1 and m.table_uploads == 1
    m(y, 50, 50)
    assert calls["dps_tweedie_sample"] == before + 2 and m.table_uploads == 1
    m(y, 50, 51)
    assert m.table_uploads == 1                                                # no entry depends on num_steps
    assert m(y, 7, 50, precision="fp16").shape == (7, 2)                       # runs the fp32x3 kernel
    assert calls["dps_tweedie_sample"] == before + 4 and calls["dps_linear_sample"] == lin
    odd = dmip.LinearDPS(2, 2, [96, 96], p.A, p.b, p.Sigma, guidance="tweedie")
    odd.sde.a.to(DEV)
    with pytest.raises(ValueError, match="no compiled kernel"):
        odd.sample_device(y.to(DEV), 4, 2)
    mixed = dmip.LinearDPS(2, 2, [64, 128], p.A, p.b, p.Sigma, guidance="tweedie")
    mixed.sde.a.to(DEV)
    with pytest.raises(ValueError, match="no compiled kernel"):
        mixed.sample_device(y.to(DEV), 4, 2)


def test_capi_refusals_that_need_a_handle(dmip):
    """DMIP_ERR_UNSUPPORTED for a SiLU prior, a shape or precision without a kernel and fp32x3 weights beyond fp16's
    range; DMIP_ERR_INVALID for a prior that is no x,t network. Zero chains: nothing is launched."""
    L = dmip._lib
    lib = L.lib()
    nets = importlib.import_module(dmip.__name__ + ".nets")
    dev = torch.device("cuda", torch.cuda.current_device())
    sde = L.vpsde(0.1, 20.0, 1.0)
    buf = ctypes.c_void_p(64)  # never dereferenced

    def call(prior, prec=L.DMIP_PREC_F32):
        return lib.dmip_dps_tweedie_sample(prior.h, ctypes.byref(sde), buf, buf, buf, buf, 2, 1, 0, 0, 5, 0.0, 1.0, 1,
                                           1.0, prec, buf, None)

    good = nets.MLP2(3, 2, [64, 64], torch.nn.Tanh()).to(dev).dmip_handle(dev, 2)
    assert call(good) == L.DMIP_OK and call(good, L.DMIP_PREC_F32X3) == L.DMIP_OK
    assert call(good, prec=7) == L.DMIP_ERR_UNSUPPORTED
    silu = nets.MLP2(3, 2, [64, 64], torch.nn.SiLU()).to(dev).dmip_handle(dev, 2)
    assert call(silu) == L.DMIP_ERR_UNSUPPORTED
    odd = nets.MLP2(3, 2, [96, 96], torch.nn.Tanh()).to(dev).dmip_handle(dev, 2)
    assert call(odd) == L.DMIP_ERR_UNSUPPORTED
    xyt = nets.MLP(5, 2, [64, 64], torch.nn.Tanh()).to(dev).dmip_handle(dev, 2)
    assert call(xyt) == L.DMIP_ERR_INVALID
    big = nets.MLP2(3, 2, [64, 64], torch.nn.Tanh()).to(dev)
    with torch.no_grad():
        big.linear_layers()[1][0].mul_(1e6)
    hb = big.dmip_handle(dev, 2)
    assert call(hb, L.DMIP_PREC_F32X3) == L.DMIP_ERR_UNSUPPORTED and b"fp16 range" in lib.dmip_last_error()
    assert call(hb, L.DMIP_PREC_F32) == L.DMIP_OK
