"""Parity of the scatterometry forward-model kernels through libdmip's C-ABI:
surrogate forward, get_log_posterior and energy_grad (exact-f32 MFMA), and the fused random-walk
Metropolis-Hastings ground-truth sampler -- against the reference's own outputs (fixture G8,
tests/golden/surrogate_io.npz) and the oracle (oracle/dmip_oracle.py F2/F3).

Tolerances: the kernel computes in f32 with fmaf-chain accumulation, the reference in f32 MKL
GEMMs: outputs agree to ~1e-6 relative; stated per test. MH trajectories are compared chain by
chain with the same draws (a borderline acceptance can flip on a last-bit energy difference, so a
few percent of chains may diverge) and by two-sample KS against the reference sampler's own run.
"""
import importlib
import os

import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def fm(dmip, golden):
    z = golden("surrogate.npz")
    pr = importlib.import_module("diffusion-modelling-for-inverse-problems_amd.problems")
    model = torch.nn.Sequential(torch.nn.Linear(3, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                                torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, 23))
    model.load_state_dict({k.replace("_", "."): torch.from_numpy(z[k]) for k in z.files})
    for p in model.parameters():
        p.requires_grad = False
    return model.to(DEV), pr, O.surrogate_params_from_npz(z)


def _handle(fm):
    model, pr, _ = fm
    return pr.surrogate_handle(model, torch.device(DEV))


def _noise(dmip):
    return dmip._lib.scat_noise(0.2, 0.01, 1000.0)


def test_surrogate_forward_vs_reference(dmip, golden, fm):
    z = golden("surrogate_io.npz")
    L = dmip._lib
    x = torch.from_numpy(z["x"]).to(DEV)
    out = torch.empty(x.shape[0], 23, device=DEV)
    L.surrogate_forward(_handle(fm), x, out)
    torch.cuda.synchronize()
    err = np.abs(out.cpu().numpy() - z["f"])
    # exact-f32 products; only the summation order differs from the reference's sgemm
    assert err.max() < 1e-5 * max(1.0, np.abs(z["f"]).max()), err.max()


def test_log_posterior_and_grad_vs_reference(dmip, golden, fm):
    z = golden("surrogate_io.npz")
    L = dmip._lib
    x = torch.from_numpy(z["x"]).to(DEV)
    y = torch.from_numpy(z["y"]).to(DEV)
    e = torch.empty(x.shape[0], device=DEV)
    g = torch.empty_like(x)
    L.log_posterior(_handle(fm), _noise(dmip), x, y, 23, e, g)
    torch.cuda.synchronize()
    e, g = e.cpu().numpy(), g.cpu().numpy()
    np.testing.assert_allclose(e, z["energy"], rtol=2e-5, atol=1e-3)
    # gradient: relative to each row's scale (the boundary term adds exact +-1000 per dimension)
    scale = np.abs(z["grad"]).max(1, keepdims=True) + 1.0
    assert np.all(np.abs(g - z["grad"]) <= 1e-4 * scale), np.abs(g - z["grad"]).max()
    # energy-only launch gives the same energies
    e2 = torch.empty(x.shape[0], device=DEV)
    L.log_posterior(_handle(fm), _noise(dmip), x, y, 23, e2, None)
    assert np.array_equal(e2.cpu().numpy(), e)


@pytest.mark.parametrize("n", [1, 17, 1000, 5003])
def test_log_posterior_ragged_broadcast_vs_oracle(dmip, golden, fm, n):
    _, _, params = fm
    L = dmip._lib
    rng = np.random.default_rng(n)
    x = rng.uniform(-1.2, 1.2, size=(n, 3)).astype(np.float32)
    y = golden("data_scat.npz")["y_test"][3]
    e = torch.empty(n, device=DEV)
    g = torch.empty(n, 3, device=DEV)
    L.log_posterior(_handle(fm), _noise(dmip), torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)[None], 0, e, g)
    torch.cuda.synchronize()
    re, rg = O.scat_log_posterior(params, x, y, grad=True)
    np.testing.assert_allclose(e.cpu().numpy(), re, rtol=2e-5, atol=1e-3)
    scale = np.abs(rg).max(1, keepdims=True) + 1.0
    assert np.all(np.abs(g.cpu().numpy() - rg) <= 1e-4 * scale)


def test_get_log_posterior_api_and_energy_grad(dmip, golden, fm):
    """The reference API on device tensors takes the fused kernel, including through autograd
    (energy_grad, models/SNF.py:234-237)."""
    model, pr, _ = fm
    z = golden("surrogate_io.npz")
    x = torch.from_numpy(z["x"]).to(DEV)
    y = torch.from_numpy(z["y"]).to(DEV)
    before = dmip._lib.calls.get("log_posterior", 0)
    energy = lambda v: pr.get_log_posterior(v, model, 0.2, 0.01, y, 1000)
    grad, e = pr.energy_grad(x.clone(), energy)
    assert dmip._lib.calls["log_posterior"] == before + 1
    np.testing.assert_allclose(e.detach().cpu().numpy(), z["energy"], rtol=2e-5, atol=1e-3)
    scale = np.abs(z["grad"]).max(1, keepdims=True) + 1.0
    assert np.all(np.abs(grad.detach().cpu().numpy() - z["grad"]) <= 1e-4 * scale)


def test_mh_replays_reference_draws(dmip, golden, fm):
    """anneal_to_energy (models/SNF.py:250-275) on the reference's captured x0, proposals and
    uniforms (64 chains x 50 steps at NOISE_STD_MCMC = 0.5): the fused kernel takes the same
    accept/reject path."""
    model, pr, _ = fm
    z = golden("surrogate_io.npz")
    S, n = z["mh_xi"].shape[:2]
    y = torch.from_numpy(z["mh_y"]).to(DEV)[None]
    x, ed = pr.mh_sample(model, {"a": 0.2, "b": 0.01, "lambd_bd": 1000}, y, n, S, float(z["mh_noise_std"]),
                         seed=0, x_init=torch.from_numpy(z["mh_x0"])[None],
                         noise=torch.from_numpy(z["mh_xi"])[:, None], unif=torch.from_numpy(z["mh_u"])[:, None],
                         return_ediff=True)
    x = x[0].cpu().numpy()
    same = np.all(np.abs(x - z["mh_x"]) <= 1e-6, axis=1)
    assert same.mean() >= 0.95, same.mean()
    np.testing.assert_allclose(ed[0].cpu().numpy()[same], z["mh_ediff"][same], rtol=1e-4, atol=2e-3)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_mh_product_rng_vs_oracle(dmip, golden, fm, precision):
    """Chain by chain against the oracle on the same RNG stream. fp32x3 (three-term fp16 splits of every
    surrogate product, ~1e-7 relative per product) takes the same accept/reject path on the same share."""
    model, pr, params = fm
    y = golden("data_scat.npz")["y_test"][5]
    n, S, seed = 300, 30, 1234
    x = pr.mh_sample(model, {"a": 0.2, "b": 0.01, "lambd_bd": 1000}, torch.from_numpy(y)[None], n, S, 0.5,
                     seed=seed, precision=precision)[0].cpu().numpy()
    ref, _ = O.mh_sample(params, y, S, 0.5, seed=seed, n_chains=n)
    same = np.all(np.abs(x - ref) <= 1e-5, axis=1)
    assert same.mean() >= 0.95, same.mean()


# (the fp32x3 cases keep their ids "1" .. "257"; the exact-f32 ones are "fp32-1" .. "fp32-257")
@pytest.mark.parametrize("precision,n", [pytest.param("fp32x3", n, id=str(n)) for n in (1, 17, 129, 257)] +
                         [pytest.param("fp32", n, id=f"fp32-{n}") for n in (1, 17, 129, 257)])
def test_mh_fp32x3_ragged_chain_counts_vs_oracle(dmip, golden, fm, precision, n):
    """The multi-tile MH kernel (two 16-chain tiles per wave, 128 chains per workgroup) and the exact-f32 one (one tile,
    128 chains per workgroup) on chain counts that leave partial tiles and idle waves, over two ys: chain by chain
    against the oracle (30 steps). The exact-f32 cases pin the kernel on the shared chain driver to the kernel before
    it: that one met the same share at every n with seed n, so no seed was changed."""
    model, pr, params = fm
    ys = golden("data_scat.npz")["y_test"][7:9]
    x = pr.mh_sample(model, {"a": 0.2, "b": 0.01, "lambd_bd": 1000}, torch.from_numpy(ys), n, 30, 0.5, seed=n,
                     precision=precision).cpu().numpy()
    assert x.shape == (2, n, 3) and np.all(np.isfinite(x))
    for k in range(2):
        ref, _ = O.mh_sample(params, ys[k], 30, 0.5, seed=n, n_chains=n, stream=k)
        same = np.all(np.abs(x[k] - ref) <= 1e-5, axis=1)
        assert same.mean() >= (0.95 if n >= 17 else 1.0), (k, same.mean())


def test_mh_fp32x3_tile_variants_bit_identical_at_small_counts(dmip, golden, fm, tmp_path):
    """The one-tile and the three-tile fp32x3 kernel (DMIP_MH_MT=1, 3: the knob is read once per process, so a fresh
    child process each, one after the other) against this process's launch, which picks two tiles at these sizes:
    tests/mh_tiles.py's runs. x and E(x_S) - E(x_0) of all three are the same bits (one RNG stream, start, step loop and
    store: dmip_mh_chains.h)."""
    import subprocess
    import sys
    import mh_tiles
    assert "DMIP_MH_MT" not in os.environ
    model, pr, _ = fm
    here = mh_tiles.runs(pr, model, golden("data_scat.npz")["y_test"][7:9])
    assert len(here) == 12 and all(np.all(np.isfinite(v)) for v in here.values())
    for mt in ("1", "3"):
        out = str(tmp_path / f"mt{mt}.npz")
        r = subprocess.run([sys.executable, os.path.join(mh_tiles.ROOT, "tests", "mh_tiles.py"), out],
                           env=dict(os.environ, DMIP_MH_MT=mt), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        z = np.load(out)
        assert sorted(z.files) == sorted(here)
        diff = [k for k in here if z[k].tobytes() != here[k].tobytes()]
        assert not diff, (mt, diff)


def test_mh_fp32x3_three_tile_launch_matches_two_tile(dmip, golden, fm):
    """300 rows x 1920 chains: the launcher picks three tiles per wave on a 256-CU MI355X (12 full workgroup rounds
    against 18 for two); rows 0 and 1 must equal a 2-row launch of the same ys (two tiles, few rounds) bit for bit --
    the RNG stream is the row index and the variants compute the same products in the same order."""
    model, pr, _ = fm
    prm = {"a": 0.2, "b": 0.01, "lambd_bd": 1000}
    y = torch.from_numpy(golden("data_scat.npz")["y_test"])
    ys = y[torch.arange(300) % y.shape[0]]
    big = pr.mh_sample(model, prm, ys, 1920, 20, 0.5, seed=31, precision="fp32x3")
    small = pr.mh_sample(model, prm, ys[:2], 1920, 20, 0.5, seed=31, precision="fp32x3")
    assert torch.equal(big[:2], small)
    assert torch.isfinite(big).all()


def test_mh_fp32x3_vs_exact_f32_chains(dmip, golden, fm):
    """fp32x3 against the exact-f32 kernel on 4 ys x 4096 chains x 200 steps from given starts: the same final
    state on >= 95% of chains, and there the energy change E(x_S) - E(x_0) agrees to 1e-3 relative + 2e-3."""
    model, pr, _ = fm
    ys = torch.from_numpy(golden("data_scat.npz")["y_test"][10:14])
    prm = {"a": 0.2, "b": 0.01, "lambd_bd": 1000}
    x0 = torch.rand(4, 4096, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1
    xa, ea = pr.mh_sample(model, prm, ys, 4096, 200, 0.5, seed=21, x_init=x0, return_ediff=True)
    xb, eb = pr.mh_sample(model, prm, ys, 4096, 200, 0.5, seed=21, x_init=x0, return_ediff=True, precision="fp32x3")
    xa, xb, ea, eb = (t.cpu().numpy() for t in (xa, xb, ea, eb))
    same = np.all(np.abs(xa - xb) <= 1e-5, axis=2)
    assert same.mean() >= 0.95, same.mean()
    np.testing.assert_allclose(eb[same], ea[same], rtol=1e-3, atol=2e-3)


def test_mh_fp32x3_refusals_and_range_fallback(dmip, golden, fm):
    model, pr, _ = fm
    prm = {"a": 0.2, "b": 0.01, "lambd_bd": 1000}
    y = torch.from_numpy(golden("data_scat.npz")["y_test"][2])[None]
    with pytest.raises(ValueError, match="injected"):
        pr.mh_sample(model, prm, y, 4, 2, 0.5, seed=0, noise=torch.zeros(2, 1, 4, 3), unif=torch.zeros(2, 1, 4),
                     precision="fp32x3")
    with pytest.raises(ValueError, match="precision"):
        pr.mh_sample(model, prm, y, 4, 2, 0.5, seed=0, precision="fp16")
    # a start beyond fp16's range: the split kernel reports it and every chain is resampled in exact f32
    x0 = torch.rand(1, 200, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1
    x0[0, 17] = 1e5
    ref = pr.mh_sample(model, prm, y, 200, 10, 0.5, seed=4, x_init=x0)
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        got = pr.mh_sample(model, prm, y, 200, 10, 0.5, seed=4, x_init=x0, precision="fp32x3")
    assert torch.equal(got, ref)
    # and the status word is clear afterwards: an in-range fp32x3 launch does not warn
    import warnings as _w
    with _w.catch_warnings():
        _w.simplefilter("error")
        pr.mh_sample(model, prm, y, 200, 10, 0.5, seed=4, precision="fp32x3")


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_mh_distribution_vs_reference_sampler(dmip, golden, fm, precision):
    """30,000 fused chains x 1000 steps (the ground-truth generator's settings) against the
    reference anneal_to_energy's own 4,000 x 1000 run for y_test[0]: per-dimension two-sample KS
    below the alpha = 0.01 critical value."""
    model, pr, _ = fm
    z = golden("surrogate_io.npz")
    ref = z["gt_samples"]
    x = pr.mh_sample(model, {"a": 0.2, "b": 0.01, "lambd_bd": 1000}, torch.from_numpy(z["mh_y"])[None], 30000,
                     int(z["gt_steps"]), 0.5, seed=77, precision=precision)[0].cpu().numpy()
    assert np.all(np.isfinite(x))
    crit = 1.63 * np.sqrt((x.shape[0] + ref.shape[0]) / (x.shape[0] * ref.shape[0]))
    for k in range(3):
        ks = O.ks_2samp_stat(x[:, k], ref[:, k])
        assert ks < crit, (k, ks, crit)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_mh_shards_and_rows_bit_identical(dmip, golden, fm, precision):
    model, pr, _ = fm
    ys = torch.from_numpy(golden("data_scat.npz")["y_test"][:3])
    prm = {"a": 0.2, "b": 0.01, "lambd_bd": 1000}
    full = pr.mh_sample(model, prm, ys, 1000, 20, 0.5, seed=9, precision=precision)
    shard = pr.mh_sample(model, prm, ys, 300, 20, 0.5, seed=9, chain_offset=500, precision=precision)
    assert torch.equal(full[:, 500:800], shard)
    one = pr.mh_sample(model, prm, ys[1:2], 1000, 20, 0.5, seed=9, precision=precision)
    # the RNG stream is the row index: row 1 of the batch is not row 0 of a single-y launch ...
    assert not torch.equal(full[1], one[0])
    # ... but re-running is deterministic
    assert torch.equal(full, pr.mh_sample(model, prm, ys, 1000, 20, 0.5, seed=9, precision=precision))


def test_generate_gt_samples_files(dmip, golden, fm, tmp_path):
    model, pr, _ = fm
    ys = golden("data_scat.npz")["y_test"][:2]
    x = pr.generate_gt_samples(model, {"a": 0.2, "b": 0.01, "lambd_bd": 1000}, ys, str(tmp_path), n_samples_x=500,
                               n_repeats=3, metr_steps=10, seed=3)
    assert x.shape == (2, 3, 500, 3)
    for i in range(2):
        for j in range(3):
            a = np.load(os.path.join(tmp_path, str(i), f"{j}.npy"))
            assert a.shape == (500, 3) and np.array_equal(a, x[i, j].cpu().numpy())


# ------------------------------------------------------------------------- DPS (BASELINE config 4)
def _dps_model(dmip, fm, seed, zeta, guidance):
    model, _, sur_params = fm
    torch.manual_seed(seed)
    m = dmip.DPS(3, 23, [256] * 3, model, zeta=zeta, guidance=guidance)
    pn = m.prior_net
    # an untrained prior drives EM + guidance chaotic within a few steps; a small, smooth output layer
    # keeps the comparison well conditioned while every layer and both Jacobian paths contribute
    with torch.no_grad():
        last = [l for l in pn if isinstance(l, torch.nn.Linear)][-1]
        last.weight.mul_(0.1)
        last.bias.fill_(0.1)
    prior = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy())
             for l in pn if isinstance(l, torch.nn.Linear)]
    return m, prior, sur_params


@pytest.mark.parametrize("precision", ["fp32x3", "fp32"])
@pytest.mark.parametrize("guidance,zeta", [("nll", 1.0), ("nll", 0.0), ("norm", 0.05)])
def test_dps_vs_oracle_product_rng(dmip, golden, fm, guidance, zeta, precision):
    """Fused DPS kernels against oracle.dps_sample with the same chain-keyed RNG; 5 steps, 300 chains:
    "fp32" = exact f32 (prior score + forward-mode Jacobian, Tweedie estimate, surrogate residual gradient, EM);
    "fp32x3" = the split-fp16 engine (the prior's J^T by a reverse pass; dmip_dps_x3.hip). The oracle computes in
    f64: |x - ref| <= 1e-3 max(1, |ref|). fp32x3 runs the default path (parallel.sample_checked): with the untrained
    prior, 'nll' at zeta = 1 throws chains to |x| ~ 1e4-7e4 within 5 steps, past fp16's range; the kernel reports it
    (device status word) and the call resamples with the exact-f32 engine -- that case must fall back, the others not."""
    import warnings
    m, prior, sur = _dps_model(dmip, fm, 3, zeta, guidance)
    y = golden("data_scat.npz")["y_test"][2]
    n, S, seed = 300, 5, 21
    before = dmip._lib.calls.get("dps_sample", 0)
    yd = torch.from_numpy(y).to(DEV)
    if precision == "fp32x3":
        assert m.precision == "fp32x3"
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            par = importlib.import_module("diffusion-modelling-for-inverse-problems_amd.parallel")
            x = par.sample_checked(m, yd, n, S, 0, 1, seed=seed)[0].cpu().numpy()
        fell_back = any("fp16 range" in str(r.message) for r in w)
        assert fell_back == (zeta == 1.0)
        assert dmip._lib.calls["dps_sample"] == before + 1 + fell_back
    else:
        x = m.sample_device(yd, n, S, seed=seed, precision=precision)[0].cpu().numpy()
        assert dmip._lib.calls["dps_sample"] == before + 1
    ref = O.dps_sample(prior, sur, y, n, S, seed, zeta=zeta, mode=guidance)
    assert np.all(np.isfinite(x))
    err = np.abs(x - ref)
    assert err.max() < 1e-3 * max(1.0, np.abs(ref).max()), err.max()
    if zeta > 0:  # the guidance is not silently skipped
        plain = O.dps_sample(prior, sur, y, n, S, seed, zeta=0.0, mode=guidance)
        assert np.abs(plain - ref).max() > 100 * err.max()


@pytest.mark.parametrize("precision", ["fp32x3", "fp32"])
def test_dps_shards_bit_identical(dmip, golden, fm, precision):
    m, _, _ = _dps_model(dmip, fm, 4, 1.0, "nll")
    ys = torch.from_numpy(golden("data_scat.npz")["y_test"][:2]).to(DEV)
    full = m.sample_device(ys, 700, 6, seed=5, precision=precision)
    shard = m.sample_device(ys, 200, 6, seed=5, chain_offset=300, precision=precision)
    # (fp32x3: this chaotic case leaves fp16's range for some chains -- NaN there, reported; compared as NaN == NaN)
    assert torch.allclose(full[:, 300:500], shard, rtol=0, atol=0, equal_nan=True)
    assert not torch.allclose(full[0], full[1], equal_nan=True)


def _trained_dps(dmip, golden, fm, zeta, guidance):
    """DPS on the fixture-trained prior (tests/golden/ckpt_prior_scat.npz: DSM on inverse_cdf_prior samples), the
    prior scripts/bench_dps.py measures."""
    model, _, _ = fm
    m = dmip.DPS(3, 23, [256] * 3, model, zeta=zeta, guidance=guidance)
    z = golden("ckpt_prior_scat.npz")
    m.prior_net.load_state_dict({k.replace("_", "."): torch.from_numpy(z[k]) for k in z.files
                                 if k.split("_")[0].isdigit()})
    m.prior_net.to(DEV)
    return m


@pytest.mark.parametrize("precision", ["fp32x3", "fp32"])
@pytest.mark.parametrize("guidance,zeta", [("norm", 0.005), ("nll", 0.0)])
def test_dps_trained_prior_vs_oracle(dmip, golden, fm, guidance, zeta, precision):
    """Both DPS engines on the fixture-trained prior against oracle.dps_sample (f64), 20 steps, 200 chains:
    |x - ref| <= 1e-4 max(1, |ref|) (measured: fp32x3 1.5e-6 / 6.7e-7, exact f32 2.0e-6 / 5.9e-7;
    profiles/r5_dps_engine_drift.jsonl)."""
    _, _, sur = fm
    m = _trained_dps(dmip, golden, fm, zeta, guidance)
    prior = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy())
             for l in m.prior_net if isinstance(l, torch.nn.Linear)]
    y = golden("data_scat.npz")["y_test"][0]
    x = m.sample_device(torch.from_numpy(y).to(DEV), 200, 20, seed=11, precision=precision)[0].cpu().numpy()
    ref = O.dps_sample(prior, sur, y, 200, 20, 11, zeta=zeta, mode=guidance)
    err = np.abs(x - ref).max()
    print(f"\n[dps] {precision} vs oracle, trained prior, {guidance} zeta={zeta}, 20 steps: {err:.2e}")
    assert err < 1e-4 * max(1.0, np.abs(ref).max()), err


@pytest.mark.parametrize("precision", ["fp32x3", "fp32"])
def test_dps_guided_worst_chain_vs_f64_oracle_50_steps(dmip, golden, fm, precision):
    """A worst-chain bound for guided DPS over a long horizon: 'norm' guidance, zeta = 0.005, the
    fixture-trained prior, y_test[0], 200 chains x 50 steps, both engines against the f64 oracle (oracle.dps_sample,
    same chain-keyed RNG): EVERY chain within 1e-3 max(1, |ref|). Measured before this test existed
    (profiles/r5_dps_engine_drift.jsonl, same chains): fp32x3 2.4e-5, exact f32 1.4e-4 -- the split engine is the
    closer of the two to the f64 map. The 200-step statistical gate (next test) stays as a second check."""
    _, _, sur = fm
    m = _trained_dps(dmip, golden, fm, 0.005, "norm")
    prior = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy())
             for l in m.prior_net if isinstance(l, torch.nn.Linear)]
    y = golden("data_scat.npz")["y_test"][0]
    n, S = 200, 50
    dmip._lib.clear_range_status(torch.device(DEV))  # an earlier test's chaotic case may have left a range report
    x = m.sample_device(torch.from_numpy(y).to(DEV), n, S, seed=11, precision=precision)[0].cpu().numpy()
    dmip._lib.device_status(torch.device(DEV))  # this launch: no range report, no hand-over timeout
    ref = O.dps_sample(prior, sur, y, n, S, 11, zeta=0.005, mode="norm")
    assert np.all(np.isfinite(x))
    e = np.abs(x.astype(np.float64) - ref).max(1) / max(1.0, np.abs(ref).max())
    print(f"\n[dps] {precision} vs f64 oracle, guided 'norm' zeta=0.005, {S} steps, {n} chains: "
          f"worst chain {e.max():.2e}, median {np.median(e):.2e}")
    assert e.max() < 1e-3, e.max()


def test_dps_fp32x3_vs_exact_f32_many_steps(dmip, golden, fm):
    """The two DPS engines chain by chain (same RNG), 2000 chains, fixture-trained prior:
    * unguided (zeta = 0), the full 1000 steps: every chain within 1e-5 (measured 6.3e-7) -- the split-fp16
      prior and its reverse-mode J^T stay fp32-accurate over a whole trajectory;
    * guided ('norm', zeta = 0.005), 200 steps: the guidance map is chaotic (the exact-f32 engine itself is
      1.4e-4 from the f64 oracle after 50 steps where fp32x3 is 2.4e-5, profiles/r5_dps_engine_drift.jsonl), so
      rounding differences grow on a few chains: median within 1e-5 (3.7e-7), 99th percentile within 1e-2
      (1.8e-3), under 5 % of the chains beyond 1e-3 (1.6 %)."""
    y = torch.from_numpy(golden("data_scat.npz")["y_test"][0]).to(DEV)
    for guidance, zeta, S in (("nll", 0.0, 1000), ("norm", 0.005, 200)):
        m = _trained_dps(dmip, golden, fm, zeta, guidance)
        a = m.sample_device(y, 2000, S, seed=11, precision="fp32x3")[0].cpu().numpy().astype(np.float64)
        b = m.sample_device(y, 2000, S, seed=11, precision="fp32")[0].cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
        e = np.abs(a - b).max(1) / max(1.0, np.abs(b).max())
        print(f"\n[dps] fp32x3 vs exact f32, {guidance} zeta={zeta}, {S} steps: max {e.max():.2e} "
              f"median {np.median(e):.2e} p99 {np.quantile(e, 0.99):.2e}")
        if zeta == 0.0:
            assert e.max() < 1e-5, e.max()
        else:
            assert np.median(e) < 1e-5 and np.quantile(e, 0.99) < 1e-2 and (e > 1e-3).mean() < 0.05
        assert not np.array_equal(a, b)  # two engines ran


def test_dps_fp32x3_out_of_range_weight_falls_back(dmip, golden, fm):
    """A prior weight beyond fp16's range in the split image: an explicit fp32x3 request is refused ("fp16 range"),
    the default precision resamples with the exact-f32 engine (parallel.sample_checked), chain for chain."""
    m, _, _ = _dps_model(dmip, fm, 6, 0.05, "norm")
    with torch.no_grad():
        [l for l in m.prior_net if isinstance(l, torch.nn.Linear)][1].weight[3, 4] = 7.0e4
    y = torch.from_numpy(golden("data_scat.npz")["y_test"][1]).to(DEV)
    with pytest.raises(ValueError, match="fp16 range"):
        m.sample_device(y, 100, 3, seed=2, precision="fp32x3")
    torch.manual_seed(8)
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        x = m(y, num_samples=100, num_steps=3)
    torch.manual_seed(8)
    assert np.array_equal(x, m(y, num_samples=100, num_steps=3, precision="fp32"))


def test_evaluate_scatterometry_driver(dmip, golden, fm, tmp_path):
    """evaluate_scatterometry (main_diffusion_scatterometry.py:40-124) end to end on the device:
    fused sampler for all repeats of a y, fused get_log_posterior for the NLLs, device histograms
    and KL. results.csv has the reference's columns; NLL_mcmc equals the reference-op torch-CPU
    get_log_posterior of the same ground-truth samples (rel 1e-4); the KL2 of our 20k samples against
    the reference sampler's own 20k draws (used as the 'ground truth' here) is below the KL2 of two
    10k halves of those draws against each other (75^3 bins with epsilon smoothing: sparse
    histograms give KL2 ~ 10 even for identical distributions)."""
    import pandas as pd
    from conftest import state_from_npz
    ev = importlib.import_module("diffusion-modelling-for-inverse-problems_amd.evaluate")
    model, pr, _ = fm
    m = dmip.CDE(3, 23, [256] * 3)
    m.sde.a.load_state_dict(state_from_npz(golden("ckpt_scat.npz")))
    s = golden("samples_scat.npz")
    gt = s["samples"].reshape(2, 10000, 3)
    ys = torch.from_numpy(np.stack([s["y"], s["y"]]).astype(np.float32)).to(DEV)
    P = pr.SCAT_PARAMS
    torch.manual_seed(0)
    kl, nlpd, mse = ev.evaluate_scatterometry(
        m, ys, model, str(tmp_path), [], 10000, lambda x, y: torch.zeros_like(x), P["a"], P["b"], P["lambd_bd"],
        None, n_repeats=2, gt_loader=lambda i, j: gt[j], num_steps=int(s["num_steps"]))
    df = pd.read_csv(tmp_path / "results.csv")
    assert list(df.columns)[1:] == ["KL2", "KL_reverse", "NLL_mcmc", "NLL_diffusion", "MSE"] and len(df) == 2
    kl_halves, _ = O.hist_kl(gt[0], gt[1], lim=(-1.2, 1.2))
    assert np.isfinite([kl, nlpd, mse]).all() and kl < kl_halves, (kl, kl_halves, nlpd)
    cpu_fm = torch.nn.Sequential(*[torch.nn.Linear(l.in_features, l.out_features) if isinstance(l, torch.nn.Linear)
                                   else torch.nn.ReLU() for l in model])
    cpu_fm.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    yy = torch.from_numpy(s["y"]).float()[None].expand(10000, -1)
    with torch.no_grad():
        nll_ref = np.mean([float(pr.get_log_posterior(torch.from_numpy(gt[j]), cpu_fm, P["a"], P["b"], yy,
                                                      P["lambd_bd"]).sum()) / 10000 for j in range(2)])
    np.testing.assert_allclose(df["NLL_mcmc"].to_numpy(), nll_ref, rtol=1e-4)
