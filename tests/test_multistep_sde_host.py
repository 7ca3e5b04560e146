"""The stochastic few-step samplers (eta= on solver="dpm2m" / "ddim": SDE-DPM-Solver++(2M), ancestral / eta-DDIM), host
side: the step table's noise column and eta-dependent coefficients against the scheme stated directly
(tests/multistep_sde_ref.py), the two marginal identities, what f32 rounding costs at the GPU parity shapes, the
closed-form Gaussian statistic on the reference alone, and the argument plumbing (include/dmip.h
dmip_multistep_sde_sample). CPU only (no compute calls)."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import heun_ref as HR
import multistep_ref as MR
import multistep_sde_ref as R
import oracle as O
import sde_cases as SC

SDES = {"default": (O.BETA_MIN, O.BETA_MAX, 1.0), "B": SC.SDES["B"]}


@pytest.fixture(scope="module")
def lib(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    return dmip._lib.lib()


# ------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("grid", ["logsnr", "uniform"])
@pytest.mark.parametrize("solver", R.SOLVERS)
def test_eta_zero_is_the_deterministic_table(dmip, solver, grid):
    """eta = 0 (and eta left out) is today's array bit for bit, at the default SDE and at SDE B, with a zero column 7."""
    for sde in SDES.values():
        for S in (1, 2, 6, 33):
            old = MR.table_of(dmip, solver, grid, S, **SC.kw(sde))
            for eta in (0.0, 0, -0.0):
                new = R.table_of(dmip, solver, grid, S, eta, **SC.kw(sde))
                assert new.dtype == np.float64
                np.testing.assert_array_equal(new, old)
            assert np.all(old[:, 7] == 0.0)


@pytest.mark.parametrize("eta", R.ETAS)
@pytest.mark.parametrize("solver", R.SOLVERS)
@pytest.mark.parametrize("sde", list(SDES), ids=list(SDES))
def test_marginal_identities(dmip, sde, solver, eta):
    """cx alpha_i + c0 + c1 = alpha_{i+1} and cx^2 sigma_i^2 + cn^2 = sigma_{i+1}^2 to rtol 1e-12: a step maps the exact
    marginal of a point mass to the exact marginal, for every eta, solver and grid."""
    kw = SC.kw(SDES[sde])
    for grid in ("logsnr", "uniform"):
        for S in (2, 8, 16, 32, 64, 128):
            tab = R.table_of(dmip, solver, grid, S, eta, **kw)
            alpha, sigma, _, _ = MR.vp(tab[:, 0], kw["beta_min"], kw["beta_max"])
            cx, c0, c1, cn = tab[:-1, 3], tab[:-1, 4], tab[:-1, 5], tab[:-1, 7]
            np.testing.assert_allclose(cx * alpha[:-1] + c0 + c1, alpha[1:], rtol=1e-12, atol=0)
            np.testing.assert_allclose(cx ** 2 * sigma[:-1] ** 2 + cn ** 2, sigma[1:] ** 2, rtol=1e-12, atol=0)
            assert np.all(cn > 0) and np.all(cx > 0)


@pytest.mark.parametrize("eta", R.ETAS + (2.5,))
@pytest.mark.parametrize("solver", R.SOLVERS)
def test_columns_match_the_scheme(dmip, solver, eta):
    """Column 7 and cx, c0, c1 against the reference module's own formulas (exp where the package uses expm1, its own
    grid), rtol 1e-10; the columns eta does not touch are the deterministic table's; the last row is (0, 1, 0, 0)."""
    for sde in SDES.values():
        kw = SC.kw(sde)
        for grid in ("logsnr", "uniform"):
            for S in (1, 2, 6, 33):
                tab = R.table_of(dmip, solver, grid, S, eta, **kw)
                tau = MR.grid(grid, S, **kw)
                np.testing.assert_array_equal(tab[:, 0], tau)
                cx, c0, c1, cn = R.coefficients(solver, eta, tau, kw["beta_min"], kw["beta_max"])
                for col, ref in ((3, cx), (4, c0), (5, c1), (7, cn)):
                    np.testing.assert_allclose(tab[:-1, col], ref, rtol=1e-10, atol=0, err_msg=f"column {col}")
                assert tuple(tab[-1, [3, 4, 5, 7]]) == (0.0, 1.0, 0.0, 0.0)
                np.testing.assert_array_equal(tab[:, [0, 1, 2, 6]], MR.table_of(dmip, solver, grid, S, **kw)[:, [0, 1, 2, 6]])
                if solver == "ddim":
                    assert np.all(tab[:, 5] == 0.0)


def test_eta_one_is_the_published_form(dmip):
    """eta = 1, "ddim" is ancestral sampling in its usual variance form: the posterior q(x_{i+1} | x_i, d) of the VP
    chain has mean weight rho = (alpha / alpha') sigma'^2 / sigma^2 on x and alpha' - rho alpha on d, and variance
    sigma'^2 (1 - (alpha sigma' / (alpha' sigma))^2)."""
    tab = R.table_of(dmip, "ddim", "logsnr", 12, 1.0)
    alpha, sigma, _, _ = MR.vp(tab[:, 0])
    a0, a1, s0, s1 = alpha[:-1], alpha[1:], sigma[:-1], sigma[1:]
    ratio = (a0 / a1) * s1 ** 2 / s0 ** 2
    np.testing.assert_allclose(tab[:-1, 3], ratio, rtol=1e-10)
    np.testing.assert_allclose(tab[:-1, 4], a1 - ratio * a0, rtol=1e-10)
    np.testing.assert_allclose(tab[:-1, 7] ** 2, s1 ** 2 * (1.0 - (a0 * s1 / (a1 * s0)) ** 2), rtol=1e-10)


def test_bad_eta_raises(dmip):
    for bad in (-0.1, -1, float("nan"), float("inf"), -float("inf"), "half", None):
        with pytest.raises(ValueError, match="eta"):
            R.table_of(dmip, "dpm2m", "logsnr", 8, bad)
    m = dmip.CDE(2, 2, [64] * 3)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eta"):
            m.sample_device(torch.zeros(2), 4, 2, solver="dpm2m", eta=bad)


# ------------------------------------------------------------------------------ the restatement
def _normals(case, S=R.PARITY_STEPS):
    kind, W, xd, yd, n = case
    return R.chain_normals(1000 + W, n, xd, S)[1]


@pytest.mark.parametrize("eta", R.ETAS)
@pytest.mark.parametrize("solver", R.SOLVERS)
@pytest.mark.parametrize("case", HR.PARITY_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_table_form_is_the_direct_form_and_f32_costs_little(dmip, case, solver, eta):
    """At the parity cases' networks with shared normals, S = 6: the table-driven update in float64 is the scheme written
    from alpha, sigma and lambda within 1e-9 max(1, |x|) at every step, and its f32 rounding order, the noise added
    last, errs below a quarter of the exact-f32 device parity bound (1e-4 max(1, |ref|)), so that bound measures the
    kernel and not the scheme."""
    _, params, prior, y, x0 = HR.parity_case(dmip, *case)
    xi = _normals(case)
    for grid in ("logsnr", "uniform"):
        tab = R.table_of(dmip, solver, grid, R.PARITY_STEPS, eta)
        ref, rs = R.direct_sample(params, x0, y, R.PARITY_STEPS, xi, solver, eta, grid, prior, snapshot_every=1)
        got, gs = R.table_sample(params, x0, y, tab, xi, prior, snapshot_every=1)
        assert np.all(np.isfinite(ref))
        assert np.all(np.abs(gs - rs) <= 1e-9 * np.maximum(1.0, np.abs(rs))), np.abs(gs - rs).max()
        r32 = R.table_sample(params, x0, y, tab, xi, prior, dtype=np.float32)
        e = HR.max_err(r32, ref)
        bound = HR.BOUND["fp32"] * max(1.0, np.abs(ref).max())
        print(f"{case[0]} W={case[1]} {solver} eta={eta} {grid}: f32 restatement vs f64 = {e:.3e}, max |ref| = "
              f"{np.abs(ref).max():.3g} (a quarter of the bound: {bound / 4:.2e})")
        assert r32.dtype == np.float32
        assert 0 < e < bound / 4, (e, bound)
        # the noise matters: without it the chains end elsewhere by far more than the bound
        assert HR.max_err(MR.direct_sample(params, x0, y, R.PARITY_STEPS, solver, grid, prior), ref) > 100 * bound


def test_zero_noise_column_is_the_deterministic_restatement(dmip):
    """table_sample with the eta = 0 table is multistep_ref.table_sample bit for bit, whatever the normals are (f32 and
    f64): cn xi = 0 changes no bit of a finite sum."""
    case = HR.PARITY_CASES[0]
    _, params, prior, y, x0 = HR.parity_case(dmip, *case)
    xi = _normals(case)
    tab = MR.table_of(dmip, "dpm2m", "logsnr", R.PARITY_STEPS)
    for dt in (np.float32, np.float64):
        np.testing.assert_array_equal(R.table_sample(params, x0, y, tab, xi, prior, dtype=dt),
                                      MR.table_sample(params, x0, y, tab, prior, dtype=dt))


def test_chain_normals_are_the_euler_samplers(dmip):
    """x0 and xi_0 .. xi_{S-1} are what oracle.em_sample(rng_state=) consumes: an Euler run fed them as injected noise
    is the oracle's product-RNG run bit for bit; and they follow chain_offset and the y index."""
    params = O.mlp_params_from_state(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                                          "ckpt_lin.npz")))
    y = np.array([0.5, 1.0], np.float32)
    x0, xi = R.chain_normals(1234, 40, 2, 5, mean=0.3, std=1.5)
    ref = O.cde_sample(params, y, 40, 5, 1234, mean=0.3, std=1.5)
    got = O.em_sample(lambda x, tau: O.cde_a(params, x, y, tau), x0, 5, noise=xi)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(x0, HR.x0_of_seed(1234, 40, 2, mean=0.3, std=1.5))
    x0s, xis = R.chain_normals(1234, 10, 2, 5, chain_offset=30, mean=0.3, std=1.5)
    np.testing.assert_array_equal(x0s, x0[30:])
    np.testing.assert_array_equal(xis, xi[:, 30:])
    assert not np.array_equal(R.chain_normals(1234, 40, 2, 5, stream=1)[1], R.chain_normals(1234, 40, 2, 5)[1])


# ------------------------------------------------------------------------------ the Gaussian statistic
def test_gaussian_recursion_figures():
    """The recursion's own figures: eta = 0 keeps corr(x_S, x_0) = 1 (a deterministic linear map), and two published
    values of the issue that introduced it."""
    for solver in R.SOLVERS:
        assert abs(R.gaussian_stats(solver, 0.0, 16)[1] - 1.0) < 1e-12
    std, corr = R.gaussian_stats("dpm2m", 1.0, 16)
    assert abs(std - 1.0445) < 5e-5 and abs(corr - 0.0063) < 5e-5
    std, corr = R.gaussian_stats("ddim", 1.0, 6)
    assert abs(std - 0.4830) < 5e-5 and abs(corr - 0.0136) < 5e-5


@pytest.mark.parametrize("solver,eta,S", R.GAUSS_CASES)
def test_gaussian_statistic_of_the_reference(solver, eta, S):
    """Data N(0, I), a = -g x exactly: 20,000 chains of the float64 scheme on the oracle's normals end with the sample
    std and corr(x_S, x_0) of the closed-form recursion within 4 standard errors, per coordinate. A missing noise term
    leaves corr = 1; a mis-scaled one moves the std by many standard errors."""
    x0, xi = R.chain_normals(31, R.GAUSS_N, 2, S)
    x = R.direct_sample(None, x0, None, S, xi, solver, eta, score_fn=R.gaussian_score)
    R.check_gaussian(x, x0, solver, eta, S)
    # the check separates: the same chains with the noise scaled by 1.1 miss it
    with pytest.raises(AssertionError):
        R.check_gaussian(R.direct_sample(None, x0, None, S, 1.1 * xi, solver, eta, score_fn=R.gaussian_score), x0,
                         solver, eta, S, "noise x 1.1: ")


# ------------------------------------------------------------------------------ plumbing
def test_new_symbols_exported(lib, dmip):
    for s in ("dmip_multistep_sde_sample", "dmip_multistep_sde_supported"):
        assert s in dmip._lib.EXPORTED and hasattr(lib, s), s
    assert lib.dmip_abi_version() == dmip._lib.ABI_VERSION == 9
    assert dmip._lib.DMIP_MULTISTEP_COLS == 8


def test_supported_shapes_are_the_deterministic_samplers(lib, dmip):
    L = dmip._lib
    for W in (64, 96, 128, 256, 512):
        for nh in (1, 2, 3, 4):
            for xd in (2, 3, 4):
                for mode in (L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR, L.DMIP_SAMPLER_CDIFFE):
                    for prec in ("fp32", "fp32x3", "fp16"):
                        assert L.multistep_sde_supported(W, nh, xd, 23, mode, prec) == \
                            L.multistep_supported(W, nh, xd, 23, mode, prec), (W, nh, xd, mode, prec)
    assert L.multistep_sde_supported(256, 3, 3, 23) and not L.multistep_sde_supported(512, 3, 3, 23, precision="fp32")


def _ms(lib, L, mode, net, prior, y, table, out, num_steps=10, cols=8, precision=None, x0=None, snapshot_every=0,
        snaps=None):
    return lib.dmip_multistep_sde_sample(mode, net, prior, y, 1, 2, 2, 10, 0, num_steps, table, cols, 0.0, 1.0, 1,
                                         L.DMIP_PREC_F32 if precision is None else precision, x0, snapshot_every, snaps,
                                         out, None)


def test_sde_sample_rejects_bad_arguments(lib, dmip):
    """dmip_multistep_sample's refusals in its order, each before any device work."""
    L = dmip._lib
    C, P = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR
    buf = (ctypes.c_float * 80)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _ms(lib, L, L.DMIP_SAMPLER_CDIFFE, None, None, p, p, p, cols=7, num_steps=0) == L.DMIP_ERR_INVALID
    assert b"CDE and Posterior" in lib.dmip_last_error()
    for cols in (0, 7, 9):
        assert _ms(lib, L, C, None, None, p, p, p, cols=cols, num_steps=0) == L.DMIP_ERR_INVALID
        assert b"table_cols" in lib.dmip_last_error()
    for S in (0, -3):
        assert _ms(lib, L, C, None, None, p, p, p, num_steps=S, snapshot_every=-1) == L.DMIP_ERR_INVALID
        assert b"num_steps" in lib.dmip_last_error()
    for every, snaps in ((-1, p), (11, p), (5, None)):
        assert _ms(lib, L, C, None, None, p, p, p, snapshot_every=every, snaps=snaps) == L.DMIP_ERR_INVALID
        assert b"snapshot_every" in lib.dmip_last_error()
    for args in ((C, None, None, p, p, p), (C, p, None, None, p, p), (C, p, None, p, None, p), (C, p, None, p, p, None),
                 (P, p, None, p, p, p)):
        assert _ms(lib, L, *args, precision=L.DMIP_PREC_FP16) == L.DMIP_ERR_INVALID
        assert b"null" in lib.dmip_last_error()
    assert _ms(lib, L, C, p, None, p, p, p, precision=L.DMIP_PREC_FP16) == L.DMIP_ERR_UNSUPPORTED
    assert b"16-bit" in lib.dmip_last_error()


def test_python_refusals(dmip):
    """ValueError before any device is looked for: eta belongs to the table solvers; noise= stays refused."""
    y2 = torch.zeros(2)
    for m in (dmip.CDE(2, 2, [64] * 3), dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)):
        for solver in ("euler", "heun"):
            with pytest.raises(ValueError, match="eta"):
                m.sample_device(y2, 4, 2, solver=solver, eta=1.0)
            with pytest.raises(ValueError, match="eta"):
                m.forward(y2, num_samples=4, num_steps=2, solver=solver, eta=0.5)
            with pytest.raises(ValueError, match="eta"):
                m.sample_trajectory(y2, 4, 2, 1, solver=solver, eta=1.0)
        for solver in dmip._lib.TABLE_SOLVERS:
            for eta in (0.0, 1.0):
                with pytest.raises(ValueError, match="noise="):
                    m.sample_device(y2, 4, 2, solver=solver, eta=eta, noise=torch.zeros(3, 1, 4, 2))
            with pytest.raises(ValueError, match="lmbd"):
                m.sample_device(y2, 4, 2, solver=solver, eta=1.0, lmbd=0.5)
            with pytest.raises(ValueError, match="t_end"):
                m.sample_device(y2, 4, 2, solver=solver, eta=1.0, t_end=0.0)


def test_loop_adds_the_noise_from_the_em_loops_streams(dmip, monkeypatch):
    """_multistep_device_loop on CPU tensors with the generator replaced by the oracle's: step i reads the normals of
    stream sid + 1 + i at the shard's chain_offset (as _em_device_loop does), x0 comes from stream sid, and the result is
    the f32 table update with cn xi added last; stochastic=False reads no step noise and is the deterministic loop."""
    est = importlib.import_module(dmip.__name__ + ".estimators")
    asked = []

    def normals(seed, chain_offset, stream_id, n, d, dev):
        asked.append((seed, chain_offset, stream_id - est._LOOP_STREAM, n, d))
        st = O.rng_init(seed, np.arange(chain_offset, chain_offset + n), stream_id)
        return torch.from_numpy(O.rng_normals(st, d).copy())

    monkeypatch.setattr(est, "_loop_normals", normals)

    class M:
        xdim = 3

    S, n, off, seed = 5, 40, 7, 11
    tab64 = R.table_of(dmip, "dpm2m", "logsnr", S, 1.0)
    tab = torch.from_numpy(tab64).to(torch.float32)
    ys = torch.zeros(2, 4)
    score = lambda x, y, tvec, g: -g * x  # noqa: E731
    out = est._multistep_device_loop(M, ys, n, seed, off, 0.25, 2.0, None, tab, score, stochastic=True)
    assert out.shape == (2, n, 3)
    assert asked == [(seed, off, (k << 40) + j, n, 3) for k in range(2) for j in range(S + 1)]
    F = np.float32
    for k in range(2):
        draw = lambda j: O.rng_normals(O.rng_init(seed, np.arange(off, off + n), est._LOOP_STREAM + (k << 40) + j), 3)
        x = (draw(0) * F(2.0) + F(0.25)).astype(F)
        d_prev = np.zeros_like(x)
        for i, (tau, p, q, cx, c0, c1, g, cn) in enumerate(tab.numpy()):
            d = (p * x + q * (-g * x)).astype(F)
            x = (((cx * x + c0 * d).astype(F) + c1 * d_prev).astype(F) + cn * draw(1 + i)).astype(F)
            d_prev = d
        np.testing.assert_array_equal(out[k].numpy(), x)
    asked.clear()
    det = est._multistep_device_loop(M, ys, n, seed, off, 0.25, 2.0, None, tab, score)
    assert asked == [(seed, off, k << 40, n, 3) for k in range(2)]
    assert not torch.equal(det, out)
