"""The few-step samplers of the probability-flow ODE (DPM-Solver++(2M), DDIM), host side: the step table against the
scheme stated directly (tests/multistep_ref.py), the orders of the two solvers on the trained checkpoints, what f32
rounding costs at the GPU parity shapes, and the C-ABI's and the Python API's argument validation (include/dmip.h
dmip_multistep_sample). CPU only (no compute calls)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import heun_ref as HR
import multistep_ref as MR
import oracle as O


@pytest.fixture(scope="module")
def lib(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    return dmip._lib.lib()


@pytest.mark.parametrize("grid", ["logsnr", "uniform"])
@pytest.mark.parametrize("solver", MR.SOLVERS)
@pytest.mark.parametrize("kind", ["cde", "posterior"])
def test_table_form_is_the_direct_form(dmip, kind, solver, grid):
    """S = 6 on random weights: the table-driven update in float64 is the scheme written from alpha, sigma and lambda,
    within 1e-12 max(1, |x|) -- at the default VP-SDE and at a non-default one with its own t_end."""
    _, params, prior, y, x0 = HR.parity_case(dmip, kind, 64, 2, 2, 40)
    for sde, t_end in (((O.BETA_MIN, O.BETA_MAX, 1.0), None), ((0.3, 7.0, 1.7), 2e-3)):
        kw = dict(T=sde[2], beta_min=sde[0], beta_max=sde[1], t_end=t_end)
        tab = MR.table_of(dmip, solver, grid, 6, **kw)
        assert tab.dtype == np.float64 and tab.shape == (6, dmip._lib.DMIP_MULTISTEP_COLS)
        got, gs = MR.table_sample(params, x0, y, tab, prior, snapshot_every=1)
        ref, rs = MR.direct_sample(params, x0, y, 6, solver, grid, prior, snapshot_every=1, **kw)
        assert np.all(np.isfinite(ref))
        assert np.all(np.abs(gs - rs) <= 1e-12 * np.maximum(1.0, np.abs(rs))), np.abs(gs - rs).max()
        np.testing.assert_array_equal(got, gs[-1])


@pytest.mark.parametrize("solver", MR.SOLVERS)
def test_one_step_is_the_denoised_estimate(dmip, golden, solver):
    """S = 1 by hand: x_1 = d_0 = (x0 + (sigma^2 / g) a(x0, y, T)) / alpha at tau = T."""
    params = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    y = np.array([0.5, 1.0])
    x0 = HR.x0_of_seed(7, 9, 2).astype(np.float64)
    B = 0.5 * (O.BETA_MAX - O.BETA_MIN) + O.BETA_MIN
    alpha, var, g = np.exp(-0.5 * B), 1.0 - np.exp(-B), np.sqrt(O.BETA_MAX)
    d0 = (x0 + (var / g) * HR.score(params, x0, y, 1.0, g)) / alpha
    for grid in ("logsnr", "uniform"):
        tab = MR.table_of(dmip, solver, grid, 1)
        assert tab[0, 0] == 1.0 and tuple(tab[0, 3:6]) == (0.0, 1.0, 0.0)
        np.testing.assert_allclose(MR.table_sample(params, x0, y, tab), d0, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(MR.direct_sample(params, x0, y, 1, solver, grid), d0, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("grid", ["logsnr", "uniform"])
def test_ddim_is_dpm2m_without_the_history(dmip, grid):
    """The "ddim" table is the "dpm2m" table with c1 zeroed and c0 = -alpha_{i+1} expm1(-h_i) alone: one kernel serves
    both. Rows 0 and S - 1 are first order in both tables."""
    for S in (1, 2, 6, 33):
        t2, t1 = MR.table_of(dmip, "dpm2m", grid, S), MR.table_of(dmip, "ddim", grid, S)
        assert np.all(t1[:, 5] == 0.0) and np.all(t1[:, 7] == 0.0) and np.all(t2[:, 7] == 0.0)
        np.testing.assert_array_equal(t2[:, [0, 1, 2, 3, 6]], t1[:, [0, 1, 2, 3, 6]])
        np.testing.assert_array_equal(t2[[0, -1]], t1[[0, -1]])
        # c0 + c1 of 2M is DDIM's c0: the history's weights sum to one
        np.testing.assert_allclose(t2[:, 4] + t2[:, 5], t1[:, 4], rtol=1e-14, atol=0)
        if S > 2:
            assert np.all(t2[1:-1, 5] < 0.0)


def test_uniform_grid_is_the_samplers_grid(dmip):
    """grid="uniform": the tau column is oracle.schedule's f32 grid bit for bit (default and non-default T), and
    grid="logsnr" runs from T to t_end, strictly decreasing, equally spaced in lambda."""
    for S, T in ((1, 1.0), (7, 1.0), (128, 1.0), (50, 1.7)):
        tab = MR.table_of(dmip, "dpm2m", "uniform", S, T=T)
        np.testing.assert_array_equal(tab[:, 0].astype(np.float32), O.schedule(S, T)[1][:S])
        np.testing.assert_array_equal(tab[:, 0], O.schedule(S, T)[1][:S].astype(np.float64))
    for t_end in (None, 1e-4):
        tab = MR.table_of(dmip, "dpm2m", "logsnr", 64, t_end=t_end)
        tau = tab[:, 0]
        assert tau[0] == 1.0 and tau[-1] == np.float64(np.float32(t_end or 1e-3)) and np.all(np.diff(tau) < 0)
        np.testing.assert_array_equal(tau, MR.grid("logsnr", 64, t_end=t_end))
        lam = MR.vp(tau)[2]
        np.testing.assert_allclose(np.diff(lam), (lam[-1] - lam[0]) / 63, rtol=2e-4)
    for bad in (0.0, 1.0, -1e-3, 2.0):
        with pytest.raises(ValueError, match="t_end"):
            MR.table_of(dmip, "dpm2m", "logsnr", 8, t_end=bad)
    with pytest.raises(ValueError, match="grid"):
        MR.table_of(dmip, "dpm2m", "cosine", 8)
    with pytest.raises(ValueError, match="solver"):
        MR.table_of(dmip, "heun", "logsnr", 8)


@functools.lru_cache(maxsize=None)
def _lin(n=256):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_lin.npz"))
    y = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_lmbd.npz"))["lin_S10_y"]
    params = O.mlp_params_from_state(z)
    x0 = HR.x0_of_seed(1234, n, 2)
    return params, y, x0, HR.heun_sample(params, x0, y, 2048)


def test_orders_on_ckpt_lin(dmip):
    """256 chains of ckpt_lin from the samplers' own x0 (seed 1234), max-abs error against Heun at 2048 steps, on the
    log-SNR grid with t_end = 1e-3: 2M falls by 3-6x from 16 to 32 evaluations (second order; the prototype measured
    4.30), DDIM by 1.6-2.4x from 32 to 64 (first order; 1.98), and 2M at 64 evaluations errs less than a quarter of
    Heun at 32 steps, which makes 64 evaluations (6.6e-4 against 1.21e-2)."""
    params, y, x0, ref = _lin()
    run = lambda solver, S: HR.max_err(MR.table_sample(params, x0, y, MR.table_of(dmip, solver, "logsnr", S)), ref)
    e2 = {S: run("dpm2m", S) for S in (16, 32, 64)}
    e1 = {S: run("ddim", S) for S in (32, 64)}
    e_heun = HR.max_err(HR.heun_sample(params, x0, y, 32), ref)
    print(f"2M {e2}; DDIM {e1}; Heun-32 {e_heun:.3e}; ratios {e2[16] / e2[32]:.2f}, {e1[32] / e1[64]:.2f}")
    assert 3.0 <= e2[16] / e2[32] <= 6.0, e2
    assert 1.6 <= e1[32] / e1[64] <= 2.4, e1
    assert e2[64] < e_heun / 4, (e2[64], e_heun)


def test_dpm2m_128_beats_euler_1000_on_ckpt_scat(dmip, golden):
    """64 chains of ckpt_scat under flow_lmbd.npz's scat_S10_y from the samplers' own x0 (seed 1234), against Heun at
    2048 steps: 2M at 128 evaluations errs less than the lmbd = 1 Euler sampler at 1000 steps. Measured at these 64
    chains: 1.88e-3 against 3.24e-3 (the prototype's 256 chains gave 1.89e-3 against 3.24e-3: the margin holds at 64)."""
    params = O.mlp_params_from_state(golden("ckpt_scat.npz"))
    y = golden("flow_lmbd.npz")["scat_S10_y"]
    x0 = HR.x0_of_seed(1234, 64, 3)
    ref = HR.heun_sample(params, x0, y, 2048)
    e2 = HR.max_err(MR.table_sample(params, x0, y, MR.table_of(dmip, "dpm2m", "logsnr", 128)), ref)
    e_euler = HR.max_err(HR.euler_sample(params, x0, y, 1000), ref)
    print(f"ckpt_scat, 64 chains: 2M-128 {e2:.3e}, Euler-1000 {e_euler:.3e}")
    assert e2 < e_euler, (e2, e_euler)


@pytest.mark.parametrize("solver", MR.SOLVERS)
@pytest.mark.parametrize("kind,W,xd,yd,n", HR.PARITY_CASES)
def test_f32_restatement_is_within_a_quarter_of_the_f32_bound(dmip, kind, W, xd, yd, n, solver):
    """The f32 rounding order of the table-driven update (d = fl(fl(p x) + fl(q a)) at p = 1 / alpha_0 ~ 150 included)
    errs below a quarter of the exact-f32 parity bound of tests/test_gpu_multistep.py (1e-4 max(1, |ref|) at S = 6) at
    every parity shape on both grids at the default VP-SDE, so that bound measures the kernel and not the scheme. The
    cancellation in d costs ~150 ulp of |x| there, but the step multiplies d by c0 = alpha_{i+1} (1 - exp(-h)),
    which gives the factor back."""
    _, params, prior, y, x0 = HR.parity_case(dmip, kind, W, xd, yd, n)
    for grid in ("logsnr", "uniform"):
        tab = MR.table_of(dmip, solver, grid, MR.PARITY_STEPS)
        ref = MR.direct_sample(params, x0, y, MR.PARITY_STEPS, solver, grid, prior)
        r32 = MR.table_sample(params, x0, y, tab, prior, dtype=np.float32)
        e = HR.max_err(r32, ref)
        bound = HR.BOUND["fp32"] * max(1.0, np.abs(ref).max())
        print(f"{kind} W={W} {solver} {grid}: f32 restatement vs f64 = {e:.3e}, max |ref| = {np.abs(ref).max():.3g} "
              f"(a quarter of the bound: {bound / 4:.2e})")
        assert r32.dtype == np.float32 and np.all(np.isfinite(ref))
        assert 0 < e < bound / 4, (e, bound)


def test_new_symbols_exported(lib, dmip):
    for s in ("dmip_multistep_sample", "dmip_multistep_supported"):
        assert s in dmip._lib.EXPORTED and hasattr(lib, s), s
    assert lib.dmip_abi_version() == dmip._lib.ABI_VERSION == 9
    assert dmip._lib.TABLE_SOLVERS == ("dpm2m", "ddim") and dmip._lib.DMIP_MULTISTEP_COLS == 8
    # not a value of dmip_solver: dmip_ode_sample keeps refusing 2
    assert dmip._lib.SOLVERS == {"euler": 0, "heun": 1}
    assert not lib.dmip_ode_sample_supported(0, 256, 3, 3, 23, dmip._lib.DMIP_PREC_F32X3, 2)


def _ms(lib, L, mode, net, prior, y, table, out, num_steps=10, cols=8, precision=None, x0=None, snapshot_every=0,
        snaps=None):
    return lib.dmip_multistep_sample(mode, net, prior, y, 1, 2, 2, 10, 0, num_steps, table, cols, 0.0, 1.0, 1,
                                     L.DMIP_PREC_F32 if precision is None else precision, x0, snapshot_every, snaps,
                                     out, None)


def test_multistep_sample_rejects_bad_arguments(lib, dmip):
    """Every refusal comes before any device work (a network handle cannot be made without a device: the checks under
    test come before it is read), with the documented code."""
    L = dmip._lib
    C, P = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR
    buf = (ctypes.c_float * 80)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # modes other than CDE / Posterior
    assert _ms(lib, L, L.DMIP_SAMPLER_CDIFFE, None, None, p, p, p) == L.DMIP_ERR_INVALID
    assert _ms(lib, L, 7, None, None, p, p, p) == L.DMIP_ERR_INVALID
    # a wrong table_cols
    for cols in (0, 7, 9):
        assert _ms(lib, L, C, None, None, p, p, p, cols=cols) == L.DMIP_ERR_INVALID
        assert b"table_cols" in lib.dmip_last_error()
    # num_steps < 1, on its own account
    for S in (0, -3):
        assert _ms(lib, L, C, None, None, p, p, p, num_steps=S) == L.DMIP_ERR_INVALID
        assert b"num_steps" in lib.dmip_last_error()
    # the snapshot rules of dmip_em_sample_lmbd
    for every, snaps in ((-1, p), (11, p), (5, None)):
        assert _ms(lib, L, C, None, None, p, p, p, snapshot_every=every, snaps=snaps) == L.DMIP_ERR_INVALID
        assert b"snapshot_every" in lib.dmip_last_error()
    # null arguments (network, y, table, output; Posterior without a prior)
    assert _ms(lib, L, C, None, None, p, p, p) == L.DMIP_ERR_INVALID
    assert b"null" in lib.dmip_last_error()
    assert _ms(lib, L, C, p, None, None, p, p) == L.DMIP_ERR_INVALID
    assert _ms(lib, L, C, p, None, p, None, p) == L.DMIP_ERR_INVALID
    assert b"null" in lib.dmip_last_error()
    assert _ms(lib, L, C, p, None, p, p, None) == L.DMIP_ERR_INVALID
    assert _ms(lib, L, P, p, None, p, p, p) == L.DMIP_ERR_INVALID
    # there is no 16-bit kernel
    assert _ms(lib, L, C, p, None, p, p, p, precision=L.DMIP_PREC_FP16) == L.DMIP_ERR_UNSUPPORTED
    assert b"16-bit" in lib.dmip_last_error()
    # dmip_ode_sample's solver stays a two-valued enum
    sde = L.vpsde(0.1, 20.0, 1.0)
    assert lib.dmip_ode_sample(C, None, None, ctypes.byref(sde), p, 1, 2, 2, 10, 0, 10, 0.0, 1.0, 1, L.DMIP_PREC_F32, 2,
                               None, 0, None, p, None) == L.DMIP_ERR_INVALID


def test_multistep_supported_shapes(lib, dmip):
    L = dmip._lib
    sup = L.multistep_supported
    P = L.DMIP_SAMPLER_POSTERIOR
    # fp32x3 (the one-tile engine): every shape of the Heun kernels
    for W in (64, 128, 256, 512):
        for nh in (1, 2, 3):
            for xd in (2, 3):
                assert sup(W, nh, xd, 23, precision="fp32x3"), (W, nh, xd)
                assert sup(W, nh, xd, 23, P, "fp32x3"), (W, nh, xd)
                for mode in (L.DMIP_SAMPLER_CDE, P):
                    for prec in ("fp32", "fp32x3"):
                        assert sup(W, nh, xd, 23, mode, prec) == L.ode_sample_supported(W, nh, xd, 23, mode, prec)
    assert sup(64, 3, 2, 2, precision="fp32") and sup(256, 3, 3, 23, precision="fp32")
    assert sup(64, 3, 2, 2, P, "fp32") and sup(128, 2, 3, 23, P, "fp32")
    # no 16-bit kernel; CDiffE has no ODE form; shapes without a sampler
    assert not sup(256, 3, 3, 23, precision="fp16")
    assert not sup(64, 3, 2, 2, L.DMIP_SAMPLER_CDIFFE, "fp32x3")
    assert not sup(96, 3, 3, 23) and not sup(256, 4, 3, 23) and not sup(256, 3, 4, 9)
    # the exact-f32 engine at width 512 with the tanh chain would spill: left out, as its Heun kernels are
    for xd in (2, 3):
        assert not sup(512, 3, xd, 23, P, "fp32") and not sup(512, 3, xd, 23, precision="fp32")


def test_python_refusals(dmip):
    """ValueError before any device is looked for."""
    y2, y23 = torch.zeros(2), torch.zeros(23)
    A = np.eye(2)
    for solver in dmip._lib.TABLE_SOLVERS:
        for m, y in ((dmip.CDiffE(2, 2, [64] * 3), y2), (dmip.DPS(3, 23, [256] * 3), y23),
                     (dmip.LinearDPS(2, 2, [64] * 3, A), y2)):
            with pytest.raises(ValueError, match=solver):
                m.sample_device(y, 4, 2, solver=solver)
        with pytest.raises(ValueError, match=solver):
            dmip.CDiffE(2, 2, [64] * 3).forward(y2, num_samples=4, num_steps=2, solver=solver)
        for m in (dmip.CDE(2, 2, [64] * 3), dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)):
            with pytest.raises(ValueError, match="lmbd"):
                m.sample_device(y2, 4, 2, solver=solver, lmbd=0.5)
            with pytest.raises(ValueError, match="lmbd"):
                m.forward(y2, num_samples=4, num_steps=2, solver=solver, lmbd=0.5)
            with pytest.raises(ValueError, match="lmbd"):
                m.sample_trajectory(y2, 4, 2, 1, solver=solver, lmbd=0.25)
            with pytest.raises(ValueError, match="noise="):
                m.sample_device(y2, 4, 2, solver=solver, noise=torch.zeros(3, 1, 4, 2))
            for bad in (0.0, 1.0, -1.0):
                with pytest.raises(ValueError, match="t_end"):
                    m.sample_device(y2, 4, 2, solver=solver, t_end=bad)
                with pytest.raises(ValueError, match="t_end"):
                    m.forward(y2, num_samples=4, num_steps=2, solver=solver, t_end=bad)
            with pytest.raises(ValueError, match="grid"):
                m.sample_device(y2, 4, 2, solver=solver, grid="cosine")
    for m in (dmip.CDE(2, 2, [64] * 3), dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)):
        # the existing messages stay: an unknown solver, Heun's own refusals, and grid= / t_end= without their solvers
        with pytest.raises(ValueError, match="solver"):
            m.sample_device(y2, 4, 2, solver="rk4")
        with pytest.raises(ValueError, match="lmbd"):
            m.sample_device(y2, 4, 2, solver="heun", lmbd=0.5)
        with pytest.raises(ValueError, match="noise="):
            m.sample_device(y2, 4, 2, x0=torch.zeros(1, 4, 2))
        for solver in ("euler", "heun"):
            with pytest.raises(ValueError, match="t_end"):
                m.sample_device(y2, 4, 2, solver=solver, t_end=1e-3)
            with pytest.raises(ValueError, match="grid"):
                m.sample_device(y2, 4, 2, solver=solver, grid="uniform")
    with pytest.raises(ValueError, match="heun"):
        dmip.CDiffE(2, 2, [64] * 3).sample_device(y2, 4, 2, solver="heun")
