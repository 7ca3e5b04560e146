"""The second-order (Heun) sampler of the probability-flow ODE, host side: the order of the restatement
(tests/heun_ref.py) on a trained checkpoint, what f32 rounding costs it at the GPU parity shapes, and the C-ABI's
argument validation (include/dmip.h dmip_ode_sample). CPU only (no compute calls)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import heun_ref as HR
import oracle as O


@pytest.fixture(scope="module")
def lib(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    return dmip._lib.lib()


def test_restatement_is_second_order_on_ckpt_lin(golden):
    """256 chains of ckpt_lin under the fixture's y from the samplers' own x0 (seed 1234), against Heun at 2048
    steps: the error falls by 3-5x per halving of the step (measured 3.65 and 3.85: order 2), and Heun at 128 steps
    (256 network evaluations) beats the lmbd = 1 Euler sampler at 1000 (measured 8.2e-4 against 2.0e-3)."""
    params = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    y = golden("flow_lmbd.npz")["lin_S10_y"]
    x0 = HR.x0_of_seed(1234, 256, 2)
    ref = HR.heun_sample(params, x0, y, 2048)
    err = {S: HR.max_err(HR.heun_sample(params, x0, y, S), ref) for S in (32, 64, 128)}
    e_euler = HR.max_err(HR.euler_sample(params, x0, y, 1000), ref)
    print(f"Heun err vs Heun-2048: {err}; Euler-1000: {e_euler:.3e}; "
          f"ratios {err[32] / err[64]:.2f}, {err[64] / err[128]:.2f}")
    assert 3.0 <= err[32] / err[64] <= 5.0, err
    assert 3.0 <= err[64] / err[128] <= 5.0, err
    assert err[128] < e_euler, (err[128], e_euler)


def test_restatement_at_one_step_is_the_trapezoid(golden):
    """S = 1 by hand: k1 at (x0, tau = T), k2 at (x0 + k1, tau = 0), x1 = x0 + (k1 + k2) / 2."""
    params = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    y = np.array([0.5, 1.0])
    x0 = HR.x0_of_seed(7, 9, 2).astype(np.float64)
    tau, beta, g = HR.grid(1)
    assert tau[0] == 1.0 and tau[1] == 0.0
    k1 = 0.5 * g[0] * HR.score(params, x0, y, tau[0], g[0]) + 0.5 * beta[0] * x0
    xt = x0 + k1
    k2 = 0.5 * g[1] * HR.score(params, xt, y, tau[1], g[1]) + 0.5 * beta[1] * xt
    np.testing.assert_allclose(HR.heun_sample(params, x0, y, 1), x0 + 0.5 * (k1 + k2), rtol=0, atol=1e-14)


@pytest.mark.parametrize("kind,W,xd,yd,n", HR.PARITY_CASES)
def test_f32_restatement_is_within_a_quarter_of_the_f32_bound(dmip, kind, W, xd, yd, n):
    """The f32 rounding order of the scheme itself errs below a quarter of the exact-f32 parity bound of
    tests/test_gpu_heun.py (1e-4 max(1, |ref|) at S = 5) at every parity shape, so that bound measures the kernel and
    not the scheme. Measured: 4.5e-5 to 8.7e-5 at |ref| of 250 to 290 (untrained weights: five steps of this ODE
    grow |x| that far), 2e-7 relative, against a quarter-bound of 6.2e-3 to 7.3e-3."""
    _, params, prior, y, x0 = HR.parity_case(dmip, kind, W, xd, yd, n)
    ref = HR.heun_sample(params, x0, y, HR.PARITY_STEPS, prior)
    r32 = HR.heun_sample(params, x0, y, HR.PARITY_STEPS, prior, dtype=np.float32)
    e = HR.max_err(r32, ref)
    bound = HR.BOUND["fp32"] * max(1.0, np.abs(ref).max())
    print(f"{kind} W={W}: f32 restatement vs f64 = {e:.3e} (a quarter of the bound: {bound / 4:.2e})")
    assert r32.dtype == np.float32 and np.all(np.isfinite(ref))
    assert 0 < e < bound / 4, (e, bound)


def test_new_symbols_exported(lib, dmip):
    for s in ("dmip_ode_sample", "dmip_ode_sample_supported"):
        assert s in dmip._lib.EXPORTED and hasattr(lib, s), s
    assert dmip._lib.DMIP_SOLVER_EULER == 0 and dmip._lib.DMIP_SOLVER_HEUN == 1


def _ode(lib, L, mode, net, prior, sde, y, out, solver=1, num_steps=10, x0=None, snapshot_every=0, snaps=None,
         precision=None):
    return lib.dmip_ode_sample(mode, net, prior, ctypes.byref(sde) if sde is not None else None, y, 1, 2, 2, 10, 0,
                               num_steps, 0.0, 1.0, 1, L.DMIP_PREC_F32 if precision is None else precision, solver, x0,
                               snapshot_every, snaps, out, None)


def test_ode_sample_rejects_bad_arguments(lib, dmip):
    """Every refusal comes before any device work (a network handle cannot be made without a device: the checks
    under test come before it is read), with the documented code."""
    L = dmip._lib
    sde = L.vpsde(0.1, 20.0, 1.0)
    C, P = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for solver in (L.DMIP_SOLVER_EULER, L.DMIP_SOLVER_HEUN):
        # modes other than CDE / Posterior
        assert _ode(lib, L, L.DMIP_SAMPLER_CDIFFE, None, None, sde, p, p, solver) == L.DMIP_ERR_INVALID
        assert _ode(lib, L, 7, None, None, sde, p, p, solver) == L.DMIP_ERR_INVALID
        # null arguments (network, sde, y, output; Posterior without a prior)
        assert _ode(lib, L, C, None, None, sde, p, p, solver) == L.DMIP_ERR_INVALID
        assert b"null" in lib.dmip_last_error()
        assert _ode(lib, L, C, p, None, None, p, p, solver) == L.DMIP_ERR_INVALID
        assert _ode(lib, L, C, p, None, sde, None, p, solver) == L.DMIP_ERR_INVALID
        assert _ode(lib, L, C, p, None, sde, p, None, solver) == L.DMIP_ERR_INVALID
        assert _ode(lib, L, P, p, None, sde, p, p, solver) == L.DMIP_ERR_INVALID
        # num_steps < 1, on its own account
        for S in (0, -3):
            assert _ode(lib, L, C, None, None, sde, p, p, solver, num_steps=S) == L.DMIP_ERR_INVALID
            assert b"num_steps" in lib.dmip_last_error()
        # the snapshot rules of dmip_em_sample_lmbd
        for every, snaps in ((-1, p), (11, p), (5, None)):
            assert _ode(lib, L, C, None, None, sde, p, p, solver, snapshot_every=every, snaps=snaps) == \
                L.DMIP_ERR_INVALID
            assert b"snapshot_every" in lib.dmip_last_error()
    # an unknown solver
    for bad in (2, -1):
        assert _ode(lib, L, C, None, None, sde, p, p, bad) == L.DMIP_ERR_INVALID
        assert b"solver" in lib.dmip_last_error()
    # Euler starts from injected noise, not from x0
    assert _ode(lib, L, C, None, None, sde, p, p, L.DMIP_SOLVER_EULER, x0=p) == L.DMIP_ERR_UNSUPPORTED
    assert b"x0" in lib.dmip_last_error()


def test_ode_sample_supported_shapes(lib, dmip):
    L = dmip._lib
    sup = L.ode_sample_supported
    P = L.DMIP_SAMPLER_POSTERIOR
    # fp32x3 (the one-tile engine): every shape of the Euler CDE / Posterior kernels
    for W in (64, 128, 256, 512):
        for nh in (1, 2, 3):
            for xd in (2, 3):
                assert sup(W, nh, xd, 23, precision="fp32x3"), (W, nh, xd)
                assert sup(W, nh, xd, 23, P, "fp32x3"), (W, nh, xd)
    assert sup(64, 3, 2, 2, precision="fp32") and sup(256, 3, 3, 23, precision="fp32")
    assert sup(64, 3, 2, 2, P, "fp32") and sup(128, 2, 3, 23, P, "fp32")
    # no 16-bit Heun kernel; CDiffE has no ODE form; shapes without a sampler
    assert not sup(256, 3, 3, 23, precision="fp16")
    assert not sup(64, 3, 2, 2, L.DMIP_SAMPLER_CDIFFE, "fp32x3")
    assert not sup(96, 3, 3, 23) and not sup(256, 4, 3, 23) and not sup(256, 3, 4, 9)
    assert not lib.dmip_ode_sample_supported(0, 256, 3, 3, 23, L.DMIP_PREC_F32X3, 2)
    # Euler: what the lmbd samplers support, in any precision
    for prec in ("fp16", "fp32", "fp32x3"):
        assert sup(256, 3, 3, 23, precision=prec, solver="euler") == L.sampler_supported(256, 3, 3, 23, precision=prec)
    # the exact-f32 engine is register-bound at width 512: with the tanh chain those Heun instantiations would spill
    # (as their Euler kernels do) and are left out
    assert sup(256, 3, 3, 23, P, "fp32") and sup(256, 3, 2, 2, precision="fp32")
    for xd in (2, 3):
        assert not sup(512, 3, xd, 23, P, "fp32") and not sup(512, 3, xd, 23, precision="fp32")


def test_python_refusals(dmip):
    """ValueError before any device is looked for."""
    y2, y23 = torch.zeros(2), torch.zeros(23)
    for m, y in ((dmip.CDiffE(2, 2, [64] * 3), y2), (dmip.DPS(3, 23, [256] * 3), y23)):
        with pytest.raises(ValueError, match="heun"):
            m.sample_device(y, 4, 2, solver="heun")
    with pytest.raises(ValueError, match="heun"):
        dmip.CDiffE(2, 2, [64] * 3).forward(y2, num_samples=4, num_steps=2, solver="heun")
    for m in (dmip.CDE(2, 2, [64] * 3), dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)):
        with pytest.raises(ValueError, match="lmbd"):
            m.sample_device(y2, 4, 2, solver="heun", lmbd=0.5)
        with pytest.raises(ValueError, match="lmbd"):
            m.forward(y2, num_samples=4, num_steps=2, solver="heun", lmbd=0.5)
        with pytest.raises(ValueError, match="noise="):
            m.sample_device(y2, 4, 2, x0=torch.zeros(1, 4, 2))
        with pytest.raises(ValueError, match="noise="):
            m.sample_device(y2, 4, 2, x0=torch.zeros(1, 4, 2), lmbd=1.0)
        with pytest.raises(ValueError, match="solver"):
            m.sample_device(y2, 4, 2, solver="rk4")
