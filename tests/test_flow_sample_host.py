"""Samples with their log-density, host side: the restatement (tests/flow_sample_ref.py) against the Heun sampler's
and against the log-likelihood's, evaluate.importance_report against closed forms, and the refusals of the Python
and C-ABI layers that need no device (include/dmip.h dmip_flow_sample). CPU only (no compute calls)."""
import ctypes
import functools
import importlib
import math
import os

import numpy as np
import pytest
import torch

import flow_ref as FR
import flow_sample_ref as FS
import heun_ref as HR
import oracle as O


@pytest.fixture(scope="module")
def lib(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    return dmip._lib.lib()


@pytest.fixture(scope="module")
def ev(dmip):
    return importlib.import_module(dmip.__name__ + ".evaluate")


# ------------------------------------------------------------------------------------- (a) the restatement's x
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_x_is_bitwise_the_heun_restatements(golden, dtype):
    """The state update is heun_ref.heun_sample's, bit for bit, for the CDE checkpoint and for a Posterior pair (the
    divergence runs beside it and never feeds back)."""
    params = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    y = golden("flow_lmbd.npz")["lin_S10_y"]
    x0 = HR.x0_of_seed(1234, 33, 2)
    x, logq = FS.sample_with_logq(params, x0, y, 7, dtype=dtype)
    assert x.dtype == dtype and logq.dtype == np.float64 and np.all(np.isfinite(logq))
    np.testing.assert_array_equal(x, HR.heun_sample(params, x0, y, 7, dtype=dtype))
    lik = O.reference_weights([2 + 2 + 1, 64, 64, 2], 11)
    pri = O.reference_weights([2 + 1, 64, 64, 2], 12)
    x, _ = FS.sample_with_logq(lik, x0, y, 3, pri, dtype=dtype)
    np.testing.assert_array_equal(x, HR.heun_sample(lik, x0, y, 3, pri, dtype=dtype))


def test_base_term_of_mean_and_std(golden):
    """S and the networks fixed, (mean, std) enters through x_0 only: logq differs from the standard-normal run of the
    same x_0 by the base densities' difference (the -d log std term and the standardised residual)."""
    params = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    y = golden("flow_lmbd.npz")["lin_S10_y"]
    x0 = HR.x0_of_seed(5, 9, 2, mean=0.3, std=1.5)
    _, l0 = FS.sample_with_logq(params, x0, y, 4)
    _, l1 = FS.sample_with_logq(params, x0, y, 4, mean=0.3, std=1.5)
    z0 = x0.astype(np.float64)
    z1 = (z0 - np.float64(np.float32(0.3))) / 1.5
    want = -2 * math.log(1.5) - 0.5 * (z1 * z1).sum(1) + 0.5 * (z0 * z0).sum(1)
    np.testing.assert_allclose(l1 - l0, want, rtol=0, atol=1e-12)


# ------------------------------------------------------------------- (b) consistency of the two discretisations
def test_logq_agrees_with_log_prob_to_second_order(golden, monkeypatch):
    """ckpt_lin under the fixture's y, 256 chains from the samplers' own x0 (seed 1234): e(S) = max |logq_S -
    flow_ref.log_prob(x_S, y, 1024)| falls by 3-5x per halving of the step, the project's band for order 2 (measured
    in f64: 0.198 / 0.0526 / 0.0134, ratios 3.76 and 3.92). flow_ref's Jacobian contractions go through numpy's
    BLAS path here (einsum optimize=True: the same sums in another order, 2e-15 on logp), which takes the 6,600
    Jacobian evaluations of this test from two minutes to ten seconds."""
    monkeypatch.setattr(np, "einsum", functools.partial(np.einsum, optimize=True))
    params = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    y = golden("flow_lmbd.npz")["lin_S10_y"]
    x0 = HR.x0_of_seed(1234, 256, 2)
    e = {}
    for S in (32, 64, 128):
        x, logq = FS.sample_with_logq(params, x0, y, S)
        e[S] = np.abs(logq - FR.log_prob(params, x, y, 1024)[0]).max()
    print(f"e(S) = {e}; ratios {e[32] / e[64]:.2f}, {e[64] / e[128]:.2f}")
    assert 3.0 <= e[32] / e[64] <= 5.0, e
    assert 3.0 <= e[64] / e[128] <= 5.0, e


# ------------------------------------------------------------------------------------- (c) importance_report
def _log_normal(x, m, s):
    """log N(x; m, diag(s^2)) rows of x (n, d)."""
    z = (x - m) / s
    return -0.5 * (z * z).sum(1) - np.log(s).sum() - 0.5 * x.shape[1] * FR.LOG_2PI


def test_importance_report_recovers_a_known_constant(ev):
    """q = N(0, I_2), target = c N(m, diag(s^2)): w / c = p / q has mean 1 and variance prod_k exp(m_k^2 / (2 -
    s_k^2)) / (s_k sqrt(2 - s_k^2)) - 1 (the Gaussian integral of p^2 / q, s_k^2 < 2), so log_z - log c is within
    5 sqrt(var / n) of 0 (delta method; 200,000 draws: var = 0.659, bound 9.1e-3) and ess / n estimates 1 / (1 + var)."""
    n, log_c = 200_000, -7.25
    m, s = np.array([0.5, 0.5]), np.array([0.8, 0.8])
    var = np.prod(np.exp(m * m / (2 - s * s)) / (s * np.sqrt(2 - s * s))) - 1
    bound = 5 * math.sqrt(var / n)
    x = np.random.default_rng(2024).normal(size=(n, 2))
    logq, logt = _log_normal(x, np.zeros(2), np.ones(2)), log_c + _log_normal(x, m, s)
    rep = ev.importance_report(torch.from_numpy(logq), logt)
    print(f"log_z - log c = {rep['log_z'] - log_c:.3e} (bound {bound:.3e}, var {var:.4f}); ess_frac {rep['ess_frac']:.4f}")
    assert abs(rep["log_z"] - log_c) <= bound
    assert abs(rep["ess_frac"] - 1 / (1 + var)) <= 0.02 and abs(rep["ess"] - rep["ess_frac"] * n) <= 1e-9 * n
    # KL(q || p) of two Gaussians, estimated with the estimated log_z
    kl = 0.5 * ((1 / (s * s)).sum() + (m * m / (s * s)).sum() - 2 + 2 * np.log(s).sum())
    assert abs(rep["reverse_kl"] - kl) <= 0.02
    w = rep["weights"]
    assert w.shape == (n,) and abs(w.sum() - 1) < 1e-12 and np.all(w >= 0)
    # f64 recomputation, the plain way (no overflow at these magnitudes)
    w0 = np.exp(logt - logq)
    assert abs(rep["ess"] - w0.sum() ** 2 / (w0 * w0).sum()) <= 1e-9 * n
    assert abs(rep["log_z"] - math.log(w0.mean())) <= 1e-12


def test_importance_report_of_the_target_itself_and_of_shifts(ev):
    """target == q: ess == n and reverse_kl == 0 exactly; log weights shifted by +-1000 neither overflow nor change
    ess, and move log_z by the shift; (n_y, n) inputs are reported per row."""
    rep_of = ev.importance_report
    g = np.random.default_rng(3)
    logq = g.normal(size=777) * 5
    rep = rep_of(logq, logq.copy())
    assert rep["ess"] == 777.0 and rep["ess_frac"] == 1.0 and rep["reverse_kl"] == 0.0 and rep["log_z"] == 0.0
    np.testing.assert_array_equal(rep["weights"], np.full(777, 1 / 777))
    logt = logq + g.normal(size=777)
    base = rep_of(logq, logt)
    for shift in (1000.0, -1000.0):
        r = rep_of(logq, logt + shift)
        assert all(np.all(np.isfinite(r[k])) for k in r)
        assert abs(r["ess"] - base["ess"]) <= 1e-9 * 777 and abs(r["log_z"] - base["log_z"] - shift) <= 1e-9
        assert abs(r["reverse_kl"] - base["reverse_kl"]) <= 1e-9
        r = rep_of(logq - shift, logt)
        assert abs(r["ess"] - base["ess"]) <= 1e-9 * 777 and abs(r["log_z"] - base["log_z"] - shift) <= 1e-9
    both = rep_of(np.stack([logq, logq]), torch.from_numpy(np.stack([logt, logq])))
    assert both["ess"].shape == (2,) and both["weights"].shape == (2, 777)
    assert abs(both["ess"][0] - base["ess"]) <= 1e-9 * 777 and both["ess"][1] == 777.0 and both["reverse_kl"][1] == 0.0
    assert abs(both["log_z"][0] - base["log_z"]) <= 1e-12
    with pytest.raises(ValueError):
        rep_of(logq, logt[:-1])


# ------------------------------------------------------------------------------------- (d) Python refusals
def test_python_refusals(dmip):
    """ValueError before any device is looked for: estimators without an ODE form, and a badly shaped x0."""
    y2, y23 = torch.zeros(2), torch.zeros(23)
    for m, y in ((dmip.CDiffE(2, 2, [64] * 3), y2), (dmip.DPS(3, 23, [256] * 3), y23)):
        with pytest.raises(ValueError, match="sample_with_log_prob"):
            m.sample_with_log_prob(y, 4, 2)
    for m in (dmip.CDE(2, 2, [64] * 3), dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)):
        for bad in (torch.zeros(4, 3), torch.zeros(5, 2), torch.zeros(2, 4, 2), torch.zeros(8)):
            with pytest.raises(ValueError, match="x0"):
                m.sample_with_log_prob(y2, 4, 2, x0=bad)
        with pytest.raises(ValueError, match="x0"):
            m.sample_with_log_prob(torch.zeros(3, 2), 4, 2, x0=torch.zeros(4, 2))  # (n, xdim) is for one y only
        with pytest.raises(ValueError, match="std"):
            m.sample_with_log_prob(y2, 4, 2, std=0)
        with pytest.raises(ValueError, match="std"):
            m.sample_with_log_prob(y2, 4, 2, std=-1.0)


def test_python_refuses_shapes_and_activations_without_a_kernel(lib, dmip):
    y23 = torch.zeros(23)
    with pytest.raises(ValueError, match="no compiled kernel"):
        dmip.CDE(3, 23, [96] * 3).sample_with_log_prob(y23, 4, 2)
    with pytest.raises(ValueError, match="no compiled kernel"):
        dmip.CDE(3, 23, [256, 128, 256]).sample_with_log_prob(y23, 4, 2)
    silu = dmip.CDE(3, 23, [256] * 3)
    silu.sde.a = dmip.MLP(3 + 23 + 1, 3, [256] * 3, torch.nn.SiLU())
    with pytest.raises(ValueError, match="tanh"):
        silu.sample_with_log_prob(y23, 4, 2)


# ------------------------------------------------------------------------------------- (e) the C-ABI
def test_new_symbols_exported(lib, dmip):
    for s in ("dmip_flow_sample", "dmip_flow_sample_supported"):
        assert s in dmip._lib.EXPORTED and hasattr(lib, s), s
    assert lib.dmip_abi_version() == 9


def _fs(lib, mode, net, prior, sde, y, x, logq, n=10, offset=0, num_steps=10, mean=0.0, std=1.0, x0=None, n_y=1):
    return lib.dmip_flow_sample(mode, net, prior, ctypes.byref(sde) if sde is not None else None, y, n_y, 2, 2, n,
                                offset, num_steps, mean, std, 1, x0, x, logq, None)


def test_flow_sample_rejects_bad_arguments(lib, dmip):
    """Every refusal comes before any device work (a network handle cannot be made without a device: the checks under
    test come before it is read), with the documented code."""
    L = dmip._lib
    sde = L.vpsde(0.1, 20.0, 1.0)
    C, P = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # modes other than CDE / Posterior
    for mode in (L.DMIP_SAMPLER_CDIFFE, 7, -1):
        assert _fs(lib, mode, None, None, sde, p, p, p) == L.DMIP_ERR_INVALID
        assert b"CDE and Posterior" in lib.dmip_last_error()
    # null arguments: network, sde, y, x_out, logq_out; Posterior without a prior (x0 may be null)
    assert _fs(lib, C, None, None, sde, p, p, p) == L.DMIP_ERR_INVALID
    assert b"null" in lib.dmip_last_error()
    assert _fs(lib, C, p, None, None, p, p, p) == L.DMIP_ERR_INVALID
    assert _fs(lib, C, p, None, sde, None, p, p) == L.DMIP_ERR_INVALID
    assert _fs(lib, C, p, None, sde, p, None, p) == L.DMIP_ERR_INVALID
    assert _fs(lib, C, p, None, sde, p, p, None) == L.DMIP_ERR_INVALID
    assert _fs(lib, P, p, None, sde, p, p, p) == L.DMIP_ERR_INVALID
    assert b"null" in lib.dmip_last_error()
    # sizes, each on its own account
    for S in (0, -3):
        assert _fs(lib, C, None, None, sde, p, p, p, num_steps=S) == L.DMIP_ERR_INVALID
        assert b"num_steps" in lib.dmip_last_error()
    for n in (0, -5):
        assert _fs(lib, C, None, None, sde, p, p, p, n=n) == L.DMIP_ERR_INVALID
        assert b"n_chains" in lib.dmip_last_error()
    for std in (0.0, -1.0, float("nan")):
        assert _fs(lib, C, None, None, sde, p, p, p, std=std) == L.DMIP_ERR_INVALID
        assert b"stdv" in lib.dmip_last_error()


def test_flow_sample_supported_shapes(lib, dmip):
    """The shapes of the log-likelihood kernel: CDE and Posterior, widths 64 to 512, 1 to 3 hidden layers, xdim 2 / 3."""
    L = dmip._lib
    sup = L.flow_sample_supported
    for mode in (L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR):
        for W in (64, 128, 256, 512):
            for nh in (1, 2, 3):
                for xd, yd in ((2, 2), (3, 23), (3, 5)):
                    assert sup(W, nh, xd, yd, mode), (mode, W, nh, xd)
                    assert sup(W, nh, xd, yd, mode) == L.flow_logp_supported(W, nh, xd, yd, mode)
        assert not sup(96, 3, 3, 23, mode) and not sup(256, 4, 3, 23, mode) and not sup(256, 3, 4, 9, mode)
    assert not sup(64, 3, 2, 2, L.DMIP_SAMPLER_CDIFFE)
