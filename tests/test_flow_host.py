"""The lambda family (sdes.py:77-87) and the probability-flow log-likelihood, host side: the f64 restatement
(tests/flow_ref.py) against the reference's own evaluation (tests/golden/flow_logp.npz, make_golden_flow.py), the
f32 rounding order of step_coef / em_update against the reference's mu and sigma tensors (flow_lmbd.npz), and the
C-ABI's argument validation. CPU only (no compute calls)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flow_ref as FR
import oracle as O


@pytest.fixture(scope="module")
def lib(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    return dmip._lib.lib()


def _params(golden, case):
    """(params, prior_params) of a flow_logp.npz case."""
    if case in ("a", "c"):
        return O.mlp_params_from_state(golden("ckpt_lin.npz")), None
    if case == "b":
        return O.mlp_params_from_state(golden("ckpt_scat.npz")), None
    return (O.mlp_params_from_state(golden("posterior_loss.npz"), "lik_"),
            O.mlp_params_from_state(golden("ckpt_prior_scat.npz")))


@pytest.mark.parametrize("case", ["a", "b", "d"])
def test_flow_ref_reproduces_reference_f64(golden, case):
    """Both sides are f64 and run the same algorithm (the reference's sde.mu with autograd divergence there,
    analytic tangents here): 1e-9."""
    z = golden("flow_logp.npz")
    params, prior = _params(golden, case)
    x, y, S = z[f"{case}_x"], z[f"{case}_y"], int(z[f"{case}_S"])
    if case != "d":
        x, y = x[None], y[None]
    for i in range(x.shape[0]):
        logp, lat = FR.log_prob(params, x[i], y[i], S, prior)
        ref_l = z[f"{case}_logp_f64"] if case != "d" else z["d_logp_f64"][i]
        ref_z = z[f"{case}_latent_f64"] if case != "d" else z["d_latent_f64"][i]
        assert np.abs(logp - ref_l).max() < 1e-9, np.abs(logp - ref_l).max()
        assert np.abs(lat - ref_z).max() < 1e-9


def test_flow_ref_f32_is_at_the_reference_f32_level(golden):
    """flow_ref's f32 evaluation (the yardstick of the shapes without a fixture) errs like the reference's."""
    z = golden("flow_logp.npz")
    params, _ = _params(golden, "a")
    l32, _ = FR.log_prob(params, z["a_x"], z["a_y"], int(z["a_S"]), dtype=np.float32)
    e_ref = np.abs(z["a_logp_f32_cpu"] - z["a_logp_f64"]).max()
    e = np.abs(l32 - z["a_logp_f64"]).max()
    assert 0 < e < 4 * e_ref + 1e-6, (e, e_ref)


@pytest.mark.parametrize("key", ["lin_S200", "lin_S10", "scat_S10"])
@pytest.mark.parametrize("lmbd", [0.5, 1.0])
def test_lmbd_rounding_order_bitwise(golden, key, lmbd):
    """The reference's one-step mu and sigma equal fl(fl(c_mu g) a) - fl(fl(-0.5 beta) x) and fl(c_sig g) bit for
    bit: lambda folds into the two per-step scalars g_mu and g_sig (csrc/dmip_device.h)."""
    z = golden("flow_lmbd.npz")
    k = f"{key}_l{lmbd}_step"
    S = int(key.split("S")[-1])
    x, a = z[f"{k}_x"], z[f"{k}_a"]
    tau = z[f"{k}_tau"]
    assert tau == O.schedule(S)[1][int(z[f"{key}_probe"])]
    mu, sigma, _ = FR.lmbd_step_f32(x, a, np.zeros_like(x), tau, 1.0 / S, lmbd)
    np.testing.assert_array_equal(mu.view(np.uint32), z[f"{k}_mu"].view(np.uint32))
    np.testing.assert_array_equal(sigma.view(np.uint32), z[f"{k}_sigma"].view(np.uint32))
    # and at lmbd = 0 both scalars are g itself
    mu0, sig0, _ = FR.lmbd_step_f32(x, a, np.zeros_like(x), tau, 1.0 / S, 0.0)
    g = O.vp_g(np.float32(tau))
    np.testing.assert_array_equal(sig0, np.broadcast_to(g, x.shape))
    np.testing.assert_array_equal(mu0, ((g * a).astype(np.float32)
                                        - ((np.float32(-0.5) * O.vp_beta(np.float32(tau))) * x).astype(np.float32)))


def test_lmbd_host_sde_matches_fixture(dmip, golden):
    """The package's own host sdes.PluginReverseSDE keeps the reference's lmbd signature: same mu / sigma bits."""
    z = golden("flow_lmbd.npz")
    m = dmip.CDE(2, 2, [64] * 3)
    from conftest import state_from_npz
    m.sde.a.load_state_dict(state_from_npz(golden("ckpt_lin.npz")))
    m.sde.a.to("cpu")
    k = "lin_S10_l0.5_step"
    x = torch.from_numpy(z[f"{k}_x"])
    ys = torch.zeros(x.shape[0], 2) + torch.from_numpy(z["lin_S10_y"])
    t = torch.ones(x.shape[0], 1) * (1 - float(z[f"{k}_tau"]))
    with torch.no_grad():
        sig = m.sde.sigma(t, x, lmbd=0.5).numpy()
    np.testing.assert_array_equal(sig, z[f"{k}_sigma"])


def test_new_symbols_exported(lib, dmip):
    for s in ("dmip_em_sample_lmbd", "dmip_flow_logp", "dmip_flow_logp_supported"):
        assert s in dmip._lib.EXPORTED and hasattr(lib, s), s
    assert lib.dmip_abi_version() == 9


def _em_lmbd(lib, L, mode, net, prior, sde, y, out, lmbd=0.5, num_steps=10):
    return lib.dmip_em_sample_lmbd(mode, net, prior, ctypes.byref(sde) if sde is not None else None, y, 1, 2, 2, 10, 0,
                                   num_steps, 0.0, 1.0, 1, L.DMIP_PREC_F32, lmbd, None, 0, None, out, None)


def _flow(lib, L, mode, net, prior, sde, x, y, out, num_steps=10):
    return lib.dmip_flow_logp(mode, net, prior, ctypes.byref(sde) if sde is not None else None, x, y, 1, 2, 2, 10,
                              num_steps, out, None, None)


def test_lmbd_and_flow_reject_bad_arguments(lib, dmip):
    """DMIP_ERR_INVALID before any device work: null handles, lmbd outside [0, 1], num_steps < 1, Posterior without
    a prior (a network handle cannot be made without a device: the checks under test come before it is read)."""
    L = dmip._lib
    sde = L.vpsde(0.1, 20.0, 1.0)
    C, P = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # null handles
    assert _em_lmbd(lib, L, C, None, None, sde, p, p) == L.DMIP_ERR_INVALID
    assert _flow(lib, L, C, None, None, sde, p, p, p) == L.DMIP_ERR_INVALID
    assert _em_lmbd(lib, L, C, None, None, None, p, p) == L.DMIP_ERR_INVALID
    assert _flow(lib, L, C, None, None, None, p, p, p) == L.DMIP_ERR_INVALID
    # lmbd outside [0, 1] (checked before the handles are looked at)
    for bad in (-0.1, 1.5, float("nan")):
        assert _em_lmbd(lib, L, C, None, None, sde, p, p, lmbd=bad) == L.DMIP_ERR_INVALID
        assert b"lmbd" in lib.dmip_last_error()
    # Posterior without a prior
    assert _em_lmbd(lib, L, P, None, None, sde, p, p) == L.DMIP_ERR_INVALID
    assert _flow(lib, L, P, None, None, sde, p, p, p) == L.DMIP_ERR_INVALID
    # modes other than CDE / Posterior
    assert _em_lmbd(lib, L, L.DMIP_SAMPLER_CDIFFE, None, None, sde, p, p) == L.DMIP_ERR_INVALID
    assert _flow(lib, L, L.DMIP_SAMPLER_CDIFFE, None, None, sde, p, p, p) == L.DMIP_ERR_INVALID


def test_lmbd_and_flow_reject_bad_step_counts(lib, dmip):
    """num_steps < 1 is refused on its own account (the message names it), before the handles are looked at."""
    L = dmip._lib
    sde = L.vpsde(0.1, 20.0, 1.0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for S in (0, -3):
        assert _em_lmbd(lib, L, L.DMIP_SAMPLER_CDE, None, None, sde, p, p, num_steps=S) == L.DMIP_ERR_INVALID
        assert b"num_steps" in lib.dmip_last_error()
        assert _flow(lib, L, L.DMIP_SAMPLER_CDE, None, None, sde, p, p, p, num_steps=S) == L.DMIP_ERR_INVALID
        assert b"num_steps" in lib.dmip_last_error()


def test_flow_entry_points_refuse_in_their_order(lib, dmip):
    """dmip_flow_logp_ex, dmip_flow_sample and dmip_flow_sample_ex with no handle, two faults at a time: the earlier
    check's status and exact message (tests/asan/capi_args.cpp's rows, through ctypes). Each entry point's sequence is
    mode, num_steps, [n_chains, stdv: the sampling forms only,] null argument, precision; `p` stands for a handle where
    the check under test comes before the handle is read."""
    L = dmip._lib
    sde = ctypes.byref(L.vpsde(0.1, 20.0, 1.0))
    C, P, X = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR, L.DMIP_SAMPLER_CDIFFE
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def logp_ex(mode, net, steps, prec):
        return lib.dmip_flow_logp_ex(mode, net, None, sde, p, p, 1, 2, 2, 4, steps, p, None, prec, None)

    def smp(ex, mode, net, steps, n_chains, stdv, prec, logq=p):
        a = (mode, net, None, sde, p, 1, 2, 2, n_chains, 0, steps, 0.0, stdv, 1, None, p, logq)
        return lib.dmip_flow_sample_ex(*a, prec, None) if ex else lib.dmip_flow_sample(*a, None)

    rows = [
        (lambda: logp_ex(X, None, 0, 7), "flow_logp: CDE and Posterior estimators only"),
        (lambda: logp_ex(C, None, 0, 7), "num_steps must be >= 1"),
        (lambda: logp_ex(C, None, 8, 7), "null argument"),
        (lambda: logp_ex(P, p, 8, 7), "null argument"),
        (lambda: logp_ex(C, p, 8, 7), "unknown precision"),
        (lambda: logp_ex(C, p, 8, -1), "unknown precision"),
        (lambda: smp(True, C, p, 8, 4, 1.0, 7), "unknown precision"),
        (lambda: smp(True, C, p, 8, 4, 1.0, 1, logq=None), "null argument"),
    ]
    for ex in (False, True):
        rows += [
            (lambda ex=ex: smp(ex, X, None, 0, 4, 1.0, 1), "flow_sample: CDE and Posterior estimators only"),
            (lambda ex=ex: smp(ex, C, None, 0, 0, 1.0, 1), "num_steps must be >= 1"),
            (lambda ex=ex: smp(ex, C, None, 8, 0, 0.0, 1), "n_chains must be >= 1"),
            (lambda ex=ex: smp(ex, C, None, 8, -3, 0.0, 1), "n_chains must be >= 1"),
            (lambda ex=ex: smp(ex, C, None, 8, 4, 0.0, 1), "stdv must be > 0"),
            (lambda ex=ex: smp(ex, C, None, 8, 4, -1.0, 1), "stdv must be > 0"),
            (lambda ex=ex: smp(ex, C, None, 8, 4, float("nan"), 1), "stdv must be > 0"),
            (lambda ex=ex: smp(ex, C, None, 8, 4, 1.0, 7), "null argument"),
            (lambda ex=ex: smp(ex, P, p, 8, 4, 1.0, 7), "null argument"),
        ]
    for i, (call, msg) in enumerate(rows):
        assert (call(), lib.dmip_last_error().decode()) == (L.DMIP_ERR_INVALID, msg), i


def test_flow_logp_supported_shapes(lib, dmip):
    sup = dmip._lib.flow_logp_supported
    P = dmip._lib.DMIP_SAMPLER_POSTERIOR
    assert sup(64, 3, 2, 2) and sup(256, 3, 3, 23) and sup(512, 1, 3, 23)
    assert sup(256, 3, 3, 23, P) and sup(128, 2, 2, 2, P)
    assert not sup(96, 3, 3, 23) and not sup(256, 4, 3, 23) and not sup(256, 3, 4, 9)
    assert not sup(256, 3, 3, 23, dmip._lib.DMIP_SAMPLER_CDIFFE)


def test_cdiffe_and_dps_refuse(dmip):
    m = dmip.CDiffE(2, 2, [64] * 3)
    with pytest.raises(ValueError):
        m.log_prob(torch.zeros(4, 2), torch.zeros(2))
    with pytest.raises(ValueError):
        m.forward(torch.zeros(2), num_samples=4, num_steps=2, lmbd=1)
    with pytest.raises(ValueError):
        m.sample_device(torch.zeros(2), 4, 2, lmbd=1.0)
    d = dmip.DPS(3, 23, [256] * 3)
    with pytest.raises(ValueError):
        d.sample_device(torch.zeros(23), 4, 2, lmbd=0.5)
    with pytest.raises(ValueError):
        d.log_prob(torch.zeros(4, 3), torch.zeros(23))
    c = dmip.CDE(2, 2, [64] * 3)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            c.forward(torch.zeros(2), num_samples=4, num_steps=2, lmbd=bad)
