"""LinearDPS on the host: the guidance table against an independent float64 builder, the algebra of G, the method
itself on the project's linear problem (covariance-corrected guidance against the DPS likelihood), the crafted
linear-score network, and the refusals of the Python and C-ABI layers that need no device (include/dmip.h
dmip_dps_linear_sample). CPU only (no compute calls)."""
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import accuracy_cases as AC
import dps_linear_ref as R
import oracle as O
import sde_cases as SC

F32, F64 = np.float32, np.float64
YS = ((0.7, -0.2), (-1.5, 2.0))
N, S, SEED = 20000, 200, 2024


@pytest.fixture(scope="module")
def lib(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    return dmip._lib.lib()


@pytest.fixture(scope="module")
def est(dmip):
    return importlib.import_module(dmip.__name__ + ".estimators")


def _problem_arrays(dmip):
    p = dmip.LinearForwardProblem()
    return p, p.A.numpy().astype(F64), p.b.numpy().astype(F64), p.Sigma.numpy().astype(F64)


# ------------------------------------------------------------------------------------- (a) the table
def _random_problem(M, D, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(M, D))
    L = rng.normal(size=(M, M)) * 0.3
    return A, rng.normal(size=M), L @ L.T + 0.2 * np.eye(M)


@pytest.mark.parametrize("sde", [SC.DEFAULT, AC.M, SC.SDES["A"], SC.SDES["B"]], ids=["default", "mild", "A", "B"])
@pytest.mark.parametrize("guidance", R.GUIDANCES)
def test_table_against_independent_builder(est, guidance, sde):
    """The package's f32 table is the independent float64 builder's, to 1e-6 relative after the rounding, with one
    matrix (n_B = 1) for 'nll' and 'norm' and one per step for 'pigdm', at every SDE of tests/sde_cases.py."""
    for M, D, steps in ((2, 2, 7), (5, 3, 50), (32, 3, 12), (1, 2, 200)):
        A, _, Sigma = _random_problem(M, D, 100 * M + D)
        B, rule = est.linear_guidance_table(A, Sigma, guidance, steps, *sde)
        want, want_rule = R.table64(A, Sigma, guidance, steps, *sde)
        assert rule == want_rule == (R.STEP_NORM if guidance == "norm" else R.STEP_BETA)
        assert B.shape == want.shape == ((steps if guidance == "pigdm" else 1), M, D)
        got = B.astype(F32).astype(F64)
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (guidance, M, D, steps)
    if guidance == "pigdm":  # the table moves with every SDE parameter (a default left in would show)
        A, _, Sigma = _random_problem(2, 2, 3)
        B = est.linear_guidance_table(A, Sigma, guidance, 7, *sde)[0]
        for name, other in SC.variants(sde).items():
            if other != sde:
                Bo = est.linear_guidance_table(A, Sigma, guidance, 7, *other)[0]
                assert np.abs(B - Bo).max() > 1e-3 * np.abs(B).max(), name


def test_model_table_cache_and_variants(dmip):
    """The model's table follows its SDE (sde_cases.set_sde) and is keyed by (num_steps, SDE, guidance, device)."""
    p, A, b, Sigma = _problem_arrays(dmip)
    m = dmip.LinearDPS.for_problem(p, [64])
    cpu = torch.device("cpu")
    At, Bt, bt, rule = m.guidance_table(9, cpu)
    assert m.table_uploads == 1 and Bt.dtype == torch.float32 and tuple(Bt.shape) == (9, 2, 2)
    assert bt.dtype == torch.float64 and rule == R.STEP_BETA
    want = R.table64(A, Sigma, "pigdm", 9)[0]
    assert np.abs(Bt.numpy().astype(F64) - want).max() <= 1e-6 * np.abs(want).max()
    m.guidance_table(9, cpu)
    assert m.table_uploads == 1
    m.guidance_table(10, cpu)
    assert m.table_uploads == 2
    SC.set_sde(dmip, m, SC.SDES["B"])
    Bs = m.guidance_table(10, cpu)[1].numpy().astype(F64)
    assert m.table_uploads == 3
    want = R.table64(A, Sigma, "pigdm", 10, *SC.SDES["B"])[0]
    assert np.abs(Bs - want).max() <= 1e-6 * np.abs(want).max()


# ------------------------------------------------------------------------------------- (b) the algebra of G
def test_guidance_with_minus_identity_jacobian():
    """With s = -x and J = -I: x0h = alpha x (alpha^2 = 1 - v), and G = -(1 - v) B^T r / alpha = -alpha B^T r; the
    update subtracts lam G, so the chain moves along +alpha B^T r. Signs and transposes, to 1e-12."""
    rng = np.random.default_rng(0)
    for M, D in ((2, 2), (5, 3), (1, 3)):
        A, b, Sigma = _random_problem(M, D, M + D)
        Bi = R.table64(A, Sigma, "nll", 3)[0][0]
        x = rng.normal(size=(11, D))
        yres = rng.normal(size=M)
        tau = 0.37
        Bt = 0.5 * tau * tau * 19.9 + tau * 0.1
        mw, var = np.exp(-0.5 * Bt), 1.0 - np.exp(-Bt)
        s, J = R.exact_score(None, x, tau)
        G, rr = R.guidance(x, s, J, A, Bi, yres, mw, var)
        r = yres[None, :] - (mw * x) @ A.T
        np.testing.assert_allclose(G, -mw * (r @ Bi), rtol=0, atol=1e-12)
        np.testing.assert_allclose(rr, (r * r).sum(1), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------- (c) the crafted network
def _rel(a, b):
    return float(np.abs(np.asarray(a, F64) - np.asarray(b, F64)).max() / np.abs(np.asarray(b, F64)).max())


@pytest.mark.parametrize("n_hidden", [1, 2, 3])
def test_crafted_network_is_the_linear_score(n_hidden):
    """s = -x and J = -I on |x| <= 4 to 1e-3 relative (the moment test moves by 6e-8 per 1e-4 of network error): in
    float64, in the f32 oracle forward, and through accuracy_cases' numpy emulation of the split engine."""
    D = 2
    params = R.crafted_params(64, n_hidden, D)
    rng = np.random.default_rng(1)
    x = rng.uniform(-4, 4, (512, D))
    x[0] = (4.0, -4.0)
    errs = {}
    for tau in (1.0, 0.3, 0.005):
        s64, J64 = R.jet(params, x, tau, F64)
        s32, J32 = R.jet(params, x.astype(F32), F32(tau), F32)
        inp = np.concatenate([x.astype(F32), np.full((len(x), 1), tau, F32)], 1)
        so = O.mlp_forward(params, inp)
        sx = AC.split_mlp(params, inp)
        eye = np.broadcast_to(-np.eye(D), J64.shape)
        for name, got, want in (("s64", s64, -x), ("J64", J64, eye), ("s32", s32, -x), ("J32", J32, eye),
                                ("oracle f32", so, -x), ("split engine", sx, -x)):
            errs[name] = max(errs.get(name, 0.0), _rel(got, want))
    print("crafted network, relative error:", ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e <= 1e-3, (name, e)
    assert errs["s64"] <= 1.5e-4  # the tanh chain's cubic term: (n_hidden + 1) (eps |x|)^2 / 3 at most


def test_crafted_network_idle_units_change_no_bit():
    """Units beyond the D identity ones have zero weights and biases: they add exact zeros to every sum, so the
    width-64 network's float64 chains are the width-2 network's, bit for bit (the moment runs use the latter)."""
    A, b, Sigma = np.array([[1.0, 0.5], [0.0, 1.0]]), np.array([0.3, 0.5]), 0.3
    for guidance in R.GUIDANCES:
        wide = R.sample(R.crafted_params(64, 3, 2), A, b, Sigma, YS[0], 50, 20, SEED, guidance)
        slim = R.sample(R.crafted_params(2, 3, 2), A, b, Sigma, YS[0], 50, 20, SEED, guidance)
        np.testing.assert_array_equal(wide, slim)


# ------------------------------------------------------------------------------------- (d) the method
@functools.lru_cache(maxsize=None)
def linear_problem_moments(guidance, yi, crafted=True):
    """(mean error, covariance error) of the float64 restatement's chains on LinearForwardProblem against
    get_posterior(y); shared, read-only."""
    dmip = importlib.import_module("conftest").load_pkg()
    p, A, b, Sigma = _problem_arrays(dmip)
    y = np.asarray(YS[yi], F64)
    post = p.get_posterior(torch.tensor(YS[yi], dtype=torch.float32), device="cpu")
    if crafted:  # (the crafted network without its idle units: test_crafted_network_idle_units_change_no_bit)
        x = R.sample(R.crafted_params(2, 3, 2), A, b, Sigma, y, N, S, SEED, guidance, 1.0, F64, stream=yi)
    else:
        x = R.sample(None, A, b, Sigma, y, N, S, SEED, guidance, 1.0, F64, stream=yi, score=R.exact_score)
    return R.moment_errors(x, post.mean.numpy(), post.covariance_matrix.numpy())


@pytest.mark.parametrize("yi", [0, 1])
def test_pigdm_is_the_posterior_where_dps_is_not(yi):
    """The covariance-corrected guidance samples get_posterior(y) to sampling noise; the DPS likelihood does not:
    pigdm's mean and covariance errors are each at most 1/5 of nll's (crafted network, float64 restatement)."""
    pm, pc = linear_problem_moments("pigdm", yi)
    nm, nc = linear_problem_moments("nll", yi)
    print(f"y = {YS[yi]}: pigdm mean err {pm:.3e}, cov err {pc:.3e}; nll mean err {nm:.3e}, cov err {nc:.3e}; "
          f"ratios {pm / nm:.3f}, {pc / nc:.3f}")
    assert pm <= nm / 5 and pc <= nc / 5


# ------------------------------------------------------------------------------------- (e) refusals, Python
def test_constructor_refusals(dmip):
    A = np.array([[1.0, 0.5], [0.0, 1.0]])
    ok = dmip.LinearDPS(2, 2, [64], A, [0.3, 0.5], 0.3)
    assert ok.guidance == "pigdm" and ok.zeta == 1.0 and ok.Sigma.shape == (2, 2)
    np.testing.assert_array_equal(dmip.LinearDPS(2, 2, [64], A, None, [0.3, 0.4]).Sigma, np.diag([0.3, 0.4]))
    bad = [dict(A=np.ones((3, 2))), dict(A=np.ones((2, 3))), dict(b=[1.0, 2.0, 3.0]), dict(Sigma=np.ones((3, 3))),
           dict(Sigma=[1.0, 2.0, 3.0]), dict(Sigma=-0.3), dict(Sigma=np.array([[1.0, 2.0], [2.0, 1.0]])),
           dict(Sigma=np.array([[1.0, 0.5], [0.0, 1.0]])), dict(Sigma=0.0), dict(guidance="dps"), dict(zeta=-1.0),
           dict(zeta=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            dmip.LinearDPS(2, 2, [64], **{**dict(A=A, b=[0.3, 0.5], Sigma=0.3), **kw})
    with pytest.raises(ValueError, match="ydim"):
        dmip.LinearDPS(2, 33, [64], np.ones((33, 2)))


def test_sampling_refusals_without_a_device(dmip):
    """lmbd, the Heun solver, x0= and noise= are refused before anything touches a device."""
    m = dmip.LinearDPS.for_problem(dmip.LinearForwardProblem(), [64] * 3)
    y = torch.tensor([0.7, -0.2])
    for kw in (dict(lmbd=0.5), dict(solver="heun"), dict(x0=torch.zeros(4, 2)), dict(noise=torch.zeros(3, 1, 4, 2))):
        with pytest.raises(ValueError):
            m.sample_device(y, 4, 2, **kw)
    with pytest.raises(ValueError):
        m(y, 4, 2, lmbd=0.5)
    with pytest.raises(ValueError):
        m(y, 4, 2, solver="heun")


def test_factory_and_constructors(dmip):
    p = dmip.LinearForwardProblem()
    m, loss = dmip.get_model_from_args({"model": "LinearDPS", "hidden_layers": [64, 64], "guidance": "nll",
                                        "zeta": 0.5}, {"xdim": 2, "ydim": 2}, None, p)
    assert isinstance(m, dmip.LinearDPS) and isinstance(loss, dmip.DSMLoss)
    assert (m.guidance, m.zeta, m.xdim, m.ydim) == ("nll", 0.5, 2, 2)
    np.testing.assert_array_equal(m.A, p.A.numpy().astype(F64))
    post = dmip.PosteriorDiffusionEstimator(2, 2, [64, 64])
    q = dmip.LinearDPS.from_posterior(post, p.A, p.b, p.Sigma)
    for (w, b), (w0, b0) in zip(q.prior_net.linear_layers(), post.sde.a.prior_net.linear_layers()):
        assert torch.equal(w.cpu(), w0.cpu()) and torch.equal(b.cpu(), b0.cpu())
    # DPS and LinearDPS share the prior's construction and its DSM epoch
    assert dmip.DPS.train_epoch is dmip.LinearDPS.train_epoch


# ------------------------------------------------------------------------------------- (f) the C-ABI
def _call(lib, L, **kw):
    sde = L.vpsde(0.1, 20.0, 1.0)
    buf = ctypes.c_void_p(64)  # never dereferenced: every refusal precedes device work
    a = dict(prior=buf, sde=ctypes.byref(sde), A=buf, B=buf, n_B=1, yres=buf, ydim=2, n_y=1, n=0, off=0, steps=5,
             mean=0.0, std=1.0, seed=1, rule=0, zeta=1.0, prec=L.DMIP_PREC_F32, out=buf, stream=None)
    a.update(kw)
    return lib.dmip_dps_linear_sample(*a.values())


def test_capi_symbols_and_supported(lib, dmip):
    L = dmip._lib
    for s in ("dmip_dps_linear_sample", "dmip_dps_linear_supported"):
        assert s in L.EXPORTED and hasattr(lib, s), s
    assert lib.dmip_abi_version() == 9
    shapes = {(w, d) for w in (64, 128, 256, 512) for d in (2, 3)}
    for w in (32, 64, 96, 128, 256, 512, 1024):
        for d in (1, 2, 3, 4):
            for nl in (0, 1, 2, 3, 4):
                for yd in (0, 1, 32, 33):
                    for prec in (L.DMIP_PREC_F32, L.DMIP_PREC_F32X3):
                        want = (w, d) in shapes and 1 <= nl <= 3 and 1 <= yd <= 32
                        assert bool(lib.dmip_dps_linear_supported(w, nl, d, yd, prec)) == want, (w, d, nl, yd, prec)
    assert not lib.dmip_dps_linear_supported(64, 3, 2, 2, 7)
    assert L.dps_linear_supported(64, 3, 2, 2, "fp16")  # runs the fp32x3 kernel


def test_capi_invalid_arguments(lib, dmip):
    L = dmip._lib
    for kw in (dict(prior=None), dict(sde=None), dict(A=None), dict(B=None), dict(yres=None), dict(out=None),
               dict(n_B=2), dict(n_B=0), dict(ydim=0), dict(ydim=33), dict(zeta=-1.0), dict(zeta=float("nan")),
               dict(zeta=float("inf")), dict(steps=0), dict(rule=2), dict(n_y=0), dict(n=-1), dict(off=-1)):
        assert _call(lib, L, **kw) == L.DMIP_ERR_INVALID, kw
        assert lib.dmip_last_error()
