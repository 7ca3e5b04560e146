"""LinearDPS's Tweedie-covariance guidance on the host: its table against an independent float64 builder, the algebra
of G (with J = -I it is 'pigdm'), the method itself on Gaussian priors with analytic scores (exact where 'pigdm' is
biased), its stability at zeta = 1 on an untrained prior, and the Python and C-ABI layers without a device
(include/dmip.h dmip_dps_tweedie_sample). CPU only (no compute calls)."""
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest
import torch

import accuracy_cases as AC
import dps_linear_ref as R
import dps_tweedie_ref as TW
import oracle as O
from test_gpu_dps_linear import _problem

F32, F64 = np.float32, np.float64
YS = ((0.7, -0.2), (-1.5, 2.0))
N, S, SEED = 20000, 200, 2024
PRIOR_MEAN, PRIOR_COV = np.array([0.5, -0.3]), np.array([[2.0, 0.9], [0.9, 0.6]])


@pytest.fixture(scope="module")
def lib(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    return dmip._lib.lib()


@pytest.fixture(scope="module")
def est(dmip):
    return importlib.import_module(dmip.__name__ + ".estimators")


def _random_problem(M, D, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(M, D))
    L = rng.normal(size=(M, M)) * 0.3
    return A, rng.normal(size=M), L @ L.T + 0.2 * np.eye(M)


# ------------------------------------------------------------------------------------- (1) the table
def test_table_against_independent_builder(est):
    """(Sigma^-1 A, A^T Sigma^-1 A) of the package (solves) against explicit inverses, to 1e-12 relative."""
    for M, D in ((2, 2), (5, 3), (32, 3), (1, 2), (23, 3)):
        A, _, Sigma = _random_problem(M, D, 100 * M + D)
        B, H = est.linear_tweedie_table(A, Sigma)
        wB, wH = TW.table64(A, Sigma)
        assert B.dtype == H.dtype == F64 and B.shape == (M, D) and H.shape == (D, D)
        assert np.abs(B - wB).max() <= 1e-12 * np.abs(wB).max(), (M, D)
        assert np.abs(H - wH).max() <= 1e-12 * np.abs(wH).max(), (M, D)


def test_model_table_is_uploaded_once(dmip):
    """The model's table depends on neither num_steps nor the SDE: one upload per device."""
    p = dmip.LinearForwardProblem()
    m = dmip.LinearDPS.for_problem(p, [64], guidance="tweedie")
    cpu = torch.device("cpu")
    At, Bt, Ht, bt = m.tweedie_table(cpu)
    assert m.table_uploads == 1 and At.dtype == Bt.dtype == Ht.dtype == torch.float32 and bt.dtype == torch.float64
    assert tuple(Bt.shape) == (2, 2) and tuple(Ht.shape) == (2, 2)
    wB, wH = TW.table64(p.A.numpy().astype(F64), p.Sigma.numpy().astype(F64))
    np.testing.assert_array_equal(Bt.numpy(), wB.astype(F32))
    np.testing.assert_array_equal(Ht.numpy(), wH.astype(F32))
    m.tweedie_table(cpu)
    assert m.table_uploads == 1


# ------------------------------------------------------------------------------------- (2) the algebra of G
def test_minus_identity_jacobian_gives_pigdm():
    """J = -I: K = (1 - v) I = alpha^2 I, C = v I, and (I + H v)^-1 A^T Sigma^-1 = A^T (Sigma + v A A^T)^-1 -- the rule is
    'pigdm', to 1e-12, over random x, A, Sigma, y'."""
    rng = np.random.default_rng(0)
    for M, D in ((2, 2), (5, 3), (1, 3), (23, 3), (1, 2)):
        A, _, Sigma = _random_problem(M, D, M + D)
        B, H = TW.table64(A, Sigma)
        for tau in (0.9, 0.37, 0.02):
            Bt = 0.5 * tau * tau * 19.9 + tau * 0.1
            mw, var = np.exp(-0.5 * Bt), 1.0 - np.exp(-Bt)
            x = rng.normal(size=(11, D))
            yres = rng.normal(size=M)
            s, J = R.exact_score(None, x, tau)
            Bp = np.linalg.inv(Sigma + var * (A @ A.T)) @ A
            want, _ = R.guidance(x, s, J, A, Bp, yres, mw, var)
            got = TW.guidance(x, s, J, A, B, H, yres, mw, var)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (M, D, tau)


def test_f32_solve_is_the_solve():
    """The adjugate solve of the f32 restatement against numpy's, on well-conditioned systems."""
    rng = np.random.default_rng(1)
    for D in (2, 3):
        Mx = (np.eye(D)[None] + 0.3 * rng.normal(size=(64, D, D))).astype(F32)
        w = rng.normal(size=(64, D)).astype(F32)
        want = np.linalg.solve(Mx.astype(F64), w.astype(F64)[..., None])[..., 0]
        assert np.abs(TW.solve32(Mx, w) - want).max() <= 1e-4 * np.abs(want).max()


# ------------------------------------------------------------------------------------- (3) the method
def _linear_problem(dmip):
    p = dmip.LinearForwardProblem()
    return p.A.numpy().astype(F64), p.b.numpy().astype(F64), p.Sigma.numpy().astype(F64)


@functools.lru_cache(maxsize=None)
def gaussian_prior_chains(guidance, yi, iso=False):
    """The float64 chains of LinearForwardProblem's A, b, Sigma under an analytic Gaussian prior score; shared,
    read-only."""
    A, b, Sigma = _linear_problem(importlib.import_module("conftest").load_pkg())
    score = R.exact_score if iso else TW.gauss_score(PRIOR_MEAN, PRIOR_COV)
    y = np.asarray(YS[yi], F64)
    if guidance == "tweedie":
        return AC._frozen(TW.sample(None, A, b, Sigma, y, N, S, SEED, 1.0, F64, score=score))
    return AC._frozen(R.sample(None, A, b, Sigma, y, N, S, SEED, guidance, 1.0, F64, score=score))


@pytest.mark.parametrize("yi", [0, 1])
def test_tweedie_is_the_posterior_where_pigdm_is_not(dmip, yi):
    """Prior N((.5, -.3), [[2, .9], [.9, .6]]): the posterior is Gaussian in closed form. Tweedie's mean and covariance
    errors are each at most 1/5 of pigdm's (20,000 chains x 200 steps, float64, deterministic)."""
    A, b, Sigma = _linear_problem(dmip)
    Si, Pi = np.linalg.inv(Sigma), np.linalg.inv(PRIOR_COV)
    pc = np.linalg.inv(Pi + A.T @ Si @ A)
    pm = pc @ (Pi @ PRIOR_MEAN + A.T @ Si @ (np.asarray(YS[yi], F64) - b))
    tm, tc = R.moment_errors(gaussian_prior_chains("tweedie", yi), pm, pc)
    gm, gc = R.moment_errors(gaussian_prior_chains("pigdm", yi), pm, pc)
    print(f"y = {YS[yi]}: tweedie mean err {tm:.3e}, cov err {tc:.3e}; pigdm mean err {gm:.3e}, cov err {gc:.3e}; "
          f"ratios {tm / gm:.3f}, {tc / gc:.3f}")
    assert tm <= gm / 5 and tc <= gc / 5


def test_on_a_standard_normal_prior_tweedie_is_pigdm():
    """N(0, I): J = -I, the two rules are one; the chains agree chain by chain to 1e-6."""
    xt, xp = gaussian_prior_chains("tweedie", 0, True), gaussian_prior_chains("pigdm", 0, True)
    d = float(np.abs(xt - xp).max())
    print(f"max |tweedie - pigdm| over {N} chains: {d:.3e}")
    assert d <= 1e-6


# ------------------------------------------------------------------------------------- (4) Python, without a device
def test_constructors_and_factory_accept_tweedie(dmip):
    p = dmip.LinearForwardProblem()
    A = np.array([[1.0, 0.5], [0.0, 1.0]])
    assert dmip.LinearDPS(2, 2, [64], A, [0.3, 0.5], 0.3, guidance="tweedie").guidance == "tweedie"
    assert dmip.LinearDPS(2, 2, [64], A).guidance == "pigdm"  # the default stays
    assert dmip.LinearDPS.for_problem(p, [64, 64], guidance="tweedie").guidance == "tweedie"
    post = dmip.PosteriorDiffusionEstimator(2, 2, [64, 64])
    assert dmip.LinearDPS.from_posterior(post, p.A, p.b, p.Sigma, guidance="tweedie").guidance == "tweedie"
    m, loss = dmip.get_model_from_args({"model": "LinearDPS", "hidden_layers": [64, 64], "guidance": "tweedie"},
                                       {"xdim": 2, "ydim": 2}, None, p)
    assert isinstance(m, dmip.LinearDPS) and isinstance(loss, dmip.DSMLoss) and (m.guidance, m.zeta) == ("tweedie", 1.0)
    with pytest.raises(ValueError):
        dmip.LinearDPS(2, 2, [64], A, guidance="tweedy")


def test_sampling_refusals_without_a_device(dmip):
    """lmbd, the other solvers, x0= and noise= are refused before anything touches a device."""
    m = dmip.LinearDPS.for_problem(dmip.LinearForwardProblem(), [64] * 3, guidance="tweedie")
    y = torch.tensor([0.7, -0.2])
    for kw in (dict(lmbd=0.5), dict(solver="heun"), dict(solver="dpm2m"), dict(solver="ddim"),
               dict(x0=torch.zeros(4, 2)), dict(noise=torch.zeros(3, 1, 4, 2))):
        with pytest.raises(ValueError):
            m.sample_device(y, 4, 2, **kw)
    with pytest.raises(ValueError):
        m(y, 4, 2, lmbd=0.5)
    with pytest.raises(ValueError):
        m(y, 4, 2, solver="heun")
    assert m.table_uploads == 0


# ------------------------------------------------------------------------------------- (5) the C-ABI
def _call(lib, L, **kw):
    sde = L.vpsde(0.1, 20.0, 1.0)
    buf = ctypes.c_void_p(64)  # never dereferenced: every refusal precedes device work
    a = dict(prior=buf, sde=ctypes.byref(sde), A=buf, B=buf, H=buf, yres=buf, ydim=2, n_y=1, n=0, off=0, steps=5,
             mean=0.0, std=1.0, seed=1, zeta=1.0, prec=L.DMIP_PREC_F32, out=buf, stream=None)
    a.update(kw)
    return lib.dmip_dps_tweedie_sample(*a.values())


def test_capi_symbols_and_supported(lib, dmip):
    L = dmip._lib
    for s in ("dmip_dps_tweedie_sample", "dmip_dps_tweedie_supported"):
        assert s in L.EXPORTED and hasattr(lib, s), s
    assert lib.dmip_abi_version() == 9
    for w in (32, 64, 96, 128, 256, 512, 1024):
        for d in (1, 2, 3, 4):
            for nl in (0, 1, 2, 3, 4):
                for yd in (0, 1, 32, 33):
                    for prec in (L.DMIP_PREC_F32, L.DMIP_PREC_F32X3, L.DMIP_PREC_FP16, 7):
                        want = bool(lib.dmip_dps_linear_supported(w, nl, d, yd, prec))
                        assert bool(lib.dmip_dps_tweedie_supported(w, nl, d, yd, prec)) == want, (w, d, nl, yd, prec)
    assert lib.dmip_dps_tweedie_supported(64, 3, 2, 2, L.DMIP_PREC_F32)
    assert lib.dmip_dps_tweedie_supported(512, 1, 3, 32, L.DMIP_PREC_F32X3)
    assert not lib.dmip_dps_tweedie_supported(64, 3, 2, 2, 7)
    assert L.dps_tweedie_supported(64, 3, 2, 2, "fp16")  # runs the fp32x3 kernel


def test_capi_invalid_arguments(lib, dmip):
    """tests/test_dps_linear_host.py's list without the two arguments this entry point does not have (n_B, the step
    rule), with H added."""
    L = dmip._lib
    for kw in (dict(prior=None), dict(sde=None), dict(A=None), dict(B=None), dict(H=None), dict(yres=None),
               dict(out=None), dict(ydim=0), dict(ydim=33), dict(zeta=-1.0), dict(zeta=float("nan")),
               dict(zeta=float("inf")), dict(steps=0), dict(n_y=0), dict(n_y=65536), dict(n=-1), dict(off=-1)):
        assert _call(lib, L, **kw) == L.DMIP_ERR_INVALID, kw
        assert lib.dmip_last_error()


# ------------------------------------------------------------------------------------- (6) stability at zeta = 1
@functools.lru_cache(maxsize=None)
def _untrained():
    """The accuracy gate's w64-L3-default-sde inputs: torch-default weights, its problem, its y."""
    W, NL, D, M = 64, 3, 2, 2
    A, b, Sigma = _problem(M, D)
    torch.manual_seed(W + NL + D)
    dims = [D + 1] + [W] * NL + [D]
    layers = [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
    params = [(l.weight.detach().numpy().astype(F32), l.bias.detach().numpy().astype(F32)) for l in layers]
    return params, A, b, Sigma, np.random.default_rng(5).uniform(0, 1, (1, M)).astype(F32)[0]


@pytest.mark.parametrize("steps", [50, 200])
def test_untrained_prior_is_stable_at_zeta_one(steps):
    """A default-initialised [64]^3 prior (J ~ 0) at the default SDE and zeta = 1, float64: the rule's chains stay
    finite (the solve damps the 1 / alpha^2 that 'pigdm' amplifies); 'pigdm''s do not fit an f32. No zeta is tuned.

    "Not finite" is f32's: float64 has the exponent range to carry pigdm's chains (every |x| is 5e39 to 1.3e43 at S =
    50 and 6e115 to 1.6e119 at S = 200, measured here), so they are finite there, but every one of them is beyond f32's
    largest number, and the f32 restatement (the device's arithmetic) ends with no finite chain at all."""
    params, A, b, Sigma, y = _untrained()
    kw = dict(T=1.0, beta_min=O.BETA_MIN, beta_max=O.BETA_MAX)
    xt = TW.sample(params, A, b, Sigma, y, 37, steps, 99, 1.0, F64, **kw)
    with np.errstate(all="ignore"):
        xp = R.sample(params, A, b, Sigma, y, 37, steps, 99, "pigdm", 1.0, F64, **kw)
        xp32 = R.sample(params, A, b, Sigma, y, 37, steps, 99, "pigdm", 1.0, F32, **kw)
    print(f"S = {steps}: tweedie max |x| = {np.abs(xt).max():.4g}; pigdm float64 |x| in [{np.abs(xp).min():.3g}, "
          f"{np.abs(xp).max():.3g}], f32 restatement finite entries: {int(np.isfinite(xp32).sum())}")
    assert np.all(np.isfinite(xt)) and np.all(np.abs(xt) < np.finfo(F32).max)
    assert not np.any(np.abs(xp) <= np.finfo(F32).max)   # nan compares false: "beyond f32's range or not finite"
    assert not np.any(np.isfinite(xp32))
