"""The paired entry points (one observation per row), host side: the restatements with a per-row y, the exports and
refusals of the C-ABI and Python layers that need no device (include/dmip.h dmip_flow_logp_pairs,
dmip_flow_sample_pairs), and evaluate.coverage_from_logq / held_out_log_prob. CPU only (no compute calls)."""
import ctypes
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


# ------------------------------------------------------------------------------------- (a) the restatements
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatements_take_a_y_per_row(dtype):
    """flow_ref.log_prob and flow_sample_ref.sample_with_logq with y (n, ydim) are, row by row, their one-y runs: the
    reference of the paired tests needs no new code. CDE and a Posterior pair. (Not bit for bit: numpy's matrix
    products sum in an order that depends on the row count. The bound is 1e-12 in float64 and 2e-5 in float32, the
    size of the f32 restatement's own error e_cpu in the GPU tests, against values of order 1.)"""
    tol = 1e-12 if dtype == np.float64 else 2e-5
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=tol, atol=tol)  # noqa: E731
    lik = O.reference_weights([2 + 2 + 1, 64, 64, 2], 11)
    pri = O.reference_weights([2 + 1, 64, 64, 2], 12)
    g = np.random.default_rng(5)
    x = g.normal(size=(7, 2)).astype(np.float32)
    ys = g.normal(size=(7, 2)).astype(np.float32)
    for prior in (None, pri):
        lp, lat = FR.log_prob(lik, x, ys, 3, prior, dtype=dtype)
        xs, lq = FS.sample_with_logq(lik, x, ys, 3, prior, dtype=dtype)
        assert lp.shape == lq.shape == (7,) and lat.shape == xs.shape == (7, 2)
        for i in (0, 3, 6):
            lp1, lat1 = FR.log_prob(lik, x[i:i + 1], ys[i], 3, prior, dtype=dtype)
            xs1, lq1 = FS.sample_with_logq(lik, x[i:i + 1], ys[i], 3, prior, dtype=dtype)
            close(lp1, lp[i:i + 1])
            close(lat1, lat[i:i + 1])
            close(xs1, xs[i:i + 1])
            close(lq1, lq[i:i + 1])
        assert np.abs(lp - FR.log_prob(lik, x, ys[0], 3, prior, dtype=dtype)[0]).max() > 1e-3  # the ys do differ


# ------------------------------------------------------------------------------------- (b) the C-ABI
def test_new_symbols_exported(lib, dmip):
    for s in ("dmip_flow_pairs_supported", "dmip_flow_logp_pairs", "dmip_flow_sample_pairs"):
        assert s in dmip._lib.EXPORTED and hasattr(lib, s), s
    assert lib.dmip_abi_version() == 9 and dmip._lib.ABI_VERSION == 9


def test_pairs_supported_is_flow_logp_supported(lib, dmip):
    L = dmip._lib
    for prec in ("fp32", "fp32x3", "fp16"):
        for mode in (L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR, L.DMIP_SAMPLER_CDIFFE):
            for W in (32, 64, 96, 128, 256, 512, 1024):
                for nh in (0, 1, 2, 3, 4):
                    for xd, yd in ((1, 2), (2, 2), (3, 23), (3, 5), (4, 9)):
                        assert L.flow_pairs_supported(W, nh, xd, yd, mode, prec) == \
                            L.flow_logp_supported(W, nh, xd, yd, mode, prec), (prec, mode, W, nh, xd)
    assert L.flow_pairs_supported(64, 3, 2, 2) and L.flow_pairs_supported(512, 1, 3, 23, L.DMIP_SAMPLER_POSTERIOR)
    assert not L.flow_pairs_supported(96, 3, 3, 23)


def _lp(lib, mode, net, prior, sde, x, y, logp, n=10, num_steps=10, precision=1):
    return lib.dmip_flow_logp_pairs(mode, net, prior, ctypes.byref(sde) if sde is not None else None, x, y, 2, 2, n,
                                    num_steps, logp, None, precision, None)


def _sp(lib, mode, net, prior, sde, y, x, logq, n=10, offset=0, num_steps=10, mean=0.0, std=1.0, x0=None, precision=1):
    return lib.dmip_flow_sample_pairs(mode, net, prior, ctypes.byref(sde) if sde is not None else None, y, 2, 2, n,
                                      offset, num_steps, mean, std, 1, x0, x, logq, precision, None)


def test_pairs_reject_bad_arguments(lib, dmip):
    """Every refusal comes before any device work (a network handle cannot be made without a device: the checks under
    test come before it is read), with dmip_flow_logp_ex's codes."""
    L = dmip._lib
    sde = L.vpsde(0.1, 20.0, 1.0)
    C, P = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for call in (_lp, _sp):
        for mode in (L.DMIP_SAMPLER_CDIFFE, 7, -1):
            assert call(lib, mode, None, None, sde, p, p, p) == L.DMIP_ERR_INVALID
            assert b"CDE and Posterior" in lib.dmip_last_error()
        # null arguments: network, sde, the two inputs / outputs in turn; Posterior without a prior
        assert call(lib, C, None, None, sde, p, p, p) == L.DMIP_ERR_INVALID
        assert b"null" in lib.dmip_last_error()
        assert call(lib, C, p, None, None, p, p, p) == L.DMIP_ERR_INVALID
        assert call(lib, C, p, None, sde, None, p, p) == L.DMIP_ERR_INVALID
        assert call(lib, C, p, None, sde, p, None, p) == L.DMIP_ERR_INVALID
        assert call(lib, C, p, None, sde, p, p, None) == L.DMIP_ERR_INVALID
        assert call(lib, P, p, None, sde, p, p, p) == L.DMIP_ERR_INVALID
        assert b"null" in lib.dmip_last_error()
        for S in (0, -3):
            assert call(lib, C, None, None, sde, p, p, p, num_steps=S) == L.DMIP_ERR_INVALID
            assert b"num_steps" in lib.dmip_last_error()
        for n in (0, -5):
            assert call(lib, C, None, None, sde, p, p, p, n=n) == L.DMIP_ERR_INVALID
            assert b"n must be" in lib.dmip_last_error()
        for prec in (3, -1, 99):
            assert call(lib, C, p, None, sde, p, p, p, precision=prec) == L.DMIP_ERR_INVALID
            assert b"precision" in lib.dmip_last_error()
    for std in (0.0, -1.0, float("nan")):
        assert _sp(lib, C, None, None, sde, p, p, p, std=std) == L.DMIP_ERR_INVALID
        assert b"stdv" in lib.dmip_last_error()


def test_pairs_refuse_in_their_order(lib, dmip):
    """Both paired entry points with no handle, two faults at a time: the earlier check's status and exact message
    (tests/asan/capi_args.cpp's rows, through ctypes). The sequence is mode, num_steps, n, [stdv: the sampling form
    only,] null argument, precision; `p` stands for a handle where the check under test comes before it is read."""
    L = dmip._lib
    sde = L.vpsde(0.1, 20.0, 1.0)
    C, P, X = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR, L.DMIP_SAMPLER_CDIFFE
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rows = []
    for who, call in (("flow_logp_pairs", _lp), ("flow_sample_pairs", _sp)):
        rows += [
            (call, dict(mode=X, net=None, num_steps=0), f"{who}: CDE and Posterior estimators only"),
            (call, dict(mode=C, net=None, num_steps=0, n=0), "num_steps must be >= 1"),
            (call, dict(mode=C, net=None, n=0, precision=7), "n must be >= 1"),
            (call, dict(mode=C, net=None, n=-3, precision=7), "n must be >= 1"),
            (call, dict(mode=C, net=None, precision=7), "null argument"),
            (call, dict(mode=P, net=p, precision=7), "null argument"),
            (call, dict(mode=C, net=p, precision=7), "unknown precision"),
        ]
    rows += [(_sp, dict(mode=C, net=None, n=0, std=0.0), "n must be >= 1")]
    rows += [(_sp, dict(mode=C, net=None, std=s), "stdv must be > 0") for s in (0.0, -1.0, float("nan"))]
    for call, kw, msg in rows:
        kw = dict(kw)
        rc = call(lib, kw.pop("mode"), kw.pop("net"), None, sde, p, p, p, **kw)
        assert (rc, lib.dmip_last_error().decode()) == (L.DMIP_ERR_INVALID, msg), (call.__name__, kw)


# ------------------------------------------------------------------------------------- (c) Python refusals
def test_python_refusals(lib, dmip):
    """ValueError before any device is looked for: estimators without an ODE form, shapes and activations without a
    kernel, x and y that disagree on n, a y that is not (n, ydim), a badly shaped x0, std <= 0."""
    x2, y2 = torch.zeros(4, 2), torch.zeros(4, 2)
    for m, x, y in ((dmip.CDiffE(2, 2, [64] * 3), x2, y2), (dmip.DPS(3, 23, [256] * 3), torch.zeros(4, 3),
                                                            torch.zeros(4, 23))):
        with pytest.raises(ValueError, match="log_prob_pairs"):
            m.log_prob_pairs(x, y, num_steps=2)
        with pytest.raises(ValueError, match="sample_with_log_prob_pairs"):
            m.sample_with_log_prob_pairs(y, 2)
    y23 = torch.zeros(4, 23)
    for bad in (dmip.CDE(3, 23, [96] * 3), dmip.CDE(3, 23, [256, 128, 256])):
        with pytest.raises(ValueError, match="no compiled paired kernel"):
            bad.log_prob_pairs(torch.zeros(4, 3), y23, num_steps=2)
        with pytest.raises(ValueError, match="no compiled paired kernel"):
            bad.sample_with_log_prob_pairs(y23, 2)
    silu = dmip.CDE(3, 23, [256] * 3)
    silu.sde.a = dmip.MLP(3 + 23 + 1, 3, [256] * 3, torch.nn.SiLU())
    with pytest.raises(ValueError, match="tanh"):
        silu.log_prob_pairs(torch.zeros(4, 3), y23, num_steps=2)
    with pytest.raises(ValueError, match="tanh"):
        silu.sample_with_log_prob_pairs(y23, 2)
    with pytest.raises(ValueError, match="precision"):
        dmip.CDE(2, 2, [64] * 3).log_prob_pairs(x2, y2, precision="fp8")
    for m in (dmip.CDE(2, 2, [64] * 3), dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)):
        with pytest.raises(ValueError, match="one y per row"):
            m.log_prob_pairs(x2, y2[:3], num_steps=2)
        with pytest.raises(ValueError, match="one y per row"):
            m.log_prob_pairs(x2[:1], y2, num_steps=2)
        for bad_y in (torch.zeros(2), torch.zeros(4, 3), torch.zeros(2, 4, 2), torch.zeros(0, 2)):
            with pytest.raises(ValueError, match="y must be"):
                m.log_prob_pairs(x2, bad_y, num_steps=2)
            with pytest.raises(ValueError, match="y must be"):
                m.sample_with_log_prob_pairs(bad_y, 2)
        with pytest.raises(ValueError, match="x must be"):
            m.log_prob_pairs(torch.zeros(4, 3), y2, num_steps=2)
        for bad_x0 in (torch.zeros(4, 3), torch.zeros(5, 2), torch.zeros(1, 4, 2), torch.zeros(8)):
            with pytest.raises(ValueError, match="x0"):
                m.sample_with_log_prob_pairs(y2, 2, x0=bad_x0)
        for std in (0, -1.0):
            with pytest.raises(ValueError, match="std"):
                m.sample_with_log_prob_pairs(y2, 2, std=std)
        with pytest.raises(ValueError, match="num_steps"):
            m.sample_with_log_prob_pairs(y2, 0)
        with pytest.raises(ValueError, match="num_steps"):
            m.log_prob_pairs(x2, y2, num_steps=0)


# ------------------------------------------------------------------------------------- (d) coverage_from_logq
def _ks_uniform(a):
    """The Kolmogorov-Smirnov distance of the sample a from U(0, 1)."""
    a = np.sort(np.asarray(a, np.float64))
    n = len(a)
    i = np.arange(1, n + 1)
    return max((i / n - a).max(), (a - (i - 1) / n).max())


def _gaussian_pairs(n, L, seed, shrink):
    """n pairs of LinearForwardProblem's joint in float64 (x ~ N(0, I), y = A x + b + N(0, 0.3 I)) and, for each, the
    log-density (up to the row's constant) of x_true and of L samples under q_i = N(posterior mean, shrink x posterior
    covariance), the samples drawn from q_i."""
    g = np.random.default_rng(seed)
    A, b, s2 = np.array([[1.0, 0.5], [0.0, 1.0]]), np.array([0.3, 0.5]), 0.3
    P = np.linalg.inv(np.eye(2) + A.T @ A / s2)  # posterior covariance
    x = g.normal(size=(n, 2))
    y = x @ A.T + b + math.sqrt(s2) * g.normal(size=(n, 2))
    mean = (y - b) @ A @ P / s2
    C = shrink * P
    Ci, Lc = np.linalg.inv(C), np.linalg.cholesky(C)
    logq = lambda r: -0.5 * np.einsum("...i,ij,...j->...", r, Ci, r)  # noqa: E731
    smp = g.normal(size=(n, L, 2)) @ Lc.T
    return logq(x - mean), logq(smp)


def test_coverage_is_uniform_for_the_exact_posterior_and_not_for_a_narrow_one(ev):
    """n = 2000 pairs, L = 1000, seed 2025, float64: alpha under the exact Gaussian posterior is within the 0.1 %
    Kolmogorov-Smirnov critical value 1.95 / sqrt(n) = 0.0436 of U(0, 1) (measured 0.0235), the expected coverage is
    within it of the level; with the covariance halved (an overconfident q) the same bound fails (measured 0.2600)
    and coverage falls below every level."""
    n, L = 2000, 1000
    bound = 1.95 / math.sqrt(n)
    lt, ls = _gaussian_pairs(n, L, 2025, 1.0)
    rep = ev.coverage_from_logq(lt, torch.from_numpy(ls))
    ks = _ks_uniform(rep["alpha"])
    print(f"exact posterior: KS {ks:.4f} (bound {bound:.4f})")
    assert rep["alpha"].shape == (n,) and rep["alpha"].dtype == np.float64
    np.testing.assert_array_equal(rep["alpha"], (ls > lt[:, None]).mean(1))
    np.testing.assert_array_equal(rep["levels"], np.arange(1, 20) / 20)
    assert ks <= bound
    assert np.abs(rep["coverage"] - rep["levels"]).max() <= bound
    lt, ls = _gaussian_pairs(n, L, 2025, 0.5)
    narrow = ev.coverage_from_logq(lt, ls, levels=(0.5, 0.9))
    ks = _ks_uniform(narrow["alpha"])
    print(f"covariance halved: KS {ks:.4f}, coverage at 0.5 / 0.9: {narrow['coverage']}")
    assert ks > bound and np.all(narrow["coverage"] < np.array([0.5, 0.9]) - bound)


def test_coverage_from_logq_small_cases(ev):
    rep = ev.coverage_from_logq([0.0, 5.0, -5.0], [[-1.0, 1.0, 2.0, 0.0], [1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0]],
                                levels=(0.0, 0.5, 1.0))
    np.testing.assert_array_equal(rep["alpha"], [0.5, 0.0, 1.0])  # strictly greater: a tie is not "exceeds"
    np.testing.assert_array_equal(rep["coverage"], [1 / 3, 2 / 3, 1.0])
    for bad in (([0.0, 1.0], [[1.0], [2.0], [3.0]]), ([0.0], [1.0]), ([0.0], np.zeros((1, 0)))):
        with pytest.raises(ValueError):
            ev.coverage_from_logq(*bad)


# ------------------------------------------------------------------------------------- (e) held_out_log_prob
class _Stub:
    def __init__(self, lp):
        self.lp, self.seen = lp, None

    def log_prob_pairs(self, x, y, num_steps=200, precision=None):
        self.seen = (tuple(x.shape), tuple(y.shape), num_steps, precision)
        return self.lp


def test_held_out_log_prob_arithmetic(ev):
    """-mean, the standard error (n - 1) and n, in float64 from the f32 tensor: values whose f32 running sum would
    lose the small terms."""
    lp = torch.tensor([-1.0e7, 0.25, -0.5, 1.0e7, -3.0], dtype=torch.float32)
    stub = _Stub(lp)
    rep = ev.held_out_log_prob(stub, torch.zeros(5, 2), torch.zeros(5, 3), num_steps=17, precision="fp32x3")
    assert stub.seen == ((5, 2), (5, 3), 17, "fp32x3")
    v = [float(t) for t in lp]
    mean = math.fsum(v) / 5
    var = math.fsum((t - mean) ** 2 for t in v) / 4
    assert rep["n"] == 5 and abs(rep["nll"] + mean) <= 1e-12 * abs(mean) + 1e-15
    assert abs(rep["stderr"] - math.sqrt(var / 5)) <= 1e-12 * math.sqrt(var / 5)
    one = ev.held_out_log_prob(_Stub(torch.tensor([-2.5])), torch.zeros(1, 2), torch.zeros(1, 3))
    assert one == {"nll": 2.5, "stderr": 0.0, "n": 1}
