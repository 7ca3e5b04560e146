"""The fp32x3 flow kernels, host side: the r-form algebra they implement (tests/flow_x3_ref.py) against the tanh-form
restatement (tests/flow_ref.py), the new C-ABI symbols and shape queries, and the Python refusals that need no
device. CPU only (no compute calls)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import flow_ref as FR
import flow_x3_ref as X3R
import oracle as O


@pytest.fixture(scope="module")
def lib(dmip):
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    return dmip._lib.lib()


def _rel(got, ref):
    """max |got - ref| / max |ref|: relative in the maximum norm."""
    return np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(np.asarray(ref)).max()


# ------------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("nl", [1, 3])
@pytest.mark.parametrize("xd,yd", [(2, 2), (3, 23)])
def test_rform_equals_tanh_form_on_seeded_networks(nl, xd, yd):
    """[64] x 1 and [64] x 3, xdim 2 and 3: the r-form fold with its dr tangents gives flow_ref's network output and
    divergence (and the whole Jacobian) to 1e-12 relative, at two times."""
    params = O.reference_weights([xd + yd + 1] + [64] * nl + [xd], 900 + 10 * nl + xd)
    g = np.random.default_rng(17 + nl + xd)
    x = g.normal(size=(29, xd))
    y = g.normal(size=(yd,))
    for tau in (0.05, 0.7):
        n = x.shape[0]
        inp = np.concatenate([x, np.broadcast_to(y, (n, yd)), np.full((n, 1), tau)], 1)
        a_ref, J_ref = FR.mlp_jet(params, inp, xd)
        a, J = X3R.mlp_jet_rform(params, inp, xd)
        assert _rel(a, a_ref) <= 1e-12 and _rel(J, J_ref) <= 1e-12, (_rel(a, a_ref), _rel(J, J_ref))
        a2_ref, dv_ref = FR.score_div(params, x, y, tau, 1.3)
        a2, dv = X3R.score_div_rform(params, x, y, tau, 1.3)
        assert _rel(a2, a2_ref) <= 1e-12 and _rel(dv, dv_ref) <= 1e-12, (_rel(a2, a2_ref), _rel(dv, dv_ref))


def test_rform_equals_tanh_form_on_ckpt_lin(golden):
    """The trained linear-problem checkpoint on the rows of fixture case (a), and as a Posterior pair with a seeded
    prior (the factor g on a and on its divergence)."""
    params = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    z = golden("flow_logp.npz")
    x, y = z["a_x"].astype(np.float64), z["a_y"].astype(np.float64)
    prior = O.reference_weights([3, 64, 64, 64, 2], 77)
    for tau, g in ((1e-3, 0.35), (0.4, 2.8), (1.0, 4.4)):
        for pr in (None, prior):
            a_ref, dv_ref = FR.score_div(params, x, y, tau, g, pr)
            a, dv = X3R.score_div_rform(params, x, y, tau, g, pr)
            assert _rel(a, a_ref) <= 1e-12 and _rel(dv, dv_ref) <= 1e-12, (tau, _rel(a, a_ref), _rel(dv, dv_ref))


def test_output_tangent_needs_no_factor():
    """The output rows are folded at scale 1 (A = -2 Wo), so A dr is da/dx itself: a factor c or 2 here would show."""
    params = O.reference_weights([5, 64, 2], 5)
    L = X3R.fold(params)
    np.testing.assert_array_equal(L[-1][0], -2.0 * np.asarray(params[-1][0], np.float64))
    np.testing.assert_allclose(L[0][0], X3R.C * np.asarray(params[0][0], np.float64), rtol=0, atol=0)


# ------------------------------------------------------------------------------------- the C-ABI
NEW = ("dmip_flow_logp_ex", "dmip_flow_sample_ex", "dmip_flow_logp_supported_precision",
       "dmip_flow_sample_supported_precision")


def test_new_symbols_exported(lib, dmip):
    for s in NEW:
        assert s in dmip._lib.EXPORTED and hasattr(lib, s), s
    assert lib.dmip_abi_version() == 9


def test_supported_precision_queries(lib, dmip):
    """DMIP_PREC_F32 answers as the old queries; DMIP_PREC_F32X3 (and FP16 / BF16, which run it) is 1 for CDE and
    Posterior at widths 64 / 128 / 256 / 512 (every one compiled free of scratch), 0 for CDiffE, other widths,
    depths and xdims, and for an unknown precision."""
    L = dmip._lib
    for q, old in ((lib.dmip_flow_logp_supported_precision, lib.dmip_flow_logp_supported),
                   (lib.dmip_flow_sample_supported_precision, lib.dmip_flow_sample_supported)):
        for mode in (L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR, L.DMIP_SAMPLER_CDIFFE):
            for W in (64, 96, 128, 256, 512):
                for nh in (1, 2, 3, 4):
                    for xd, yd in ((2, 2), (3, 23), (3, 5), (4, 9)):
                        assert q(L.DMIP_PREC_F32, mode, W, nh, xd, yd) == old(mode, W, nh, xd, yd)
                        want = int(mode != L.DMIP_SAMPLER_CDIFFE and W != 96 and nh <= 3 and xd in (2, 3))
                        for prec in (L.DMIP_PREC_F32X3, L.DMIP_PREC_FP16, L.DMIP_PREC_BF16):
                            assert q(prec, mode, W, nh, xd, yd) == want, (prec, mode, W, nh, xd, yd)
                        assert q(7, mode, W, nh, xd, yd) == 0
    # the Python helpers
    assert L.flow_logp_supported(256, 3, 3, 23, precision="fp32x3")
    assert L.flow_sample_supported(64, 1, 2, 2, precision="bf16")
    assert not L.flow_logp_supported(64, 3, 2, 2, L.DMIP_SAMPLER_CDIFFE, precision="fp32x3")
    assert L.flow_logp_supported(256, 3, 3, 23) == L.flow_logp_supported(256, 3, 3, 23, precision="fp32")


def test_ex_entry_points_reject_bad_arguments(lib, dmip):
    """The existing codes, before any device work and before the network handle is read: a mode other than CDE /
    Posterior, null arguments, bad sizes -- at every precision; then an unknown precision."""
    L = dmip._lib
    sde = L.vpsde(0.1, 20.0, 1.0)
    C, P = L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    s = ctypes.byref(sde)

    def lp(mode, net, prior, sde_, x, y, out, prec, n=10, S=10):
        return lib.dmip_flow_logp_ex(mode, net, prior, sde_, x, y, 1, 2, 2, n, S, out, None, prec, None)

    def fs(mode, net, prior, sde_, y, x, logq, prec, n=10, S=10, std=1.0):
        return lib.dmip_flow_sample_ex(mode, net, prior, sde_, y, 1, 2, 2, n, 0, S, 0.0, std, 1, None, x, logq, prec,
                                       None)

    for prec in (L.DMIP_PREC_F32, L.DMIP_PREC_F32X3, L.DMIP_PREC_BF16):
        for mode in (L.DMIP_SAMPLER_CDIFFE, 7):
            assert lp(mode, p, None, s, p, p, p, prec) == L.DMIP_ERR_INVALID
            assert b"CDE and Posterior" in lib.dmip_last_error()
            assert fs(mode, p, None, s, p, p, p, prec) == L.DMIP_ERR_INVALID
            assert b"CDE and Posterior" in lib.dmip_last_error()
        for args in ((C, None, None, s, p, p, p), (C, p, None, None, p, p, p), (C, p, None, s, None, p, p),
                     (C, p, None, s, p, None, p), (C, p, None, s, p, p, None), (P, p, None, s, p, p, p)):
            assert lp(*args, prec) == L.DMIP_ERR_INVALID
            assert b"null" in lib.dmip_last_error()
            assert fs(*args, prec) == L.DMIP_ERR_INVALID
            assert b"null" in lib.dmip_last_error()
        assert lp(C, None, None, s, p, p, p, prec, S=0) == L.DMIP_ERR_INVALID and b"num_steps" in lib.dmip_last_error()
        assert fs(C, None, None, s, p, p, p, prec, S=0) == L.DMIP_ERR_INVALID and b"num_steps" in lib.dmip_last_error()
        assert fs(C, None, None, s, p, p, p, prec, n=0) == L.DMIP_ERR_INVALID and b"n_chains" in lib.dmip_last_error()
        assert fs(C, None, None, s, p, p, p, prec, std=0.0) == L.DMIP_ERR_INVALID and b"stdv" in lib.dmip_last_error()
    for prec in (3, -1, 99):  # (checked once every pointer is known to be there, before the handle is read)
        assert lp(C, p, None, s, p, p, p, prec) == L.DMIP_ERR_INVALID and b"precision" in lib.dmip_last_error()
        assert fs(C, p, None, s, p, p, p, prec) == L.DMIP_ERR_INVALID and b"precision" in lib.dmip_last_error()


# ------------------------------------------------------------------------------------- the code objects
def test_flow_kernels_use_no_scratch(dmip):
    """All 32 kernels (2 kernels x CDE / Posterior x widths 64 / 128 / 256 / 512 x xdim 2 / 3) are in the library,
    spill nothing, call nothing outlined and need no dynamic stack (scripts/check_isa.py on the built code objects)."""
    import importlib
    import sys
    from conftest import ROOT
    if not os.path.exists(dmip._lib.LIB_PATH):
        pytest.skip("libdmip.so not built")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    isa = importlib.import_module("check_isa").analyse(dmip._lib.LIB_PATH)
    for kern in ("x3_flow_kernel", "x3_flow_sample_kernel"):
        mine = {k: v for k, v in isa.items() if kern in k}
        assert len(mine) == 16, (kern, sorted(mine))
        bad = {k: v for k, v in mine.items()
               if v.get("private_segment_fixed_size", 0) or v.get("calls", 0) or v.get("uses_dynamic_stack")}
        assert not bad, bad


# ------------------------------------------------------------------------------------- Python refusals, no launch
def test_python_refusals_launch_nothing(lib, dmip, monkeypatch):
    """CDiffE, a SiLU network, a shape without a kernel and an unknown precision raise ValueError before any launch
    (no device is touched: these run on a CPU-only host); a shape that only the exact-f32 engine has names
    precision="fp32"."""
    y23 = torch.zeros(23)
    x3 = torch.zeros(4, 3)
    before = dict(dmip._lib.calls)
    for prec in ("fp32x3", "fp16", "bf16"):
        with pytest.raises(ValueError, match="log_prob"):
            dmip.CDiffE(3, 23, [256] * 3).log_prob(x3, y23, 2, precision=prec)
        with pytest.raises(ValueError, match="sample_with_log_prob"):
            dmip.CDiffE(3, 23, [256] * 3).sample_with_log_prob(y23, 4, 2, precision=prec)
        with pytest.raises(ValueError, match='no compiled.*precision="fp32"'):
            dmip.CDE(3, 23, [96] * 3).log_prob(x3, y23, 2, precision=prec)
        with pytest.raises(ValueError, match='no compiled.*precision="fp32"'):
            dmip.CDE(3, 23, [256, 128, 256]).sample_with_log_prob(y23, 4, 2, precision=prec)
        silu = dmip.CDE(3, 23, [256] * 3)
        silu.sde.a = dmip.MLP(3 + 23 + 1, 3, [256] * 3, torch.nn.SiLU())
        with pytest.raises(ValueError, match="tanh"):
            silu.log_prob(x3, y23, 2, precision=prec)
        with pytest.raises(ValueError, match="tanh"):
            silu.sample_with_log_prob(y23, 4, 2, precision=prec)
    m = dmip.CDE(3, 23, [256] * 3)
    with pytest.raises(ValueError, match="precision must be one of"):
        m.log_prob(x3, y23, 2, precision="nonsense")
    with pytest.raises(ValueError, match="precision must be one of"):
        m.sample_with_log_prob(y23, 4, 2, precision="nonsense")
    # a shape the exact-f32 engine has and the split engine has not
    L = dmip._lib
    only_f32 = lambda *a, **k: (a[5] if len(a) > 5 else k.get("precision", "fp32")) == "fp32"  # noqa: E731
    monkeypatch.setattr(L, "flow_logp_supported", only_f32)
    monkeypatch.setattr(L, "flow_sample_supported", only_f32)
    with pytest.raises(ValueError, match='precision="fp32"'):
        m.log_prob(x3, y23, 2, precision="fp32x3")
    with pytest.raises(ValueError, match='precision="fp32"'):
        m.sample_with_log_prob(y23, 4, 2, precision="fp32x3")
    assert dict(dmip._lib.calls) == before
