"""The host launch path of the C-ABI samplers (csrc/dmip_capi_sample.cpp) and of the probability-flow entry points
(csrc/dmip_capi_flow.cpp) with real handles. Needs an MI355X: `pytest -m gpu`.

(a) Refusals: every sampler, flow, DPS and MH entry point through ctypes with one argument wrong at a time, and two
    at a time where two entry points share a check (the first check's refusal wins). Status and dmip_last_error text
    are literals: sharing a check must not change what a caller is told, or which of two faults it is told first.
    The eight flow entry points share one implementation; each keeps its own order and wording (FLOW_MORE), checked
    at the smallest compiled shape, where a valid call launches one tiny grid.
(b) One small launch (64 chains, 4 steps, 2 ys, fixed seed) through every branch of that path -- each engine's
    per-launch scratch, each layer-1 image, the ring images at width 512, Heun with and without x0, snapshots,
    lmbd = 1, injected noise, log_prob, DPS and MH -- against the oracle at the tolerance the engine's own test file
    uses (named at each case).
"""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import heun_ref as HR
import oracle as O
from conftest import ROOT, state_from_npz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID, UNSUPPORTED = 1, 2
N, S, SEED = 64, 4, 20240
# err / max(1, |ref|) of the product-RNG samplers against the float32 oracle: tests/test_gpu_parity.py (16-bit: CDE,
# Posterior, CDiffE), tests/test_gpu_f32.py and tests/test_gpu_x3.py (both fp32 engines, every mode)
TOL16 = {"cde": 1e-4, "posterior": 7e-4, "cdiffe": 1.2e-4}
TOL32 = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _rel(out, ref):
    return float(np.abs(out - ref).max() / max(1.0, np.abs(ref).max()))


def _ys(yd, seed=5):
    return np.random.default_rng(seed).uniform(0, 1, (2, yd)).astype(np.float32)


def _surrogate(golden):
    z = golden("surrogate.npz")
    model = torch.nn.Sequential(torch.nn.Linear(3, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                                torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, 23))
    model.load_state_dict({k.replace("_", "."): torch.from_numpy(z[k]) for k in z.files})
    for p in model.parameters():
        p.requires_grad = False
    return model.to(DEV), O.surrogate_params_from_npz(z)


# ------------------------------------------------------------------------------------------- (a) refusals
SIG = {
    "dmip_em_sample": "net sde y n_y ydim xdim n_chains off steps mean stdv seed precision noise x_out stream",
    "dmip_em_sample_posterior": "prior net sde y n_y ydim xdim n_chains off steps mean stdv seed precision x_out stream",
    "dmip_em_sample_cdiffe": "net sde y n_y ydim xdim n_chains off steps mean stdv seed precision corr snr x_out stream",
    "dmip_em_sample_snapshots": "mode net prior sde y n_y ydim xdim n_chains off steps mean stdv seed precision corr "
                                "snr every snap x_out stream",
    "dmip_em_sample_lmbd": "mode net prior sde y n_y ydim xdim n_chains off steps mean stdv seed precision lmbd noise "
                           "every snap x_out stream",
    "dmip_ode_sample": "mode net prior sde y n_y ydim xdim n_chains off steps mean stdv seed precision solver x0 every "
                       "snap x_out stream",
    "dmip_flow_logp": "mode net prior sde x y n_y ydim xdim n_chains steps logp latent stream",
    "dmip_flow_logp_ex": "mode net prior sde x y n_y ydim xdim n_chains steps logp latent precision stream",
    "dmip_flow_sample": "mode net prior sde y n_y ydim xdim n_chains off steps mean stdv seed x0 x_out logq stream",
    "dmip_flow_sample_ex": "mode net prior sde y n_y ydim xdim n_chains off steps mean stdv seed x0 x_out logq "
                           "precision stream",
    "dmip_flow_logp_pairs": "mode net prior sde x y ydim xdim n_chains steps logp latent precision stream",
    "dmip_flow_sample_pairs": "mode net prior sde y ydim xdim n_chains off steps mean stdv seed x0 x_out logq precision "
                              "stream",
    "dmip_dps_sample_ex": "dps_prior sur nz sde y23 n_y n_chains off steps mean stdv seed dps_mode zeta precision "
                          "x_out stream",
    "dmip_mh_sample_ex": "sur nz y23 n_y n_chains off steps noise_std seed x_init inj_noise inj_unif precision x_out "
                         "e_out stream",
}
SAMPLERS = ["dmip_em_sample", "dmip_em_sample_posterior", "dmip_em_sample_cdiffe", "dmip_em_sample_snapshots",
            "dmip_em_sample_lmbd", "dmip_ode_sample"]
# the flow entry points beside dmip_flow_logp: (who in the messages, what the count is called, rows or chains, per-y,
# takes a precision, kind in "no compiled <kind>", the SiLU refusal's tail)
FLOW_MORE = {
    "dmip_flow_logp_ex": ("flow_logp", None, True, True, True, "log-likelihood kernel", "no SiLU log-likelihood kernel"),
    "dmip_flow_sample": ("flow_sample", "n_chains", False, True, False, "flow_sample kernel", "no SiLU kernel"),
    "dmip_flow_sample_ex": ("flow_sample", "n_chains", False, True, True, "flow_sample kernel", "no SiLU kernel"),
    "dmip_flow_logp_pairs": ("flow_logp_pairs", "n", True, False, True, "paired flow kernel", "no SiLU kernel"),
    "dmip_flow_sample_pairs": ("flow_sample_pairs", "n", False, False, True, "paired flow kernel", "no SiLU kernel"),
}
WITH_MODE = ["dmip_em_sample_snapshots", "dmip_em_sample_lmbd", "dmip_ode_sample", "dmip_flow_logp"] + list(FLOW_MORE)


@pytest.fixture(scope="module")
def env(dmip, golden):
    """Handles and buffers of the refusal cases: CDE / CDiffE / Posterior (2, 2, [64]*3), a prior with other hidden
    layers, a DPS prior and the golden surrogate. Every case returns before any device work."""
    L = dmip._lib
    dev = torch.device(DEV)
    torch.manual_seed(1)
    cde, cdiffe = dmip.CDE(2, 2, [64] * 3), dmip.CDiffE(2, 2, [64] * 3)
    post, post2 = dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3), dmip.PosteriorDiffusionEstimator(2, 2, [64] * 2)
    dps = dmip.DPS(3, 23, [256] * 3)
    pr = importlib.import_module("diffusion-modelling-for-inverse-problems_amd.problems")
    sur_model, _ = _surrogate(golden)
    # the smallest compiled shape, for the flow entry points: width 64, 1 hidden layer, xdim 2; a SiLU network of that
    # shape, and xdim 4, which has no flow kernel
    cde1, post1, cde_x4 = dmip.CDE(2, 2, [64]), dmip.PosteriorDiffusionEstimator(2, 2, [64]), dmip.CDE(4, 2, [64])
    silu1 = dmip.MLP(2 + 2 + 1, 2, [64], torch.nn.SiLU()).to(DEV)
    buf = torch.zeros(4096, device=DEV)
    # (the handles live as long as their networks)
    keep = [cde, cdiffe, post, post2, dps, sur_model, cde1, post1, cde_x4, silu1, buf]
    h = lambda net, xdim=2: net.dmip_handle(dev, xdim).h
    v = dict(
        cde=h(cde.sde.a), cdiffe=h(cdiffe.sde.a), lik=h(post.sde.a.likelihood_net), prior=h(post.sde.a.prior_net),
        prior_other=h(post2.sde.a.prior_net), dps_prior=h(dps.prior_net, 3), sur=pr.surrogate_handle(sur_model, dev).h,
        sde=L.vpsde(0.1, 20.0, 1.0), sde_t0=L.vpsde(0.1, 20.0, 0.0), nz=L.scat_noise(0.2, 0.01, 1000.0),
        nz_bad=L.scat_noise(0.2, 0.0, 1000.0), buf=L.ptr(buf), keep=keep,
        cde1=h(cde1.sde.a), lik1=h(post1.sde.a.likelihood_net), prior1=h(post1.sde.a.prior_net), silu1=h(silu1),
        cde_x4=h(cde_x4.sde.a, 4), out1=L.ptr(buf[1024:]), out2=L.ptr(buf[2048:]), out3=L.ptr(buf[3072:]))
    return L, v


def _call(env, entry, **over):
    """(rc, dmip_last_error) of `entry` with valid arguments of its mode except for `over`."""
    L, v = env
    mode = over.get("mode", L.DMIP_SAMPLER_POSTERIOR if entry == "dmip_em_sample_posterior" else
                    L.DMIP_SAMPLER_CDIFFE if entry == "dmip_em_sample_cdiffe" else L.DMIP_SAMPLER_CDE)
    a = dict(mode=mode, net={0: v["cde"], 1: v["lik"], 2: v["cdiffe"]}.get(mode, v["cde"]),
             prior=v["prior"] if mode == L.DMIP_SAMPLER_POSTERIOR else None, sde=v["sde"], y=v["buf"], y23=v["buf"],
             n_y=2, ydim=2, xdim=2, n_chains=N, off=0, steps=S, mean=0.0, stdv=1.0, seed=SEED,
             precision=L.DMIP_PREC_F32, noise=None, x_out=v["buf"], stream=None, corr=0, snr=0.16, every=2,
             snap=v["buf"], lmbd=1.0, solver=L.DMIP_SOLVER_HEUN, x0=None, x=v["buf"], logp=v["buf"], latent=None,
             dps_prior=v["dps_prior"], sur=v["sur"], nz=v["nz"], dps_mode=L.DMIP_DPS_NORM, zeta=0.05, noise_std=0.5,
             x_init=None, inj_noise=None, inj_unif=None, e_out=None, logq=v["buf"])
    a.update(over)
    args = [ctypes.byref(a[k]) if k in ("sde", "nz") and a[k] is not None else a[k] for k in SIG[entry].split()]
    lib = L.lib()
    rc = getattr(lib, entry)(*args)
    return rc, lib.dmip_last_error().decode()


def _ydim_msg(entry):
    # (CDiffE's network puts out xdim + ydim rows, so a wrong ydim fails the output-rows check first)
    return "xdim does not match the network" if entry == "dmip_em_sample_cdiffe" else "ydim does not match the network"


def _modes(L, entry):
    return [L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR] if entry in WITH_MODE else [None]


def _each(L, entries):
    for entry in entries:
        for mode in _modes(L, entry):
            yield entry, ({} if mode is None else {"mode": mode})


def test_valid_arguments_are_accepted_with_no_chains(env):
    """The argument sets the refusals below start from are valid: with n_chains = 0 every entry point returns OK (and
    launches nothing)."""
    L, _ = env
    for entry, kw in _each(L, [e for e in SIG if e not in FLOW_MORE]):
        rc, msg = _call(env, entry, n_chains=0, **kw)
        assert rc == 0, (entry, kw, rc, msg)


def test_sampler_and_flow_refusals_one_fault(env):
    L, v = env
    nets = SAMPLERS + ["dmip_flow_logp"]
    cases = []  # (entry, overrides, rc, message)
    for entry, kw in _each(L, nets):
        who = "flow_logp" if entry == "dmip_flow_logp" else "sampler"
        cases += [
            (entry, dict(kw, net=v["prior"]), INVALID, f"{who} needs an x,y,t network"),
            (entry, dict(kw, xdim=3), INVALID, "xdim does not match the network"),
            (entry, dict(kw, ydim=3), INVALID, _ydim_msg(entry)),
            (entry, dict(kw, n_y=0), INVALID, "n_y must be in [1, 65535]"),
            (entry, dict(kw, n_y=65536), INVALID, "n_y must be in [1, 65535]"),
            (entry, dict(kw, n_chains=-1), INVALID,
             "negative row count" if entry == "dmip_flow_logp" else "negative chain count/offset"),
            (entry, dict(kw, steps=0), INVALID,
             # (dmip_em_sample_snapshots checks snapshot_every against num_steps first)
             "snapshot_every must be in [1, num_steps]" if entry == "dmip_em_sample_snapshots" else
             "num_steps must be >= 1"),
            (entry, dict(kw, sde=v["sde_t0"]), INVALID, "T must be > 0"),
        ]
        if entry != "dmip_flow_logp":
            cases += [(entry, dict(kw, off=-1), INVALID, "negative chain count/offset")]
            cases += [(entry, dict(kw, precision=7), INVALID, "unknown precision")]
        if kw.get("mode") == L.DMIP_SAMPLER_POSTERIOR or entry == "dmip_em_sample_posterior":
            cases += [
                (entry, dict(kw, prior=v["prior_other"]), UNSUPPORTED,
                 "prior and likelihood networks must have the same hidden layers"),
                (entry, dict(kw, prior=v["lik"]), INVALID, "prior must be an x,t network with out_dim == xdim"),
                (entry, dict(kw, prior=None), INVALID, "null argument"),
            ]
    for mode in (L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR):
        kw = {"mode": mode}
        cases += [
            ("dmip_em_sample_lmbd", dict(kw, lmbd=1.5), INVALID, "lmbd must be in [0, 1]"),
            ("dmip_ode_sample", dict(kw, precision=L.DMIP_PREC_FP16), UNSUPPORTED,
             f"no compiled Heun sampler (mode {mode}, precision 0) for width 64, layers 3, xdim 2"),
            ("dmip_ode_sample", dict(kw, solver=L.DMIP_SOLVER_EULER, x0=v["buf"]), UNSUPPORTED,
             "ode_sample: x0_dev needs DMIP_SOLVER_HEUN (the Euler samplers start from injected noise: "
             "dmip_em_sample_lmbd's noise_dev)"),
            ("dmip_ode_sample", dict(kw, solver=2), INVALID, "unknown solver"),
        ]
    cases += [
        ("dmip_em_sample_lmbd", dict(mode=L.DMIP_SAMPLER_CDIFFE, lmbd=0.5), INVALID,
         "em_sample_lmbd: CDE and Posterior samplers only"),
        ("dmip_ode_sample", dict(mode=L.DMIP_SAMPLER_CDIFFE), INVALID, "ode_sample: CDE and Posterior samplers only"),
        ("dmip_flow_logp", dict(mode=L.DMIP_SAMPLER_CDIFFE), INVALID, "flow_logp: CDE and Posterior estimators only"),
        ("dmip_em_sample_lmbd", dict(mode=L.DMIP_SAMPLER_POSTERIOR, noise=v["buf"]), INVALID,
         "noise injection: CDE sampler only"),
        ("dmip_em_sample_snapshots", dict(mode=L.DMIP_SAMPLER_CDE, corr=1), INVALID,
         "corrector steps: CDiffE sampler only"),
        ("dmip_em_sample_cdiffe", dict(corr=-1), INVALID, "corrector_steps must be >= 0"),
        ("dmip_em_sample_cdiffe", dict(corr=1, snr=0.0), INVALID, "snr must be > 0"),
        ("dmip_em_sample_snapshots", dict(mode=L.DMIP_SAMPLER_CDIFFE, corr=1, snr=0.0), INVALID, "snr must be > 0"),
    ]
    for entry in ("dmip_em_sample_lmbd", "dmip_ode_sample"):
        for over in (dict(every=-1), dict(every=S + 1), dict(every=2, snap=None)):
            cases += [(entry, over, INVALID, "snapshot_every must be 0 or in [1, num_steps] with a snapshot buffer")]
    for entry, over, rc, msg in cases:
        assert _call(env, entry, **over) == (rc, msg), (entry, over)


def test_sampler_and_flow_refusals_two_faults_keep_their_order(env):
    """Pairs of faults across the checks the samplers and dmip_flow_logp share: the earlier check refuses."""
    L, v = env
    cases = []
    for entry, kw in _each(L, SAMPLERS + ["dmip_flow_logp"]):
        who = "flow_logp" if entry == "dmip_flow_logp" else "sampler"
        flow = entry == "dmip_flow_logp"
        cases += [
            (entry, dict(kw, net=v["prior"], n_y=0), f"{who} needs an x,y,t network"),
            (entry, dict(kw, xdim=3, ydim=3), "xdim does not match the network"),
            (entry, dict(kw, ydim=3, n_y=0), _ydim_msg(entry)),
            (entry, dict(kw, n_y=0, n_chains=-1), "n_y must be in [1, 65535]"),
            (entry, dict(kw, n_chains=-1, sde=v["sde_t0"]), "negative row count" if flow else "negative chain count/offset"),
        ]
        if not flow:
            cases += [(entry, dict(kw, precision=7, net=v["prior"]), "unknown precision")]
        if not flow and entry != "dmip_em_sample_snapshots":
            cases += [(entry, dict(kw, steps=0, sde=v["sde_t0"], **({"every": 0} if "every" in SIG[entry] else {})),
                       "num_steps must be >= 1")]
        if flow:  # num_steps before the handles here
            cases += [(entry, dict(kw, steps=0, net=v["prior"]), "num_steps must be >= 1")]
    for mode in (L.DMIP_SAMPLER_CDE, L.DMIP_SAMPLER_POSTERIOR):
        cases += [
            ("dmip_em_sample_lmbd", dict(mode=mode, lmbd=1.5, steps=0), "lmbd must be in [0, 1]"),
            ("dmip_em_sample_lmbd", dict(mode=mode, every=S + 1, net=v["prior"]),
             "snapshot_every must be 0 or in [1, num_steps] with a snapshot buffer"),
            ("dmip_ode_sample", dict(mode=mode, every=S + 1, net=v["prior"]),
             "snapshot_every must be 0 or in [1, num_steps] with a snapshot buffer"),
            ("dmip_ode_sample", dict(mode=mode, sde=v["sde_t0"], precision=L.DMIP_PREC_FP16), "T must be > 0"),
        ]
    cases += [("dmip_em_sample_lmbd", dict(mode=L.DMIP_SAMPLER_POSTERIOR, prior=v["prior_other"], n_y=0),
               "prior and likelihood networks must have the same hidden layers"),
              ("dmip_flow_logp", dict(mode=L.DMIP_SAMPLER_POSTERIOR, prior=v["prior_other"], n_y=0),
               "prior and likelihood networks must have the same hidden layers")]
    for entry, over, msg in cases:
        rc, got = _call(env, entry, **over)
        assert got == msg and rc in (INVALID, UNSUPPORTED), (entry, over, rc, got)


def _fcall(env, entry, **over):
    """_call for the flow entry points of FLOW_MORE at their smallest shape: the 1-hidden-layer handles, 8 rows or
    chains, 2 steps, outputs apart from the inputs."""
    L, v = env
    post = over.get("mode", L.DMIP_SAMPLER_CDE) == L.DMIP_SAMPLER_POSTERIOR
    a = dict(mode=L.DMIP_SAMPLER_CDE, net=v["lik1"] if post else v["cde1"], prior=v["prior1"] if post else None,
             n_chains=8, steps=2, x_out=v["out1"], logp=v["out2"], logq=v["out2"])
    a.update(over)
    return _call(env, entry, **a)


def test_flow_entry_points_launch_and_take_no_rows_as_they_do(env):
    """The argument sets the flow refusals below start from are valid: each entry point launches its tiny grid, in
    exact f32 and (where it takes a precision) fp32x3, and the device reports nothing. n = 0 is OK for dmip_flow_logp
    and its _ex form only: the other four refuse it by name."""
    L, v = env
    for entry, kw in _each(L, list(FLOW_MORE)):
        who, count, rows, per_y, has_prec, _, _ = FLOW_MORE[entry]
        for prec in ([L.DMIP_PREC_F32, L.DMIP_PREC_F32X3] if has_prec else [L.DMIP_PREC_F32]):
            over = dict(kw, precision=prec, latent=v["out3"])
            assert _fcall(env, entry, **over)[0] == 0, (entry, over, L.lib().dmip_last_error())
            L.device_status(torch.device(DEV))
            rc, msg = _fcall(env, entry, n_chains=0, **over)
            if count is None:
                assert rc == 0, (entry, over, msg)
            else:
                assert (rc, msg) == (INVALID, f"{count} must be >= 1"), (entry, over)


def test_flow_refusals_one_fault(env):
    """test_sampler_and_flow_refusals_one_fault for the other flow entry points: check_nets' messages with each one's
    name, rows against chains, the three SiLU wordings, "no compiled ..." with and without the precision."""
    L, v = env
    cases = []
    for entry, kw in _each(L, list(FLOW_MORE)):
        who, count, rows, per_y, has_prec, kind, silu = FLOW_MORE[entry]
        cases += [
            (entry, dict(kw, net=v["prior1"]), INVALID, f"{who} needs an x,y,t network"),
            (entry, dict(kw, xdim=3), INVALID, "xdim does not match the network"),
            (entry, dict(kw, ydim=3), INVALID, "ydim does not match the network"),
            (entry, dict(kw, n_chains=-1), INVALID, "negative row count" if count is None else f"{count} must be >= 1"),
            (entry, dict(kw, steps=0), INVALID, "num_steps must be >= 1"),
            (entry, dict(kw, sde=v["sde_t0"]), INVALID, "T must be > 0"),
            (entry, dict(kw, net=None), INVALID, "null argument"),
            (entry, dict(kw, sde=None), INVALID, "null argument"),
            (entry, dict(kw, y=None), INVALID, "null argument"),
            (entry, dict(kw, **({"logp": None} if rows else {"x_out": None})), INVALID, "null argument"),
        ]
        if per_y:
            cases += [(entry, dict(kw, n_y=n_y), INVALID, "n_y must be in [1, 65535]") for n_y in (0, 65536)]
        if not rows:
            cases += [(entry, dict(kw, off=-1), INVALID, "negative chain count/offset"),
                      (entry, dict(kw, stdv=0.0), INVALID, "stdv must be > 0"),
                      (entry, dict(kw, logq=None), INVALID, "null argument")]
        if has_prec:
            cases += [(entry, dict(kw, precision=7), INVALID, "unknown precision")]
        if kw["mode"] == L.DMIP_SAMPLER_POSTERIOR:
            cases += [
                (entry, dict(kw, prior=v["prior_other"]), UNSUPPORTED,
                 "prior and likelihood networks must have the same hidden layers"),
                (entry, dict(kw, prior=v["lik1"]), INVALID, "prior must be an x,t network with out_dim == xdim"),
                (entry, dict(kw, prior=None), INVALID, "null argument"),
            ]
        else:
            shape = "for width 64, layers 1, xdim 4"
            cases += [
                (entry, dict(kw, net=v["silu1"]), UNSUPPORTED, f"{who}: the tanh chain only ({silu})"),
                (entry, dict(kw, net=v["cde_x4"], xdim=4), UNSUPPORTED, f"no compiled {kind} (mode 0) {shape}"),
            ]
            if has_prec:
                cases += [(entry, dict(kw, net=v["cde_x4"], xdim=4, precision=prec), UNSUPPORTED,
                           f"no compiled {kind} (mode 0, precision 2) {shape}")
                          for prec in (L.DMIP_PREC_F32X3, L.DMIP_PREC_FP16)]
        cases += [(entry, dict(mode=L.DMIP_SAMPLER_CDIFFE), INVALID, f"{who}: CDE and Posterior estimators only")]
    for entry, over, rc, msg in cases:
        assert _fcall(env, entry, **over) == (rc, msg), (entry, over)


def test_flow_refusals_two_faults_keep_their_order(env):
    """Pairs of faults down each flow entry point's own sequence: the earlier check refuses. The sampling forms check
    their count and stdv before the null arguments; dmip_flow_logp[_ex] leaves its count to the networks' check."""
    L, v = env
    cases = []
    for entry, kw in _each(L, list(FLOW_MORE)):
        who, count, rows, per_y, has_prec, kind, silu = FLOW_MORE[entry]
        cases += [
            (entry, dict(kw, mode=L.DMIP_SAMPLER_CDIFFE, steps=0), f"{who}: CDE and Posterior estimators only"),
            (entry, dict(kw, steps=0, n_chains=0, net=v["prior1"]), "num_steps must be >= 1"),
            (entry, dict(kw, net=v["prior1"], sde=v["sde_t0"]), f"{who} needs an x,y,t network"),
            (entry, dict(kw, xdim=3, ydim=3), "xdim does not match the network"),
            (entry, dict(kw, ydim=3, sde=v["sde_t0"]), "ydim does not match the network"),
        ]
        if count is None:
            cases += [(entry, dict(kw, n_chains=-1, sde=v["sde_t0"]), "negative row count"),
                      (entry, dict(kw, n_y=0, n_chains=-1), "n_y must be in [1, 65535]")]
        else:
            cases += [(entry, dict(kw, n_chains=0, net=None, **({} if rows else {"stdv": 0.0})), f"{count} must be >= 1")]
        if not rows:
            cases += [(entry, dict(kw, stdv=0.0, net=None), "stdv must be > 0"),
                      (entry, dict(kw, off=-1, sde=v["sde_t0"]), "negative chain count/offset")]
            if per_y:
                cases += [(entry, dict(kw, n_y=0, off=-1), "n_y must be in [1, 65535]")]
        if has_prec:
            cases += [(entry, dict(kw, net=None, precision=7), "null argument"),
                      (entry, dict(kw, precision=7, net=v["prior1"]), "unknown precision")]
        if kw["mode"] == L.DMIP_SAMPLER_POSTERIOR:
            cases += [(entry, dict(kw, prior=v["prior_other"], sde=v["sde_t0"]),
                       "prior and likelihood networks must have the same hidden layers")]
        else:
            cases += [(entry, dict(kw, sde=v["sde_t0"], net=v["silu1"]), "T must be > 0"),
                      (entry, dict(kw, sde=v["sde_t0"], net=v["cde_x4"], xdim=4), "T must be > 0")]
    for entry, over, msg in cases:
        rc, got = _fcall(env, entry, **over)
        assert got == msg and rc in (INVALID, UNSUPPORTED), (entry, over, rc, got)


def test_dps_and_mh_refusals(env):
    L, v = env
    dps_prior_msg = "DPS prior must be an x,t network (MLP2) with xdim 3 and hidden layers [256]*3"
    cases = []
    for prec in (L.DMIP_PREC_F32, L.DMIP_PREC_F32X3):
        d, m = "dmip_dps_sample_ex", "dmip_mh_sample_ex"
        kw = {"precision": prec}
        cases += [
            (d, dict(kw, n_y=0), INVALID, "n_y must be in [1, 65535]"),
            (d, dict(kw, n_chains=-1), INVALID, "negative chain count/offset"),
            (d, dict(kw, off=-1), INVALID, "negative chain count/offset"),
            (d, dict(kw, steps=0), INVALID, "num_steps must be >= 1"),
            (d, dict(kw, sde=v["sde_t0"]), INVALID, "T must be > 0"),
            (d, dict(kw, zeta=-1.0), INVALID, "zeta must be >= 0"),
            (d, dict(kw, dps_mode=7), INVALID, "unknown DPS guidance mode"),
            (d, dict(kw, dps_prior=v["prior"]), UNSUPPORTED, dps_prior_msg),
            (d, dict(kw, dps_mode=L.DMIP_DPS_NLL, nz=v["nz_bad"]), INVALID,
             "noise model needs b > 0, a >= 0, lambd_bd >= 0"),
            (d, dict(kw, sur=None), INVALID, "null argument"),
            # two faults: the handles' checks come before the sizes, the sizes in their order
            (d, dict(kw, dps_prior=v["prior"], n_y=0), UNSUPPORTED, dps_prior_msg),
            (d, dict(kw, dps_mode=7, n_y=0), INVALID, "unknown DPS guidance mode"),
            (d, dict(kw, n_y=0, zeta=-1.0), INVALID, "n_y must be in [1, 65535]"),
            (d, dict(kw, steps=0, sde=v["sde_t0"]), INVALID, "num_steps must be >= 1"),
            (m, dict(kw, sur=None), INVALID, "null surrogate handle"),
            (m, dict(kw, n_chains=-1), INVALID, "n < 0"),
            (m, dict(kw, nz=v["nz_bad"]), INVALID, "noise model needs b > 0, a >= 0, lambd_bd >= 0"),
            (m, dict(kw, x_out=None), INVALID, "null argument"),
            (m, dict(kw, n_y=0), INVALID, "n_y must be in [1, 65535]"),
            (m, dict(kw, off=-1), INVALID, "negative chain offset"),
            (m, dict(kw, steps=-1), INVALID, "num_steps must be >= 0"),
            (m, dict(kw, noise_std=-1.0), INVALID, "noise_std must be >= 0"),
            (m, dict(kw, nz=v["nz_bad"], n_y=0), INVALID, "noise model needs b > 0, a >= 0, lambd_bd >= 0"),
            (m, dict(kw, n_y=0, noise_std=-1.0), INVALID, "n_y must be in [1, 65535]"),
            (m, dict(kw, noise_std=-1.0, inj_noise=v["buf"]), INVALID, "noise_std must be >= 0"),
        ]
    cases += [
        ("dmip_dps_sample_ex", dict(precision=L.DMIP_PREC_FP16, sur=None), INVALID,
         "DPS precision: DMIP_PREC_F32 or DMIP_PREC_F32X3"),
        ("dmip_mh_sample_ex", dict(precision=L.DMIP_PREC_FP16, sur=None), INVALID,
         "MH precision: DMIP_PREC_F32 or DMIP_PREC_F32X3"),
        ("dmip_mh_sample_ex", dict(precision=L.DMIP_PREC_F32, inj_noise=v["buf"]), INVALID,
         "inject both the proposal normals and the uniforms, or neither"),
        ("dmip_mh_sample_ex", dict(precision=L.DMIP_PREC_F32X3, inj_noise=v["buf"], inj_unif=v["buf"]), UNSUPPORTED,
         "fp32x3 MH: injected draws need DMIP_PREC_F32"),
    ]
    for entry, over, rc, msg in cases:
        assert _call(env, entry, **over) == (rc, msg), (entry, over)


# ------------------------------------------------------------------ (b) one launch through every host branch
def _model(dmip, kind, xd, yd, W, seed):
    torch.manual_seed(seed)
    cls = {"cde": dmip.CDE, "cdiffe": dmip.CDiffE, "posterior": dmip.PosteriorDiffusionEstimator}[kind]
    return cls(xd, yd, [W] * 3)


def _oracle(m, kind, ys):
    """The float32 oracle's chains for both ys (the y index is the RNG stream), computed once per case."""
    if kind == "posterior":
        prior, lik = HR.params_of(m.sde.a.prior_net), HR.params_of(m.sde.a.likelihood_net)
        return np.stack([O.posterior_sample(prior, lik, ys[k], N, S, SEED, stream=k) for k in range(2)])
    fn = O.cde_sample if kind == "cde" else O.cdiffe_sample
    return np.stack([fn(HR.params_of(m.sde.a), ys[k], N, S, SEED, stream=k) for k in range(2)])


SDE_CASES = {  # name: (model kind, xdim, ydim, width, precisions) -- and the host branch each precision takes
    # 16-bit: per-y a1 prep; exact f32: per-y l1y prep; fp32x3: the width-64 latency engine (no prep launch)
    "cde64": ("cde", 2, 2, 64, ["fp16", "fp32", "fp32x3"]),
    "cde128": ("cde", 2, 2, 128, ["fp32x3"]),                 # fp32x3 with the bias_y prep
    "cde256": ("cde", 3, 23, 256, ["fp32x3"]),                # the k-major engine (x3k)
    "cdiffe64": ("cdiffe", 2, 2, 64, ["fp32", "fp32x3"]),     # f32 without l1y; fp32x3 on the full layer-1 image
    "cdiffe512": ("cdiffe", 3, 23, 512, ["fp16", "fp32x3"]),  # ring_l1; the L1R stream
    "post64": ("posterior", 2, 2, 64, ["fp16", "fp32", "fp32x3"]),
}
_cases = {}


def _sde_case(dmip, name):
    if name not in _cases:
        kind, xd, yd, W, _ = SDE_CASES[name]
        m = _model(dmip, kind, xd, yd, W, 100 + W + xd)
        ys = _ys(yd)
        ref = _oracle(m, kind, ys)
        ref.setflags(write=False)
        _cases[name] = (m, ys, ref)
    return _cases[name]


@pytest.mark.parametrize("name,prec", [(k, p) for k, c in SDE_CASES.items() for p in c[4]])
def test_reverse_sde_launch_vs_oracle(dmip, name, prec):
    L = dmip._lib
    kind, xd, yd, W, _ = SDE_CASES[name]
    mode = {"cde": L.DMIP_SAMPLER_CDE, "posterior": L.DMIP_SAMPLER_POSTERIOR, "cdiffe": L.DMIP_SAMPLER_CDIFFE}[kind]
    if not L.sampler_supported(W, 3, xd, yd, mode, prec):
        print(f"not compiled: {kind} sampler at width {W}, xdim {xd}, ydim {yd}, {prec}")
        pytest.skip("no compiled kernel")
    m, ys, ref = _sde_case(dmip, name)
    key = {"cde": "em_sample", "posterior": "em_sample_posterior", "cdiffe": "em_sample_cdiffe"}[kind]
    before = L.calls[key]
    x = m.sample_device(torch.from_numpy(ys).to(DEV), N, S, seed=SEED, precision=prec)
    L.device_status(torch.device(DEV))
    assert L.calls[key] == before + 1
    x = x.cpu().numpy()
    err = _rel(x, ref)
    tol = TOL16[kind] if prec == "fp16" else TOL32
    print(f"{name} {prec}: err / max(1, |x|) = {err:.3e} (bound {tol:.1e})")
    assert x.shape == (2, N, xd) and np.all(np.isfinite(x)) and err < tol, err


_CHILD = """
import importlib, sys, numpy as np, torch
sys.path.insert(0, {root!r})
dmip = importlib.import_module("diffusion-modelling-for-inverse-problems_amd")
torch.manual_seed({seed})
m = dmip.CDE(3, 23, [256] * 3)
ys = torch.from_numpy(np.load({ys!r})).to("cuda:0")
x = m.sample_device(ys, {n}, {s}, seed={rng}, precision="fp32x3")
dmip._lib.device_status(torch.device("cuda:0"))
np.save({out!r}, x.cpu().numpy())
"""


def test_one_tile_engine_at_the_x3k_shape_in_a_child_process(dmip, tmp_path):
    """DMIP_X3K=0 (read at each launch, set for a child so nothing leaks into this process): the one-tile fp32x3
    engine with its bias_y prep at CDE(3, 23, [256]*3), against the same oracle chains as the k-major engine."""
    m, ys, ref = _sde_case(dmip, "cde256")
    np.save(tmp_path / "ys.npy", ys)
    code = _CHILD.format(root=ROOT, seed=100 + 256 + 3, ys=str(tmp_path / "ys.npy"), n=N, s=S, rng=SEED,
                         out=str(tmp_path / "x.npy"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DMIP_X3K="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    x = np.load(tmp_path / "x.npy")
    err = _rel(x, ref)
    print(f"cde256 fp32x3, DMIP_X3K=0: err / max(1, |x|) = {err:.3e} (bound {TOL32:.1e})")
    assert np.all(np.isfinite(x)) and err < TOL32, err


@pytest.mark.parametrize("with_x0", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
def test_heun_launch_vs_restatement(dmip, prec, with_x0):
    """dmip_ode_sample, Heun, from the chains' own start states and from x0=: HR.BOUND (tests/test_gpu_heun.py)."""
    L = dmip._lib
    if not L.ode_sample_supported(64, 3, 2, 2, L.DMIP_SAMPLER_CDE, prec):
        print(f"not compiled: Heun CDE sampler at width 64, {prec}")
        pytest.skip("no compiled kernel")
    m, ys, _ = _sde_case(dmip, "cde64")
    if with_x0:
        x0 = np.random.default_rng(9).normal(size=(2, N, 2)).astype(np.float32)
    else:
        x0 = np.stack([HR.x0_of_seed(SEED, N, 2, stream=k) for k in range(2)])
    before = L.calls["ode_sample"]
    x = m.sample_device(torch.from_numpy(ys).to(DEV), N, S, seed=SEED, precision=prec, solver="heun",
                        x0=torch.from_numpy(x0) if with_x0 else None)
    L.device_status(torch.device(DEV))
    assert L.calls["ode_sample"] == before + 1
    x = x.cpu().numpy()
    params = HR.params_of(m.sde.a)
    for k in range(2):
        ref = HR.heun_sample(params, x0[k], ys[k], S)
        err, bound = HR.max_err(x[k], ref), HR.BOUND[prec] * max(1.0, float(np.abs(ref).max()))
        print(f"heun {prec} x0={with_x0} y{k}: {err:.3e} (bound {bound:.1e})")
        assert np.all(np.isfinite(x[k])) and err < bound, err


def test_snapshots_launch_vs_oracle(dmip):
    """dmip_em_sample_snapshots (fp32x3): the states after steps 2 and 4, tests/test_gpu_x3.py's 1e-4."""
    L = dmip._lib
    m, ys, ref = _sde_case(dmip, "cde64")
    before = L.calls["em_sample_snapshots"]
    x, snaps = m.sample_trajectory(torch.from_numpy(ys).to(DEV), N, S, snapshot_every=2, seed=SEED, precision="fp32x3")
    L.device_status(torch.device(DEV))
    assert L.calls["em_sample_snapshots"] == before + 1 and tuple(snaps.shape) == (2, 2, N, 2)
    assert torch.equal(snaps[-1], x) and _rel(x.cpu().numpy(), ref) < TOL32
    params = HR.params_of(m.sde.a)
    for k in range(2):
        _, rs = O.cde_sample(params, ys[k], N, S, SEED, stream=k, snapshots={2, 4})
        for i, step in enumerate((2, 4)):
            assert _rel(snaps[i, k].cpu().numpy(), rs[step]) < TOL32


def test_lmbd1_launch_vs_restatement(dmip):
    """dmip_em_sample_lmbd at lmbd = 1 (exact f32): the f64 Euler restatement from the chains' own start states, to
    the exact-f32 engine's bound HR.BOUND["fp32"] (tests/test_gpu_lmbd.py's short runs)."""
    L = dmip._lib
    m, ys, _ = _sde_case(dmip, "cde64")
    before = L.calls["em_sample_lmbd"]
    x = m.sample_device(torch.from_numpy(ys).to(DEV), N, S, seed=SEED, precision="fp32", lmbd=1.0)
    L.device_status(torch.device(DEV))
    assert L.calls["em_sample_lmbd"] == before + 1
    x = x.cpu().numpy()
    params = HR.params_of(m.sde.a)
    for k in range(2):
        ref = HR.euler_sample(params, HR.x0_of_seed(SEED, N, 2, stream=k), ys[k], S)
        err, bound = HR.max_err(x[k], ref), HR.BOUND["fp32"] * max(1.0, float(np.abs(ref).max()))
        print(f"lmbd=1 fp32 y{k}: {err:.3e} (bound {bound:.1e})")
        assert np.all(np.isfinite(x[k])) and err < bound, err


def test_injected_noise_launch_vs_oracle(dmip):
    """dmip_em_sample with noise_dev (exact f32): the oracle's EM loop on the same normals, tests/test_gpu_f32.py's
    short-run 1e-4."""
    m, ys, _ = _sde_case(dmip, "cde64")
    nz = np.random.default_rng(3).normal(size=(S + 1, 2, N, 2)).astype(np.float32)
    x = m.sample_device(torch.from_numpy(ys).to(DEV), N, S, noise=torch.from_numpy(nz).to(DEV), precision="fp32")
    dmip._lib.device_status(torch.device(DEV))
    x = x.cpu().numpy()
    params = HR.params_of(m.sde.a)
    for k in range(2):
        ref = O.em_sample(lambda xx, tau: O.cde_a(params, xx, ys[k], tau), nz[0, k], S, noise=nz[1:, k])
        assert np.all(np.isfinite(x[k])) and _rel(x[k], ref) < TOL32, _rel(x[k], ref)


def test_log_prob_launch_vs_fixture(dmip, golden):
    """dmip_flow_logp on fixture case (a) of flow_logp.npz (ckpt_lin, 37 rows, S = 20), at the gate of
    tests/test_gpu_flow_logp.py: e_gpu <= 4 e_cpu + 1e-6 against the f64 values."""
    z = golden("flow_logp.npz")
    m = dmip.CDE(2, 2, [64] * 3)
    m.sde.a.load_state_dict(state_from_npz(golden("ckpt_lin.npz")))
    before = dmip._lib.calls["flow_logp"]
    logp, lat = m.log_prob(torch.from_numpy(z["a_x"]).to(DEV), torch.from_numpy(z["a_y"]).to(DEV),
                           num_steps=int(z["a_S"]), return_latent=True)
    assert dmip._lib.calls["flow_logp"] == before + 1
    for got, r64, r32 in ((logp, z["a_logp_f64"], z["a_logp_f32_cpu"]), (lat, z["a_latent_f64"], z["a_latent_f32_cpu"])):
        got = got.cpu().numpy().astype(np.float64)
        e_gpu, e_cpu = np.abs(got - r64).max(), np.abs(r32.astype(np.float64) - r64).max()
        assert np.all(np.isfinite(got)) and e_gpu <= 4 * e_cpu + 1e-6, (e_gpu, e_cpu)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_dps_and_mh_launch_vs_oracle(dmip, golden, precision):
    """dmip_dps_sample_ex and dmip_mh_sample_ex at their one shape with the golden surrogate, at the bounds of
    tests/test_gpu_surrogate.py: DPS |x - ref| < 1e-3 max(1, |ref|) against the f64 oracle (a prior with a small,
    smooth output layer, as there); MH at least 95 % of the chains within 1e-5 of the oracle's."""
    L = dmip._lib
    sur_model, sur = _surrogate(golden)
    ys = golden("data_scat.npz")["y_test"][7:9].astype(np.float32)
    torch.manual_seed(3)
    m = dmip.DPS(3, 23, [256] * 3, sur_model, zeta=0.05, guidance="norm")
    with torch.no_grad():
        last = [l for l in m.prior_net if isinstance(l, torch.nn.Linear)][-1]
        last.weight.mul_(0.1)
        last.bias.fill_(0.1)
    prior = HR.params_of(m.prior_net)
    before = L.calls["dps_sample"], L.calls["mh_sample"]
    x = m.sample_device(torch.from_numpy(ys).to(DEV), N, S, seed=SEED, precision=precision)
    L.device_status(torch.device(DEV))
    x = x.cpu().numpy()
    for k in range(2):
        ref = O.dps_sample(prior, sur, ys[k], N, S, SEED, zeta=0.05, mode="norm", stream=k)
        err = np.abs(x[k] - ref).max()
        print(f"dps {precision} y{k}: {err:.3e}")
        assert np.all(np.isfinite(x[k])) and err < 1e-3 * max(1.0, np.abs(ref).max()), err
    pr = importlib.import_module("diffusion-modelling-for-inverse-problems_amd.problems")
    xm = pr.mh_sample(sur_model, {"a": 0.2, "b": 0.01, "lambd_bd": 1000}, torch.from_numpy(ys), N, S, 0.5, seed=SEED,
                      precision=precision).cpu().numpy()
    assert (L.calls["dps_sample"], L.calls["mh_sample"]) == (before[0] + 1, before[1] + 1)
    for k in range(2):
        ref, _ = O.mh_sample(sur, ys[k], S, 0.5, seed=SEED, n_chains=N, stream=k)
        same = np.all(np.abs(xm[k] - ref) <= 1e-5, axis=1)
        assert np.all(np.isfinite(xm[k])) and same.mean() >= 0.95, (k, same.mean())
