"""Every kernel family at two VP-SDEs that are not the default (beta_min 0.1, beta_max 20, T 1): the forward process
is an argument of every entry point (dmip_vpsde), read from the model at call time, and no other test passes anything
but the default. Needs an MI355X: `pytest -m gpu`.

The SDEs, the cases, their references and their bounds are tests/sde_cases.py's; each bound is the one the project
asserts for that kernel against that reference at the default SDE (named there). tests/test_sde_params_host.py shows on
the CPU that every case's reference moves by at least 50 of its bounds when any one of beta_min, beta_max, T is reset to
its default, so a kernel that ignored a parameter, took 1 - ts for T - ts or 1 / S for T / S would fail here; it also
pins the references to the reference implementation's own output at these SDEs (tests/golden/sde_params.npz).
Every sampler case (Euler, injected noise, Heun and its snapshots, the per-step loop, sample_with_log_prob, DPS) and
log_prob also asserts that two chain_offset shards are bit-identical to the whole run (log_prob has no chains: its rows
are independent) and that in a launch with two observations each equals its single launch bit for bit -- where the
chains come from the generator, whose stream is keyed by the observation's index, the first does, and the second is
compared with the reference on stream 1. Every case prints its observed error (DESIGN.md section 6 lists them).
"""
import ctypes
import importlib
import warnings

import numpy as np
import pytest
import torch

import heun_ref as HR
import oracle as O
import sde_cases as C
from conftest import GOLDEN
from flow_gpu import DEV, bits, dev, gate

pytestmark = pytest.mark.gpu

TAGS = list(C.SDES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _tr(dmip):
    return importlib.import_module(dmip.__name__ + ".training")


def _at(dmip, m, tag):
    return C.set_sde(dmip, m, C.SDES[tag])


# ------------------------------------------------------------------------------------------ schedule kernel
@pytest.mark.parametrize("S", [7, 200])
@pytest.mark.parametrize("tag", TAGS)
def test_schedule_bit_exact(dmip, golden, tag, S):
    L = dmip._lib
    z = golden("sde_params.npz")
    bmin, bmax, T = C.SDES[tag]
    out = torch.empty(S + 1, 4, device=DEV)
    L.check(L.lib().dmip_schedule(S, ctypes.byref(L.vpsde(bmin, bmax, T)), L.ptr(out), L.stream_of(out.device)))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    ts, tau = O.schedule(S, T)
    for col, name, ora in ((0, "ts", ts), (1, "tau", tau), (2, "beta", O.vp_beta(tau, bmin, bmax))):
        assert np.array_equal(o[:, col], z[f"{tag}_{name}_{S}"]), name
        assert np.array_equal(o[:, col], ora), name
    # g: correctly rounded on the device; torch-CPU's vectorised sqrt is within one ulp (tests/test_gpu_parity.py)
    assert np.array_equal(o[:, 3], O.vp_g(tau, bmin, bmax))
    assert np.abs(o[:, 3].view(np.int32) - z[f"{tag}_g_{S}"].view(np.int32)).max() <= 1


# ------------------------------------------------------------------------------------------ Euler samplers
def _sample(dmip, m, cid, ys, n, **kw):
    cls, W, xd, yd, _, prec, bound, extra = C.EULER[cid]
    key = {"CDE": "em_sample", "Posterior": "em_sample_posterior", "CDiffE": "em_sample_cdiffe"}[cls]
    before = dmip._lib.calls[key]
    x = m.sample_device(dev(ys), n, C.EULER_STEPS, C.MEAN, C.STD, seed=C.EULER_SEED, precision=prec, **extra, **kw)
    dmip._lib.device_status(torch.device(DEV))
    assert dmip._lib.calls[key] == before + 1  # the fused kernel ran
    return x


@pytest.mark.parametrize("cid", list(C.EULER))
@pytest.mark.parametrize("tag", TAGS)
def test_euler_samplers_vs_oracle(dmip, tag, cid):
    """The fused reverse-SDE samplers of every engine with mean 0.3, std 1.5 against the oracle's chains (it restates
    the product RNG); two chain_offset shards are bit-identical to the whole run; in a launch with two observations
    the first is bit-identical to its single launch and the second (RNG stream 1) meets the oracle's to the bound."""
    cls, W, xd, yd, n, prec, bound, extra = C.EULER[cid]
    sde = C.SDES[tag]
    m, _, _, ys = C.euler_model(dmip, cid)
    _at(dmip, m, tag)
    ref = C.euler_ref(dmip, cid, sde)
    x = _sample(dmip, m, cid, ys[0], n)
    err = C.rel(x[0].cpu().numpy(), ref)
    print(f"SDE {tag} {cid}: max |kernel - oracle| / max(1, |ref|) = {err:.3e} (bound {bound:.1e}; max |ref| "
          f"{np.abs(ref).max():.4g})")
    assert torch.isfinite(x).all() and err < bound, err
    n0 = n // 3
    lo = _sample(dmip, m, cid, ys[0], n0, chain_offset=0)
    hi = _sample(dmip, m, cid, ys[0], n - n0, chain_offset=n0)
    np.testing.assert_array_equal(bits(torch.cat([lo, hi], 1)), bits(x))
    two = _sample(dmip, m, cid, ys, n)
    np.testing.assert_array_equal(bits(two[0]), bits(x[0]))
    err1 = C.rel(two[1].cpu().numpy(), C.euler_ref(dmip, cid, sde, 1))
    print(f"SDE {tag} {cid}: second observation {err1:.3e}")
    assert err1 < bound, err1


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("lmbd", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("tag", TAGS)
def test_injected_noise_trajectory_matches_reference(dmip, golden, tag, lmbd, prec):
    """The reference's own loop at this SDE (sde_params.npz: lmbd = 0 its forward() with mean 0.3, std 1.5; lmbd 0.5
    and 1 its loop body with sde.mu / sde.sigma), its x0 normals and per-step normals injected; the bounds of
    tests/test_gpu_lmbd.py test_lmbd_trajectory_matches_reference at 10 steps."""
    z = golden("sde_params.npz")
    m = dmip.CDE(2, 2, [64] * 3)
    m.sde.a.load_state_dict({f"{i}.{k}": torch.from_numpy(z[f"net_{i}_{k}"]) for i in (0, 3, 5, 7)
                             for k in ("weight", "bias")})
    _at(dmip, m, tag)
    noise = np.concatenate([z[f"{tag}_z0"][None], z[f"{tag}_xi"]], 0)[:, None]
    S, n = noise.shape[0] - 1, noise.shape[2]
    mean, std = (C.MEAN, C.STD) if lmbd == 0.0 else (0.0, 1.0)
    out = m.sample_device(dev(z[f"{tag}_y"]), n, S, mean, std, noise=dev(noise), precision=prec, lmbd=lmbd)
    dmip._lib.device_status(torch.device(DEV))
    ref = z[f"{tag}_l{lmbd}_final"]
    err = np.abs(out[0].cpu().numpy() - ref).max()
    bound = (1e-4 if prec == "fp32" else 1e-3) * max(1.0, np.abs(ref).max())
    print(f"SDE {tag} lmbd={lmbd} {prec}: max |kernel - reference| = {err:.3e} (bound {bound:.1e})")
    assert torch.isfinite(out).all() and err < bound, err
    # two observations in one launch share the injected normals: the first equals its single launch
    ys2 = np.stack([z[f"{tag}_y"], z[f"{tag}_y"] + 0.5]).astype(np.float32)
    two = m.sample_device(dev(ys2), n, S, mean, std, noise=dev(np.repeat(noise, 2, 1)), precision=prec, lmbd=lmbd)
    one = m.sample_device(dev(ys2[1]), n, S, mean, std, noise=dev(noise), precision=prec, lmbd=lmbd)
    np.testing.assert_array_equal(bits(two[0]), bits(out[0]))
    np.testing.assert_array_equal(bits(two[1]), bits(one[0]))


# ------------------------------------------------------------------------------------------ Heun
def _heun_bound(prec, ref):
    return HR.BOUND[prec] * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("cid", list(C.HEUN))
@pytest.mark.parametrize("tag", TAGS)
def test_heun_vs_restatement(dmip, tag, cid, prec):
    """solver="heun", x0 injected, S = 5, against heun_ref in f64 to HR.BOUND (the per-step loop where the exact-f32
    kernel is left out, as tests/test_gpu_heun.py); shards from the seed with mean 0.3, std 1.5 are bit-identical to
    the whole run and the run meets the restatement from the same start states; two observations equal their single
    launches."""
    kind, W, xd, yd, n = C.HEUN[cid]
    m, params, prior, y, x0 = C.heun_model(dmip, cid)
    _at(dmip, m, tag)
    sde = C.SDES[tag]
    ref = C.heun_ref(dmip, cid, sde)
    mode = dmip._lib.DMIP_SAMPLER_CDE if kind == "cde" else dmip._lib.DMIP_SAMPLER_POSTERIOR
    fused = dmip._lib.ode_sample_supported(W, 3, xd, yd, mode, prec)
    before = dmip._lib.calls.get("ode_sample", 0)
    run = lambda yy, k, **kw: m.sample_device(dev(yy), k, C.HEUN_STEPS, solver="heun", precision=prec, **kw)  # noqa: E731
    out = run(y, n, x0=dev(x0))
    dmip._lib.device_status(torch.device(DEV))
    assert dmip._lib.calls.get("ode_sample", 0) == before + int(fused)
    err = HR.max_err(out[0].cpu().numpy(), ref)
    print(f"SDE {tag} heun {cid} {prec}: max |kernel - f64 restatement| = {err:.3e} (bound {_heun_bound(prec, ref):.1e})")
    assert torch.isfinite(out).all() and err < _heun_bound(prec, ref), err
    ys2 = np.stack([y, y + 0.5]).astype(np.float32)
    two = run(ys2, n, x0=dev(np.stack([x0, x0])))
    np.testing.assert_array_equal(bits(two[0]), bits(out[0]))
    np.testing.assert_array_equal(bits(two[1]), bits(run(ys2[1], n, x0=dev(x0))[0]))
    # from the seed, mean 0.3 and std 1.5
    seeded = lambda k, off: m.sample_device(dev(y), k, C.HEUN_STEPS, C.MEAN, C.STD, seed=77, chain_offset=off,  # noqa: E731
                                            solver="heun", precision=prec)
    full = seeded(n, 0)
    np.testing.assert_array_equal(bits(torch.cat([seeded(n // 3, 0), seeded(n - n // 3, n // 3)], 1)), bits(full))
    if fused:  # (the loop draws its start states from its own stream: test_unfused_loop)
        x0s = HR.x0_of_seed(77, n, xd, mean=C.MEAN, std=C.STD)
        rs = HR.heun_sample(params, x0s, y, C.HEUN_STEPS, prior, **C.kw(sde))
        errs = HR.max_err(full[0].cpu().numpy(), rs)
        print(f"SDE {tag} heun {cid} {prec}: from the seed, mean 0.3 std 1.5: {errs:.3e} (bound "
              f"{_heun_bound(prec, rs):.1e})")
        assert errs < _heun_bound(prec, rs), errs


@pytest.mark.parametrize("tag", TAGS)
def test_heun_snapshots(dmip, tag):
    """sample_trajectory(solver="heun") on the width-64 CDE: the states after every full step against heun_ref's,
    for both observations of one launch (RNG streams 0 and 1); the first equals its single launch and two
    chain_offset shards equal the whole run, snapshots included, bit for bit."""
    m, params, prior, y, _ = C.heun_model(dmip, "cde64")
    _at(dmip, m, tag)
    n, seed = 100, 9
    traj = lambda yy, k, off: m.sample_trajectory(dev(yy), k, C.HEUN_STEPS, snapshot_every=1, seed=seed,  # noqa: E731
                                                  chain_offset=off, precision="fp32", solver="heun")
    x, snaps = traj(y, n, 0)
    dmip._lib.device_status(torch.device(DEV))
    assert tuple(snaps.shape) == (C.HEUN_STEPS, 1, n, 2) and torch.equal(snaps[-1], x)
    ys2 = np.stack([y, y + 0.5]).astype(np.float32)
    x2, snaps2 = traj(ys2, n, 0)
    np.testing.assert_array_equal(bits(x2[0]), bits(x[0]))
    np.testing.assert_array_equal(bits(snaps2[:, 0]), bits(snaps[:, 0]))
    for k in range(2):
        xr, sr = HR.heun_sample(params, HR.x0_of_seed(seed, n, 2, stream=k), ys2[k], C.HEUN_STEPS, snapshot_every=1,
                                **C.kw(C.SDES[tag]))
        for i in range(C.HEUN_STEPS):
            err = HR.max_err(snaps2[i, k].cpu().numpy(), sr[i])
            assert err < _heun_bound("fp32", sr[i]), (k, i, err)
        print(f"SDE {tag} heun snapshots, observation {k}: final {HR.max_err(x2[k].cpu().numpy(), xr):.3e} (bound "
              f"{_heun_bound('fp32', xr):.1e})")
    (xl, sl), (xh, sh) = traj(y, 30, 0), traj(y, n - 30, 30)
    np.testing.assert_array_equal(bits(torch.cat([xl, xh], 1)), bits(x))
    np.testing.assert_array_equal(bits(torch.cat([sl, sh], 2)), bits(snaps))


@pytest.mark.parametrize("solver", ["heun", "euler"])
@pytest.mark.parametrize("tag", TAGS)
def test_unfused_loop(dmip, tag, solver):
    """A shape without a fused sampler (xdim 4) steps through the per-step loop, which reads T and the coefficients
    from the model's SDE objects: Heun from x0, and the lmbd = 1 Euler loop from its own start states (mean 0.3, std
    1.5), against the f64 restatements to HR.BOUND["fp32"]; shards are bit-identical, and in a launch with two
    observations the first equals its single launch (Heun from x0: both do)."""
    m, params, y, x0 = C.loop_model(dmip)
    _at(dmip, m, tag)
    assert not dmip._lib.sampler_supported(64, 3, 4, 5, dmip._lib.DMIP_SAMPLER_CDE, "fp32")
    ref = C.loop_ref(dmip, solver, C.SDES[tag])
    before = dmip._lib.calls["mlp_forward"]
    if solver == "heun":
        run = lambda k, off, **kw: m.sample_device(dev(y), k, C.LOOP_STEPS, solver="heun", chain_offset=off, **kw)  # noqa: E731
        out = run(C.LOOP_N, 0, x0=dev(x0))
        full = run(90, 0, seed=C.LOOP_SEED)
        parts = [run(40, 0, seed=C.LOOP_SEED), run(50, 40, seed=C.LOOP_SEED)]
    else:
        run = lambda k, off: m.sample_device(dev(y), k, C.LOOP_STEPS, C.MEAN, C.STD, seed=C.LOOP_SEED,  # noqa: E731
                                             chain_offset=off, lmbd=1.0)
        out = full = run(C.LOOP_N, 0)
        parts = [run(70, 0), run(C.LOOP_N - 70, 70)]
    assert dmip._lib.calls["mlp_forward"] > before
    err = HR.max_err(out[0].cpu().numpy(), ref)
    print(f"SDE {tag} loop {solver}: max |loop - f64 restatement| = {err:.3e} (bound {_heun_bound('fp32', ref):.1e})")
    assert torch.isfinite(out).all() and err < _heun_bound("fp32", ref), err
    np.testing.assert_array_equal(bits(torch.cat(parts, 1)), bits(full))
    ys2 = np.stack([y, y + 0.5]).astype(np.float32)
    if solver == "heun":
        two = m.sample_device(dev(ys2), C.LOOP_N, C.LOOP_STEPS, solver="heun", x0=dev(np.stack([x0, x0])))
        one = m.sample_device(dev(ys2[1]), C.LOOP_N, C.LOOP_STEPS, solver="heun", x0=dev(x0))
        np.testing.assert_array_equal(bits(two[1]), bits(one[0]))
    else:  # (the second observation draws from its own streams)
        two = m.sample_device(dev(ys2), C.LOOP_N, C.LOOP_STEPS, C.MEAN, C.STD, seed=C.LOOP_SEED, lmbd=1.0)
        assert torch.isfinite(two).all() and not torch.equal(two[1], two[0])
    np.testing.assert_array_equal(bits(two[0]), bits(out[0]))


# ------------------------------------------------------------------------------------------ flow kernels
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("cid", list(C.FLOW))
@pytest.mark.parametrize("tag", TAGS)
def test_log_prob_vs_flow_ref(dmip, tag, cid, prec):
    """log_prob and its latent against flow_ref.log_prob: the flow tests' gate e_gpu <= 8 max(e_cpu, 1e-7), never above
    the 4 e_cpu + 1e-6 it replaced (that one scaled by max(1, |f64|) on the split engine; tests/flow_cases.py). Two observations equal their single launches."""
    m, params, prior, x, y = C.flow_model(dmip, cid)
    _at(dmip, m, tag)
    sde = C.SDES[tag]
    (l64, z64), (l32, z32) = C.flow_logp_ref(dmip, cid, sde), C.flow_logp_ref(dmip, cid, sde, np.float32)
    logp, lat = m.log_prob(dev(x), dev(y), num_steps=C.FLOW_STEPS, return_latent=True, precision=prec)
    scaled = prec != "fp32"
    gate(f"SDE {tag} {cid} {prec} logp", logp.cpu().numpy(), l64, l32, scaled=scaled)
    gate(f"SDE {tag} {cid} {prec} latent", lat.cpu().numpy(), z64, z32, scaled=scaled)
    ys2 = np.stack([y, y + 0.5]).astype(np.float32)
    two = m.log_prob(dev(np.stack([x, x])), dev(ys2), num_steps=C.FLOW_STEPS, precision=prec)
    np.testing.assert_array_equal(bits(two[0]), bits(logp))
    np.testing.assert_array_equal(bits(two[1]), bits(m.log_prob(dev(x), dev(ys2[1]), num_steps=C.FLOW_STEPS,
                                                                precision=prec)))


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("cid", list(C.FLOW))
@pytest.mark.parametrize("tag", TAGS)
def test_sample_with_log_prob_vs_restatement(dmip, tag, cid, prec):
    """sample_with_log_prob with mean 0.3, std 1.5 from given start states against flow_sample_ref (the scaled gate
    of tests/test_gpu_flow_sample.py); shards from the seed are bit-identical to the whole run, and two observations
    in one launch equal their single launches."""
    m, params, prior, x, y = C.flow_model(dmip, cid)
    _at(dmip, m, tag)
    sde = C.SDES[tag]
    (x64, q64), (x32, q32) = C.flow_sample_ref(dmip, cid, sde), C.flow_sample_ref(dmip, cid, sde, np.float32)
    n = x.shape[0]
    xs, logq = m.sample_with_log_prob(dev(y), n, C.FLOW_STEPS, C.MEAN, C.STD, x0=dev(C.flow_x0(dmip, cid)),
                                      precision=prec)
    gate(f"SDE {tag} {cid} {prec} sample x", xs.cpu().numpy(), x64, x32)
    gate(f"SDE {tag} {cid} {prec} sample logq", logq.cpu().numpy(), q64, q32)
    full = m.sample_with_log_prob(dev(y), 37, C.FLOW_STEPS, C.MEAN, C.STD, seed=5, precision=prec)
    lo = m.sample_with_log_prob(dev(y), 13, C.FLOW_STEPS, C.MEAN, C.STD, seed=5, precision=prec)
    hi = m.sample_with_log_prob(dev(y), 24, C.FLOW_STEPS, C.MEAN, C.STD, seed=5, chain_offset=13, precision=prec)
    for k in range(2):
        np.testing.assert_array_equal(bits(torch.cat([lo[k], hi[k]], 0)), bits(full[k]))
    ys2 = np.stack([y, y + 0.5]).astype(np.float32)
    x0 = C.flow_x0(dmip, cid)
    two = m.sample_with_log_prob(dev(ys2), n, C.FLOW_STEPS, C.MEAN, C.STD, x0=dev(np.stack([x0, x0])), precision=prec)
    one = m.sample_with_log_prob(dev(ys2[1]), n, C.FLOW_STEPS, C.MEAN, C.STD, x0=dev(x0), precision=prec)
    for k, single in enumerate((xs, logq)):
        np.testing.assert_array_equal(bits(two[k][0]), bits(single))
        np.testing.assert_array_equal(bits(two[k][1]), bits(one[k]))


# ------------------------------------------------------------------------------------------ DPS
@pytest.fixture(scope="module")
def surrogate(dmip):
    fm, _ = dmip.load_forward_model(GOLDEN)
    return fm.to(DEV)


@pytest.mark.parametrize("prec", ["fp32x3", "fp32"])
@pytest.mark.parametrize("guidance,zeta", C.DPS_PAIRS)
@pytest.mark.parametrize("tag", list(C.DPS_SDES))
def test_dps_vs_oracle(dmip, surrogate, tag, guidance, zeta, prec):
    """The fused DPS kernels against oracle.dps_sample(T=, beta_min=, beta_max=), as
    tests/test_gpu_surrogate.py test_dps_vs_oracle_product_rng: 1e-3 max(1, |ref|); fp32x3 through the default path,
    which resamples in exact f32 when a chain leaves fp16's range. Whether it does is asserted
    (sde_cases.dps_falls_back), so that what is compared is known to be the split engine's own result with its
    coefficient table (dps_x3_coef_kernel) at A and at C -- C = (1.1, 8, 1.25) has beta_min and beta_max - beta_min
    inexact in f32 and T above 1 -- and the documented resampling at B, where the Tweedie estimate divides by
    mean_weight(T) = e^-10 and passes 65504 in the first step. Shards are bit-identical to the whole run; in a launch
    with two observations the first is its single launch bit for bit and the second (RNG stream 1) meets the oracle's."""
    m, _ = C.dps_model(dmip, guidance, zeta, surrogate)
    sde = C.DPS_SDES[tag]
    C.set_sde(dmip, m, sde)
    ys = C.dps_ys()
    ref = C.dps_ref(dmip, guidance, zeta, sde)
    n, S, seed = C.DPS_N, C.DPS_STEPS, C.DPS_SEED
    par = importlib.import_module(dmip.__name__ + ".parallel")

    def run(yy, k, off=0):
        """(x, resampled in exact f32?)"""
        if prec == "fp32":
            x = m.sample_device(dev(yy), k, S, seed=seed, chain_offset=off, precision=prec)
            dmip._lib.device_status(torch.device(DEV))
            return x, False
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            x = par.sample_checked(m, dev(yy), k, S, 0, 1, seed=seed, chain_offset=off)
        return x, any("fp16 range" in str(r.message) for r in w)

    before = dmip._lib.calls.get("dps_sample", 0)
    x, fell_back = run(ys[0], n)
    assert fell_back == (prec == "fp32x3" and C.dps_falls_back(tag, guidance, zeta))
    assert dmip._lib.calls["dps_sample"] == before + 1 + fell_back
    err = C.rel(x[0].cpu().numpy(), ref)
    print(f"SDE {tag} dps {guidance} zeta={zeta} {prec}: {err:.3e} (bound {C.DPS_BOUND:.1e}; max |ref| "
          f"{np.abs(ref).max():.4g}; resampled in f32: {fell_back})")
    assert torch.isfinite(x).all() and err < C.DPS_BOUND, err
    np.testing.assert_array_equal(bits(torch.cat([run(ys[0], 20)[0], run(ys[0], n - 20, 20)[0]], 1)), bits(x))
    two, fb2 = run(ys, n)
    np.testing.assert_array_equal(bits(two[0]), bits(x[0]))
    err1 = C.rel(two[1].cpu().numpy(), C.dps_ref(dmip, guidance, zeta, sde, 1))
    print(f"SDE {tag} dps {guidance} zeta={zeta} {prec}: second observation {err1:.3e} (resampled in f32: {fb2})")
    assert err1 < C.DPS_BOUND, err1


# ------------------------------------------------------------------------------------------ training kernels
def _fused(dmip, m, lf, batch, precision):
    tr = _tr(dmip)
    cfg = tr.fused_config(m, lf)
    assert cfg is not None
    key = "loss_grad" if precision == "bf16" else "loss_grad_f32"
    before = dmip._lib.calls.get(key, 0)
    loss, info = tr.fused_loss_grad(m, lf, cfg, *[dev(a) for a in batch], precision=precision)
    assert dmip._lib.calls[key] == before + 1
    return float(loss), {k: float(v) for k, v in info.items()}, [p.grad.detach().cpu().numpy()
                                                                  for p in m.sde.a.parameters()]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["pinn", "dsm"])
def test_fused_loss_grad_vs_reference_at_sde_a(dmip, golden, name, precision):
    """DSMLoss and PINNLoss(FPE, L2 / L1) on the reference's batch at SDE A (sde_params.npz) against its autograd
    value and gradients: exact f32 to tests/test_gpu_train_f32.py test_f32_loss_grad_vs_reference_width64's bounds,
    the bf16 engine to tests/test_gpu_parity.py test_fused_loss_grad_vs_reference_fixture's."""
    z = golden("sde_params.npz")
    m = dmip.CDE(2, 2, [64] * 3)
    m.sde.a.load_state_dict({f"{i}.{k}": torch.from_numpy(z[f"net_{i}_{k}"]) for i in (0, 3, 5, 7)
                             for k in ("weight", "bias")})
    m.sde.a.to(DEV)
    _at(dmip, m, "A")
    loss, info, grads = _fused(dmip, m, C.loss_objects(dmip)[name], [z[f"loss_{k}"] for k in ("x", "y", "t", "eps")],
                               precision)
    ref_loss = float(z["pinn_loss"]) if name == "pinn" else float(z["dsm_rows"].mean())
    errs = [C.rel_l2(g, z[f"{name}_grad_{k}"]) for g, k in zip(grads, C.GRAD_KEYS)]
    lrel = abs(loss - ref_loss) / abs(ref_loss)
    loss_tol, pde_tol, grad_tol = (3e-6, 1e-4, 3e-6) if precision == "fp32" else (1e-4, 2e-2, 1e-2)
    print(f"SDE A fixture {name} {precision}: loss rel {lrel:.2e} (bound {loss_tol:.0e}), max grad rel L2 "
          f"{max(errs):.2e} (bound {grad_tol:.0e})")
    assert lrel < loss_tol, lrel
    if name == "pinn":
        assert info["PDE-Loss"] == pytest.approx(float(z["pinn_PDE_Loss"]), rel=pde_tol, abs=1e-7)
    assert max(errs) < grad_tol, errs


@pytest.mark.parametrize("tag", TAGS)
def test_f32_loss_grad_vs_oracle(dmip, tag):
    """(100, 2 hidden, n = 777) with t on [1e-4, T] against oracle.loss_grad(beta_min=, beta_max=): the bounds of
    tests/test_gpu_train_f32.py test_f32_loss_grad_vs_oracle."""
    sde = C.SDES[tag]
    m, _, batch = C.oracle_loss_case(dmip, sde[2])
    m.sde.a.to(DEV)
    _at(dmip, m, tag)
    loss, _, grads = _fused(dmip, m, C.loss_objects(dmip)["pinn"], batch, "fp32")
    ref_loss, ref = C.oracle_loss_ref(dmip, sde[2], sde)
    errs = [C.rel_l2(g, r) for g, r in zip(grads, ref)]
    print(f"SDE {tag} loss_grad_f32 vs oracle: loss rel {abs(loss - ref_loss) / abs(ref_loss):.2e} (bound 3e-7), "
          f"max grad rel L2 {max(errs):.2e} (bound 1e-6)")
    assert loss == pytest.approx(ref_loss, rel=3e-7)
    assert max(errs) < 1e-6, errs


@pytest.mark.parametrize("tag", TAGS)
def test_posterior_loss_vs_oracle(dmip, surrogate, tag):
    """(64, 2 hidden, B = 333) with t on [1e-4, T]: the bounds of tests/test_gpu_posterior_loss.py."""
    sde = C.SDES[tag]
    m, _, _, batch = C.posterior_loss_case(dmip, sde[2])
    m.sde.a.to(DEV)
    _at(dmip, m, tag)
    lf = dmip.PosteriorLoss(surrogate, 0.2, 0.01, 0.01)
    loss, info, tgt = _tr(dmip).posterior_loss_grad(m, lf, *[dev(a) for a in batch], want_target=True)
    rl, rinfo, gp, gl, rt = C.posterior_loss_ref(dmip, sde[2], sde)
    terr = np.abs(tgt.cpu().numpy() - rt).max() / np.abs(rt).max()
    worst = 0.0
    for net, ref in ((m.sde.a.prior_net, gp), (m.sde.a.likelihood_net, gl)):
        lins = [l for l in net if isinstance(l, torch.nn.Linear)]
        for lin, (gw, gb) in zip(lins, ref):
            for got, r in ((lin.weight.grad, gw), (lin.bias.grad, gb)):
                e = np.abs(got.cpu().numpy() - r).max() / (np.abs(r).max() + 1e-300)
                worst = max(worst, e)
                assert np.abs(got.cpu().numpy() - r).max() <= 1e-3 * np.abs(r).max() + 1e-12
    print(f"SDE {tag} posterior loss: loss rel {abs(float(loss) - rl) / abs(rl):.2e} (bound 1e-4), target "
          f"{terr:.2e} and worst gradient {worst:.2e} of max |ref| (bound 1e-3)")
    assert float(loss) == pytest.approx(rl, rel=1e-4)
    assert float(info["PriorLoss"]) == pytest.approx(rinfo["PriorLoss"], rel=1e-4)
    assert terr <= 1e-3


def _check_draws(t, eps, sde, t_eps, debias, B, xdim, seed, k, what):
    rt, reps = C.draws_ref(sde, t_eps, debias, B, xdim, seed, k)
    t, eps = t.cpu().numpy(), eps.cpu().numpy()
    terr = (np.abs(t - rt) / (C.T_RTOL * np.abs(rt) + C.T_ATOL)).max()
    print(f"{what}: t within {terr:.3f} of its bound (rtol 1e-4, atol 1e-6), eps max err "
          f"{np.abs(eps - reps).max():.2e} (bound 2e-5), t in [{t.min():.3e}, {t.max():.6f}], T = {sde[2]}")
    np.testing.assert_allclose(t, rt, rtol=C.T_RTOL, atol=C.T_ATOL)
    np.testing.assert_allclose(eps, reps, rtol=0, atol=C.EPS_ATOL)
    assert t.min() > 0 and t.max() <= sde[2]


@pytest.mark.parametrize("B", C.DRAWS_B)
@pytest.mark.parametrize("debias", [True, False])
@pytest.mark.parametrize("tag,t_eps", C.DRAWS)
def test_train_draws_vs_oracle(dmip, tag, t_eps, debias, B):
    L = dmip._lib
    sde = C.SDES[tag]
    t, eps = torch.empty(B, device=DEV), torch.empty(B, 2, device=DEV)
    L.check(L.lib().dmip_train_draws(ctypes.c_uint64(C.DRAWS_SEED), ctypes.c_uint64(C.DRAWS_K), B, 2, int(debias),
                                     ctypes.byref(L.vpsde(*sde)), t_eps, 1e-4, L.ptr(t), L.ptr(eps),
                                     L.stream_of(t.device)))
    torch.cuda.synchronize()
    _check_draws(t, eps, sde, t_eps, debias, B, 2, C.DRAWS_SEED, C.DRAWS_K,
                 f"SDE {tag} train_draws debias={debias} B={B}")


def _lin_batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 2, generator=g)
    y = x @ torch.tensor([[1, 0.5], [0, 1.]]).T + torch.tensor([0.3, 0.5]) + 0.3 * torch.randn(n, 2, generator=g)
    return x.to(DEV), y.to(DEV)


@pytest.mark.parametrize("debias", [True, False])
@pytest.mark.parametrize("graph", ["1", "0"])
def test_device_train_step_draws_t_on_the_models_T(dmip, monkeypatch, graph, debias):
    """DeviceTrainStep on a model with T = 0.75 (SDE A): the t of its first two steps are oracle.train_draws' at
    the model's (beta_min, beta_max, t_epsilon, T) -- sample_t, which the device step replaces, draws on [.., sde.T]
    -- and none exceeds T."""
    monkeypatch.setenv("DMIP_TRAIN_GRAPH", graph)
    tr = _tr(dmip)
    sde = C.SDES["A"]
    torch.manual_seed(11)
    m = dmip.CDE(2, 2, [64] * 3)
    m.sde.a.to(DEV)
    _at(dmip, m, "A")
    m.sde.debias = debias
    lf = C.loss_objects(dmip)["pinn"]
    step = tr.DeviceTrainStep(m, lf, torch.optim.Adam(m.sde.a.parameters(), lr=1e-3), precision="fp32")
    assert step.graph == (graph == "1")
    B = 4096
    for k in range(2):
        out = step(*_lin_batch(B, k))
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        _check_draws(step.t, step.eps, sde, m.sde.base_sde.t_epsilon, debias, B, 2, step.seed, k,
                     f"DeviceTrainStep graph={graph} debias={debias} step {k}")


def test_training_refuses_a_T_mismatch(dmip):
    """As the samplers' _prepare: a reverse SDE whose T is not its base SDE's is refused by every training entry."""
    tr = _tr(dmip)
    sdes = importlib.import_module(dmip.__name__ + ".sdes")
    m = dmip.CDE(2, 2, [64] * 3)
    m.sde.a.to(DEV)
    m.sde = sdes.PluginReverseSDE(sdes.VariancePreservingSDE(0.5, 4.0, 1.0), m.sde.a, T=0.75, debias=True)
    lf = dmip.DSMLoss()
    with pytest.raises(ValueError, match="must equal the base SDE's T"):
        tr.DeviceTrainStep(m, lf, torch.optim.Adam(m.sde.a.parameters(), lr=1e-3))
    x, y = _lin_batch(8, 0)
    with pytest.raises(ValueError, match="must equal the base SDE's T"):
        tr.fused_loss_grad(m, lf, tr.fused_config(m, lf), x, y, torch.full((8, 1), 0.5, device=DEV),
                           torch.randn(8, 2, device=DEV))
