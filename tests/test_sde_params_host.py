"""The references of the non-default VP-SDE tests, on the CPU (no device):

  1. the oracle and heun_ref / flow_ref, given (beta_min, beta_max, T), reproduce the reference's own output at two
     SDEs that are not its default (tests/golden/sde_params.npz, written by tests/golden/make_golden_sde.py): the
     schedule bit for bit, the trajectories to test_oracle_golden.py's G3 bound, loss and gradients to its G5 bound;
  2. at the default SDE the new keywords change nothing: bit-identical to the hard-coded formulas they replace;
  3. every case of tests/test_gpu_sde_params.py can fail: with any one of beta_min, beta_max, T at its default the
     case's reference moves by at least 50 times the bound the case asserts, in the same norm (tests/sde_cases.py).
     A kernel that ignored one parameter would miss by 50 bounds. Two device cases do NOT reach 50 on their own, on
     the bf16 training kernel's wide bounds (loss 1e-4, gradients 1e-2): test_fused_loss_grad_vs_reference_at_sde_a
     [dsm-bf16] moves by 14.7 bounds when beta_min is reset, and [pinn-bf16] by 43.8 when beta_max is. No beta_min in
     [0.5, 4] or beta_max in [2, 64] carries DSM's gradients past 25 bounds for beta_min (they see it only through
     g(t) and alpha(t) at small t). What is asserted for that kernel is the weaker statement that the pair of runs on
     the fixture batch, one kernel with both losses, moves by 50 (266 for beta_min through PINN, 59.6 for beta_max
     through DSM); a kernel that ignored a parameter in one loss only would still miss by 14 bounds or more;
  4. the training entry points hand the kernels the model's own (beta_min, beta_max, T).
"""
import numpy as np
import pytest

import flow_ref as FR
import heun_ref as HR
import oracle as O
import sde_cases as C

TAGS = list(C.SDES)
F = np.float32


# ------------------------------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("S", [7, 200])
@pytest.mark.parametrize("tag", TAGS)
def test_schedule_bit_exact(golden, tag, S):
    z = golden("sde_params.npz")
    bmin, bmax, T = z[f"{tag}_sde"]
    assert (bmin, bmax, T) == C.SDES[tag]
    ts, tau = O.schedule(S, T)
    assert np.array_equal(ts, z[f"{tag}_ts_{S}"])
    assert np.array_equal(tau, z[f"{tag}_tau_{S}"])
    assert np.array_equal(O.vp_beta(tau, bmin, bmax), z[f"{tag}_beta_{S}"])
    # torch-CPU's vectorised sqrt is not correctly rounded on a handful of entries (test_oracle_golden.py)
    ulp = np.abs(O.vp_g(tau, bmin, bmax).view(np.int32) - z[f"{tag}_g_{S}"].view(np.int32))
    assert ulp.max() <= 1 and (ulp > 0).sum() <= 10
    np.testing.assert_allclose(O.vp_mean_weight(tau, bmin, bmax), z[f"{tag}_mw_{S}"], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(O.vp_var(tau, bmin, bmax), z[f"{tag}_var_{S}"], rtol=2e-6, atol=1e-7)
    assert float(z[f"{tag}_delta_{S}"]) == T / S
    # heun_ref's f32 grid is the same schedule
    htau, hbeta, hg = HR.grid(S, T, np.float32, bmin, bmax)
    assert np.array_equal(htau, tau) and np.array_equal(hbeta, z[f"{tag}_beta_{S}"])
    # and a schedule at any other (beta_min, beta_max, T) is not
    for v in C.variants(C.SDES[tag]).values():
        vt = O.schedule(S, v[2])[1]
        assert not np.array_equal(O.vp_beta(vt, v[0], v[1]), z[f"{tag}_beta_{S}"])


def _fixture_net(z):
    return O.mlp_params_from_state(z, "net_")


@pytest.mark.parametrize("lmbd", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("tag", TAGS)
def test_trajectory_injected_noise(golden, tag, lmbd):
    """The reference's loop at this SDE, its x0 and per-step normals injected: lmbd = 0 through oracle.em_sample
    (the reference's own forward with mean 0.3, std 1.5), lmbd 0.5 and 1 through flow_ref.lmbd_step_f32; the G3
    bound of test_oracle_golden.py test_em_trajectory_injected_noise."""
    z = golden("sde_params.npz")
    bmin, bmax, T = C.SDES[tag]
    p = _fixture_net(z)
    y, z0, xi = z[f"{tag}_y"], z[f"{tag}_z0"], z[f"{tag}_xi"]
    S = xi.shape[0]
    ref = z[f"{tag}_l{lmbd}_final"]
    if lmbd == 0.0:
        x0 = (z0 * np.float32(C.STD) + np.float32(C.MEAN)).astype(np.float32)
        out = O.em_sample(lambda x, tau: O.cde_a(p, x, y, tau), x0, S, T=T, noise=xi, beta_min=bmin, beta_max=bmax)
    else:
        _, tau = O.schedule(S, T)
        out = z0
        for i in range(S):
            out = FR.lmbd_step_f32(out, O.cde_a(p, out, y, tau[i]), xi[i], tau[i], T / S, lmbd, bmin, bmax)[2]
    err = np.abs(out - ref).max()
    print(f"SDE {tag} lmbd={lmbd}: max |oracle - reference| = {err:.3e}, max |ref| = {np.abs(ref).max():.4g}")
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(ref).max()))
    if lmbd == 1.0:  # heun_ref's f64 Euler loop is the same scheme
        assert C.rel(HR.euler_sample(p, z0, y, S, T=T, beta_min=bmin, beta_max=bmax), ref) < 1e-4


@pytest.mark.parametrize("name", ["pinn", "dsm"])
def test_loss_grad_at_sde_a(golden, name):
    """oracle.loss_grad(beta_min=, beta_max=) against the reference's autograd at SDE A; the G5 bounds of
    test_oracle_golden.py test_loss_grad_jets_match_reference_autograd."""
    z = golden("sde_params.npz")
    bmin, bmax, T = C.SDES["A"]
    assert 1e-4 <= z["loss_t"].min() and z["loss_t"].max() <= T and z["loss_t"].max() > 0.9 * T
    loss, comps, grads = O.loss_grad(_fixture_net(z), z["loss_x"], z["loss_y"], z["loss_t"], z["loss_eps"],
                                     **C.LOSS_CFGS[name], **C.LIN_IC, beta_min=bmin, beta_max=bmax)
    if name == "pinn":
        assert loss == pytest.approx(float(z["pinn_loss"]), rel=5e-5)
        assert comps["PDE"] == pytest.approx(float(z["pinn_PDE_Loss"]), rel=5e-5)
    else:
        assert loss == pytest.approx(float(z["dsm_rows"].mean()), rel=5e-5)
    for (gW, gb), k in zip(grads, ["0", "3", "5", "7"]):
        rW, rb = z[f"{name}_grad_{k}_weight"], z[f"{name}_grad_{k}_bias"]
        assert np.abs(gW - rW).max() <= 1e-4 * np.abs(rW).max()
        assert np.abs(gb - rb).max() <= 1e-4 * np.abs(rb).max()


# ------------------------------------------------------------------------------------------ 2. the defaults
def test_defaults_are_bit_identical(golden):
    """heun_ref.grid and oracle.cde_sample without the new keywords equal the hard-coded default formulas they had."""
    for S in (5, 200):
        _, tau = O.schedule(S)
        t32, b32, g32 = HR.grid(S, dtype=np.float32)
        lit = (F(0.1) + (F(19.9) * tau).astype(F)).astype(F)  # sdes.py:21-22 with the default's literals
        assert np.array_equal(t32, tau) and np.array_equal(b32, lit) and np.array_equal(g32, np.sqrt(lit))
        t64, b64, g64 = HR.grid(S)
        old = O.BETA_MIN + (O.BETA_MAX - O.BETA_MIN) * tau.astype(np.float64)
        assert np.array_equal(t64, tau.astype(np.float64)) and np.array_equal(b64, old)
        assert np.array_equal(g64, np.sqrt(old))
        ft, fb, fg, fh = FR.flow_grid(S)
        ftau = (O.linspace_f32(S) * np.float32(1.0)).astype(np.float32).astype(np.float64)
        assert np.array_equal(fb, np.float64(O.BETA_MIN) + np.float64(O.BETA_MAX - O.BETA_MIN) * ftau)
    p = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    y = np.array([0.5, 1.0], np.float32)
    n, S, seed = 64, 10, 1234
    new = O.cde_sample(p, y, n, S, seed)
    st = O.rng_init(seed, np.arange(n), 0)
    x0 = O.rng_normals(st, 2)  # (times 1, plus 0: exact)
    old = O.em_sample(lambda x, tau: O.cde_a(p, x, y, tau), x0, S, rng_state=st, xdim=2)
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32))
    # and the loop written out with the default's literals (em_step's rounding order, models/diffusion.py:40-42)
    st = O.rng_init(seed, np.arange(n), 0)
    x = O.rng_normals(st, 2)
    tau = (F(1.0) - O.linspace_f32(S)).astype(F)
    d32, sd32 = F(1.0 / S), F(np.sqrt(1.0 / S))
    for i in range(S):
        beta = F(F(0.1) + F(F(19.9) * tau[i]))
        g = np.sqrt(beta)
        mu = ((g * O.cde_a(p, x, y, tau[i])).astype(F) - (F(F(-0.5) * beta) * x).astype(F)).astype(F)
        x = (x + (d32 * mu).astype(F)).astype(F)
        x = (x + (F(sd32 * g) * O.rng_normals(st, 2)).astype(F)).astype(F)
    assert np.array_equal(new.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(O.cde_sample(p, y, n, S, seed, beta_min=0.1, beta_max=20.0, T=1.0).view(np.uint32),
                          new.view(np.uint32))
    mz = golden("mlp_io.npz")
    pp, pl = O.mlp_params_from_state(mz, "lin_prior_"), O.mlp_params_from_state(mz, "lin_lik_")
    t = mz["lin_t"]
    s = (O.mlp2_a(pp, mz["lin_x"], t) + O.cde_a(pl, mz["lin_x"], mz["lin_y"], t)).astype(np.float32)
    assert np.array_equal(O.posterior_a(pp, pl, mz["lin_x"], mz["lin_y"], t),
                          (O.vp_g(np.broadcast_to(t, s.shape)) * s).astype(np.float32))


# ------------------------------------------------------------------------------------------ 3. discrimination
def _moves(what, ref, var_refs, tol, dist=None):
    """Every variant's reference is at least FACTOR tol from the test SDE's, in the case's norm."""
    dist = dist or (lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()))
    for name, v in var_refs.items():
        d = dist(v, ref)
        print(f"{what}: {name} at its default moves the reference by {d:.3e} = {d / tol:.3g} bounds")
        assert d >= C.FACTOR * tol, (what, name, d, tol)


def _scale(ref):
    return max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("cid", list(C.EULER))
@pytest.mark.parametrize("tag", TAGS)
def test_euler_cases_discriminate(dmip, tag, cid):
    sde = C.SDES[tag]
    ref = C.euler_ref(dmip, cid, sde)
    assert np.all(np.isfinite(ref))
    _moves(f"{cid} SDE {tag}", ref, {k: C.euler_ref(dmip, cid, v) for k, v in C.variants(sde).items()},
           C.EULER[cid][6] * _scale(ref))


@pytest.mark.parametrize("lmbd", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("tag", TAGS)
def test_fixture_trajectories_discriminate(golden, tag, lmbd):
    """The injected-noise case: the oracle at a variant SDE against the fixture's trajectory; 1e-4 max(1, |ref|) is
    the tighter of the two engines' bounds (exact f32 at 10 steps, tests/test_gpu_lmbd.py)."""
    z = golden("sde_params.npz")
    p = _fixture_net(z)
    y, z0, xi = z[f"{tag}_y"], z[f"{tag}_z0"], z[f"{tag}_xi"]
    ref = z[f"{tag}_l{lmbd}_final"]
    x0 = (z0 * np.float32(C.STD) + np.float32(C.MEAN)).astype(np.float32) if lmbd == 0.0 else z0

    def run(v):
        _, tau = O.schedule(10, v[2])
        out = x0
        for i in range(10):
            out = FR.lmbd_step_f32(out, O.cde_a(p, out, y, tau[i]), xi[i], tau[i], v[2] / 10, lmbd, v[0], v[1])[2]
        return out

    assert C.rel(run(C.SDES[tag]), ref) < 1e-4
    _moves(f"trajectory lmbd={lmbd} SDE {tag}", ref, {k: run(v) for k, v in C.variants(C.SDES[tag]).items()},
           1e-3 * _scale(ref))


@pytest.mark.parametrize("cid", list(C.HEUN))
@pytest.mark.parametrize("tag", TAGS)
def test_heun_cases_discriminate(dmip, tag, cid):
    sde = C.SDES[tag]
    ref = C.heun_ref(dmip, cid, sde)
    e32 = HR.max_err(C.heun_ref(dmip, cid, sde, np.float32), ref)
    print(f"heun {cid} SDE {tag}: max |ref| = {np.abs(ref).max():.4g}, f32 restatement - f64 = {e32:.3e} "
          f"({e32 / _scale(ref):.2e} relative)")
    assert np.all(np.isfinite(ref)) and e32 < HR.BOUND["fp32"] * _scale(ref) / 4  # as tests/test_gpu_heun.py
    _moves(f"heun {cid} SDE {tag}", ref, {k: C.heun_ref(dmip, cid, v) for k, v in C.variants(sde).items()},
           HR.BOUND["fp32x3"] * _scale(ref))  # (the wider of the two engines' bounds)


@pytest.mark.parametrize("solver", ["heun", "euler"])
@pytest.mark.parametrize("tag", TAGS)
def test_loop_cases_discriminate(dmip, tag, solver):
    sde = C.SDES[tag]
    ref = C.loop_ref(dmip, solver, sde)
    _moves(f"loop {solver} SDE {tag}", ref, {k: C.loop_ref(dmip, solver, v) for k, v in C.variants(sde).items()},
           HR.BOUND["fp32"] * _scale(ref))


@pytest.mark.parametrize("cid", list(C.FLOW))
@pytest.mark.parametrize("tag", TAGS)
def test_flow_cases_discriminate(dmip, tag, cid):
    """log_prob (logp and latent) and sample_with_log_prob (x and logq), each against the scaled gate's tolerance
    (the wider of the two the device tests use)."""
    sde = C.SDES[tag]
    for what, fn in (("log_prob", C.flow_logp_ref), ("sample", C.flow_sample_ref)):
        r64, r32 = fn(dmip, cid, sde), fn(dmip, cid, sde, np.float32)
        var = {k: fn(dmip, cid, v) for k, v in C.variants(sde).items()}
        for j in range(2):
            assert np.all(np.isfinite(r64[j]))
            _moves(f"{what}[{j}] {cid} SDE {tag}", r64[j], {k: v[j] for k, v in var.items()},
                   C.flow_tol(r64[j], r32[j], scaled=True))


@pytest.mark.parametrize("guidance,zeta", C.DPS_PAIRS)
@pytest.mark.parametrize("tag", list(C.DPS_SDES))
def test_dps_cases_discriminate(dmip, tag, guidance, zeta):
    sde = C.DPS_SDES[tag]
    ref = C.dps_ref(dmip, guidance, zeta, sde)
    assert np.all(np.isfinite(ref))
    _moves(f"dps {guidance} {zeta} SDE {tag}", ref,
           {k: C.dps_ref(dmip, guidance, zeta, v) for k, v in C.variants(sde).items()}, C.DPS_BOUND * _scale(ref))


def _beta_variants(sde):
    """The loss kernels take t as an input and do not read T: the variants that can move them are the two betas."""
    return {k: v for k, v in C.variants(sde).items() if k != "T"}


def _loss_moves(what, name, d_loss, loss_bound, d_grad, grad_bound):
    """A loss case asserts the value and every gradient tensor, and fails when any of them misses: its distance is
    the largest move among them, each in its own bound."""
    k = max(d_loss / loss_bound, d_grad / grad_bound)
    print(f"{what}: {name} at its default moves the loss by {d_loss:.3e} ({d_loss / loss_bound:.3g} bounds), the "
          f"most-moved gradient tensor by {d_grad:.3e} ({d_grad / grad_bound:.3g} bounds)")
    assert k >= C.FACTOR, (what, name, k)


@pytest.mark.parametrize("tag", TAGS)
def test_loss_cases_discriminate(dmip, golden, tag):
    """The exact-f32 engine on the oracle batch (tests/test_gpu_train_f32.py test_f32_loss_grad_vs_oracle: loss 3e-7,
    gradients 1e-6 relative L2), the posterior loss (tests/test_gpu_posterior_loss.py: 1e-4, 1e-3 of max |ref|), and
    at SDE A the fixture batch on both engines."""
    sde = C.SDES[tag]
    T = sde[2]
    loss, grads = C.oracle_loss_ref(dmip, T, sde)
    for name, v in _beta_variants(sde).items():
        vl, vg = C.oracle_loss_ref(dmip, T, v)
        _loss_moves(f"loss_grad oracle batch SDE {tag}", name, abs(vl - loss) / abs(loss), 3e-7,
                    max(C.rel_l2(a, b) for a, b in zip(vg, grads)), 1e-6)
    pl = C.posterior_loss_ref(dmip, T, sde)
    for name, v in _beta_variants(sde).items():
        vp = C.posterior_loss_ref(dmip, T, v)
        dg = max(np.abs(a - b).max() / np.abs(b).max() for gv, gr in ((vp[2], pl[2]), (vp[3], pl[3]))
                 for wa, wb in zip(gv, gr) for a, b in zip(wa, wb))
        _loss_moves(f"posterior loss SDE {tag}", name, abs(vp[0] - pl[0]) / abs(pl[0]), 1e-4, dg, 1e-3)
    if tag == "A":
        z = golden("sde_params.npz")
        for name, v in _beta_variants(sde).items():
            bf16 = 0.0
            for kind in ("pinn", "dsm"):
                ref_loss = float(z["pinn_loss"]) if kind == "pinn" else float(z["dsm_rows"].mean())
                vl, _, vg = O.loss_grad(_fixture_net(z), z["loss_x"], z["loss_y"], z["loss_t"], z["loss_eps"],
                                        **C.LOSS_CFGS[kind], **C.LIN_IC, beta_min=v[0], beta_max=v[1])
                d = abs(vl - ref_loss) / abs(ref_loss)
                dg = max(C.rel_l2(a, z[f"{kind}_grad_{k}"]) for a, k in zip([a for wb in vg for a in wb], C.GRAD_KEYS))
                # the exact-f32 engine (tests/test_gpu_train_f32.py test_f32_loss_grad_vs_reference_width64: 3e-6, 3e-6)
                _loss_moves(f"fixture {kind} SDE A, exact f32", name, d, 3e-6, dg, 3e-6)
                k = max(d / 1e-4, dg / 1e-2)
                print(f"fixture {kind} SDE A, bf16 bounds: {name} at its default moves it by {k:.3g} bounds")
                bf16 = max(bf16, k)
            # the bf16 engine (tests/test_gpu_parity.py test_fused_loss_grad_vs_reference_fixture: loss 1e-4, gradients
            # 1e-2 relative L2) is one kernel, dmip_loss_grad, run on this batch with both losses: the case is the
            # pair. DSM's gradients alone hardly depend on beta_min (6 to 25 of these wide bounds at any beta_min in
            # [0.5, 4]: they see beta_min through g(t) and alpha(t) at small t only); PINN's initial condition
            # divides by g(0) = sqrt(beta_min) and moves by hundreds. beta_max = 4 and not 12 is what carries the
            # pair past 50 bounds for beta_max (12 gave 28).
            assert bf16 >= C.FACTOR, ("fixture batch on the bf16 engine", name, bf16)


@pytest.mark.parametrize("debias", [True, False])
@pytest.mark.parametrize("tag,t_eps", C.DRAWS)
def test_train_draws_cases_discriminate(tag, t_eps, debias):
    """t at fixed u: the generator's u does not depend on the SDE, so the variants differ in t alone. The uniform
    branch t = t_add + u T reads T only (a kernel that ignored the betas there would be right): its beta variants
    are not asked to move."""
    sde = C.SDES[tag]
    for B in C.DRAWS_B:
        t, eps = C.draws_ref(sde, t_eps, debias, B)
        assert t.max() <= sde[2] and t.min() > 0
        for name, v in C.variants(sde).items():
            if not debias and name != "T":
                continue
            vt, veps = C.draws_ref(v, t_eps, debias, B)
            assert np.array_equal(veps, eps)
            d = np.abs(vt - t) / (C.T_RTOL * np.abs(t) + C.T_ATOL)
            print(f"train_draws SDE {tag} debias={debias} B={B}: {name} moves t by up to {d.max():.3g} bounds")
            assert d.max() >= C.FACTOR


# ------------------------------------------------------------------------------------------ the training entry points
def test_training_struct_carries_the_models_sde(dmip):
    """training.model_vpsde: what DeviceTrainStep, _TrainPlan, fused_loss_grad and posterior_loss_grad hand to the
    kernels is the model's (beta_min, beta_max, T), not T = 1; a reverse SDE whose T is not its base SDE's is refused
    as the samplers refuse it."""
    import importlib
    tr = importlib.import_module(dmip.__name__ + ".training")
    sdes = importlib.import_module(dmip.__name__ + ".sdes")
    m = dmip.CDE(2, 2, [64] * 3)
    assert tuple(getattr(tr.model_vpsde(m), k) for k in ("beta_min", "beta_max", "T")) == C.DEFAULT
    for sde in C.SDES.values():
        s = tr.model_vpsde(C.set_sde(dmip, m, sde))
        assert (s.beta_min, s.beta_max, s.T) == sde
    m.sde = sdes.PluginReverseSDE(sdes.VariancePreservingSDE(0.5, 4.0, 1.0), m.sde.a, T=0.75)
    with pytest.raises(ValueError, match="must equal the base SDE's T"):
        tr.model_vpsde(m)
